"""K3's min / argmin pass (k_vstat_part / k_vstat_final) and the velocity-gradient finalize K4
(k_fin_rows / k_fin_cols) cell by cell against fp64 autograd, with no time loop: the test fills the
adjoint accumulators gA / gk_part / gbeta itself.  The end-to-end gradient tests hold K4 to a rel-L2 of
the whole field, which does not move when one cell is wrong, and K4's special branches (sponge term on
the first argmin of the padded field, source cells, fold strips, nx == 1, the shot unroll's tail, the
256-segment gk_part sum) each touch one cell or one strip.

Reference (fp64 torch autograd, the chain of pde.py:63-71, 38-52, 91):
    v_pad = F.pad(v_phys, (nbc,) * 4, "replicate")
    L = sum(gA_sum (v_pad dt / dx)^2) + sum_s gbeta[s] (v_pad[isz, isx[s]] dt)^2 + GK min(v_pad) / vmin0
with torch.min(v_pad.view(B, -1), dim=-1) (pde.py:41: its backward goes to the first index), GK =
sum(gk_part), vmin0 the detached minimum; expected = dL/dv (times 1500 for normalised input).  v_phys
is the kernel's fp32 denormalisation (+1, /2, *3000, +1500) and dt the fp32 value the C ABI carries,
both widened to fp64, so the reference sees the kernel's inputs.

Bar per output cell, derived from k_fin_rows and not from its output: forming a padded cell's alpha term
rounds to fp32 ns + 4 times (v dt, / dx, ns - 1 shot additions, ga (2 a1), / dx, dt; 2 a1 is exact), a
source term 3 times; everything after is fp64 until the one final rounding of the output.  (A budget of
ns + 8 roundings was proposed for this check; the count read from the kernel is ns + 4, so the bar is
the tighter)
    |got - ref| <= (ns + 4) 2^-24 M + 2^-24 |ref|
M being the same fold of the absolute per-cell terms (sum_s |gA_s| times the chain factor, |gbeta
term|, |GK / vmin|), computed by the same fp64 reference on the absolute accumulators."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import record_margin
from test_gpu_fwi import bits_equal, make_fwi

pytestmark = pytest.mark.gpu

DT, DX = 0.001, 10.0
U = 2.0 ** -24


def denorm32(vn):
    """v_denormalize in the kernel's fp32 operation order."""
    t = vn.astype(np.float32) + np.float32(1.0)
    t = t / np.float32(2.0)
    t = t * np.float32(3000.0)
    return t + np.float32(1500.0)


def model(B, nz, nx, seed, mins):
    """Normalised velocities in [-0.8, 0.8] with the value -0.95 at mins[b] = [(iz, ix), ...]."""
    vn = np.random.default_rng(seed).uniform(-0.8, 0.8, (B, 1, nz, nx)).astype(np.float32)
    for b, cells in enumerate(mins):
        for iz, ix in cells:
            vn[b, 0, iz, ix] = -0.95
    return vn


def reference(vphys32, nbc, isz, isx, gA_sum, GK, gb, scale):
    """dL/dv of the module docstring's L in fp64; also torch.min's padded flat argmin per model."""
    dt = float(np.float32(DT))
    vp = torch.from_numpy(vphys32.astype(np.float64)).requires_grad_(True)
    v_pad = F.pad(vp, (nbc,) * 4, mode="replicate")
    B = vp.shape[0]
    vmin, idx = torch.min(v_pad.reshape(B, -1), dim=-1)
    L = (gA_sum * (v_pad[:, 0] * dt / DX) ** 2).sum()
    for s, x in enumerate(isx):
        L = L + (gb[:, s] * (v_pad[:, 0, isz, x] * dt) ** 2).sum()
    L = L + (GK * vmin / vmin.detach()).sum()
    g, = torch.autograd.grad(L, vp)
    return (g * scale).numpy(), idx.numpy()


def run_case(cuda, case, v_in, nbc, sx, sz_row, vel_mode=0, seed=0, view=False):
    """K3 + K4 on v_in (normalised, or m/s with vel_mode = 1) with random accumulators; asserts vmin /
    argmin and the per-cell bar, returns (gradient, vmin, argmin, coefficient fields)."""
    B, _, nz, nx = v_in.shape
    ns = len(sx)
    ctx = dict(n_grid=nx, nt=150, dx=DX, dt=DT, nbc=nbc, f=15.0, sz=sz_row * DX, gz=0.0, ng=1, ns=ns,
               sx=list(sx), gx=[0])
    fwi = make_fwi(ctx)
    plan = fwi._plan(nz, nx, cuda)
    sz = plan.sizes(B)
    assert (sz.Hp, sz.Wp) == (nz + 2 * nbc, nx + 2 * nbc)
    t = torch.from_numpy(v_in)
    if view:                                   # how InversionEngine passes the model
        t = F.pad(t, (1, 1, 1, 1)).to(cuda)[:, :, 1:-1, 1:-1]
        assert not t.is_contiguous()
    else:
        t = t.to(cuda)
    coeffs, vstat = plan.coeffs(t, vel_mode)
    plan.status()
    rng = np.random.default_rng(1000 + seed)
    gA = rng.standard_normal((B, ns, sz.Hp, sz.ld)).astype(np.float32)
    nblk = int(sz.gk_part) // 8 // (B * ns)
    gk = 0.1 * rng.standard_normal((B, ns * nblk))                         # fp64, mixed signs
    gb = (0.01 * rng.standard_normal((B, ns))).astype(np.float32)
    g = plan.finalize(coeffs, vstat, torch.from_numpy(gA).to(cuda).flatten(), torch.from_numpy(gk).to(cuda).flatten(),
                      torch.from_numpy(gb).to(cuda).flatten(), B, vel_mode).cpu().numpy()
    plan.status()
    raw = vstat.cpu().numpy()
    off = (4 * B + 15) // 16 * 16
    vmin, amin = raw[:4 * B].view(np.float32), raw[off:off + 8 * B].view(np.int64)
    vphys = denorm32(v_in) if vel_mode == 0 else v_in.astype(np.float32)
    flat = vphys.reshape(B, -1)
    assert bits_equal(vmin, flat.min(1)), (case, vmin, flat.min(1))
    assert np.array_equal(amin, flat.argmin(1)), (case, amin, flat.argmin(1))   # first index, row-major

    isx = [int(np.around(x)) + nbc for x in sx]
    gA64 = torch.from_numpy(gA[..., :sz.Wp].astype(np.float64))
    gk64, gb64 = torch.from_numpy(gk), torch.from_numpy(gb.astype(np.float64))
    scale = 1500.0 if vel_mode == 0 else 1.0
    ref, idx = reference(vphys, nbc, sz_row + nbc, isx, gA64.sum(1), gk64.sum(1), gb64, scale)
    M, _ = reference(vphys, nbc, sz_row + nbc, isx, gA64.abs().sum(1), gk64.sum(1).abs(), gb64.abs(), scale)
    vpad = np.pad(vphys[:, 0], ((0, 0), (nbc, nbc), (nbc, nbc)), mode="edge").reshape(B, -1)
    assert np.array_equal(idx, vpad.argmin(1)), case        # torch.min(dim): the first index
    bar = (ns + 4) * U * M + U * np.abs(ref)
    err = np.abs(g.astype(np.float64) - ref)
    ratio = float((err / bar).max())
    record_margin("finalize_per_cell_err_over_bar", case, ratio, 1.0)
    worst = np.unravel_index(np.argmax(err / bar), err.shape)
    assert ratio <= 1.0, (case, ratio, worst, float(g[worst]), float(ref[worst]))
    cf = coeffs[:6 * B * sz.Hp * sz.ld].view(6, B, sz.Hp, sz.ld)[..., :sz.Wp].cpu().numpy()
    return g, vmin.copy(), amin.copy(), cf


NZ, NX, NBC = 10, 12, 8
ARGMIN_CELLS = [(0, 0), (0, NX - 1), (NZ - 1, 0), (NZ - 1, NX - 1),            # corners
                (0, NX // 2), (NZ - 1, NX // 2), (NZ // 2, 0), (NZ // 2, NX - 1),   # edge middles
                (4, 7)]                                                           # interior


@pytest.mark.parametrize("cell", ARGMIN_CELLS)
def test_argmin_position_places_sponge_term(cuda, cell):
    """Branch: apz / apx, the padded cell of the sponge term GK / vmin.  A unique minimum at each
    corner, each edge's middle and an interior cell of a 10 x 12 model: the first padded index of a
    minimum in model row 0 / column 0 is padded row 0 / column 0, otherwise the cell's own padded
    position, so the term lands in one known output cell; vmin bit-equal to the fp32 denormalised
    minimum and argmin equal to np.argmin.  (Every padded copy of an edge cell folds into the same
    output cell, so which copy of an edge minimum takes the term cannot show in the output: only a
    term that leaves the cell's strip, e.g. apx without its + nbc, fails here.)"""
    vn = model(2, NZ, NX, 3, [[cell], [cell]])
    run_case(cuda, f"argmin@{cell}", vn, NBC, [2, 5, 9], 3)


@pytest.mark.parametrize("cells", [[(0, 5), (3, 0)], [(2, NX - 1), (3, 0)]])
def test_argmin_ties_first_index(cuda, cells):
    """Branch: the (value, then index) comparison of vstat_reduce.  The same minimum at two cells
    whose padded copies interleave: the first index in row-major model order wins (torch.min's rule)."""
    vn = model(1, NZ, NX, 4, [cells])
    _, _, amin, _ = run_case(cuda, f"tie@{cells}", vn, NBC, [2, 5, 9], 3)
    assert amin[0] == cells[0][0] * NX + cells[0][1]


@pytest.mark.parametrize("n,kind", [(96, "last"), (96, "tie"), (130, "last"), (130, "tie")])
def test_vstat_parts_and_strided_view(cuda, n, kind):
    """Branch: more than one K3 part (k_vstat_part's chunks, k_vstat_final's combine).  96 x 96 = 9216
    cells run 2 parts, 130 x 130 = 16900 run 3 with a chunk (5634) that is no multiple of 256.  'last':
    the unique minimum is the very last cell (the short last part); 'tie': the same minimum on both
    sides of every part boundary, the lowest index wins.  The model passed as the engine's strided view
    mu[:, :, 1:-1, 1:-1] and as a contiguous tensor gives bit-equal results."""
    cells = n * n
    parts = (cells + 8191) // 8192
    chunk = (cells + parts - 1) // parts
    assert parts == (2 if n == 96 else 3) and (n == 96 or chunk % 256)
    if kind == "last":
        idx = [cells - 1]
    else:
        idx = [p * chunk - 1 for p in range(1, parts)] + [p * chunk for p in range(1, parts)]
    vn = model(2, n, n, 5, [[divmod(i, n) for i in idx]] * 2)
    out = [run_case(cuda, f"parts,n={n},{kind},view={view}", vn, 4, [0, n // 2, n - 1], 2, view=view)
           for view in (False, True)]
    assert out[0][2][0] == min(idx)
    assert bits_equal(out[0][0], out[1][0]) and bits_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])
    for a, b in zip(out[0][3], out[1][3]):
        assert bits_equal(a, b)


@pytest.mark.parametrize("n", [8, 40])
def test_fold_strips_wider_than_a_wave(cuda, n):
    """Branch: the two nbc + 1-wide fold strips of k_fin_rows (lane loop x += 64 over 121 columns) and
    the 121-row folds of k_fin_cols (its 16-row unroll and tail), nbc = 120.  The 8 x 8 model gives
    Hp = Wp = 248 (one pass of the 256-thread row loop), the 40 x 40 one Wp = 280 (the row loop strides)."""
    vn = model(1, n, n, 6, [[(n // 2, n // 2 - 1)]])
    run_case(cuda, f"strips,n={n}", vn, 120, [0, n // 2, n - 1], 2)


@pytest.mark.parametrize("ns", [1, 3, 4, 5])
def test_source_terms_and_shot_unroll(cuda, ns):
    """Branch: the source term z == isz && isx[s] == x and the 4-shot unroll of the gA sum (ns = 4: no
    tail, 5: a tail of one, 1 / 3: tail only).  Shots share a column (summed), sit at ix = 0 and
    ix = nx - 1 (inside the fold strips) and on the argmin cell (source and sponge terms on one cell)."""
    am = (3, 7)
    sx = [am[1], 0, am[1], NX - 1, 4][:ns]
    vn = model(2, NZ, NX, 7, [[am], [am]])
    run_case(cuda, f"sources,ns={ns}", vn, NBC, sx, am[0], seed=ns)


def test_source_row_zero_with_argmin_in_row_zero(cuda):
    """Branch: z == isz against z == apz.  sz on model row 0 and the minimum in row 0 on a source
    column: the source term stays on padded row nbc while the sponge term moves to padded row 0 (the
    first copy of the minimum); both fold into the same output cell."""
    vn = model(2, NZ, NX, 8, [[(0, 5)], [(0, 0)]])
    run_case(cuda, "sz=0,argmin row 0", vn, NBC, [5, 0, 5, NX - 1, 2], 0)


@pytest.mark.parametrize("nz,nx", [(6, 1), (1, 6)])
def test_single_column_and_single_row_models(cuda, nz, nx):
    """Branch: nx == 1 in k_fin_rows (one output column folds the whole padded row: wave 0's strip plus
    a serial tail) and nz == 1 in k_fin_cols (one output row folds every padded row)."""
    vn = model(2, nz, nx, 9, [[(nz // 2, nx // 2)], [(0, 0)]])
    run_case(cuda, f"nz={nz},nx={nx}", vn, 8, [0, nx - 1, 0], 0)


def test_physical_velocity_mode(cuda):
    """Branch: vel_mode = 1 (RDQ_VEL_PHYSICAL), a.scale = 1.  The same velocities in m/s: the gradient
    is the reference's without the factor 1500, and kappa / alpha (every coefficient field) equal the
    normalised call's bit for bit."""
    vn = model(2, NZ, NX, 10, [[(4, 7)], [(0, NX - 1)]])
    gn, vmin_n, amin_n, cf_n = run_case(cuda, "vel_mode=0", vn, NBC, [2, 5, 9], 3)
    gp, vmin_p, amin_p, cf_p = run_case(cuda, "vel_mode=1", denorm32(vn), NBC, [2, 5, 9], 3, vel_mode=1)
    assert bits_equal(vmin_n, vmin_p) and np.array_equal(amin_n, amin_p)
    for name, a, b in zip(("alpha", "temp1", "temp2", "kappa", "beta", "v"), cf_n, cf_p):
        assert bits_equal(a, b), name


def test_batch_of_three_distinct_argmins(cuda):
    """Branch: the batch strides of amin / vmin / gk_part / gbeta.  B = 3 with a different argmin cell
    (corner, edge, interior) per model."""
    vn = model(3, NZ, NX, 11, [[(NZ - 1, NX - 1)], [(0, 4)], [(5, 6)]])
    _, _, amin, _ = run_case(cuda, "B=3", vn, NBC, [2, 5, 9, 5, 0], 3)
    assert list(amin) == [(NZ - 1) * NX + NX - 1, 4, 5 * NX + 6]
