"""Acquisition geometries the other FWI tests never run (they all have sz == gz == 10 and at most one
receiver per padded column), on every time-loop kernel family:

* several receivers on one padded column (ng > n_grid, repeated gx): the plan folds the residuals per
  column (k_rcv_fold, rlane = folded column index, dstride = ncolr) and every forward kernel stores the
  column's extra receivers from one lane (the `if (rmulti)` branches);
* source row != receiver row, on the first / last model row: injection (isz) and recording (igz) are
  keyed separately, and with sz == gz both rows belong to the same wave of the same workgroup;
* two shots on one source column.

Fixtures fwd_multi_rcv / fwd_rcv_list / fwd_split_depth / grad_* come from the reference
(tests/golden/make_golden.py: gen_geometry_paths); tests/test_oracle_golden.py pins the oracle on them,
so the larger grids here lean on the oracle.  Bars are those of tests/test_gpu_fwi.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import ctx_of, load_golden, record_margin, vnorm
from oracle import oracle as O
from test_gpu_fwi import _shot_sum, bits_equal, make_fwi

pytestmark = pytest.mark.gpu

GEOM = ("fwd_multi_rcv", "fwd_rcv_list", "fwd_split_depth")
CKPT_K = 48          # nt = 160 = 3 * 48 + 16: four segments, the first one run short


def _igx(ctx):
    return O.geometry(ctx)[2]


@functools.lru_cache(maxsize=None)
def _small_case(name):
    """Fixture, a random dseis and the oracle's adjoint on it (computed once, read-only)."""
    z = load_golden(name)
    ctx = ctx_of(z)
    vn = vnorm(z["v"])
    B = vn.shape[0]
    f = O.OracleFWI(ctx, B)
    so, c = f.forward(vn, keep_history=True)
    assert bits_equal(so, z["seis"])
    dseis = np.random.default_rng(1).standard_normal(so.shape).astype(np.float32)
    oA, oK, ob = f.adjoint(c, dseis)
    go = f.finalize(c, oA, oK, ob)
    for a in (dseis, oA, oK, ob, go):
        a.setflags(write=False)
    return z, ctx, vn, dseis, oA, oK, ob, go


def _select(plan, family, T, B, exact=True):
    """Pick one kernel family at depth T and assert from launch_info / wide_info / ckpt_info that it is
    the one a call runs.  The wide adjoint runs depth T + 1 (2 and the default 5), which also tells it
    from the narrow one in launch_info."""
    nt = plan.nt
    plan.set_tuning(T, T, 1)
    plan.set_wide_adj_steps(T + 1)
    if family == "persistent" or isinstance(family, int):
        plan.set_persistent(True if family == "persistent" else family)
        plan.set_variant(adj_exact=exact)
        info = plan.launch_info(B)
        assert info["fwd_persistent"] and info["adj_persistent"], info
        assert (info["fwd_T"], info["adj_T"]) == (T, T), info
        if isinstance(family, int):
            assert info["fwd_class"] == family and info["adj_class"] == family, info
        return
    wide = family != "narrow"
    plan.set_persistent(False)
    plan.set_variant(adj_exact=exact, wide_chunked=wide)
    info = plan.launch_info(B)
    assert not info["fwd_persistent"] and not info["adj_persistent"], info
    Ta = T + 1 if wide else T
    assert (info["fwd_T"], info["adj_T"]) == (T, Ta), info
    assert info["fwd_launches"] == -(-nt // T) and info["adj_launches"] == -(-nt // Ta), info
    if not wide:
        wi = plan.wide_info(B)
        assert wi["fwd_spw"] == 1 and wi["adj_spw"] == 1, wi
    if family == "ckpt":
        ci = plan.ckpt_info(B, CKPT_K)
        assert ci["fwd_class"] == 0 and ci["nseg"] == -(-nt // CKPT_K) and nt % CKPT_K, ci


def _run(plan, v, B, dseis, family):
    """(seis ring path, seis history path, per-shot gA [B, ns, Hp, Wp], gbeta [B, ns], gk sum [B], dL/dv)
    of the selected family; plan.status() after every GPU call."""
    sz = plan.sizes(B)
    coeffs, vstat = plan.coeffs(v, 0)
    plan.status()
    if family == "ckpt":
        seis, ck = plan.forward_ckpt(coeffs, B, CKPT_K)
        plan.status()
        seis_r = seis
        gA, gk, gb = plan.adjoint_ckpt(coeffs, ck, dseis, B, CKPT_K)
        plan.status()
    else:
        seis_r, _ = plan.forward(coeffs, B, keep_history=False)
        plan.status()
        seis, hist = plan.forward(coeffs, B, keep_history=True)
        plan.status()
        gA, gk, gb = plan.adjoint(coeffs, hist, dseis, B)
        plan.status()
        del hist
    g = plan.finalize(coeffs, vstat, gA, gk, gb, B, 0)
    plan.status()
    return (seis_r.cpu().numpy(), seis.cpu().numpy(),
            gA.view(B, plan.ns, sz.Hp, sz.ld)[..., :sz.Wp].cpu().numpy(), gb.view(B, -1).cpu().numpy(),
            gk.view(B, -1).sum(1).cpu().numpy(), g.cpu().numpy())


def _assert_exact(got, seis, oA, oK, ob, go, tag):
    """The recipe of test_adjoint_accumulators_bitexact_vs_oracle."""
    assert bits_equal(got[0], seis), (tag, "seis, ring path")
    assert bits_equal(got[1], seis), (tag, "seis, history path")
    assert bits_equal(_shot_sum(got[2]), oA), (tag, "gA")
    assert bits_equal(got[3], ob), (tag, "gbeta")
    np.testing.assert_allclose(got[4], oK, rtol=1e-7, atol=0)
    rel = float(np.linalg.norm(got[5] - go) / np.linalg.norm(go))
    assert rel < 1e-6, (tag, rel)
    return rel


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("family", ["persistent", "narrow", "wide", "ckpt"])
@pytest.mark.parametrize("name", GEOM)
def test_geometry_fixtures_every_family(cuda, name, family, T):
    """Reference fixtures on the 16 x 16 grid (32 x 32 padded), each kernel family at depths 1 and 4:
    seismograms (ring and history paths) bit-equal to the reference's; with the exact-order adjoint and
    a random dseis, shot-summed gA and gbeta bit-equal to the oracle's, gk to fp64 summation order
    (rtol 1e-7), dL/dv within 1e-6 rel-L2 of the oracle's."""
    z, ctx, vn, dseis, oA, oK, ob, go = _small_case(name)
    fwi = make_fwi(ctx)
    v = torch.from_numpy(vn).to(cuda)
    B = v.shape[0]
    plan = fwi._plan(v.shape[2], v.shape[3], v.device)
    assert (plan.ns, plan.ng) == z["seis"].shape[1::2]
    _select(plan, family, T, B)
    got = _run(plan, v, B, torch.tensor(dseis).to(cuda), family)
    rel = _assert_exact(got, z["seis"], oA, oK, ob, go, (name, family, T))
    record_margin("geometry_dLdv_vs_oracle_rel_l2", f"{name},{family},T={T}", rel, 1e-6)


@pytest.mark.parametrize("name", ["grad_multi_rcv", "grad_rcv_list"])
def test_geometry_gradient_vs_reference_autograd(cuda, name):
    """The reference's L1 loss and autograd gradient with receivers sharing columns (its index backward
    accumulates them; one fixture masked), through the product's autograd path: the body of
    test_gradient_vs_reference_autograd."""
    from red_diffeq.core.losses import LossCalculator
    z = load_golden(name)
    fwi = make_fwi(ctx_of(z))
    vn = torch.from_numpy(vnorm(z["v_init"])).to(cuda).requires_grad_(True)
    y = torch.from_numpy(z["y"]).to(cuda)
    mask = torch.from_numpy(z["mask"]).to(cuda) if "mask" in z.files else None
    loss = LossCalculator(None).observation_loss(fwi(vn), y, mask=mask)
    loss.sum().backward()
    fwi.check()
    np.testing.assert_allclose(loss.detach().cpu().numpy(), z["loss"], rtol=2e-6)
    g = vn.grad.cpu().numpy()
    ref = z["grad"]
    err = np.linalg.norm(g - ref) / np.linalg.norm(ref)
    record_margin("grad_vs_reference_autograd_rel_l2", name, err, 5e-5)
    assert err < 5e-5, err
    f = O.OracleFWI(ctx_of(z), vn.shape[0])
    seis, c = f.forward(vnorm(z["v_init"]), keep_history=True)
    _, ds = O.l1_loss(seis, z["y"], z["mask"] if "mask" in z.files else None)
    go = f.finalize(c, *f.adjoint(c, ds))
    err = np.linalg.norm(g - go) / np.linalg.norm(go)
    record_margin("grad_vs_oracle_rel_l2", name, err, 5e-6)
    assert err < 5e-6, err


# OpenFWI-size grid: 70 x 70 model, nbc = 120 (310 x 310 padded), 100 receivers on 70 columns (1 and 2
# per column mixed), receivers on padded row 121 (gz = 10), sources on padded row 144 (sz = 240)
OPENFWI_GEOM = dict(n_grid=70, nt=160, dx=10.0, dt=0.001, nbc=120, f=15.0, sz=240, gz=10, ng=100, ns=3)


@functools.lru_cache(maxsize=None)
def _openfwi_case(st):
    from red_diffeq.utils.synthetic import make_model
    ctx = dict(OPENFWI_GEOM)
    vn = vnorm(make_model("curvefault", 70, 70, seed=13, batch=1))
    f = O.OracleFWI(ctx, 1, sample_temporal=st)
    assert (f.g.isz, f.g.igz) == (144, 121)
    counts = np.bincount(f.igx)
    assert set(counts[counts > 0]) == {1, 2}
    so, c = f.forward(vn, keep_history=True)
    dseis = np.random.default_rng(23 + st).standard_normal(so.shape).astype(np.float32)
    oA, oK, ob = f.adjoint(c, dseis)
    go = f.finalize(c, oA, oK, ob)
    for a in (so, dseis, oA, oK, ob, go):
        a.setflags(write=False)
    return ctx, vn, so, dseis, oA, oK, ob, go


_chunked = {}


def _openfwi_run(cuda, st, mode):
    ctx, vn, so, dseis, oA, oK, ob, go = _openfwi_case(st)
    fwi = make_fwi(ctx, sample_temporal=st)
    v = torch.from_numpy(vn).to(cuda)
    plan = fwi._plan(70, 70, v.device)
    ds = torch.tensor(dseis).to(cuda)
    family = "wide" if mode is False else mode
    _select(plan, family, 4, 1)
    got = _run(plan, v, 1, ds, family)
    _assert_exact(got, so, oA, oK, ob, go, (st, mode))
    if mode is False:
        _chunked[st] = got
    else:
        if st not in _chunked:                   # persistent == chunked, the gk partials included
            _select(plan, "wide", 4, 1)
            _chunked[st] = _run(plan, v, 1, ds, "wide")
        for a, b in zip(got, _chunked[st]):
            if a.dtype == np.float32:
                assert bits_equal(a, b)
            else:
                np.testing.assert_allclose(a, b, rtol=1e-12)
    # the default adjoint of the family (persistent: recurrence / FMA; chunked: exact order)
    _select(plan, family, 4, 1, exact=False)
    g = _run(plan, v, 1, ds, family)[5]
    rel = float(np.linalg.norm(g - go) / np.linalg.norm(go))
    record_margin("geometry_default_adjoint_dLdv_vs_oracle_rel_l2", f"openfwi,st={st},mode={mode}", rel, 5e-6)
    assert rel < 5e-6, rel


@pytest.mark.parametrize("mode", [16, 12, 8, False])
def test_openfwi_grid_split_rows_region_classes(cuda, mode):
    """The three persistent region classes and the wide chunked kernels at depth 4 (halo H = 8) on a
    310 x 310 padded grid with the receiver row (padded 121) and the source row (padded 144) apart.
    A tile of a class covers IH = rows - 2 H padded rows from ty * IH, and wave w holds region rows
    [w R, w R + R), i.e. padded rows ty * IH - H + w R + r (PT_REGION_GEOM: uz0), so row z belongs to
    tile row ty = z / IH, wave (z - ty IH + H) / R:

      class 16 (16 waves x 4 rows, IH 48): row 121 -> tile row 2, wave 8; row 144 -> tile row 3, wave 2
      class 12 (16 waves x 6 rows, IH 80): row 121 -> tile row 1, wave 8; row 144 -> tile row 1, wave 12
      class  8 ( 8 waves x 8 rows, IH 48): row 121 -> tile row 2, wave 4; row 144 -> tile row 3, wave 1

    Different waves record and inject in every class, different workgroups in classes 16 and 8 (with
    sz = 100, row 130 would share row 121's workgroup in all three: waves 10 / 9 / 5).  Row 144 is
    also the first interior row of its tile in classes 16 and 8.  Checks: seismograms bit-equal to the
    oracle's; exact-order gA / gbeta bit-equal, gk rtol 1e-7, dL/dv < 1e-6; persistent == chunked bit for
    bit; the default (recurrence / FMA) adjoint's dL/dv < 5e-6 rel-L2 of the oracle's."""
    _openfwi_run(cuda, 1, mode)


@pytest.mark.parametrize("mode", [12, False])
def test_openfwi_grid_split_rows_sample_temporal(cuda, mode):
    """The same grid at sample_temporal = 3: the residual row index (k - 1) / st times the folded
    stride dstride = ncolr (54 records of 70 columns, not of 100 receivers)."""
    _openfwi_run(cuda, 3, mode)


def _fold(dseis, igx):
    """A column's residuals summed in receiver order, fp32 (k_rcv_fold), columns ascending."""
    out = []
    for x in np.unique(igx):
        r = np.flatnonzero(igx == x)
        acc = dseis[..., r[0]].copy()
        for j in r[1:]:
            acc = acc + dseis[..., j]
        out.append(acc)
    return np.stack(out, -1).astype(np.float32)


@pytest.mark.parametrize("persist", [True, False])
def test_folded_residuals_graph_replay_and_ring_layout(cuda, persist):
    """The fold launch sits in front of the adjoint's cached graph and hands the kernels the fold
    buffer in place of dseis.  Two adjoint calls with graphs on, the same dseis tensor overwritten in
    place between them: the second equals a graphs-off run on the second contents bit for bit (a replay
    must read the new residuals).  The ring is allocated at exactly sizes(B).ring: the fold output
    starts behind the wavefield part (4 B ns Hp ld 8-byte granules), ends at the buffer's end, and
    holds the per-column sums."""
    from red_diffeq import _hip
    z, ctx, vn, _, _, _, _, _ = _small_case("fwd_multi_rcv")
    fwi = make_fwi(ctx)
    v = torch.from_numpy(vn).to(cuda)
    B = v.shape[0]
    plan = fwi._plan(v.shape[2], v.shape[3], v.device)
    _select(plan, "persistent" if persist else "wide", 4, B)
    sz = plan.sizes(B)
    igx = _igx(ctx)
    ncolr = len(np.unique(igx))
    assert ncolr < plan.ng
    wave_bytes = 4 * B * plan.ns * sz.Hp * sz.ld * 8
    fold_bytes = B * plan.ns * sz.nrec * ncolr * 4
    assert wave_bytes + fold_bytes == sz.ring          # the fold ends exactly at the buffer's end
    coeffs, _ = plan.coeffs(v, 0)
    _, hist = plan.forward(coeffs, B, keep_history=True)
    plan.status()
    f32 = lambda n: torch.empty(int(n) // 4, device=cuda)
    ring, gA, gb = f32(sz.ring), f32(sz.gA), f32(sz.gbeta)
    gk = torch.empty(int(sz.gk_part) // 8, dtype=torch.float64, device=cuda)
    rng = np.random.default_rng(41)
    d = [rng.standard_normal(z["seis"].shape).astype(np.float32) for _ in range(2)]
    dseis = torch.empty(z["seis"].shape, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = _hip.ptr

    def run(contents):
        dseis.copy_(torch.from_numpy(contents))
        ring.view(torch.int32).fill_(0x7FC00000)       # NaN: nothing stale can pass for a result
        _hip.check(plan.lib.rdq_fwi_adjoint(plan.handle, B, P(coeffs), P(hist), P(dseis), P(ring), P(gA), P(gk),
                                            P(gb), st), "adj")
        plan.status()
        return [t.cpu().numpy().copy() for t in (gA, gb, gk)], ring[wave_bytes // 4:].cpu().numpy().copy()

    try:
        plan.set_graphs(False)
        want, _ = run(d[1])
        plan.set_graphs(True)
        run(d[0])                                      # capture (chunked) on the first contents
        got, tail = run(d[1])                          # replay on the second
    finally:
        plan.set_graphs(True)
    for name, a, b in zip(("gA", "gbeta"), got, want):
        assert bits_equal(a, b), name
    assert np.array_equal(got[2], want[2])
    assert tail.size * 4 == fold_bytes
    assert bits_equal(tail.reshape(B, plan.ns, sz.nrec, ncolr), _fold(d[1], igx))


def test_batch_independence_shared_columns(cuda):
    """fwd_rcv_list (repeated gx, two shots on one column): model 1 alone equals model 1 in the batch
    bit for bit, seismograms and the exact-order gA."""
    z, ctx, vn, dseis, _, _, _, _ = _small_case("fwd_rcv_list")
    fwi = make_fwi(ctx)
    v = torch.from_numpy(vn).to(cuda)
    plan = fwi._plan(v.shape[2], v.shape[3], v.device)
    ds = torch.tensor(dseis).to(cuda)
    for family in ("persistent", "wide"):
        _select(plan, family, 4, 2)
        both = _run(plan, v, 2, ds, family)
        _select(plan, family, 4, 1)
        one = _run(plan, v[1:2].contiguous(), 1, ds[1:2].contiguous(), family)
        assert bits_equal(one[1][0], both[1][1]) and bits_equal(one[0][0], both[0][1]), family
        assert bits_equal(one[2][0], both[2][1]), family
