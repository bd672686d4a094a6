"""Caller-supplied source wavelets on the HIP path: FWIForward(..., wavelet=) (the plan's wavelet, every kernel
family) and forward(v, wavelet=) (per model and per shot, differentiable, the narrow chunked kernels' SRC
instantiations), against tests/golden/wavelet.npz (the reference run with an injected wavelet tensor, fp32 and fp64,
tests/golden/make_wavelet.py) and against the CPU oracle driven with the same wavelets (tests/wavelet_cases.py,
pinned without a GPU by tests/test_wavelet_host.py).

Bars.  The forward is the reference's fp32 operation order: bitwise.  The wavelet gradient is one multiply per
element on an adjoint field computed in a different but valid fp32 order than the reference's autograd, so its
yardstick is the reference's own fp32 error against fp64, eref_w[b] per model, with the factor 4 that
tests/test_gpu_born.py and tests/test_gpu_sampling.py use; against the oracle, whose adjoint field it shares, it is
bitwise.  dL/dv keeps the project's 5e-5 (tests/test_gpu_fwi.py).  Everything that is a property of the schedule or
of linearity is bitwise, except dL/dv across settings that change the adjoint's launches (another depth, a
checkpoint interval that is no multiple of it): there the sponge partials gk_part are summed in another fp64
order, and the rule of tests/test_gpu_checkpoint.py applies (rel-L2 < 1e-6, bitwise where the launches are the
same)."""
import numpy as np
import pytest
import torch

from conftest import record_margin
from wavelet_cases import CASES, Fixture, WaveletOracle, bits_equal

pytestmark = pytest.mark.gpu

GRAD_BAR = 5e-5          # dL/dv against the reference's autograd, rel-L2 (tests/test_gpu_fwi.py)
GK_ORDER_BAR = 1e-6      # dL/dv between two fp64 summation orders of gk_part (tests/test_gpu_checkpoint.py)


class Case(Fixture):
    def __init__(self, tag, cuda):
        super().__init__(tag)
        self.tv, self.tW, self.tr = (torch.from_numpy(a).to(cuda) for a in (self.v, self.W, self.r))
        self.tdW = torch.from_numpy(self.dW).to(cuda)
        self._ref = None

    def gradients(self, fwi, W=None, want_w=True, want_v=True, r=None):
        """(seis, w.grad, v.grad) of <fwi(v, wavelet=W), r>, as numpy (None where not asked for)."""
        v = self.tv.clone().requires_grad_(want_v)
        w = (self.tW if W is None else W).clone().requires_grad_(want_w)
        seis = fwi(v, wavelet=w)
        (seis * (self.tr if r is None else r)).sum().backward()
        return (seis.detach().cpu().numpy(), w.grad.cpu().numpy() if want_w else None,
                v.grad.cpu().numpy() if want_v else None)

    def reference(self):
        """The per-call path on a fresh operator's defaults, computed once and shared."""
        if self._ref is None:
            fwi = self.fwi()
            self._ref = self.gradients(fwi)
            fwi.check()
        return self._ref


@pytest.fixture(scope="module")
def cases(cuda):
    return {tag: Case(tag, cuda) for tag in CASES}


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def per_model(a):
    return np.sqrt((np.asarray(a, np.float64) ** 2).reshape(a.shape[0], -1).sum(1))


# ------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("tag", CASES)
def test_forward_is_the_references_bits(cuda, cases, tag):
    c = cases[tag]
    fwi = c.fwi()
    assert bits_equal(c.reference()[0], c.seis32)                       # the call that keeps its history
    with torch.no_grad():
        seis = fwi(c.tv, wavelet=c.tW)
        assert seis.dtype == torch.float32 and not seis.requires_grad
        assert bits_equal(seis.cpu().numpy(), c.seis32)
        # (ns, nt): model 0's wavelets for every model; (nt,): one wavelet for every shot and model
        per_shot = fwi(c.tv, wavelet=c.tW[0])
        assert bits_equal(per_shot[0].cpu().numpy(), c.seis32[0])
        assert torch.equal(per_shot, fwi(c.tv, wavelet=c.tW[:1].expand(c.B, -1, -1).contiguous()))
        for s in range(c.ns):
            shared = fwi(c.tv, wavelet=c.tW[0, s])
            assert torch.equal(shared[:, s], per_shot[:, s]), (tag, s)
        assert torch.equal(fwi(c.tv, wavelet=c.tW.double()), seis)      # non-fp32 input: .float()
        if tag == "short":      # no constructor wavelet and no Ricker that fits: only per-call wavelets are served
            with pytest.raises(ValueError):
                fwi(c.tv)
            with pytest.raises(ValueError):
                c.fwi()(c.tv)
    fwi.check()


# ------------------------------------------------------------------------------ 2. constructor wavelet
@pytest.mark.parametrize("tag", CASES)
def test_constructor_wavelet_in_every_kernel_family(cuda, cases, tag):
    """FWIForward(..., wavelet=W[0, s]) models shot s of model 0 with the reference's bits on the persistent
    kernels of every region class that fits, and on both chunked widths.  `short` (nt = 10) has no Ricker."""
    c = cases[tag]
    v0 = c.tv[:1].contiguous()
    ran = set()
    for s in range(c.ns):
        fwi = c.fwi(wavelet=c.W[0, s] if s else torch.from_numpy(c.W[0, s]))      # array-like and tensor
        plan = fwi._plan(v0.shape[2], v0.shape[3], v0.device)
        for mode, wide in ((1, True), (16, True), (12, True), (8, True), (0, True), (0, False)):
            plan.set_persistent(mode)
            plan.set_variant(wide_chunked=wide)
            info = plan.launch_info(1)
            with torch.no_grad():
                seis = fwi(v0)
            fwi.check()
            ran.add((info["fwd_class"], wide))
            assert bits_equal(seis[0, s].cpu().numpy(), c.seis32[0, s]), (tag, s, mode, wide, info)
    print(f"constructor wavelet {tag}: (persistent class, wide) run: {sorted(ran)}")
    assert {(0, True), (0, False)} <= ran and any(k for k, _ in ran)


def test_constructor_wavelet_serves_born(cuda, cases):
    """born / gauss_newton read the plan's wavelet.  With the Ricker array handed in explicitly, born is the
    Born fixture's J dv (tests/golden/born.npz, same model) within the Born tests' own bar, 4 E_ref per model, and
    bitwise the default operator's.  With a fixture
    wavelet, the forward born returns is the per-call forward's bits, the fused pass agrees with the history pass
    bit for bit, and gauss_newton is the three lines it stands for on the same operator."""
    from conftest import load_golden
    from red_diffeq.solvers.pde import ricker
    c = cases["tiles"]
    z = load_golden("born")
    assert np.array_equal(z["tiles_v"], c.v)
    dv = torch.from_numpy(z["tiles_dv"]).to(cuda)
    jdv64, eref = z["tiles_jdv64"], z["tiles_eref"]
    rk = ricker(c.ctx["f"], c.ctx["dt"], c.nt)
    ds_default = c.fwi().born(c.tv, dv)
    ds = c.fwi(wavelet=rk).born(c.tv, dv)
    assert torch.equal(ds, ds_default)
    for b in range(c.B):
        e = rel_l2(ds[b].cpu().numpy(), jdv64[b])
        record_margin("wavelet_constructor_born_vs_fp64_over_4Eref", f"tiles[{b}]", e, 4 * eref[b])
        assert e <= 4 * eref[b], (b, e, eref[b])
    w = c.W[0, 0]
    a = c.fwi(wavelet=w)
    seis, ds = a.born(c.tv, dv, return_seis=True)
    with torch.no_grad():
        assert torch.equal(seis, a(c.tv, wavelet=torch.from_numpy(w).to(cuda)))
    assert torch.equal(ds, a.born(c.tv, dv, history=False)) and not torch.equal(ds, ds_default)
    vv = c.tv.clone().requires_grad_(True)
    a(vv).backward(ds)
    assert torch.equal(a.gauss_newton(c.tv, dv), vv.grad)
    a.check()


# ------------------------------------------------------------------------------- 3. default equivalence
@pytest.mark.parametrize("tag", ["wrap", "tiles", "geom"])
def test_ricker_per_call_equals_the_default_call(cuda, cases, tag):
    from red_diffeq.solvers.pde import ricker
    c = cases[tag]
    rk = torch.from_numpy(ricker(c.ctx["f"], c.ctx["dt"], c.nt).astype(np.float32)).to(cuda)
    fwi = c.fwi()
    with torch.no_grad():
        assert torch.equal(fwi(c.tv, wavelet=rk), fwi(c.tv))            # whatever kernels the default runs
    plan = fwi._plan(c.tv.shape[2], c.tv.shape[3], c.tv.device)
    plan.set_persistent(0)
    plan.set_variant(wide_chunked=False)
    v1, v2 = c.tv.clone().requires_grad_(True), c.tv.clone().requires_grad_(True)
    s1 = fwi(v1)
    (s1 * c.tr).sum().backward()
    s2 = fwi(v2, wavelet=rk)
    (s2 * c.tr).sum().backward()
    fwi.check()
    assert torch.equal(s1, s2) and torch.equal(v1.grad, v2.grad)


# ------------------------------------------------------------------------- 4. gradients against fp64
@pytest.mark.parametrize("tag", CASES)
def test_wavelet_gradient_against_the_references_fp64(cuda, cases, tag):
    c = cases[tag]
    _, gw, gv = c.reference()
    assert gw.shape == c.gw64.shape and gw.dtype == np.float32
    for b in range(c.B):
        e = rel_l2(gw[b], c.gw64[b])
        print(f"w.grad vs fp64 {tag}[{b}]: rel-L2 {e:.3e}, E_ref {c.eref_w[b]:.3e}, ratio to the bar "
              f"{e / (4 * c.eref_w[b]):.3f}")
        record_margin("wavelet_grad_vs_fp64_over_4Eref", f"{tag}[{b}]", e, 4 * c.eref_w[b])
    ev = rel_l2(gv, c.gv64)
    print(f"v.grad vs fp64 {tag}: rel-L2 {ev:.3e}")
    record_margin("wavelet_dLdv_vs_fp64", tag, ev, GRAD_BAR)
    for b in range(c.B):
        assert rel_l2(gw[b], c.gw64[b]) <= 4 * c.eref_w[b], (tag, b)
    assert ev <= GRAD_BAR, ev


@pytest.mark.parametrize("tag", ["tiles", "wrap"])
def test_broadcast_wavelets_receive_the_sum(cuda, cases, tag):
    """A (ns, nt) wavelet receives the sum over models, a (nt,) wavelet the sum over models and shots, of the
    gradient the same samples get as a full (B, ns, nt) tensor: against fp64 with the same bar (the sums of the
    per-model bars), and against torch.sum of the kernel's own rows."""
    c = cases[tag]
    fwi = c.fwi()
    # (ns, nt): model 0's wavelets for every model.  fp64 yardstick: the seismograms are linear in w and gw64[b]
    # does not depend on w, so the fixture's gw64 is the gradient at ANY wavelet: sum it over the shared axes.
    w2 = c.tW[0]
    _, g2, _ = c.gradients(fwi, W=w2, want_v=False)
    _, gfull, _ = c.gradients(fwi, W=w2.expand(c.B, -1, -1).contiguous(), want_v=False)
    assert g2.shape == (c.ns, c.nt)
    assert bits_equal(g2, torch.from_numpy(gfull).to(cuda).sum(0).cpu().numpy())
    want2 = c.gw64.sum(0)
    bar2 = float((4 * c.eref_w * per_model(c.gw64)).sum())
    e2 = float(np.linalg.norm(g2.astype(np.float64) - want2))
    record_margin("wavelet_grad_shared_models_over_bound", tag, e2, bar2)
    assert e2 <= bar2, (e2, bar2)
    w1 = c.tW[0, 0]
    _, g1, _ = c.gradients(fwi, W=w1, want_v=False)
    _, gfull, _ = c.gradients(fwi, W=w1.expand(c.B, c.ns, -1).contiguous(), want_v=False)
    assert g1.shape == (c.nt,)
    assert bits_equal(g1, torch.from_numpy(gfull).to(cuda).sum((0, 1)).cpu().numpy())
    e1 = float(np.linalg.norm(g1.astype(np.float64) - c.gw64.sum((0, 1))))
    record_margin("wavelet_grad_shared_all_over_bound", tag, e1, bar2)
    assert e1 <= bar2, (e1, bar2)
    fwi.check()


# --------------------------------------------------------------------- 5. gradient against the oracle
@pytest.mark.parametrize("tag", ["wrap", "tiles"])
def test_wavelet_gradient_is_the_oracles_adjoint_field_times_beta(cuda, cases, tag):
    """The oracle's adjoint with a unit impulse at j as its wavelet leaves gbeta[b, s] = L_{j+1}(src) exactly;
    w.grad[b, s, j] must be fp32(L_{j+1}(src) * beta[b, isz, isx[s]]), bit for bit."""
    c = cases[tag]
    gw = c.reference()[1]
    o = WaveletOracle(c, c.v)
    beta = o.source_beta()
    assert beta.shape == (c.B, c.ns) and (beta > 0).all()
    for j in (0, 1, c.nt // 2, c.nt - 2, c.nt - 1):
        L = o.source_adjoint_field(c.r, j)
        want = (L.astype(np.float32) * beta.astype(np.float32)).astype(np.float32)
        assert np.abs(want).max() > 0
        assert bits_equal(gw[:, :, j], want), (tag, j, gw[:, :, j], want)


# ------------------------------------------------------------------------- 6. schedule independence
@pytest.mark.parametrize("graphs", [True, False])
def test_schedule_independence_bitwise(cuda, cases, graphs):
    """Depths 1..4 (nt = 160 leaves a one-step tail at depth 3), 1 and 3 launch chains, graphs on / off, both
    coefficient sources, any persistent / wide setting of the plan: one seis and one w.grad, bit for bit; one
    v.grad, bit for bit where the adjoint's depth is the reference run's and within the gk_part rule elsewhere.
    Three chains run as direct launches only: a captured graph with parallel branches is the open host fault of
    DESIGN's Born section, which later tests stay clear of, and the chains' launches are the same either way."""
    c = cases["tiles"]
    seis0, gw0, gv0 = c.reference()                                     # defaults: depth 4, one chain
    fwi = c.fwi()
    plan = fwi._plan(c.tv.shape[2], c.tv.shape[3], c.tv.device)
    plan.set_graphs(graphs)
    for depth in (1, 2, 3, 4):
        for chains in ((1,) if graphs else (1, 3)):
            plan.set_tuning(depth, depth, chains)
            plan.set_variant(fwd_gen_coeffs=(depth + chains) % 2 == 0)
            seis, gw, gv = c.gradients(fwi)
            assert bits_equal(seis, seis0) and bits_equal(gw, gw0), (depth, chains, graphs)
            if depth == 4:
                assert bits_equal(gv, gv0), (chains, graphs)
            else:
                e = rel_l2(gv, gv0)
                record_margin("wavelet_dLdv_across_depths", f"depth={depth},chains={chains}", e, GK_ORDER_BAR)
                assert e < GK_ORDER_BAR, (depth, chains, e)
    plan.set_tuning(4, 4, 1)
    for mode, wide, adj_exact in ((1, True, False), (12, True, True), (0, True, False), (0, False, False)):
        plan.set_persistent(mode)
        plan.set_variant(wide_chunked=wide, adj_exact=adj_exact)
        seis, gw, gv = c.gradients(fwi)
        assert bits_equal(seis, seis0) and bits_equal(gw, gw0) and bits_equal(gv, gv0), (mode, wide, graphs)
    fwi.check()


@pytest.mark.parametrize("K", [1, 7, 40, 160, 320])
def test_checkpointed_gradient(cuda, cases, K):
    """checkpoint=K for K in {1, 7, 40, nt, 2 nt}: seis and w.grad bitwise, v.grad by the gk_part rule (bitwise
    when K is a multiple of the adjoint's depth 4, or one segment)."""
    c = cases["tiles"]
    assert c.nt == 160
    seis0, gw0, gv0 = c.reference()
    fwi = c.fwi(checkpoint=K)
    seis, gw, gv = c.gradients(fwi)
    fwi.check()
    assert bits_equal(seis, seis0) and bits_equal(gw, gw0), K
    e = rel_l2(gv, gv0)
    record_margin("wavelet_checkpoint_dLdv_vs_store_all", f"K={K}", e, GK_ORDER_BAR)
    assert e < GK_ORDER_BAR, (K, e)
    if K % 4 == 0 or K >= c.nt:
        assert bits_equal(gv, gv0), K
    with torch.no_grad():                                               # no gradient: the ring forward, no store
        assert bits_equal(fwi(c.tv, wavelet=c.tW).cpu().numpy(), seis0)


def test_checkpointed_short_record(cuda, cases):
    c = cases["short"]
    seis0, gw0, gv0 = c.reference()
    for K in (3, 4):
        seis, gw, gv = c.gradients(c.fwi(checkpoint=K))
        assert bits_equal(seis, seis0) and bits_equal(gw, gw0) and rel_l2(gv, gv0) < GK_ORDER_BAR, K


# ------------------------------------------------------------------------------------- 7. linearity
@pytest.mark.parametrize("tag", CASES)
def test_linearity_bitwise(cuda, cases, tag):
    """fwi(v, 2^j W) == 2^j fwi(v, W) bit for bit, j = +-3, and a zero wavelet gives zeros.

    Where.  A power of two scales a linear fp32 recurrence exactly unless a value leaves the normal range, and this
    forward is the reference's recurrence, bit for bit, at whatever scale the wavelet has.  So it is exactly
    homogeneous exactly where the reference's own fp32 arithmetic is, and which cases those are is read from the
    fixture, which the reference wrote on the CPU (`<tag>_homogeneous`, tests/golden/make_wavelet.py), not from this
    code: wrap, geom and short.  On tiles the reference is not (its numerical precursor crosses the 88 x 118 grid
    through the subnormal range, where products are rounded on an absolute grid; the CPU oracle shows the same and
    where it starts, tests/test_wavelet_host.py::test_scaling_is_exact_only_outside_the_subnormal_range), and there
    the statement that can hold is the stricter one it is replaced by: fwi(v, 2^j W) is the reference's fp32 record
    for 2^j W, bit for bit (`tiles_seis32_scaled_*`), the samples where that differs from 2^j seis32 included
    (measured on an MI355X before this was understood: 1204 of 23040 samples at j = 3, the largest 2.4e-21 under a
    peak of 41.6)."""
    c = cases[tag]
    fwi = c.fwi()
    with torch.no_grad():
        seis = fwi(c.tv, wavelet=c.tW)
        assert bits_equal(seis.cpu().numpy(), c.seis32)
        for j, homogeneous, ref_scaled in c.scales:
            out = fwi(c.tv, wavelet=c.tW * 2.0 ** j)
            if homogeneous:
                assert torch.equal(out, seis * 2.0 ** j), (tag, j)
            else:
                assert bits_equal(out.cpu().numpy(), ref_scaled), (tag, j)
                assert not torch.equal(out, seis * 2.0 ** j)            # (the fixture's flag is about this record)
        assert torch.count_nonzero(fwi(c.tv, wavelet=torch.zeros_like(c.tW))) == 0
    assert tag == "tiles" or all(h for _, h, _ in c.scales)               # three of the four cases are exact
    fwi.check()


@pytest.mark.parametrize("tag", CASES)
def test_adjoint_identity(cuda, cases, tag):
    """<fwi(v, dW), r> = <dW, w.grad>, J_w dW being fwi(v, wavelet=dW) under no_grad.  Bound, as identity_bound
    in tests/test_gpu_born.py: the left side is the reference's fp32 forward bit for bit (bar 1), so it may sit
    E_fwd |F dW| |r| from the fp64 value, E_fwd the reference's own fp32 forward error on this case (seis32 against
    seis64, per model; the forward is linear in the wavelet, so the relative error carries over), with the factor
    4; the right side is within 4 eref_w |dW| |gw64| (bar 4)."""
    c = cases[tag]
    fwi = c.fwi()
    with torch.no_grad():
        jdw = fwi(c.tv, wavelet=c.tdW).cpu().numpy()
    gw = c.reference()[1]
    lhs = float((jdw.astype(np.float64) * c.r).sum())
    rhs = float((c.dW.astype(np.float64) * gw).sum())
    efwd = per_model(c.seis32.astype(np.float64) - c.seis64) / per_model(c.seis64)
    bound = float((4 * efwd * per_model(jdw) * per_model(c.r) + 4 * c.eref_w * per_model(c.dW) * per_model(c.gw64)).sum())
    print(f"adjoint identity {tag}: lhs {lhs:.9e} rhs {rhs:.9e} fp64 {c.ip[0]:.9e} bound {bound:.3e}")
    record_margin("wavelet_adjoint_identity_over_bound", tag, abs(lhs - rhs), bound)
    record_margin("wavelet_lhs_vs_fp64_over_bound", tag, abs(lhs - c.ip[0]), bound)
    record_margin("wavelet_rhs_vs_fp64_over_bound", tag, abs(rhs - c.ip[0]), bound)
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    assert abs(lhs - c.ip[0]) <= bound and abs(rhs - c.ip[0]) <= bound, (lhs, rhs, c.ip, bound)
    fwi.check()


# -------------------------------------------------------------------------------------- 8. plumbing
def test_ops_opcheck(cuda, cases):
    from torch.library import opcheck
    c = cases["wrap"]
    fwi = c.fwi()
    plan = fwi._plan(c.tv.shape[2], c.tv.shape[3], c.tv.device)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    ops = torch.ops.red_diffeq
    v, w = c.tv.clone().requires_grad_(True), c.tW.clone().requires_grad_(True)
    opcheck(ops.fwi_src, (v, w, plan.op_id, 1, True), test_utils=utils)
    opcheck(ops.fwi_src, (c.tv, c.tW[0].expand(c.B, -1, -1), plan.op_id, 1, False), test_utils=utils)
    opcheck(ops.fwi_ckpt_src, (v, w, plan.op_id, 1, 7), test_utils=utils)
    coeffs, _ = ops.fwi_coeffs(c.tv, plan.op_id, 1)
    opcheck(ops.fwi_forward_src, (coeffs, c.tW, plan.op_id, c.B, True), test_utils=utils)
    seis, hist = ops.fwi_forward_src(coeffs, c.tW, plan.op_id, c.B, True)
    assert bits_equal(seis.cpu().numpy(), c.seis32)
    for want in (True, False):
        opcheck(ops.fwi_adjoint_src, (coeffs, c.tW, hist, c.tr, plan.op_id, c.B, want), test_utils=utils)
    opcheck(ops.fwi_forward_ckpt_src, (coeffs, c.tW, plan.op_id, c.B, 7), test_utils=utils)
    _, ckpt = ops.fwi_forward_ckpt_src(coeffs, c.tW, plan.op_id, c.B, 7)
    seg = torch.empty(int(plan.ckpt_sizes(c.B, 7).seg) // 4, device=cuda)
    opcheck(ops.fwi_adjoint_ckpt_src, (coeffs, c.tW, ckpt, seg, c.tr, plan.op_id, c.B, 7, True), test_utils=utils)
    with pytest.raises(ValueError, match="expected fp32 of shape"):
        ops.fwi_forward_src(coeffs, c.tW[:, :1], plan.op_id, c.B, False)
    fwi.check()


def test_shot_sharding(cuda, cases):
    """shots=(1, 3) on tiles: this rank's shots of the full call, bit for bit, from the survey-wide wavelet tensor;
    the other shots' gradient rows are zero."""
    c = cases["tiles"]
    seis0, gw0, _ = c.reference()
    part = c.fwi(shots=(1, 3))
    seis, gw, _ = c.gradients(part, r=c.tr[:, 1:3].contiguous())
    part.check()
    assert bits_equal(seis, seis0[:, 1:3])
    assert gw.shape == gw0.shape and not gw[:, 0].any() and bits_equal(gw[:, 1:3], gw0[:, 1:3])
    _, g2, _ = c.gradients(part, W=c.tW[0], want_v=False, r=c.tr[:, 1:3].contiguous())
    assert g2.shape == (c.ns, c.nt) and not g2[0].any() and g2[1:].any()


@pytest.mark.parametrize("ckpt", [None, 40])
def test_no_wavelet_gradient_requests_no_gwav(cuda, cases, ckpt, monkeypatch):
    """w.requires_grad = False: the adjoint op is called with want_gw = False, gives the kernel no gwav and
    allocates none (its gw output is empty); v.grad is the same bits either way."""
    from red_diffeq import ops as O
    c = cases["tiles"]
    name = "fwi_adjoint_src" if ckpt is None else "fwi_adjoint_ckpt_src"
    real = getattr(O, name)
    seen = []

    def spy(*args):
        out = real(*args)
        seen.append((bool(args[-1]), tuple(out[3].shape)))
        return out
    monkeypatch.setattr(O, name, spy)
    fwi = c.fwi(checkpoint=ckpt)
    _, _, gv_only = c.gradients(fwi, want_w=False)
    _, gw, gv = c.gradients(fwi)
    _, gw_only, none = c.gradients(fwi, want_v=False)
    fwi.check()
    assert seen == [(False, (0,)), (True, c.W.shape), (True, c.W.shape)], seen
    assert bits_equal(gv_only, gv) and bits_equal(gw_only, gw) and none is None


def test_fresh_wavelet_tensors_are_read_afresh(cuda, cases):
    """A second call with another wavelet tensor, and a second call with the SAME tensor changed in place, give
    that wavelet's result: no stale cached graph, no stale copy."""
    c = cases["tiles"]
    fwi = c.fwi()
    with torch.no_grad():
        a = fwi(c.tv, wavelet=c.tW)
        other = (c.tW.flip(1) * 0.5).contiguous()
        b = fwi(c.tv, wavelet=other)
        assert bits_equal(a.cpu().numpy(), c.seis32) and not torch.equal(a, b)
        buf = c.tW.clone()
        assert torch.equal(fwi(c.tv, wavelet=buf), a)
        buf.copy_(other)
        assert torch.equal(fwi(c.tv, wavelet=buf), b)                     # same pointer, new contents
        assert torch.equal(fwi(c.tv, wavelet=c.tW), a)
    fwi.check()
