"""Checkpointed FWI gradient (rdq_fwi_forward_ckpt / rdq_fwi_adjoint_ckpt; include/red_diffeq_fwi.h):
the wavefield history bounded by recomputation must give the store-all results, bit for bit: the
recomputed levels are the forward's own bits and the chunked adjoint accumulates per launch in fixed k
order.  Against the store-all chunked run on the same plan and the oracle, on the shapes the suite uses
for the chunked kernels (tests/test_gpu_fwi.py: test_wide_chunked_kernels_vs_oracle).

The persistent first pass of the design (a checkpoint-emitting k_fwd_pt) is not built: the first pass
always runs the chunked kernels (ckpt_info's class is 0), so there is no test of it here."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import ctx_of, load_golden, record_margin, vnorm
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NT, B, NS = 162, 2, 3
T, TW = 4, 5                       # forward / narrow adjoint depth; the wide adjoint's depth
SHAPES = [(71, 10), (84, 10), (40, 4)]
KS = [1, 7, 40, 162, 500]


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def make_fwi(ctx, **kw):
    from red_diffeq.solvers.pde import FWIForward
    from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize
    return FWIForward(dict(ctx), "cuda", normalize=True, v_denorm_func=v_denormalize,
                      s_norm_func=s_normalize_none, **kw)


def shot_sum(gA):
    acc = gA[:, 0].copy()                      # shots in order, fp32 (the K4 / oracle order)
    for s in range(1, gA.shape[1]):
        acc = acc + gA[:, s]
    return acc


def configure(plan, wide):
    """_chunked_run's recipe (tests/test_gpu_fwi.py): chunked kernels, one chain, depths T / TW."""
    plan.set_persistent(False)
    plan.set_variant(adj_exact=not wide, wide_chunked=wide)
    plan.set_tuning(T, T, 1)
    plan.set_wide_adj_steps(TW)


def outputs(plan, nb, seis, gA, gk, gb, g):
    sz = plan.sizes(nb)
    return {"seis": seis.cpu().numpy(), "gA": gA.view(nb, plan.ns, sz.Hp, sz.ld)[..., :sz.Wp].cpu().numpy(),
            "gb": gb.view(nb, -1).cpu().numpy(), "gk_raw": gk.cpu().numpy(),
            "gk": gk.view(nb, -1).sum(1).cpu().numpy(), "g": g.cpu().numpy()}


def store_all_run(plan, v, nb, dseis, wide):
    configure(plan, wide)
    assert not plan.launch_info(nb)["adj_persistent"]
    coeffs, vstat = plan.coeffs(v, 0)
    seis, hist = plan.forward(coeffs, nb, keep_history=True)
    gA, gk, gb = plan.adjoint(coeffs, hist, dseis, nb)
    g = plan.finalize(coeffs, vstat, gA, gk, gb, nb, 0)
    plan.status()
    return outputs(plan, nb, seis, gA, gk, gb, g)


def ckpt_run(plan, v, nb, dseis, wide, K):
    configure(plan, wide)
    coeffs, vstat = plan.coeffs(v, 0)
    seis, ckpt = plan.forward_ckpt(coeffs, nb, K)
    assert ckpt.numel() * 4 == plan.ckpt_sizes(nb, K).ckpt
    gA, gk, gb = plan.adjoint_ckpt(coeffs, ckpt, dseis, nb, K)
    g = plan.finalize(coeffs, vstat, gA, gk, gb, nb, 0)
    plan.status()
    return outputs(plan, nb, seis, gA, gk, gb, g)


class Case:
    """One shape: operator, inputs, ONE oracle evaluation, and the store-all chunked runs (made on first
    use, then shared and left unchanged)."""

    def __init__(self, ctx, vn, dev, rng_seed, **kw):
        self.ctx, self.vn, self.kw = dict(ctx), vn, kw
        self.fwi = make_fwi(ctx, **kw)
        self.v = torch.from_numpy(vn).to(dev)
        self.nb = vn.shape[0]
        self.plan = self.fwi._plan(vn.shape[2], vn.shape[3], self.v.device)
        sz = self.plan.sizes(self.nb)
        self.dseis_np = np.random.default_rng(rng_seed).standard_normal(
            (self.nb, self.plan.ns, sz.nrec, self.plan.ng)).astype(np.float32)
        self.dseis = torch.from_numpy(self.dseis_np).to(dev)
        f = O.OracleFWI(dict(ctx), self.nb, **kw)
        so, c = f.forward(vn, keep_history=True)
        oA, oK, ob = f.adjoint(c, self.dseis_np)
        self.oracle = {"seis": so, "gA": oA, "gk": oK, "gb": ob}
        self._store_all = {}

    def store_all(self, wide):
        if wide not in self._store_all:
            self._store_all[wide] = store_all_run(self.plan, self.v, self.nb, self.dseis, wide)
        return self._store_all[wide]


@pytest.fixture(scope="module")
def cases(cuda):
    from red_diffeq.utils.synthetic import make_model
    made = {}

    def get(nx, nbc):
        if (nx, nbc) not in made:
            ctx = dict(n_grid=nx, nt=NT, dx=10.0, dt=0.001, nbc=nbc, f=15.0, sz=10, gz=10, ng=nx, ns=NS)
            vn = vnorm(make_model("curvefault", 40, nx, seed=31, batch=B))
            made[(nx, nbc)] = Case(ctx, vn, cuda, 11)
            assert made[(nx, nbc)].plan.sizes(B).Wp == nx + 2 * nbc
        return made[(nx, nbc)]
    return get


@pytest.fixture(scope="module")
def decimated(cuda):
    z = load_golden("fwd_small_st3")
    return Case(ctx_of(z), vnorm(z["v"]), cuda, 11, sample_temporal=3, sample_spatial=0.5)


def rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)      # (nbc = 4 grows to 1e25: fp64 norms)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def check_against_store_all_and_oracle(case, wide, K, label):
    nt = case.plan.nt
    want = case.store_all(wide)
    got = ckpt_run(case.plan, case.v, case.nb, case.dseis, wide, K)
    sizes = case.plan.ckpt_sizes(case.nb, K)
    Ke = min(K, nt)
    assert (sizes.nseg, sizes.seg_levels) == (-(-nt // Ke), Ke + 2)
    level = case.plan.sizes(case.nb).history // (nt + 2)
    assert (sizes.ckpt, sizes.seg) == (2 * (sizes.nseg - 1) * level, (Ke + 2) * level)
    # against the store-all chunked run on the same plan, same kernels, same finalize
    for name in ("seis", "gA", "gb"):
        assert bits_equal(got[name], want[name]), (label, name)
    krel = float(np.max(np.abs(got["gk"] - want["gk"]) / np.abs(want["gk"])))
    grel = rel_l2(got["g"], want["g"])
    print(f"{label}: gk rel {krel:.3e} (bar 1e-12), g_v rel-L2 {grel:.3e} (bar 1e-6)")
    record_margin("checkpoint_gk_rel_vs_store_all", label, krel, 1e-12)
    record_margin("checkpoint_dLdv_rel_l2_vs_store_all", label, grel, 1e-6)
    np.testing.assert_allclose(got["gk"], want["gk"], rtol=1e-12)
    assert grel < 1e-6
    depth = TW if wide else T
    if K % depth == 0 or K >= nt:        # the adjoint's launches are the store-all run's: every bit
        assert np.array_equal(got["gk_raw"], want["gk_raw"]), label
        assert bits_equal(got["g"], want["g"]), label
    # against the oracle
    o = case.oracle
    assert bits_equal(got["seis"], o["seis"]), label
    assert bits_equal(shot_sum(got["gA"]), o["gA"]), label
    assert bits_equal(got["gb"].reshape(o["gb"].shape), o["gb"]), label
    okrel = float(np.max(np.abs(got["gk"] - o["gk"]) / np.abs(o["gk"])))
    record_margin("checkpoint_gk_rel_vs_oracle", label, okrel, 1e-7)
    np.testing.assert_allclose(got["gk"], o["gk"], rtol=1e-7)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "narrow"])
@pytest.mark.parametrize("nx,nbc", SHAPES)
def test_bitwise_vs_store_all_and_oracle(cases, nx, nbc, wide, K):
    """Odd and even padded width and the thin sponge (its field grows to 1e25: a stale level cannot
    hide); K = 1 (single-step segments), 7 (162 = 23 x 7 + 1: a one-step segment, K a multiple of no
    depth), 40 (a multiple of the depths 4 and 5: the store-all run's launches), nt, and beyond nt."""
    check_against_store_all_and_oracle(cases(nx, nbc), wide, K, f"nx={nx},nbc={nbc},wide={wide},K={K}")


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "narrow"])
def test_decimated_receivers(decimated, wide):
    """sample_temporal = 3, half the receivers: record indices inside a segment stay absolute."""
    check_against_store_all_and_oracle(decimated, wide, 7, f"fwd_small_st3,wide={wide},K=7")


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "narrow"])
def test_graph_replays_on_poisoned_buffers(cases, cuda, wide):
    """Through the raw C ABI, every buffer the calls write filled with NaN before every call: direct
    launches once, then a graph capture and two replays, all bit-equal (each call zeroes what it
    accumulates into; the segment buffer's first two levels come from the checkpoint or from zeros)."""
    from red_diffeq import _hip
    case = cases(71, 10)
    plan, v, K = case.plan, case.v, 7
    configure(plan, wide)
    sz, cs = plan.sizes(B), plan.ckpt_sizes(B, K)
    coeffs, _ = plan.coeffs(v, 0)
    f32 = lambda n: torch.empty(int(n) // 4, device=cuda)
    seis = torch.empty(B, plan.ns, sz.nrec, plan.ng, device=cuda)
    ckpt, seg, ring, gA, gb = f32(cs.ckpt), f32(cs.seg), f32(sz.ring), f32(sz.gA), f32(sz.gbeta)
    gk = torch.empty(int(sz.gk_part) // 8, dtype=torch.float64, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = _hip.ptr

    def run():
        for t in (seis, ckpt, seg, ring, gA, gb, gk):
            t.fill_(float("nan"))
        _hip.check(plan.lib.rdq_fwi_forward_ckpt(plan.handle, B, K, P(coeffs), P(seis), P(ckpt), P(ring), st), "fwd")
        _hip.check(plan.lib.rdq_fwi_adjoint_ckpt(plan.handle, B, K, P(coeffs), P(ckpt), P(seg), P(case.dseis), P(ring),
                                                 P(gA), P(gk), P(gb), st), "adj")
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (seis, gA, gb, gk)]

    try:
        plan.set_graphs(False)
        want = run()
        assert not np.isnan(want[0]).any() and not np.isnan(want[1]).any()
        assert bits_equal(want[0], case.oracle["seis"])
        plan.set_graphs(True)
        for rep in range(3):                  # capture, then two replays of the same graph execs
            got = run()
            for name, a, b in zip(("seis", "gA", "gbeta"), got, want):
                assert bits_equal(a, b), (rep, name)
            assert np.array_equal(got[3], want[3]), rep
    finally:
        plan.set_graphs(True)


def test_recompute_records_nothing(cases, cuda):
    """The backward's recompute must not touch the seismograms (the caller's tensor may be gone)."""
    from red_diffeq import _hip
    case = cases(71, 10)
    plan, v, K = case.plan, case.v, 7
    for wide in (True, False):
        configure(plan, wide)
        sz, cs = plan.sizes(B), plan.ckpt_sizes(B, K)
        coeffs, _ = plan.coeffs(v, 0)
        f32 = lambda n: torch.empty(int(n) // 4, device=cuda)
        seis = torch.empty(B, plan.ns, sz.nrec, plan.ng, device=cuda)
        ckpt, seg, ring, gA, gb = f32(cs.ckpt), f32(cs.seg), f32(sz.ring), f32(sz.gA), f32(sz.gbeta)
        gk = torch.empty(int(sz.gk_part) // 8, dtype=torch.float64, device=cuda)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        P = _hip.ptr
        _hip.check(plan.lib.rdq_fwi_forward_ckpt(plan.handle, B, K, P(coeffs), P(seis), P(ckpt), P(ring), st), "fwd")
        torch.cuda.synchronize()
        assert bits_equal(seis.cpu().numpy(), case.oracle["seis"])
        seis.fill_(float("nan"))
        _hip.check(plan.lib.rdq_fwi_adjoint_ckpt(plan.handle, B, K, P(coeffs), P(ckpt), P(seg), P(case.dseis), P(ring),
                                                 P(gA), P(gk), P(gb), st), "adj")
        torch.cuda.synchronize()
        assert bool(torch.isnan(seis).all()), wide
        assert bits_equal(gA.view(B, plan.ns, sz.Hp, sz.ld)[..., :sz.Wp].cpu().numpy(), case.store_all(wide)["gA"])


def test_autograd_and_memory(cases, cuda):
    """FWIForward(checkpoint=16): v.grad equals a store-all operator's on the same chunked kernels, and the
    step's peak allocation stays below the store-all history ALONE (K = 16 holds about 20 + 18 levels, two
    rings and gA; store-all holds 164 levels: a factor of about three in hand)."""
    case = cases(71, 10)
    w = torch.from_numpy(np.random.default_rng(3).standard_normal(case.oracle["seis"].shape).astype(np.float32)).to(cuda)

    def step(fwi):
        plan = fwi._plan(40, 71, cuda)
        configure(plan, True)
        v = case.v.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        seis = fwi(v)
        (seis * w).sum().backward()
        torch.cuda.synchronize()
        plan.status()
        peak = torch.cuda.max_memory_allocated() - base
        return seis.detach().cpu().numpy(), v.grad.cpu().numpy(), peak, plan

    s_ck, g_ck, peak_ck, plan_ck = step(make_fwi(case.ctx, checkpoint=16))
    s_sa, g_sa, peak_sa, plan_sa = step(make_fwi(case.ctx))
    history = plan_ck.sizes(B).history
    print(f"peak allocated: checkpoint=16 {peak_ck} B, store-all {peak_sa} B, store-all history alone {history} B")
    record_margin("checkpoint_peak_bytes_vs_history", "nx=71,K=16", peak_ck, history)
    assert bits_equal(s_ck, s_sa) and bits_equal(s_ck, case.oracle["seis"])
    assert peak_ck < history < peak_sa
    rel = rel_l2(g_ck, g_sa)
    record_margin("checkpoint_autograd_dLdv_rel_l2", "nx=71,K=16", rel, 1e-6)
    assert rel < 1e-6, rel
    # the gA-driven terms, bit for bit: the operators' accumulators through the plans' own calls
    coeffs, _ = plan_ck.coeffs(case.v, 0)
    _, ckpt = plan_ck.forward_ckpt(coeffs, B, 16)
    gA_ck, _, gb_ck = plan_ck.adjoint_ckpt(coeffs, ckpt, w, B, 16)
    _, hist = plan_sa.forward(coeffs, B, keep_history=True)
    gA_sa, _, gb_sa = plan_sa.adjoint(coeffs, hist, w, B)
    assert bits_equal(gA_ck.cpu().numpy(), gA_sa.cpu().numpy()) and bits_equal(gb_ck.cpu().numpy(), gb_sa.cpu().numpy())
    # budget-driven: store-all while it fits, else the largest K that fits
    gib = 2.0 ** 30
    assert make_fwi(case.ctx, history_budget_gb=history / gib).checkpoint_interval(plan_ck, B) is None
    auto = make_fwi(case.ctx, checkpoint="auto", history_budget_gb=0.5 * history / gib)
    K = auto.checkpoint_interval(plan_ck, B)
    cs = plan_ck.ckpt_sizes(B, K)
    assert K is not None and cs.ckpt + cs.seg <= 0.5 * history
    s_au, g_au, peak_au, _ = step(auto)
    assert bits_equal(s_au, s_sa) and rel_l2(g_au, g_sa) < 1e-6 and peak_au < history


def test_default_path_unchanged(cases, cuda):
    """checkpoint=None: the store-all path, same launches and same bits as an operator built without
    the option; no gradient asked: the no-grad ring forward whatever the option says."""
    case = cases(71, 10)
    plain, none, ck = make_fwi(case.ctx), make_fwi(case.ctx, checkpoint=None), make_fwi(case.ctx, checkpoint=16)
    outs = []
    for fwi in (plain, none):
        plan = fwi._plan(40, 71, cuda)
        info = plan.launch_info(B)
        v = case.v.clone().requires_grad_(True)
        seis = fwi(v)
        seis.backward(case.dseis)
        plan.status()
        outs.append((info, seis.detach().cpu().numpy(), v.grad.cpu().numpy()))
    assert outs[0][0] == outs[1][0]                                       # launch_info: the same kernels
    assert bits_equal(outs[0][1], outs[1][1]) and bits_equal(outs[0][2], outs[1][2])
    assert bits_equal(outs[0][1], case.oracle["seis"])
    with torch.no_grad():
        assert bits_equal(ck(case.v).cpu().numpy(), case.oracle["seis"])
    assert ck._plan(40, 71, cuda).launch_info(B) == outs[0][0]


def test_arguments(cases, cuda):
    from red_diffeq import _hip
    case = cases(71, 10)
    plan = case.plan
    configure(plan, True)
    sz = plan.sizes(B)
    coeffs, _ = plan.coeffs(case.v, 0)
    f32 = lambda n: torch.empty(int(n) // 4, device=cuda)
    seis = torch.empty(B, plan.ns, sz.nrec, plan.ng, device=cuda)
    cs = plan.ckpt_sizes(B, 7)
    ckpt, seg, ring, gA, gb = f32(cs.ckpt), f32(cs.seg), f32(sz.ring), f32(sz.gA), f32(sz.gbeta)
    gk = torch.empty(int(sz.gk_part) // 8, dtype=torch.float64, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = _hip.ptr
    INVALID = -10001
    for K in (0, -1):
        out = _hip.FwiCkptSizes()
        assert plan.lib.rdq_fwi_ckpt_sizes(plan.handle, B, K, ctypes.byref(out)) == INVALID
        assert plan.lib.rdq_fwi_ckpt_info(plan.handle, B, K, (ctypes.c_int32 * 4)()) == INVALID
        assert plan.lib.rdq_fwi_forward_ckpt(plan.handle, B, K, P(coeffs), P(seis), P(ckpt), P(ring), st) == INVALID
        assert plan.lib.rdq_fwi_adjoint_ckpt(plan.handle, B, K, P(coeffs), P(ckpt), P(seg), P(case.dseis), P(ring),
                                             P(gA), P(gk), P(gb), st) == INVALID
        with pytest.raises(RuntimeError):
            plan.forward_ckpt(coeffs, B, K)
    # several segments need a checkpoint store
    assert plan.lib.rdq_fwi_forward_ckpt(plan.handle, B, 7, P(coeffs), P(seis), None, P(ring), st) == INVALID
    # a seg or ckpt tensor of the wrong size raises in the op
    _, good = plan.forward_ckpt(coeffs, B, 7)
    op = torch.ops.red_diffeq.fwi_adjoint_ckpt
    with pytest.raises((ValueError, RuntimeError)):
        op(coeffs, good, seg[:-1], case.dseis, plan.op_id, B, 7)
    with pytest.raises((ValueError, RuntimeError)):
        op(coeffs, good[:-1], seg, case.dseis, plan.op_id, B, 7)
    with pytest.raises((ValueError, RuntimeError)):
        op(coeffs, good, f32(plan.ckpt_sizes(B, 8).seg), case.dseis, plan.op_id, B, 7)
    torch.cuda.synchronize()
    info = plan.ckpt_info(B, 7)
    assert info["fwd_class"] == 0 and info["nseg"] == 24
    assert info["fwd_launches"] == 23 * 2 + 1 and info["bwd_launches"] == (23 * 2 + 1) * 2     # ceil(7 / 4) = ceil(7 / 5) = 2
    assert plan.ckpt_info(B, 500) == {"fwd_class": 0, "nseg": 1, "fwd_launches": 41, "bwd_launches": 41 + 33}
