"""The fused forward + Born pass (k_fwd_born_tb, rdq_fwi_born_fused; born / gauss_newton with history=False) on the
HIP path, on the cases of tests/golden/born.npz.

The fused kernel computes the two P levels the tangent reads instead of loading them from a stored history, in the
chunked forward's own operation order, so everything here is bitwise against the existing paths: the record and the
linearised record against born(history=True), the checkpoint store against forward_ckpt's, the Gauss-Newton
product against the checkpointed autograd path.  The only tolerances are the existing ones (4 E_ref against the
reference's fp64 jvp; the gradient bar between the two adjoints) and the memory conditions of the budget test.

Graph capture.  A Born call that captures a new graph with more than one launch chain has ended in a host
segmentation fault once (Born section; cause unknown).  Every depth x chain loop here runs with graph
capture off, and graphs are captured with one chain only."""
import copy

import pytest
import torch

from conftest import record_margin
from test_gpu_born import CASES, GRAD_BAR, Case, rel_l2

pytestmark = pytest.mark.gpu

KS = (None, 7, 40, 160, 1000)     # nt = 160: no store; a 6-step first segment and tails at every depth; 4 segments;
                                  # K = nt and K > nt (one segment, nothing stored)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """torch.equal on the bit patterns: a NaN equals itself, +0 differs from -0."""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def plan_of(fwi, c):
    return fwi._plan(c.v.shape[2], c.v.shape[3], c.v.device)


def vel_mode_of(c):
    return 0 if c.normalize else 1


@pytest.fixture(scope="module")
def cases(cuda):
    return {tag: Case(tag, cuda) for tag in CASES}


@pytest.fixture(scope="module")
def stored(cuda, cases):
    """(forward(v), J dv) of every case on the store-all history: today's path, the reference of this file."""
    out = {}
    for tag, c in cases.items():
        fwi = c.fwi()
        out[tag] = fwi.born(c.v, c.dv, return_seis=True)
        fwi.check()
    return out


# ------------------------------------------------------------------------------------------ 1. against today's path
@pytest.mark.parametrize("tag", CASES)
def test_fused_born_equals_the_stored_history_path_bitwise(cuda, cases, stored, tag):
    c = cases[tag]
    fwi = c.fwi()
    seis, ds = fwi.born(c.v, c.dv, return_seis=True, history=False)
    fwi.check()
    assert not ds.requires_grad and ds.dtype == torch.float32
    assert torch.equal(seis, stored[tag][0]) and same_bits(seis, stored[tag][0])
    assert torch.equal(ds, stored[tag][1]) and same_bits(ds, stored[tag][1])
    assert same_bits(fwi.born(c.v, c.dv, history=False), ds)             # and without return_seis
    err = rel_l2(ds, c.jdv64)
    for b, (e, eref) in enumerate(zip(err, c.eref)):
        print(f"fused born vs fp64 {tag}[{b}]: rel-L2 {e:.3e}, E_ref {eref:.3e}, ratio to the bar {e / (4 * eref):.3f}")
        record_margin("born_fused_vs_fp64_over_4Eref", f"{tag}[{b}]", e, 4 * eref)
    assert (err <= 4 * c.eref).all(), (err, c.eref)


# ------------------------------------------------------------------------------------------ 2. schedule and segments
def test_schedule_and_segment_independence_bitwise(cuda, cases):
    """Depths 1..4 x 1 and 3 launch chains x both coefficient sources x K in {none, 7, 40, 160, 1000}, through the
    plan binding, direct launches: one record and one linearised record, those of forward + born on the stored
    history.  K = 7 leaves a 6-step first segment (160 = 22 x 7 + 6) and launch tails at every depth."""
    c = cases["tiles"]
    fwi = c.fwi()
    plan = plan_of(fwi, c)
    plan.set_graphs(False)
    B, vm = c.v.shape[0], vel_mode_of(c)
    coeffs, vstat = plan.coeffs(c.v, vm)
    seis_ref, hist = plan.forward(coeffs, B, True)
    ds_ref = plan.born(coeffs, vstat, hist, c.dv, B, vm)
    del hist
    assert float(ds_ref.abs().max()) > 0
    for depth in (1, 2, 3, 4):
        for chains in (1, 3):
            plan.set_tuning(depth, depth, chains)
            for gen in (True, False):
                plan.set_variant(fwd_gen_coeffs=gen)
                for K in KS:
                    seis, ds, ckpt = plan.born_fused(coeffs, vstat, c.dv, B, vm, K)
                    assert same_bits(seis, seis_ref) and same_bits(ds, ds_ref), (depth, chains, gen, K)
                    want = 0 if K is None else int(plan.ckpt_sizes(B, K).ckpt) // 4
                    assert ckpt.numel() == want, (K, ckpt.numel(), want)
    fwi.check()


def test_graph_replays_bitwise(cuda, cases, stored):
    """Cached graphs (kind 6), one launch chain, depth 4, without and with a checkpoint store: the capture and two
    replays, each into fresh outputs."""
    c = cases["tiles"]
    fwi = c.fwi()
    plan = plan_of(fwi, c)
    plan.set_graphs(True)
    plan.set_tuning(4, 4, 1)
    B, vm = c.v.shape[0], vel_mode_of(c)
    coeffs, vstat = plan.coeffs(c.v, vm)
    for K in (None, 7):
        for call in range(3):
            seis, ds, _ = plan.born_fused(coeffs, vstat, c.dv, B, vm, K)
            assert same_bits(seis, stored["tiles"][0]) and same_bits(ds, stored["tiles"][1]), (K, call)
    fwi.check()


def test_op_opcheck(cuda, cases):
    """torch.ops.red_diffeq.fwi_born_fused: schema, autograd registration, and the fake implementation's shapes
    against the real outputs, without and with a checkpoint store (the utilities tests/test_gpu_ops.py uses for
    the FWI operators)."""
    from torch.library import opcheck
    c = cases["tiles"]
    fwi = c.fwi()
    plan = plan_of(fwi, c)
    B, vm = c.v.shape[0], vel_mode_of(c)
    coeffs, vstat = plan.coeffs(c.v, vm)
    for K in (0, 40):
        opcheck(torch.ops.red_diffeq.fwi_born_fused, (coeffs, vstat, c.dv, plan.op_id, B, vm, K),
                test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    with pytest.raises(ValueError, match="K must be"):
        plan.born_fused(coeffs, vstat, c.dv, B, vm, 0)
    fwi.check()


# ------------------------------------------------------------------------------------------ 3. the checkpoint store
@pytest.mark.parametrize("K", [7, 40])
def test_checkpoint_store_equals_forward_ckpt_bitwise(cuda, cases, K):
    """Every cell of the padded grid in every stored level (the row padding past Wp is written by neither)."""
    c = cases["tiles"]
    fwi = c.fwi()
    plan = plan_of(fwi, c)
    B, vm = c.v.shape[0], vel_mode_of(c)
    sz, cs = plan.sizes(B), plan.ckpt_sizes(B, K)
    coeffs, vstat = plan.coeffs(c.v, vm)
    seis_ref, ref = plan.forward_ckpt(coeffs, B, K)
    seis, _, ckpt = plan.born_fused(coeffs, vstat, c.dv, B, vm, K)
    fwi.check()
    shape = (2 * (cs.nseg - 1), B, c.ctx["ns"], sz.Hp, sz.ld)
    assert cs.nseg == -(-c.ctx["nt"] // K) and cs.nseg > 1 and ckpt.numel() == ref.numel()
    got, want = ckpt.view(shape)[..., :sz.Wp], ref.view(shape)[..., :sz.Wp]
    assert float(want.abs().max()) > 0
    assert same_bits(got, want)
    assert same_bits(seis, seis_ref)


# ------------------------------------------------------------------------------------------ 4. record tails
@pytest.mark.parametrize("nt", [157, 159, 161])
def test_record_length_tails_bitwise(cuda, cases, nt):
    """Record lengths that leave launch tails of 1 .. 3 steps at depths 2, 3 and 4 in the last segment as well as
    in the first one (K = 7), against born(history=True) at the same nt.  Direct launches."""
    c = copy.copy(cases["wrap"])
    c.ctx = dict(c.ctx, nt=nt)
    fwi = c.fwi()
    plan = plan_of(fwi, c)
    plan.set_graphs(False)
    seis_ref, ds_ref = fwi.born(c.v, c.dv, return_seis=True)
    assert ds_ref.shape == seis_ref.shape and float(ds_ref.abs().max()) > 0
    B, vm = c.v.shape[0], vel_mode_of(c)
    coeffs, vstat = plan.coeffs(c.v, vm)
    for depth in (2, 3, 4):
        plan.set_tuning(depth, depth, 1)
        seis, ds, _ = plan.born_fused(coeffs, vstat, c.dv, B, vm, 7)
        assert same_bits(seis, seis_ref) and same_bits(ds, ds_ref), (nt, depth)
    fwi.check()


# ------------------------------------------------------------------------------------------ 5. Gauss-Newton
def by_hand(fwi, c, weight):
    vv = c.v.clone().requires_grad_(True)
    s = fwi(vv)
    ds = fwi.born(c.v, c.dv)
    s.backward(ds if weight is None else weight * ds)
    return vv.grad


@pytest.mark.parametrize("custom", [False, True])
@pytest.mark.parametrize("K", [7, 40])
def test_gauss_newton_without_history(cuda, cases, K, custom):
    """FWIForward(checkpoint=K): gauss_newton(history=False) is the checkpointed autograd path's bits (fwi_ckpt:
    forward_ckpt, then adjoint_ckpt on weight * born), and within the gradient bar of history=True (whose adjoint
    is the default persistent one).  tiles is a normalised case; `custom` is the affine callable of
    tests/test_gpu_born.py::test_custom_denormalisation_and_shot_sharding, chained with torch.func."""
    c = cases["tiles"]
    assert c.normalize
    kw = dict(v_denorm_func=lambda x: (x + 1) * 1500 + 1500) if custom else {}
    fwi = c.fwi(checkpoint=K, **kw)
    assert fwi._fused_denorm() != custom
    weight = (torch.rand(c.w.shape, generator=torch.Generator().manual_seed(7)) > 0.3).float().to(cuda) * 0.5
    for w in (None, weight):
        h = fwi.gauss_newton(c.v, c.dv, w, history=False)
        assert h.shape == c.v.shape and not h.requires_grad and float(h.abs().max()) > 0
        assert same_bits(h, by_hand(fwi, c, w)), (K, custom, w is None)
        err = rel_l2(h, fwi.gauss_newton(c.v, c.dv, w).double())
        for b, e in enumerate(err):
            record_margin("born_fused_gauss_newton_vs_history_over_grad_bar",
                          f"tiles K {K} custom {custom} weight {w is not None}[{b}]", e, GRAD_BAR)
        assert (err <= GRAD_BAR).all(), (K, custom, err)
    fwi.check()


# ------------------------------------------------------------------------------------------ 6. under a budget
def test_history_budget(cuda, cases, stored):
    """A budget of a quarter of the store-all history: born(history=True) still refuses; the fused calls run, give
    the unbudgeted bits, and stay below half the history (born) / the history (gauss_newton) in peak memory."""
    c = cases["tiles"]
    free = c.fwi()
    B = c.v.shape[0]
    hist_bytes = int(plan_of(free, c).sizes(B).history)
    fwi = c.fwi(history_budget_gb=hist_bytes / 4 / 2 ** 30)
    with pytest.raises(ValueError, match=r"\d+ bytes"):
        fwi.born(c.v, c.dv)
    with pytest.raises(ValueError, match=r"\d+ bytes"):
        fwi.gauss_newton(c.v, c.dv)
    K = fwi.checkpoint_interval(plan_of(fwi, c), B)
    assert K is not None and 1 <= K < c.ctx["nt"]

    def peak_rise(f):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = f()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base

    (seis, ds), rise = peak_rise(lambda: fwi.born(c.v, c.dv, return_seis=True, history=False))
    print(f"born(history=False): peak rise {rise} bytes, store-all history {hist_bytes} bytes")
    assert same_bits(seis, stored["tiles"][0]) and same_bits(ds, stored["tiles"][1])
    assert same_bits(ds, free.born(c.v, c.dv, history=False))
    assert rise < hist_bytes / 2, (rise, hist_bytes)
    h, rise = peak_rise(lambda: fwi.gauss_newton(c.v, c.dv, history=False))
    print(f"gauss_newton(history=False), K = {K}: peak rise {rise} bytes, store-all history {hist_bytes} bytes")
    assert same_bits(h, c.fwi(checkpoint=K).gauss_newton(c.v, c.dv, history=False))
    assert rise < hist_bytes, (rise, hist_bytes)
    fwi.check()


# ------------------------------------------------------------------------------------------ 7. batch and shards
def test_batch_rows_and_shot_shards_bitwise(cuda, cases, stored):
    c = cases["tiles"]
    seis_ref, ds_ref = stored["tiles"]
    one = c.fwi()
    seis, ds = one.born(c.v[1:2].contiguous(), c.dv[1:2].contiguous(), return_seis=True, history=False)
    one.check()
    assert same_bits(seis[0], seis_ref[1]) and same_bits(ds[0], ds_ref[1])
    ns = c.ctx["ns"]
    assert ns >= 2
    parts = []
    for lo, hi in ((0, ns // 2), (ns // 2, ns)):
        shard = c.fwi(shots=(lo, hi))
        parts.append(shard.born(c.v, c.dv, return_seis=True, history=False))
        shard.check()
    assert same_bits(torch.cat([p[0] for p in parts], dim=1), seis_ref)
    assert same_bits(torch.cat([p[1] for p in parts], dim=1), ds_ref)


# ------------------------------------------------------------------------------------------ 8. linearity
@pytest.mark.parametrize("tag", CASES)
def test_linearity_bitwise(cuda, cases, stored, tag):
    """born(v, 2^j dv) = 2^j born(v, dv) bit for bit (the prologue's power-of-two scale), far below and far above
    the direction's own size; a zero direction gives zeros and leaves the record alone."""
    c = cases[tag]
    fwi = c.fwi()
    ds = stored[tag][1]
    assert float(ds.abs().max()) > 0
    for j in (-30, 40):
        assert same_bits(fwi.born(c.v, 2.0 ** j * c.dv, history=False), 2.0 ** j * ds), (tag, j)
    seis, zero = fwi.born(c.v, torch.zeros_like(c.dv), return_seis=True, history=False)
    fwi.check()
    assert torch.count_nonzero(zero) == 0
    assert same_bits(seis, stored[tag][0])
