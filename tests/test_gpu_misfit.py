"""K13, the misfits beyond L1 (csrc/misfit.hip: L2, Huber, trace-normalised correlation), per model, per trace
and per element against the two references of tests/misfit_refs.py (mixed: include/red_diffeq_misfit.h in
numpy; full: torch fp64 with autograd), through the C entry points, torch.ops.red_diffeq.misfit /
misfit_backward, red_diffeq.core.losses.misfit, LossCalculator and InversionEngine.optimize.
tests/test_misfit_refs_host.py checks the references and the branch each size is for on the CPU.

The bars are rounding counts read from the kernels and the header (u = 2^-24, e = 2^-53), never measured;
R.bar(k) = (1 + u)^k (1 + e)^16 - 1 compounds k fp32 roundings and the fp64 stages behind them.

L2 / Huber forward   vs mixed: the fp64 sums differ only in order (n e relative, n < 2^22 here), which can move
                     the one final rounding across a tie: at most 1 ulp of fp32.  nobs bit-equal (the fp64 sum
                     of 0 / 1 / 0.5 values is exact), 1 ulp allowed for the fractional mask.
                     vs full: d = fl32(pred - y) carries 2 u into d d, and into Huber's rho as well (rho' is
                     d / delta or 1 and rho >= |d| / 2 in the tails), the final rounding 1; all terms are
                     non-negative, so the bound carries to the sum: R.bar(3), R.bar(4) with a fractional mask
                     (nobs rounded to fp32).
L2 / Huber backward  elementwise, correctly rounded IEEE operations in the header's order: bit-equal to the mixed
                     formula.  vs fp64 autograd d (1) and the final rounding (1): R.bar(2), R.bar(3) with a
                     fractional mask; exactly 0 where mask == 0 or d == 0.
NCC sums             (a, c, q) of a trace are read back from the partial slabs and added in chunk order, as pass 2
                     does.  vs mixed (numpy's order) two orders of nt exact or once-rounded terms differ by at
                     most eps = 2 nt e of the sum of the terms' absolute values: a, c relative eps; q eps Q,
                     Q = sum |pt yt|.
NCC coefficients     (inv, r, J) bit-equal to the header's formulas applied in numpy to the kernel's own sums:
                     IEEE fp64 multiply, sqrt, divide and subtract, each correctly rounded.  vs full:
                     |dJ| <= 2 eps + 8 e (the cosine moves by (2 eps + 4 e) Q / sqrt(a c) <= 2 eps + 4 e by
                     Cauchy-Schwarz, 1 - cos rounds once more).  ntr bit-equal.
NCC loss             fl32(sum J / ntr): u |loss| + 2 (2 eps + 8 e) against both references.
NCC backward         bit-equal to the mixed formula on the kernel's own (inv, r).  vs fp64 autograd, per element,
                     |got - ref| <= 2 u M, M = |m gout / ntr| (|r pt| + |yt|) / sqrt(a c): the final rounding
                     (u |value| <= u M) and the fp64 stages (a few eps M, far below u M for nt < 2^20).
                     Orthogonality |sum_t dpred_t p_t| <= sum_t 2 u M_t |p_t|.  Exactly 0 on dead traces and
                     where a == 0.
Shards               per-trace and per-element results of a shot slice are the full call's bits.  The shard
                     losses fl32(fl32(S_i / n_i) fl32(n_i / N)) carry 3 roundings each against the full loss's 1,
                     all terms non-negative: |sum_i - full| <= R.bar(3) sum_i + u full.

Measured on the MI355X (profiles/r23/misfit_margins.jsonl): see the record_margin lines."""
import numpy as np
import pytest
import torch

import misfit_refs as R
from conftest import record_margin
from test_gpu_fwi import bits_equal

pytestmark = pytest.mark.gpu

U, E = R.U, R.E
ELEMENTWISE = ("l2", "huber")


def dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


def code(kind):
    from red_diffeq.ops import MISFIT_KINDS
    return MISFIT_KINDS[kind]


def delta_of(kind):
    return R.DELTA if kind == "huber" else 0.0


def eps_of(nt):
    return 2 * nt * E


def j_bar(nt):
    return 2 * eps_of(nt) + 8 * E


def same64(a, b):
    """Number of elements whose fp64 bits differ (+0 and -0 count as equal)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape
    return int(((a.view(np.int64) != b.view(np.int64)) & ~((a == 0) & (b == 0))).sum())


# ------------------------------------------------------------------------------ 1. L2 / Huber forward
@pytest.mark.parametrize("kind", ELEMENTWISE)
@pytest.mark.parametrize("size,mask_kind", R.mf_forward_cases())
def test_mf_forward_per_model(cuda, kind, size, mask_kind):
    """K5's size ladder from the new constants (misfit_refs.mf_sizes; the branch each is for is asserted on the
    host) with every mask kind: 1 ulp against the mixed reference, nobs bit-equal (1 ulp fractional),
    R.bar(3) (4 fractional) against fp64.  The Python misfit() returns the op's loss bit for bit."""
    from red_diffeq.core.losses import misfit
    shape = R.mf_shape(size)
    pred, y, mask = R.mf_inputs(kind, shape, mask_kind)
    p, t, m = dev(pred, cuda), dev(y, cuda), dev(mask, cuda)
    loss_t, nobs_t, coef_t = torch.ops.red_diffeq.misfit(p, t, m, code(kind), delta_of(kind))
    assert loss_t.dtype == nobs_t.dtype == torch.float32 and loss_t.shape == nobs_t.shape == (shape[0],)
    assert coef_t.numel() == 0
    loss, nobs = host(loss_t), host(nobs_t)
    assert bits_equal(host(misfit(p, t, m, kind, R.DELTA)), loss)
    ref, ref_nobs = R.mf_mixed(kind, pred, y, mask)
    full, full_nobs, _ = R.mf_full(kind, pred, y, mask)
    d_nobs = int(R.ulps(nobs, ref_nobs).max())
    d_loss = int(R.ulps(loss, ref).max())
    rel = float(np.max(np.abs(loss.astype(np.float64) - full) / np.where(full > 0, full, 1.0)))
    k = 4 if mask_kind == "frac" else 3
    print(f"K13 {kind} fwd {size} {mask_kind}: loss {d_loss} ulp vs mixed, {rel / U:.3f} u vs fp64 (bar {k}), "
          f"nobs {d_nobs} ulp")
    record_margin(f"{kind}_forward_ulps_vs_mixed", f"{size},{mask_kind}", d_loss, 1)
    record_margin(f"{kind}_forward_rel_vs_fp64", f"{size},{mask_kind}", rel, R.bar(k))
    assert d_nobs <= (1 if mask_kind == "frac" else 0), (nobs, ref_nobs)
    assert (np.abs(nobs - full_nobs) <= U * full_nobs).all()
    assert d_loss <= 1, (loss, ref)
    assert (np.abs(loss.astype(np.float64) - full) <= R.bar(k) * full).all(), (loss, full)
    if mask_kind == "zero_model":
        b0 = R.zero_model(shape[0])
        assert nobs[b0] == 1.0 and loss[b0] == 0.0


# ------------------------------------------------------------------------------ 2. L2 / Huber backward
@pytest.mark.parametrize("kind", ELEMENTWISE)
@pytest.mark.parametrize("size,mask_kind", R.mf_backward_cases())
def test_mf_backward_per_element(cuda, kind, size, mask_kind):
    """k_mf_backward at the B = 3 sizes and the record at B = 3, every mask kind, with the upstream gradients
    (-0.7, 0, 2) through the op and the expanded stride-0 gradient of .sum().backward() through misfit():
    bit-equal to the mixed formula, R.bar(2) (3 fractional) of fp64 autograd, exactly 0 where mask == 0 or
    d == 0 (Huber's inputs hold |d| == delta, its fp32 neighbours and d == 0: misfit_refs.mf_pair)."""
    from red_diffeq.core.losses import misfit
    shape = R.mf_backward_shape(size)
    pred, y, mask = R.mf_inputs(kind, shape, mask_kind)
    p, t, m = dev(pred, cuda), dev(y, cuda), dev(mask, cuda)
    _, nobs_t, coef_t = torch.ops.red_diffeq.misfit(p, t, m, code(kind), delta_of(kind))
    nobs = host(nobs_t)
    zero = pred == y
    if mask is not None:
        zero |= mask == 0
    k = 3 if mask_kind == "frac" else 2
    worst = 0.0
    for tag, gout in (("distinct", np.array(R.GOUT, np.float32)), ("sum", np.ones(3, np.float32))):
        if tag == "distinct":
            got_t = torch.ops.red_diffeq.misfit_backward(p, t, m, nobs_t, coef_t, dev(gout, cuda), code(kind),
                                                         delta_of(kind))
        else:
            q = p.clone().requires_grad_(True)
            misfit(q, t, m, kind, R.DELTA).sum().backward()
            got_t = q.grad
        assert got_t.dtype == torch.float32 and got_t.shape == shape and got_t.is_contiguous()
        got = host(got_t)
        want = R.mf_backward_mixed(kind, pred, y, mask, nobs, gout)
        assert bits_equal(got + np.float32(0), want + np.float32(0)), (size, mask_kind, tag)
        _, _, full = R.mf_full(kind, pred, y, mask, gout)
        err = np.abs(got.astype(np.float64) - full)
        assert (err <= R.bar(k) * np.abs(full)).all(), (size, mask_kind, tag)
        assert (got[zero] == 0).all() and (full[zero] == 0).all()
        live = full != 0
        if live.any():
            worst = max(worst, float((err[live] / np.abs(full[live])).max()))
    print(f"K13 {kind} bwd {size} {mask_kind}: {worst / U:.3f} u vs fp64 (bar {k}), bit-equal to the mixed formula")
    record_margin(f"{kind}_backward_rel_vs_fp64", f"{size},{mask_kind}", worst, R.bar(k))


# ------------------------------------------------------------------------------ 3. NCC per trace and per model
def ncc_raw(cuda, pred, y, mask):
    """One rdq_misfit_forward(NCC) call on buffers of the test's own: the per-trace sums read back from the
    partial slabs [B][ns][ntc][3][ng] and added in chunk order as pass 2 adds them, and coef, loss, ntr."""
    from red_diffeq import _hip
    L = _hip.lib()
    B, ns, nt, ng = pred.shape
    tc = R.kernel_constants()["NCC_TC"]
    ntc = -(-nt // tc)
    p, t, m = dev(pred, cuda), dev(y, cuda), dev(mask, cuda)
    loss, ntr = torch.empty(B, device=cuda), torch.empty(B, device=cuda)
    nbytes = L.rdq_misfit_workspace_bytes(3, B, ns, nt, ng)
    assert nbytes % 8 == 0 and nbytes // 8 >= B * ns * ntc * 3 * ng
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=cuda)
    coef = torch.full((B, ns, ng, 3), float("nan"), dtype=torch.float64, device=cuda)
    assert coef.numel() * 8 == L.rdq_misfit_coef_bytes(3, B, ns, ng)
    _hip.check(L.rdq_misfit_forward(3, B, ns, nt, ng, 0.0, _hip.ptr(p), _hip.ptr(t), _hip.ptr(m), _hip.ptr(loss),
                                    _hip.ptr(ntr), _hip.ptr(coef), _hip.ptr(ws), _hip.stream_of(p)), "rdq_misfit_forward")
    torch.cuda.synchronize()
    part = host(ws)[:B * ns * ntc * 3 * ng].reshape(B, ns, ntc, 3, ng)
    assert np.isfinite(host(ws)).all()                     # every slot of the workspace was written
    sums = np.zeros((3, B, ns, ng))
    for ch in range(ntc):
        for j in range(3):
            sums[j] += part[:, :, ch, j]
    return dict(a=sums[0], c=sums[1], q=sums[2], coef=host(coef), loss=host(loss), ntr=host(ntr), tensors=(p, t, m))


@pytest.mark.parametrize("shape", R.ncc_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_ncc_per_trace_and_per_model(cuda, shape):
    """Every shape of misfit_refs.ncc_shapes (ns in {1, 2}; ng 1, 3, 64, 70, block + 1; nt 1, 2, TC - 1, TC,
    TC + 1, 2 TC + 1; the record) with every mask kind: the per-trace sums against the mixed reference within
    the order-of-summation bound, (inv, r, J) bit-equal to the header's formulas on the kernel's own sums and
    J within 2 eps + 8 e of fp64, ntr bit-equal, the loss within u |loss| + 2 (2 eps + 8 e) of both references.
    The op returns the raw call's bits."""
    B, ns, nt, ng = shape
    eps = eps_of(nt)
    worst = dict(a=0.0, c=0.0, q=0.0, J=0.0, loss=0.0)
    coef_diff = 0
    for mask_kind in R.MASKS:
        pred, y, mask = R.ncc_inputs(shape, mask_kind)
        got = ncc_raw(cuda, pred, y, mask)
        mx = R.ncc_mixed(pred, y, mask)
        fl = R.ncc_full(pred, y, mask)
        for k, scale in (("a", mx["a"]), ("c", mx["c"]), ("q", mx["Q"])):
            err = np.abs(got[k] - mx[k])
            assert (err <= eps * scale).all(), (mask_kind, k, float(err.max()))
            nz = scale > 0
            if nz.any():
                worst[k] = max(worst[k], float((err[nz] / scale[nz]).max()))
        inv, r, J, live = R.ncc_coef(got["a"], got["c"], got["q"])
        assert np.array_equal(live, mx["live"]) and np.array_equal(live, fl["live"])
        coef_diff += same64(got["coef"][..., 0], inv) + same64(got["coef"][..., 1], r) + same64(got["coef"][..., 2], J)
        errJ = np.abs(got["coef"][..., 2] - fl["J"])
        worst["J"] = max(worst["J"], float(errJ.max()))
        assert (errJ <= j_bar(nt)).all(), (mask_kind, float(errJ.max()))
        assert (np.abs(got["coef"][..., 2] - mx["J"]) <= j_bar(nt)).all()
        assert bits_equal(got["ntr"], mx["ntr"]) and np.array_equal(got["ntr"].astype(np.float64), fl["ntr"])
        for ref in (mx["loss"].astype(np.float64), fl["loss"]):
            err = np.abs(got["loss"].astype(np.float64) - ref)
            lbar = U * np.abs(ref) + 2 * j_bar(nt)
            assert (err <= lbar).all(), (mask_kind, got["loss"], ref)
            worst["loss"] = max(worst["loss"], float((err / lbar).max()))
        if mask_kind == "zero_model":
            b0 = R.zero_model(B)
            assert got["ntr"][b0] == 1.0 and got["loss"][b0] == 0.0 and not got["coef"][b0].any()
        loss_t, ntr_t, coef_t = torch.ops.red_diffeq.misfit(*got["tensors"], 3, 0.0)
        assert bits_equal(host(loss_t), got["loss"]) and bits_equal(host(ntr_t), got["ntr"])
        assert coef_t.shape == (B, ns, ng, 3) and same64(host(coef_t), got["coef"]) == 0
    case = "x".join(map(str, shape))
    print(f"K13 ncc {case}: sums a {worst['a'] / E:.1f} c {worst['c'] / E:.1f} q {worst['q'] / E:.1f} e (bar {eps / E:.0f}), "
          f"J {worst['J'] / E:.1f} e vs fp64 (bar {j_bar(nt) / E:.0f}), loss err / bar {worst['loss']:.3f}, "
          f"{coef_diff} coefficients differ from the header's formulas in fp64")
    for k in "acq":
        record_margin(f"ncc_sum_{k}_vs_mixed", case, worst[k], eps)
    record_margin("ncc_J_vs_fp64", case, worst["J"], j_bar(nt))
    record_margin("ncc_loss_err_over_bar", case, worst["loss"], 1.0)
    record_margin("ncc_coefficients_not_bit_equal", case, coef_diff, 1)
    assert coef_diff == 0


# ------------------------------------------------------------------------------ 4. NCC backward
def backward_shape(shape):
    return (3,) + tuple(shape[1:])


@pytest.mark.parametrize("shape", R.ncc_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_ncc_backward_per_element(cuda, shape):
    """k_ncc_backward at every NCC shape (the record at B = 3) and mask kind, upstream gradients (-0.7, 0, 2)
    through the op and ones through misfit().sum().backward(): bit-equal to the mixed formula on the kernel's
    (inv, r), |got - ref| <= 2 u M against fp64 autograd per element, orthogonal to the predicted trace within
    the same bars summed over time, exactly 0 on dead traces."""
    from red_diffeq.core.losses import misfit
    shape = backward_shape(shape)
    worst = orth_worst = 0.0
    for mask_kind in R.MASKS:
        pred, y, mask = R.ncc_inputs(shape, mask_kind)
        p, t, m = dev(pred, cuda), dev(y, cuda), dev(mask, cuda)
        _, ntr_t, coef_t = torch.ops.red_diffeq.misfit(p, t, m, 3, 0.0)
        coef, ntr = host(coef_t), host(ntr_t)
        dead = np.broadcast_to((coef[..., 0] == 0)[:, :, None, :], shape)
        for tag, gout in (("distinct", np.array(R.GOUT, np.float32)), ("sum", np.ones(3, np.float32))):
            if tag == "distinct":
                got_t = torch.ops.red_diffeq.misfit_backward(p, t, m, ntr_t, coef_t, dev(gout, cuda), 3, 0.0)
            else:
                q = p.clone().requires_grad_(True)
                misfit(q, t, m, "ncc").sum().backward()
                got_t = q.grad
            assert got_t.dtype == torch.float32 and got_t.shape == shape and got_t.is_contiguous()
            got = host(got_t)
            want, M = R.ncc_backward_mixed(pred, y, mask, coef[..., 0], coef[..., 1], ntr, gout)
            assert bits_equal(got + np.float32(0), want + np.float32(0)), (mask_kind, tag)
            full = R.ncc_full(pred, y, mask, gout)["grad"]
            err = np.abs(got.astype(np.float64) - full)
            assert (got[dead] == 0).all() and (full[dead] == 0).all()
            assert (got[M == 0] == 0).all()
            ratio = np.where(M > 0, err / np.where(M > 0, 2 * U * M, 1.0), 0.0)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (mask_kind, tag, float(ratio.max()))
            orth = np.abs((got.astype(np.float64) * pred).sum(2))
            obar = (2 * U * M * np.abs(pred)).sum(2)
            assert (orth <= obar).all(), (mask_kind, tag)
            if (obar > 0).any():
                orth_worst = max(orth_worst, float((orth[obar > 0] / obar[obar > 0]).max()))
    case = "x".join(map(str, shape))
    print(f"K13 ncc bwd {case}: err / (2 u M) {worst:.3f}, orthogonality / bar {orth_worst:.3f}, bit-equal to mixed")
    record_margin("ncc_backward_err_over_bar", case, worst, 1.0)
    record_margin("ncc_backward_orthogonality_over_bar", case, orth_worst, 1.0)


# ------------------------------------------------------------------------------ 5. NCC exact cases
def ncc_run(cuda, pred, y, mask, gout):
    p, t, m = dev(pred, cuda), dev(y, cuda), dev(mask, cuda)
    loss, ntr, coef = torch.ops.red_diffeq.misfit(p, t, m, 3, 0.0)
    grad = torch.ops.red_diffeq.misfit_backward(p, t, m, ntr, coef, dev(gout, cuda), 3, 0.0)
    return host(loss), host(ntr), host(coef), host(grad)


def test_ncc_exact_cases(cuda):
    """misfit_refs.ncc_exact_case: a masked column, zero observed traces and a model with every trace dead give
    J = 0, a zero gradient and ntr counting the live traces only (1 and loss 0 for the dead model); a zero
    predicted trace under a live observed one gives J = 1 and a zero gradient; pred == y gives a zero gradient
    (r = q / a of identical sums is 1, r pt - yt = 0) and, with a correctly rounded sqrt, J = 0 exactly
    (sqrt(fl(a a)) = a, q / a = 1), within 4 e otherwise (a c, sqrt, the quotient, the difference);
    pred -> 2^k pred, k in {-3, 5}, leaves the loss and every J bit-equal and scales the gradient by exactly
    2^-k (a c scales by 4^k, a correctly rounded sqrt by 2^k, r by 2^-k: all exact)."""
    pred, y, mask, dead, zero_pred = R.ncc_exact_case()
    gout = np.array(R.GOUT, np.float32)
    loss, ntr, coef, grad = ncc_run(cuda, pred, y, mask, gout)
    assert not coef[dead].any() and (coef[zero_pred] == [0.0, 0.0, 1.0]).all()
    assert ntr.tolist() == [float((~dead[0]).sum()), 1.0, float((~dead[2]).sum())] and loss[1] == 0.0
    off = np.broadcast_to((dead | zero_pred)[:, :, None, :], pred.shape)
    assert (grad[off] == 0).all() and grad[0][~off[0]].any() and not grad[1].any()
    mx = R.ncc_mixed(pred, y, mask)
    assert np.array_equal(mx["live"], ~dead) and bits_equal(ntr, mx["ntr"])

    loss_same, _, coef_same, grad_same = ncc_run(cuda, y, y, mask, gout)
    assert not grad_same.any()
    worst = float(np.abs(coef_same[..., 2]).max())
    print(f"K13 ncc pred == y: max |J| {worst / E:.2f} e (bar 4; 0 with a correctly rounded sqrt), loss {loss_same}")
    record_margin("ncc_J_at_pred_equal_y", "exact_case", worst, 4 * E)
    assert worst <= 4 * E and (np.abs(loss_same) <= 4 * E).all()
    assert (coef_same[~dead][:, 1] == 1.0).all()

    for k in (-3, 5):
        s = np.float32(2.0 ** k)
        loss_k, ntr_k, coef_k, grad_k = ncc_run(cuda, pred * s, y, mask, gout)
        assert bits_equal(loss_k, loss) and bits_equal(ntr_k, ntr), k
        assert same64(coef_k[..., 2], coef[..., 2]) == 0, k
        assert same64(coef_k[..., 0] * 2.0 ** k, coef[..., 0]) == 0 and same64(coef_k[..., 1] * 2.0 ** k, coef[..., 1]) == 0
        assert bits_equal(grad_k * s + np.float32(0), grad + np.float32(0)), k
        assert np.array_equal(grad_k == 0, grad == 0)


# ------------------------------------------------------------------------------ 6. launch-shape independence
@pytest.mark.parametrize("mask_kind", ["none", "rand01"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_shot_shards_are_the_full_surveys_bits(cuda, kind, mask_kind):
    """An ns = 4 survey against its shot slices [0, 1) and [1, 4) called alone with norm= the survey's
    normaliser: the NCC per-trace coefficients and dpred of every kind are the full call's bits, and the shard
    losses add up to the full loss within R.bar(3) sum_i + u full."""
    from red_diffeq.core.losses import misfit
    tc = R.kernel_constants()["NCC_TC"]
    shape = (3, 4, tc + 1, 70)
    pred, y, mask = (R.ncc_inputs if kind == "ncc" else lambda s, m: R.mf_inputs(kind, s, m))(shape, mask_kind)
    gout = dev(np.array(R.GOUT, np.float32), cuda)
    p, t, m = dev(pred, cuda), dev(y, cuda), dev(mask, cuda)
    loss, norm, coef = torch.ops.red_diffeq.misfit(p, t, m, code(kind), delta_of(kind))
    full_grad = torch.ops.red_diffeq.misfit_backward(p, t, m, norm, coef, gout, code(kind), delta_of(kind))
    total = np.zeros(3)
    for s0, s1 in ((0, 1), (1, 4)):
        sl = slice(s0, s1)
        ps = p[:, sl].contiguous().requires_grad_(True)
        ts, ms = t[:, sl].contiguous(), None if m is None else m[:, sl].contiguous()
        shard = misfit(ps, ts, ms, kind, R.DELTA, norm=norm)
        shard.backward(gout)
        assert bits_equal(host(ps.grad), host(full_grad[:, sl])), (s0, s1)
        if kind == "ncc":
            _, _, coef_s = torch.ops.red_diffeq.misfit(ps.detach(), ts, ms, 3, 0.0)
            assert same64(host(coef_s), host(coef[:, sl])) == 0
        assert (host(shard) >= 0).all()
        total += host(shard).astype(np.float64)
    full = host(loss).astype(np.float64)
    err = np.abs(total - full)
    lbar = R.bar(3) * total + U * full
    print(f"K13 {kind} shards {mask_kind}: |sum - full| / bar {float((err / lbar).max()):.3f}")
    record_margin(f"{kind}_shard_losses_err_over_bar", mask_kind, float((err / lbar).max()), 1.0)
    assert (err <= lbar).all(), (total, full)


# ------------------------------------------------------------------------------ 7. Python entry
SMALL = (3, 2, 50, 7)


@pytest.mark.parametrize("kind", R.KINDS)
def test_python_entry_strides_and_dtypes(cuda, kind):
    """misfit() as test_l1_python_entry_strides_and_dtypes demands of l1_misfit: a permuted view of a leaf, a
    non-contiguous leaf, a float64 y and a float64 leaf give the contiguous fp32 call's loss bit for bit, the
    gradient lands in the leaf's own layout, and the float64 leaf gets a float64 gradient of the same value.
    Two runs are bit-identical."""
    from red_diffeq.core.losses import misfit
    pred, y, mask = (R.ncc_inputs if kind == "ncc" else lambda s, m: R.mf_inputs(kind, s, m))(SMALL, "rand01")
    gout = dev(np.array(R.GOUT, np.float32), cuda)
    t, m = dev(y, cuda), dev(mask, cuda)

    def run(leaf, view=None, target=t):
        loss = misfit(leaf if view is None else view, target, m, kind, R.DELTA)
        loss.backward(gout)
        return host(loss), leaf.grad

    want_loss, g = run(dev(pred, cuda).requires_grad_(True))
    want = host(g)
    again_loss, again = run(dev(pred, cuda).requires_grad_(True))
    assert bits_equal(again_loss, want_loss) and bits_equal(host(again), want)

    base = dev(pred.transpose(0, 3, 2, 1), cuda).requires_grad_(True)      # (3, 7, 50, 2) leaf
    view = base.permute(0, 3, 2, 1)
    assert not view.is_contiguous() and view.shape == SMALL
    l2, g2 = run(base, view)
    assert bits_equal(l2, want_loss) and bits_equal(host(g2.permute(0, 3, 2, 1)), want)

    wide = torch.zeros(3, 2, 50, 9, device=cuda)
    wide[..., 1:-1] = dev(pred, cuda)
    leaf = wide[..., 1:-1].detach().requires_grad_(True)                  # a non-contiguous leaf
    assert not leaf.is_contiguous()
    l3, g3 = run(leaf)
    assert bits_equal(l3, want_loss) and bits_equal(host(g3), want)

    l4, g4 = run(dev(pred, cuda).requires_grad_(True), target=t.double())  # float64 y
    assert bits_equal(l4, want_loss) and bits_equal(host(g4), want)

    l5, g5 = run(dev(pred, cuda).double().requires_grad_(True))           # float64 pred that requires grad
    assert bits_equal(l5, want_loss)
    assert g5.dtype == torch.float64 and g5.shape == SMALL
    assert np.array_equal(host(g5), want.astype(np.float64))


def test_l1_kind_is_l1_misfit_and_ops_pass_opcheck(cuda):
    from torch.library import opcheck
    from red_diffeq.core.losses import LossCalculator, l1_misfit, misfit
    from red_diffeq.regularization.base import RegularizationMethod
    pred, y, mask = R.ncc_inputs(SMALL, "rand01")
    gout = dev(np.array(R.GOUT, np.float32), cuda)
    t, m = dev(y, cuda), dev(mask, cuda)
    a, b = dev(pred, cuda).requires_grad_(True), dev(pred, cuda).requires_grad_(True)
    la, lb = misfit(a, t, m, kind="l1"), l1_misfit(b, t, m)
    la.backward(gout)
    lb.backward(gout)
    assert bits_equal(host(la), host(lb)) and bits_equal(host(a.grad), host(b.grad))
    nobs = torch.full((3,), 900.0, device=cuda)
    assert bits_equal(host(misfit(a, t, m, "l1", norm=nobs)), host(l1_misfit(b, t, m, nobs)))
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    ops = torch.ops.red_diffeq
    for kind in R.KINDS:
        calc = LossCalculator(RegularizationMethod("tv"), kind, R.DELTA if kind == "huber" else None)
        assert bits_equal(host(calc.observation_loss(a, t, m)), host(misfit(a, t, m, kind, R.DELTA)))
        p = dev(pred, cuda)
        for mm in (m, None):
            opcheck(ops.misfit, (p, t, mm, code(kind), delta_of(kind)), test_utils=utils)
            _, norm, coef = ops.misfit(p, t, mm, code(kind), delta_of(kind))
            opcheck(ops.misfit_backward, (p, t, mm, norm, coef, gout, code(kind), delta_of(kind)), test_utils=utils)
    with pytest.raises(ValueError, match="ncc"):
        ops.misfit(p.reshape(3, -1), t.reshape(3, -1), None, 3, 0.0)
    with pytest.raises(RuntimeError, match="rdq_misfit_forward"):
        ops.misfit(p, t, None, 2, 0.0)                                    # Huber refused by the C entry point


# ------------------------------------------------------------------------------ 8. engine
CTX = dict(n_grid=24, nt=200, dx=10.0, dt=0.001, nbc=10, f=15.0, sz=10, gz=10, ng=24, ns=3)


@pytest.fixture(scope="module")
def survey(cuda):
    """The smoke geometry: B = 2 curved-fault models, their record, a second pair of models as the start."""
    from red_diffeq.solvers.pde import FWIForward
    from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize
    from red_diffeq.utils.synthetic import make_model
    from conftest import vnorm
    fwi = FWIForward(dict(CTX), cuda, v_denorm_func=v_denormalize, s_norm_func=s_normalize_none)
    v_true = make_model("curvefault", 24, 24, seed=1, batch=2).astype(np.float32)
    v0 = vnorm(make_model("curvefault", 24, 24, seed=5, batch=2))
    with torch.no_grad():
        y = fwi(dev(vnorm(v_true), cuda)).clone()
    mu0 = torch.nn.functional.pad(torch.from_numpy(v0), (1, 1, 1, 1), "constant", 0)
    return fwi, torch.from_numpy(v_true), y, mu0


def engine_run(cuda, survey, **kw):
    from red_diffeq.core.inversion import InversionEngine
    from red_diffeq.utils.ssim import SSIM
    fwi, v_true, y, mu0 = survey

    class dm:
        device = cuda
    eng = InversionEngine(dm, SSIM(window_size=11), None, show_progress=False)
    eng.model_trace = []
    mu, hist = eng.optimize(mu0, v_true, y, fwi, ts=2, lr=0.03, reg_lambda=0.01, regularization=None, **kw)
    return [host(x) for x in eng.model_trace], hist, host(mu)


@pytest.mark.parametrize("kind", ("l1",) + R.KINDS)
def test_engine_runs_the_misfit_it_is_given(cuda, survey, kind):
    """optimize(misfit=kind) on the smoke geometry, no regulariser, no noise, ts = 2: obs_losses[0] is
    misfit(fwi(v0), y, kind) and the model after step 1 a hand-written fwi -> misfit -> backward ->
    FusedAdamClamp step, both bit for bit."""
    from red_diffeq.core.fused import FusedAdamClamp
    from red_diffeq.core.losses import misfit
    fwi, _, y, mu0 = survey
    hd = 0.05 if kind == "huber" else None
    trace, hist, _ = engine_run(cuda, survey, misfit=kind, huber_delta=hd)
    mu = mu0.clone().to(cuda).requires_grad_(True)
    loss = misfit(fwi(mu[:, :, 1:-1, 1:-1]), y, None, kind, hd)
    opt = FusedAdamClamp(mu, lr=0.03, clamp=(-1.0, 1.0))
    opt.zero_grad()
    loss.sum().backward()
    opt.step()
    assert bits_equal(np.array([h["obs_losses"][0] for h in hist], np.float32), host(loss)), kind
    assert (host(loss) > 0).all()
    assert bits_equal(trace[0], host(mu)[:, :, 1:-1, 1:-1]), kind
    assert not np.array_equal(trace[0], host(mu0)[:, :, 1:-1, 1:-1])


def test_engine_l1_is_the_default_bit_for_bit(cuda, survey):
    a = engine_run(cuda, survey)
    b = engine_run(cuda, survey, misfit="l1")
    assert len(a[0]) == len(b[0]) == 2
    for x, z in zip(a[0], b[0]):
        assert bits_equal(x, z)
    assert bits_equal(a[2], b[2])
    for ha, hb in zip(a[1], b[1]):
        for k in ha:
            assert bits_equal(np.array(ha[k], np.float32), np.array(hb[k], np.float32)), k


def test_engine_ncc_with_missing_traces_counts_live_traces(cuda, survey, monkeypatch):
    """missing_number = 2 with the ncc misfit runs, and the kernel reports ntr = ns (ng - 2) per model: the
    masked receivers are dead traces, every other trace of the record is live."""
    from red_diffeq.core import losses
    seen = []
    real = losses.misfit

    def spy(predicted, target, mask=None, kind="l2", delta=None, norm=None):
        seen.append(torch.ops.red_diffeq.misfit(predicted.detach(), target, mask, code(kind), 0.0)[1])
        return real(predicted, target, mask, kind, delta, norm)

    monkeypatch.setattr(losses, "misfit", spy)
    trace, hist, _ = engine_run(cuda, survey, misfit="ncc", missing_number=2)
    assert len(seen) == 2
    for ntr in seen:
        assert host(ntr).tolist() == [float(CTX["ns"] * (CTX["ng"] - 2))] * 2
    obs = np.array([h["obs_losses"] for h in hist])
    assert np.isfinite(obs).all() and (obs > 0).all() and (obs < 2).all()
    assert all(np.isfinite(x).all() for x in trace)
