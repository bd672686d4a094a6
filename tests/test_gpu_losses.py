"""The loss-side kernels of csrc/fwi.hip element by element against fp64: K5, the masked L1 misfit
(k_l1_partial, k_l1_final, k_l1_backward), and K6, TV / Tikhonov (k_smooth_fwd, k_smooth_bwd), through
torch.ops.red_diffeq.* and the Python entry points l1_misfit, total_variation_loss, tikhonov_loss and
LossCalculator.  Case tables, inputs and the two references (mixed: the kernel's definition, full: the
reference's formulas in fp64 with autograd) are tests/loss_refs.py; tests/test_loss_refs_host.py checks them
on the CPU, with the branch each size is for.

The bars are rounding counts read from the kernels (u = 2^-24), never measured from them:

K5 forward   vs mixed: the fp64 sums differ only in order (n 2^-53 relative), which can move the one final
             rounding across a tie: at most 1 ulp of fp32; a dropped or doubled chunk is at least 1 / nchunk,
             thousands of ulps at every size here.  nobs bit-equal (the fp64 sum of 0 / 1 / 0.5 values is
             exact below 2^53), within 1 ulp allowed for the fractional mask.
             vs full: fl32(y - pred) (1), fl32(d mask) (1; exact for 0 / 1 masks), the final cast (1);
             nobs is exact for n < 2^24: 3 u relative, 4 u with a fractional mask.
K5 backward  one division fl32(gout / nobs), one product with the mask, a sign: bit-equal to the mixed
             formula, within 2 u relative of fp64 autograd, exactly 0 where pred == y or the mask is 0.
K6 forward   vs mixed: at most 1 ulp, as K5.  vs full, all terms non-negative so per-term bounds carry to
             the sums: TV e (1), tx / ty (1), tx + ty (1) = 3 <= 4 u; Tikhonov e (2: it is squared), e e (1),
             tx / ty (1), tx + ty (1) = 5 u.
K6 backward  per cell |got - ref| <= k u M, M the fp64 sum of the absolute values of the cell's up to four
             terms.  TV: gout / N (1) and three additions of four terms (the first lands on 0, exact): k = 4.
             Tikhonov: gout / N (1), d (1), 2 d g (1; 2 d is exact), three additions: k = 6.  A cell whose
             terms are all 0 is exactly 0.  (The library builds fwi.hip with -ffp-contract=off; a
             contracted 2 d g - acc would round once less, inside the same bar.)"""
import numpy as np
import pytest
import torch

import loss_refs as R
from conftest import record_margin
from test_gpu_fwi import bits_equal

pytestmark = pytest.mark.gpu

U = R.U


def dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------- K5
@pytest.mark.parametrize("size,kind", R.k5_forward_cases())
def test_l1_forward_per_model(cuda, size, kind):
    """K5 forward and nobs at every size of loss_refs.k5_sizes (what each size is for stands there and is
    asserted in test_loss_refs_host.py) with every mask kind.  Bars: 1 ulp against the mixed reference,
    nobs bit-equal (1 ulp with the fractional mask), 3 u relative against fp64 (4 u fractional): the
    subtraction, the product, the final cast.  The Python l1_misfit returns the op's loss bit for bit."""
    from red_diffeq.core.losses import l1_misfit
    shape = R.k5_shape(size)
    pred, y, mask = R.k5_inputs(shape, kind)
    p, t, m = dev(pred, cuda), dev(y, cuda), dev(mask, cuda)
    loss_t, nobs_t = torch.ops.red_diffeq.l1_misfit(p, t, m)
    assert loss_t.dtype == nobs_t.dtype == torch.float32 and loss_t.shape == nobs_t.shape == (shape[0],)
    loss, nobs = host(loss_t), host(nobs_t)
    assert bits_equal(host(l1_misfit(p, t, m)), loss)
    ref, ref_nobs = R.l1_mixed(pred, y, mask)
    full, full_nobs, _ = R.l1_full(pred, y, mask)
    d_nobs = int(R.ulps(nobs, ref_nobs).max())
    d_loss = int(R.ulps(loss, ref).max())
    rel = float(np.max(np.abs(loss.astype(np.float64) - full) / np.where(full > 0, full, 1.0)))
    k = 4 if kind == "frac" else 3
    print(f"K5 fwd {size} {kind}: loss {d_loss} ulp vs mixed, {rel / U:.3f} u vs fp64 (bar {k}), nobs {d_nobs} ulp")
    record_margin("l1_forward_ulps_vs_mixed", f"{size},{kind}", d_loss, 1)
    record_margin("l1_forward_rel_vs_fp64", f"{size},{kind}", rel, k * U)
    assert d_nobs <= (1 if kind == "frac" else 0), (nobs, ref_nobs)
    assert (np.abs(nobs - full_nobs) <= U * full_nobs).all()
    assert d_loss <= 1, (loss, ref)
    assert (np.abs(loss.astype(np.float64) - full) <= k * U * full).all(), (loss, full)
    if kind == "zero_model":
        b0 = R.zero_model(shape[0])
        assert nobs[b0] == 1.0 and loss[b0] == 0.0


@pytest.mark.parametrize("size,kind", R.k5_backward_cases())
def test_l1_backward_per_element(cuda, size, kind):
    """k_l1_backward at the B = 3 sizes and the product's record at B = 3, every mask kind, with the
    upstream gradients (-0.7, 0, 2) through the op and with the expanded stride-0 gradient of
    .sum().backward() through the Python l1_misfit.  One division, one product, a sign: bit-equal to the
    mixed formula, within 2 u relative of fp64 autograd, exactly 0 where pred == y or the mask is 0."""
    from red_diffeq.core.losses import l1_misfit
    shape = R.k5_backward_shape(size)
    pred, y, mask = R.k5_inputs(shape, kind)
    p, t, m = dev(pred, cuda), dev(y, cuda), dev(mask, cuda)
    _, nobs_t = torch.ops.red_diffeq.l1_misfit(p, t, m)
    nobs = host(nobs_t)
    assert bits_equal(nobs, R.l1_mixed(pred, y, mask)[1]) or kind == "frac"
    zero = pred == y
    if mask is not None:
        zero |= mask == 0
    worst = 0.0
    for tag, gout in (("distinct", np.array(R.K5_GOUT, np.float32)), ("sum", np.ones(3, np.float32))):
        if tag == "distinct":
            got_t = torch.ops.red_diffeq.l1_misfit_backward(p, t, m, nobs_t, dev(gout, cuda))
        else:
            q = p.clone().requires_grad_(True)
            l1_misfit(q, t, m).sum().backward()
            got_t = q.grad
        assert got_t.dtype == torch.float32 and got_t.shape == shape and got_t.is_contiguous()
        got = host(got_t)
        assert bits_equal(got, R.l1_backward_mixed(pred, y, mask, nobs, gout)), (size, kind, tag)
        _, _, full = R.l1_full(pred, y, mask, gout)
        err = np.abs(got.astype(np.float64) - full)
        assert (err <= 2 * U * np.abs(full)).all(), (size, kind, tag)
        assert (got[zero] == 0).all() and (full[zero] == 0).all()
        live = full != 0
        if live.any():
            worst = max(worst, float((err[live] / np.abs(full[live])).max()))
    print(f"K5 bwd {size} {kind}: {worst / U:.3f} u vs fp64 (bar 2), bit-equal to the mixed formula")
    record_margin("l1_backward_rel_vs_fp64", f"{size},{kind}", worst, 2 * U)


SMALL = (3, 2, 50, 7)        # a record of 700 samples per model, as test_l1_and_smooth_reg_kernels uses


def test_l1_python_entry_strides_and_dtypes(cuda):
    """The Python l1_misfit with a non-contiguous pred that requires grad (a permuted view of a leaf, and a
    non-contiguous leaf), a float64 y, and a float64 pred that requires grad: the loss is the contiguous
    fp32 call's bit for bit, the gradient lands in the leaf's own layout, and the float64 leaf gets a
    float64 gradient equal in value to the fp32 run's."""
    from red_diffeq.core.losses import l1_misfit
    pred, y, mask = R.k5_inputs(SMALL, "rand01")
    gout = dev(np.array(R.K5_GOUT, np.float32), cuda)
    t, m = dev(y, cuda), dev(mask, cuda)
    p = dev(pred, cuda).requires_grad_(True)
    loss = l1_misfit(p, t, m)
    loss.backward(gout)
    want_loss, want = host(loss), host(p.grad)
    assert bits_equal(want, R.l1_backward_mixed(pred, y, mask, R.l1_mixed(pred, y, mask)[1], R.K5_GOUT))

    base = dev(pred.transpose(0, 3, 2, 1), cuda).requires_grad_(True)      # (3, 7, 50, 2) leaf
    view = base.permute(0, 3, 2, 1)
    assert not view.is_contiguous() and view.shape == SMALL
    l2 = l1_misfit(view, t, m)
    l2.backward(gout)
    assert bits_equal(host(l2), want_loss) and bits_equal(host(base.grad.permute(0, 3, 2, 1)), want)

    wide = torch.zeros(3, 2, 50, 9, device=cuda)
    wide[..., 1:-1] = dev(pred, cuda)
    leaf = wide[..., 1:-1].detach().requires_grad_(True)                  # a non-contiguous leaf
    assert not leaf.is_contiguous()
    l3 = l1_misfit(leaf, t, m)
    l3.backward(gout)
    assert bits_equal(host(l3), want_loss) and bits_equal(host(leaf.grad), want)

    p4 = dev(pred, cuda).requires_grad_(True)                             # float64 y
    l4 = l1_misfit(p4, t.double(), m)
    l4.backward(gout)
    assert bits_equal(host(l4), want_loss) and bits_equal(host(p4.grad), want)

    p5 = dev(pred, cuda).double().requires_grad_(True)                    # float64 pred that requires grad
    l5 = l1_misfit(p5, t, m)
    l5.backward(gout)
    assert bits_equal(host(l5), want_loss)
    assert p5.grad.dtype == torch.float64 and p5.grad.shape == SMALL
    assert np.array_equal(host(p5.grad), want.astype(np.float64))


def test_l1_sharded_nobs_override(cuda):
    """The nobs= override of l1_misfit (a shot shard normalised by the survey's observation count) and
    LossCalculator.global_nobs: loss = fl32(loss_local fl32(nobs_local / nobs_global)) bit for bit, the
    backward is the mixed formula with the global count bit for bit, and both are the fp64 S / nobs_global
    and its autograd within 5 u (the local loss 3, the ratio, the product) and 2 u."""
    from red_diffeq.core.losses import LossCalculator, l1_misfit
    from red_diffeq.regularization.base import RegularizationMethod
    pred, y, mask = R.k5_inputs(SMALL, "columns")
    loc, nobs_loc = R.l1_mixed(pred, y, mask)
    nobs_glob = (nobs_loc * np.float32(3) + np.array([0, 140, 7], np.float32)).astype(np.float32)
    gout = np.array(R.K5_GOUT, np.float32)
    want = loc * (nobs_loc / nobs_glob)
    assert want.dtype == np.float32
    full, full_nobs, full_grad = R.l1_full(pred, y, mask, gout)
    scale = (full_nobs / nobs_glob.astype(np.float64))
    calc = LossCalculator(RegularizationMethod("tv"))
    for how in ("l1_misfit", "LossCalculator"):
        p = dev(pred, cuda).requires_grad_(True)
        if how == "l1_misfit":
            loss = l1_misfit(p, dev(y, cuda), dev(mask, cuda), nobs=dev(nobs_glob, cuda))
        else:
            calc.global_nobs = dev(nobs_glob, cuda)
            loss = calc.observation_loss(p, dev(y, cuda), dev(mask, cuda))
        loss.backward(dev(gout, cuda))
        got, grad = host(loss), host(p.grad)
        assert bits_equal(got, want), (how, got, want)
        assert bits_equal(grad, R.l1_backward_mixed(pred, y, mask, nobs_glob, gout)), how
        assert (np.abs(got.astype(np.float64) - full * scale) <= 5 * U * full * scale).all()
        ref = full_grad * scale.reshape(3, 1, 1, 1)
        assert (np.abs(grad.astype(np.float64) - ref) <= 2 * U * np.abs(ref)).all()
    calc.global_nobs = None                                               # unsharded: the local count
    got = host(calc.observation_loss(dev(pred, cuda), dev(y, cuda), dev(mask, cuda)))
    assert bits_equal(got, host(torch.ops.red_diffeq.l1_misfit(dev(pred, cuda), dev(y, cuda), dev(mask, cuda))[0]))
    assert R.ulps(got, loc).max() <= 1


# ------------------------------------------------------------------------------------------- K6
def entry(kind):
    from red_diffeq.regularization.benchmark import tikhonov_loss, total_variation_loss
    return total_variation_loss if kind == R.TV else tikhonov_loss


@pytest.mark.parametrize("kind", [R.TV, R.L2], ids=["tv", "l2"])
@pytest.mark.parametrize("H,W,B,inp", R.k6_cases())
def test_smooth_forward_and_backward_per_cell(cuda, H, W, B, inp, kind):
    """K6 at every shape of loss_refs.K6_SHAPES (what each is for: loss_refs.K6_WHY), B in {1, 3} and 25 at
    72 x 72, every input kind, the spike at every cell of loss_refs.spike_cells in turn.  Forward: 1 ulp
    against the mixed reference; against fp64 TV 4 u, Tikhonov 5 u relative.  Backward, every cell:
    |got - ref| <= k u M with k = 4 (TV: gout / N, three additions) or 6 (Tikhonov: gout / N, d, the
    product, three additions), exactly 0 where all the cell's terms are 0; the largest ratio is reported
    for corner, edge and interior cells separately.  A constant model gives 0 everywhere."""
    kf, kb = (4, 4) if kind == R.TV else (5, 6)
    gout = R.k6_gout(B)
    cls = np.broadcast_to(R.cell_classes(H, W), (B, 1, H, W))
    d_loss, rel, by_class = 0, 0.0, [0.0, 0.0, 0.0]
    for label, mu in R.k6_variants(H, W, B, inp):
        x = dev(mu, cuda).requires_grad_(True)
        loss_t = entry(kind)(x)
        loss_t.backward(dev(gout, cuda))
        assert loss_t.dtype == torch.float32 and loss_t.shape == (B,)
        assert x.grad.dtype == torch.float32 and x.grad.shape == mu.shape
        loss, grad = host(loss_t), host(x.grad)
        assert bits_equal(host(torch.ops.red_diffeq.smooth_reg(x.detach(), kind)), loss)
        ref = R.smooth_mixed(mu, kind)
        full, full_grad = R.smooth_full(mu, kind, gout)
        d_loss = max(d_loss, int(R.ulps(loss, ref).max()))
        assert d_loss <= 1, (label, loss, ref)
        assert (np.abs(loss.astype(np.float64) - full) <= kf * U * full).all(), (label, loss, full)
        rel = max(rel, float(np.max(np.abs(loss.astype(np.float64) - full) / np.where(full > 0, full, 1.0))))
        M = R.smooth_term_sum(mu, kind, gout)
        err = np.abs(grad.astype(np.float64) - full_grad)
        dead = M == 0
        assert (grad[dead] == 0).all() and (full_grad[dead] == 0).all(), label
        ratio = np.where(dead, 0.0, err / np.where(dead, 1.0, kb * U * M))
        for c in R.classes_possible(H, W):
            by_class[c] = max(by_class[c], float(ratio[cls == c].max()))
        if ratio.max() > 1.0:
            w = np.unravel_index(np.argmax(ratio), ratio.shape)
            raise AssertionError((label, w, R.CLASS_NAMES[cls[w]], float(grad[w]), float(full_grad[w]), float(ratio.max())))
        if inp == "constant":
            assert not loss.any() and not grad.any()
    case = f"{H}x{W},B={B},{inp},{'tv' if kind == R.TV else 'l2'}"
    print(f"K6 {case}: fwd {d_loss} ulp vs mixed, {rel / U:.3f} u vs fp64 (bar {kf}); bwd err / bar " +
          ", ".join(f"{R.CLASS_NAMES[c]} {by_class[c]:.3f}" for c in R.classes_possible(H, W)))
    record_margin("smooth_forward_ulps_vs_mixed", case, d_loss, 1)
    record_margin("smooth_forward_rel_vs_fp64", case, rel, kf * U)
    for c in R.classes_possible(H, W):
        record_margin("smooth_backward_err_over_bar_" + R.CLASS_NAMES[c], case, by_class[c], 1.0)


@pytest.mark.parametrize("kind", [R.TV, R.L2], ids=["tv", "l2"])
def test_smooth_expanded_upstream_gradient(cuda, kind):
    """.sum().backward() hands k_smooth_bwd's wrapper an expanded stride-0 gout: the gradient is the one of
    a contiguous gout of ones bit for bit, and within the per-cell bar of fp64 autograd."""
    mu = R.k6_input(16, 17, 3, "uniform")
    a, b = dev(mu, cuda).requires_grad_(True), dev(mu, cuda).requires_grad_(True)
    entry(kind)(a).sum().backward()
    entry(kind)(b).backward(torch.ones(3, device=cuda))
    assert bits_equal(host(a.grad), host(b.grad))
    ones = np.ones(3, np.float32)
    _, ref = R.smooth_full(mu, kind, ones)
    bar = (4 if kind == R.TV else 6) * U * R.smooth_term_sum(mu, kind, ones)
    assert (np.abs(host(a.grad).astype(np.float64) - ref) <= bar).all()


@pytest.mark.parametrize("H,W", [(1, 9), (9, 1), (1, 1)])
def test_smooth_rejects_a_single_row_or_column(cuda, H, W):
    """H = 1 or W = 1 has an empty difference set (the reference's mean of nothing): the C entry points
    return an error before any launch, so the output buffers keep their contents, and the ops and the
    Python entry points raise."""
    from red_diffeq import _hip
    mu = torch.rand(2, 1, H, W, device=cuda)
    gout = torch.ones(2, device=cuda)
    for kind in (R.TV, R.L2):
        loss = torch.full((2,), 7.0, device=cuda)
        grad = torch.full((2, 1, H, W), 7.0, device=cuda)
        L, st = _hip.lib(), _hip.stream_of(mu)
        assert L.rdq_smooth_reg_forward(kind, 2, H, W, _hip.ptr(mu), _hip.ptr(loss), st) != 0
        assert L.rdq_smooth_reg_backward(kind, 2, H, W, _hip.ptr(mu), _hip.ptr(gout), _hip.ptr(grad), st) != 0
        torch.cuda.synchronize()
        assert (loss == 7.0).all() and (grad == 7.0).all()
        with pytest.raises(RuntimeError, match="rdq_smooth_reg_forward"):
            torch.ops.red_diffeq.smooth_reg(mu, kind)
        with pytest.raises(RuntimeError, match="rdq_smooth_reg_backward"):
            torch.ops.red_diffeq.smooth_reg_backward(mu, gout, kind)
        with pytest.raises(RuntimeError, match="rdq_smooth_reg_forward"):
            entry(kind)(mu.clone().requires_grad_(True))
    ok = dev(R.k6_input(2, 2, 1, "checker"), cuda)                        # and the next valid call is right
    assert host(entry(R.TV)(ok)).tolist() == [4.0]
