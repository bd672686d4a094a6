"""The serial-tail kernels of csrc/loop.hip element by element against fp64: K11, the fused Adam + clamp
(k_adam), one step from a prepared state through torch.ops.red_diffeq.adam_clamp_, and K12, the fused MAE /
RMSE / SSIM (k_metrics_tile, k_metrics_final), through torch.ops.red_diffeq.metrics and the C ABI.  Case
tables, inputs, references and the derivation of every bar are tests/loop_refs.py; tests/test_loop_refs_host.py
checks them on the CPU, with the branch each size is for.

The bars are rounding counts (u = 2^-24), never measured from the kernels:

K11  per element bar_m = 2u (|m| + |g|), bar_v = 3u v', bar_p = 2u |p'| + |step_size| bar_m / den +
     |upd| (4u + bar_v / (2 v')) against torch's multi-tensor formula in fp64.  At the default betas the
     kernel's 1 - beta (fp32 from the fp32 beta) is not torch's (double, then fp32): the bars carry the
     exactly derived allowance |c2_k - c2_t| g^2, |c1_k - c1_t| |g - m| and what they do to p, recorded
     under its own name (adam_constant_allowance_share_*).  Elements whose fp64 pre-clamp value is within
     4 bar_p of a clamp bound are not compared in p (at most 1 %, asserted on the CPU); they must lie inside
     the bounds.  Everything else about the clamp, the guard word and rows that must not move is bitwise.
K12  per model against the mixed reference before its final cast: MAE and RMSE 2u relative, SSIM
     u |ref| + n 2^-52 mean |map|; the distance to the full reference (the reference's formulas in fp64)
     is recorded and held to that bar plus the 8u the two references may differ by plus the window
     allowance: rdq_metrics' window sum is one ulp under the reference's, which moves the SSIM of a smooth
     pair by up to 81u; loop_refs.window_allowance computes that exactly per case from the two windows, and
     it is recorded under its own name (metrics_window_allowance_share_of_full_bar).  Strides, workspace
     contents, batching and repetition are bitwise."""
import ctypes

import numpy as np
import pytest
import torch

import loop_refs as R
from conftest import record_margin
from test_gpu_fwi import bits_equal

pytestmark = pytest.mark.gpu

U = R.U


@pytest.fixture(autouse=True, scope="module")
def registered_ops():
    import red_diffeq.ops  # noqa: F401  (registers torch.ops.red_diffeq.*)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


def ratio(err, bar):
    """max err / bar; a zero bar asks for a zero error."""
    if err.size == 0:
        return 0.0
    return float(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)).max())


# ------------------------------------------------------------------------------------------- K11
def adam_step(cuda, p, g, m, v, scalars, clamp, guard=None):
    """One launch of k_adam on copies of the state: (p, m, v) as numpy."""
    P, G, M, V = (dev(a, cuda) for a in (p, g, m, v))
    lo, hi = clamp if clamp is not None else (0.0, 0.0)
    torch.ops.red_diffeq.adam_clamp_(P, G, M, V, *scalars, clamp is not None, float(lo), float(hi), guard)
    assert bits_equal(host(G), g)
    return host(P), host(M), host(V)


@pytest.mark.parametrize("n,b,t,c", R.adam_cases())
def test_adam_step_per_element(cuda, n, b, t, c):
    """One step at every beta pair x t x clamp at 4099 elements and at every size of loop_refs.adam_sizes
    (1, 255, 256, 257, one full sweep, a second sweep of one element, a third of three): p, m' and v' of
    every element within their bars; rows with g = m = v = 0 keep p bit for bit, on a clamp bound too; rows
    with g = v = 0, m != 0 and every element whose fp64 value is past a bound land on the bound exactly."""
    betas, clamp = R.BETAS[b], R.CLAMPS[c]
    p, g, m, v, still, jump = R.adam_inputs(n, t, clamp)
    sc = R.adam_scalars(betas, t)
    ref = R.adam_ref(p, g, m, v, *sc, clamp)
    gp, gm, gv = adam_step(cuda, p, g, m, v, sc, clamp)
    rp, rm, rv = R.adam_errors(gp, gm, gv, ref)
    case = f"n={n},betas={betas},t={t},clamp={clamp}"
    print(f"K11 {case}: err / bar p {rp:.3f}, m {rm:.3f}, v {rv:.3f}; {int((~ref['keep']).sum())} not compared")
    for name, r in (("p", rp), ("m", rm), ("v", rv)):
        record_margin(f"adam_{name}_err_over_bar", case, r, 1.0)
    if b == 2:
        for name in ("p", "m", "v"):
            bar, alw = ref["bar_" + name], ref["alw_" + name]
            record_margin(f"adam_constant_allowance_share_{name}", case, ratio(alw, bar), 1.0)
    assert max(rp, rm, rv) <= 1.0, (case, rp, rm, rv)
    assert bits_equal(gp[still], p[still]) and not gm[still].any() and not gv[still].any()
    if clamp is not None:
        lo, hi = np.float32(clamp[0]), np.float32(clamp[1])
        assert (gp >= lo).all() and (gp <= hi).all()
        below, above = ref["keep"] & (ref["pre"] < lo), ref["keep"] & (ref["pre"] > hi)
        assert (gp[below] == lo).all() and (gp[above] == hi).all()
        assert below[jump[m[jump] > 0]].all() and above[jump[m[jump] < 0]].all()
        if n >= R.MID:
            assert below.any() and above.any() and (ref["keep"] & ~below & ~above).sum() > n // 2


@pytest.mark.parametrize("n,b,t", [(R.MID, 0, 10), (R.MID, 1, 2), (R.MID, 2, 1000), ("2cap+3", 2, 2)])
@pytest.mark.parametrize("c", [0, 1])
def test_adam_clamp_is_the_clip_of_the_unclamped_step(cuda, n, b, t, c):
    """On finite inputs the clamped step is np.clip of the unclamped step bit for bit, in p; m' and v' do
    not depend on the clamp."""
    n = R.adam_sizes().get(n, n)
    clamp = R.CLAMPS[c]
    p, g, m, v, _, _ = R.adam_inputs(n, t, clamp)
    sc = R.adam_scalars(R.BETAS[b], t)
    fp, fm, fv = adam_step(cuda, p, g, m, v, sc, None)
    cp, cm, cv = adam_step(cuda, p, g, m, v, sc, clamp)
    assert np.isfinite(fp).all()
    assert bits_equal(cp, np.clip(fp, np.float32(clamp[0]), np.float32(clamp[1])))
    assert bits_equal(cm, fm) and bits_equal(cv, fv)
    assert (fp < clamp[0]).any() and (fp > clamp[1]).any()


@pytest.mark.parametrize("n,b,c", [(R.MID, 0, 0), (R.MID, 1, 0), (R.MID, 2, 0), (R.MID, 2, 2), ("2cap+3", 2, 1)])
def test_adam_keeps_nan_and_inf_gradients_visible(cuda, n, b, c):
    """NaN and +inf gradients at loop_refs.nonfinite_positions (the ends of the first block and of the
    first sweep, the middle, the last elements): p is NaN at exactly those positions, clamped or not, and
    m' and v' are NaN (a NaN gradient) or +inf / NaN as torch's lerp and addcmul leave them (+inf), exactly
    as torch.optim.Adam + clamp_ (asserted on the CPU against torch itself).  Every other element stays
    within its bar.  fminf(fmaxf(p, lo), hi) alone returned lo for a NaN p: a diverged inversion showed a
    model of vmin."""
    n = R.adam_sizes().get(n, n)
    t, clamp = 10, R.CLAMPS[c]
    p, g, m, v, _, _ = R.adam_inputs(n, t, clamp)
    nan_at, inf_at = R.nonfinite_positions(n)
    g = g.copy()
    g[nan_at], g[inf_at] = np.nan, np.inf
    sc = R.adam_scalars(R.BETAS[b], t)
    ref = R.adam_ref(p, g, m, v, *sc, clamp)
    gp, gm, gv = adam_step(cuda, p, g, m, v, sc, clamp)
    bad = np.zeros(n, bool)
    bad[nan_at] = bad[inf_at] = True
    assert np.isnan(ref["p"][bad]).all() and np.isfinite(ref["p"][~bad]).all()
    assert np.array_equal(np.isnan(gp), bad), (np.flatnonzero(bad), gp[bad])
    for got, want in ((gm, ref["m"]), (gv, ref["v"])):
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
        assert np.array_equal(~np.isfinite(got), bad)
    ok = dict((k, a[~bad]) for k, a in ref.items())
    rp, rm, rv = R.adam_errors(gp[~bad], gm[~bad], gv[~bad], ok)
    assert max(rp, rm, rv) <= 1.0, (rp, rm, rv)


@pytest.mark.parametrize("n", [R.MID, "cap+1"])
def test_adam_guard_word(cuda, n):
    """Guard words 1 and -1 (any non-zero bit pattern) leave p, m and v bit for bit as they were; guard word
    0 gives the unguarded step bit for bit."""
    n = R.adam_sizes().get(n, n)
    clamp = R.CLAMPS[0]
    p, g, m, v, _, _ = R.adam_inputs(n, 10, clamp)
    sc = R.adam_scalars(R.BETAS[2], 10)
    want = adam_step(cuda, p, g, m, v, sc, clamp)
    assert not bits_equal(want[0], p) and not bits_equal(want[1], m) and not bits_equal(want[2], v)
    for word in (1, -1):
        got = adam_step(cuda, p, g, m, v, sc, clamp, torch.tensor([word], dtype=torch.int32, device=cuda))
        assert bits_equal(got[0], p) and bits_equal(got[1], m) and bits_equal(got[2], v), word
    got = adam_step(cuda, p, g, m, v, sc, clamp, torch.zeros(1, dtype=torch.int32, device=cuda))
    assert all(bits_equal(a, b) for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------- K12
def run_metrics(cuda, pred, tru):
    out = torch.ops.red_diffeq.metrics(dev(pred, cuda), dev(tru, cuda))
    assert out.dtype == torch.float32 and out.shape == (3, pred.shape[0])
    return host(out)


def metric_ratios(got, pred, tru):
    """(err / bar of MAE, RMSE, SSIM against the mixed reference, |SSIM - full| over its bar, the share of
    that bar that is the window allowance), the worst model."""
    n = pred.shape[2] * pred.shape[3]
    mae, rmse, ssim, map_abs = R.metrics_mixed(pred, tru)
    bars = R.metric_bars(mae, rmse, ssim, map_abs, n)
    g = got.astype(np.float64)
    r = [ratio(np.abs(g[k] - want), bar) for k, (want, bar) in enumerate(zip((mae, rmse, ssim), bars))]
    full = R.metrics_full(pred, tru)[2]
    alw = R.window_allowance(pred, tru)
    full_bar = bars[2] + 8 * U + alw
    return r + [ratio(np.abs(g[2] - full), full_bar), ratio(alw, full_bar)]


NAMES = ("mae_vs_mixed_err_over_bar", "rmse_vs_mixed_err_over_bar", "ssim_vs_mixed_err_over_bar",
         "ssim_vs_full_err_over_bar", "window_allowance_share_of_full_bar")


@pytest.mark.parametrize("H,W,B,kind", R.metric_cases())
def test_metrics_per_model(cuda, H, W, B, kind):
    """K12 at every shape of loop_refs.metric_shapes (a pixel, under the window, one tile, a second tile of
    one row / column, 2 x 3 tiles, the product's 70 x 70, one row of 256 and of 257 tiles: the second sweep
    of k_metrics_final), B in {1, 3}, every input kind.  Against the mixed reference: MAE and RMSE 2u
    relative, SSIM u |ref| + n 2^-52 mean |map|; against the full one: that plus 8u plus the window
    allowance.  Identical images give MAE = RMSE = 0 and SSIM = 1.0f exactly."""
    pred, tru = R.metric_inputs(H, W, B, kind)
    got = run_metrics(cuda, pred, tru)
    r = metric_ratios(got, pred, tru)
    case = f"{H}x{W},B={B},{kind}"
    print(f"K12 {case}: err / bar MAE {r[0]:.3f}, RMSE {r[1]:.3f}, SSIM {r[2]:.3f} vs mixed, SSIM {r[3]:.3f} vs full "
          f"(window allowance {r[4]:.3f} of that bar)")
    for name, x in zip(NAMES, r):
        record_margin("metrics_" + name, case, x, 1.0)
    assert max(r[:4]) <= 1.0, (case, r, got)
    if kind == "identical":
        assert not got[0].any() and not got[1].any() and (got[2] == np.float32(1)).all()
    if kind == "constants":
        assert (got[0] == 2).all() and (got[1] == 2).all()


def test_metrics_one_bumped_pixel_at_the_seams(cuda):
    """pred = the layered truth but for one pixel raised by 0.5, at each pixel of loop_refs.seam_pixels in
    turn (image corners, both sides of a tile corner, HALO before and after a seam in each direction, where
    the pixel's window starts or stops reaching across): the bars of test_metrics_per_model.  Each bump
    moves the SSIM by more than a thousand bars (asserted on the CPU), a tile that misses it by as much."""
    mt = R.kernel_constants()[0]
    H, W = 2 * mt, 2 * mt + 1
    _, tru = R.metric_inputs(H, W, 1, "layered")
    worst = np.zeros(5)
    for name, (y, x) in R.seam_pixels(H, W).items():
        pred = tru.copy()
        pred[0, 0, y, x] += np.float32(0.5)
        r = metric_ratios(run_metrics(cuda, pred, tru), pred, tru)
        assert max(r[:4]) <= 1.0, (name, r)
        worst = np.maximum(worst, r)
    for name, x in zip(NAMES, worst):
        record_margin("metrics_" + name, f"{H}x{W},seams", x, 1.0)


def test_metrics_strided_views_bitwise(cuda):
    """Every view gives the result of its contiguous copy bit for bit: the engine's interior view of a
    padded model, a channel slice [:, 1:2] of three channels, a transposed view (s3 != 1), a model expanded
    over the batch (s0 = 0), and a non-contiguous true_norm."""
    H, W, B = 33, 45, 3
    pred, tru = R.metric_inputs(H, W, B, "uniform")
    p, t = dev(pred, cuda), dev(tru, cuda)
    op = torch.ops.red_diffeq.metrics
    want = host(op(p, t))
    assert max(metric_ratios(want, pred, tru)[:4]) <= 1.0

    padded = torch.full((B, 1, H + 2, W + 2), 7.0, device=cuda)
    padded[:, :, 1:-1, 1:-1] = p
    view = padded[:, :, 1:-1, 1:-1]
    assert not view.is_contiguous() and bits_equal(host(op(view, t)), want)

    three = torch.full((B, 3, H, W), 7.0, device=cuda)
    three[:, 1:2] = p
    view = three[:, 1:2]
    assert view.stride(0) == 3 * H * W and bits_equal(host(op(view, t)), want)

    view = p.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert view.stride(3) == H and view.stride(2) == 1 and bits_equal(host(op(view, t)), want)

    view = p[1:2].expand(B, 1, H, W)
    assert view.stride(0) == 0
    assert bits_equal(host(op(view, t)), host(op(view.contiguous(), t)))
    assert bits_equal(host(op(view, t))[:, 1], want[:, 1])

    wide = torch.full((B, 1, H, W + 3), 7.0, device=cuda)
    wide[..., :W] = t
    view = wide[..., :W]
    assert not view.is_contiguous() and bits_equal(host(op(p, view)), want)


@pytest.mark.parametrize("H,W", [(70, 70), (1, "second sweep")])
def test_metrics_workspace_batch_and_repeat_bitwise(cuda, H, W):
    """Through the C ABI with the workspace and the output filled with NaN first the result is the op's bit
    for bit (every partial the final pass reads is written by the tile pass); model b inside a batch of
    three equals model b alone; a second run equals the first."""
    from red_diffeq import _hip
    if W == "second sweep":
        H, W = R.metric_shapes()[-1]
    B = 3
    pred, tru = R.metric_inputs(H, W, B, "layered")
    p, t = dev(pred, cuda), dev(tru, cuda)
    want = host(torch.ops.red_diffeq.metrics(p, t))
    assert bits_equal(host(torch.ops.red_diffeq.metrics(p, t)), want)
    L = _hip.lib()
    nbytes = int(L.rdq_metrics_ws_bytes(B, H, W))
    assert nbytes % 8 == 0 and nbytes >= B * R.metric_tiles(H, W) * 3 * 8
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=cuda)
    out = torch.full((3, B), float("nan"), device=cuda)
    strides = (ctypes.c_int64 * 4)(*p.stride())
    assert L.rdq_metrics(B, H, W, _hip.ptr(p), strides, _hip.ptr(t), _hip.ptr(out), _hip.ptr(ws), _hip.stream_of(p)) == 0
    assert bits_equal(host(out), want)
    for b in range(B):
        alone = host(torch.ops.red_diffeq.metrics(p[b:b + 1], t[b:b + 1]))
        assert bits_equal(alone[:, 0], want[:, b]), b


def test_metrics_rejects_what_it_would_misread(cuda):
    """The op checks what adam_clamp_ checks: fp32, (B, 1, H, W), one device, as many elements in true_norm
    as in pred.  Only with inputs that an unchecked kernel would still have read inside their buffers."""
    op = torch.ops.red_diffeq.metrics
    p = torch.zeros(2, 1, 12, 13, device=cuda)
    t = torch.zeros(2, 1, 12, 13, device=cuda)
    assert host(op(p, t))[2].tolist() == [1.0, 1.0]
    bad = (RuntimeError, ValueError)
    with pytest.raises(bad, match="metrics: pred and true_norm must be fp32"):
        op(p.double(), t)
    with pytest.raises(bad, match="metrics: pred and true_norm must be fp32"):
        op(p, t.double())
    with pytest.raises(bad, match="metrics: true_norm must have the elements of pred"):
        op(p, torch.zeros(2, 1, 13, 13, device=cuda))
    with pytest.raises(bad, match=r"metrics: pred must be \(B, 1, H, W\)"):
        op(torch.zeros(2, 2, 12, 13, device=cuda), torch.zeros(2, 2, 12, 13, device=cuda))
    with pytest.raises(bad, match=r"metrics: pred must be \(B, 1, H, W\)"):
        op(torch.zeros(2, 2, 12, 13, device=cuda), t)
    assert host(op(p, t))[2].tolist() == [1.0, 1.0]
