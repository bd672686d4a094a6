"""The references, case tables and inputs of tests/test_gpu_loop_tail.py (tests/loop_refs.py), checked on the
CPU: the K11 bars against a numpy fp32 emulation of k_adam's statements and against torch.optim.Adam itself,
the K12 mixed reference against the full one, every case against the conditions the GPU tests rely on, and
CosineLR against torch's scheduler."""
import math

import numpy as np
import pytest
import torch

import loop_refs as R

U = R.U


# ------------------------------------------------------------------------------------------- tables
def test_sizes_at_the_current_constants():
    """With MT = 32, WIN = 11, blocks of 256 and a cap of 2048 the tables are the ones the sizes were chosen
    as; with other constants the sizes move and the branch tests below speak."""
    if R.kernel_constants() != (32, 11, 256, 2048, 256):
        return
    assert list(R.adam_sizes().values()) == [1, 255, 256, 257, 524288, 524289, 1048579]
    assert R.metric_shapes() == ((1, 1), (7, 9), (11, 11), (32, 32), (33, 32), (32, 33), (64, 65), (70, 70),
                                 (1, 8192), (1, 8193))


def test_sizes_hit_their_branches():
    _, win, blk, cap, fblk = R.kernel_constants()
    s = R.adam_sizes()
    assert [R.adam_sweeps(n) for n in s.values()] == [1, 1, 1, 1, 1, 2, 3]
    assert R.adam_sweeps(R.MID) == 1 and R.MID % blk not in (0, 1) and R.MID > blk
    tiles = [R.metric_tiles(H, W) for H, W in R.metric_shapes()]
    assert tiles == [1, 1, 1, 1, 2, 2, 6, 9, fblk, fblk + 1]
    assert [H < win or W < win for H, W in R.metric_shapes()[:3]] == [True, True, False]
    cases = R.adam_cases()
    assert len(set(cases)) == len(cases) == 36 + 21
    for n in (s["cap+1"], s["2cap+3"]):      # the multi-sweep sizes see every beta pair, two clamps or more
        mine = [c for c in cases if c[0] == n]
        assert {c[1] for c in mine} == {0, 1, 2} and len({c[3] for c in mine}) >= 2
    assert {(c[2], c[3]) for c in cases if c[0] == R.MID} == {(t, c) for t in R.STEPS for c in range(3)}
    assert len(R.metric_cases()) == 10 * 2 * 5


def test_constant_conventions():
    """The dyadic pairs have one constant under either convention; the default pair has the two deviations
    DESIGN.md states (c2 1.29e-5, c1 2.2e-7 relative), and only (0.25, 0.75) takes lerp's other branch."""
    for i, betas in enumerate(R.BETAS):
        c1t, c2t, c1k, c2k = R.adam_constants(*betas)
        if i < 2:
            assert (c1t, c2t) == (c1k, c2k) == (1 - betas[0], 1 - betas[1])
        assert (abs(c1k) >= 0.5) == (i == 1) == (abs(c1t) >= 0.5)
    c1t, c2t, c1k, c2k = R.adam_constants(0.9, 0.999)
    assert (np.float32(c2k), np.float32(c2t)) == (np.float32(0.00099998713), np.float32(0.00100000005))
    assert 1.28e-5 < abs(c2k - c2t) / c2t < 1.30e-5 and 2.1e-7 < abs(c1k - c1t) / c1t < 2.3e-7
    # torch itself: lerp_ and addcmul_ with the double 1 - beta on an fp32 tensor use c1_t and c2_t
    g = torch.tensor([0.37], dtype=torch.float32)
    assert torch.zeros(1).lerp_(g, 1 - 0.9).item() == float(np.float32(c1t) * g.numpy()[0])
    assert torch.zeros(1).addcmul_(g, g, value=1 - 0.999).item() == float(np.float32(c2t) * (g * g).numpy()[0])


# ------------------------------------------------------------------------------------------- K11
def torch_adam(p, g, m, v, betas, t, clamp):
    """torch.optim.Adam at step t from the state (m, v), then clamp_: (p, m, v) fp32."""
    q = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([q], lr=R.LR, betas=betas, eps=R.EPS)
    opt.state[q] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.from_numpy(m.copy()),
                        exp_avg_sq=torch.from_numpy(v.copy()))
    q.grad = torch.from_numpy(g.copy())
    opt.step()
    if clamp is not None:
        with torch.no_grad():
            q.clamp_(*clamp)
    st = opt.state[q]
    assert st["step"].item() == t
    return q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("n,b,t,c", [x for x in R.adam_cases() if x[0] <= R.MID])
def test_adam_reference_is_torch_adam(n, b, t, c):
    """The fp64 reference against torch.optim.Adam (fp32, CPU) on the same state: torch is inside the bars
    without any allowance, since the reference uses torch's constants."""
    p, g, m, v, _, _ = R.adam_inputs(n, t, R.CLAMPS[c])
    ref = R.adam_ref(p, g, m, v, *R.adam_scalars(R.BETAS[b], t), R.CLAMPS[c])
    tight = dict(ref, bar_m=ref["bar_m"] - ref["alw_m"], bar_v=ref["bar_v"] - ref["alw_v"],
                 bar_p=ref["bar_p"] - ref["alw_p"])
    rp, rm, rv = R.adam_errors(*torch_adam(p, g, m, v, R.BETAS[b], t, R.CLAMPS[c]), tight)
    assert max(rp, rm, rv) <= 1.0, (rp, rm, rv)


@pytest.mark.parametrize("b", range(len(R.BETAS)))
def test_adam_emulation_within_bars(b):
    """k_adam's statements in numpy fp32 (every operation rounded) over 2 M elements at t in {1, 2, 10,
    1000}: inside bar_m, bar_v and bar_p, the default betas only with the allowance, and the allowance is
    the smaller part of the bar everywhere but in v."""
    worst = np.zeros(3)
    for t in R.STEPS:
        p, g, m, v, _, _ = R.adam_inputs(500_000, t, None, "emu")
        sc = R.adam_scalars(R.BETAS[b], t)
        ref = R.adam_ref(p, g, m, v, *sc)
        got = R.adam_emulate(p, g, m, v, *sc)
        worst = np.maximum(worst, R.adam_errors(*got, ref))
        if b < 2:
            assert not ref["alw_m"].any() and not ref["alw_v"].any() and not ref["alw_p"].any()
        else:
            live = g != 0
            assert (ref["alw_v"][live] > 0).all() and (ref["alw_p"] <= ref["bar_p"]).all()
            # 2.2e-8 |g - m| beside 2u (|g| + |m|) = 1.19e-7 (|g| + |m|): at most 0.16 of their sum
            assert (ref["alw_m"] <= 0.16 * ref["bar_m"]).all()
    print(f"K11 emulation {R.BETAS[b]}: err / bar p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}")
    assert (worst <= 1.0).all(), worst


@pytest.mark.parametrize("n,b,t,c", R.adam_cases())
def test_adam_case_conditions(n, b, t, c):
    """The inputs are what the builder says, at most 1 % of the elements lie too close to a clamp bound to
    be compared, the rows that must not move do not move in the reference, and the rows with g = v = 0,
    m != 0 land on a bound exactly."""
    clamp = R.CLAMPS[c]
    p, g, m, v, still, jump = R.adam_inputs(n, t, clamp)
    assert all(a.dtype == np.float32 and a.shape == (n,) for a in (p, g, m, v))
    lo, hi = clamp if clamp is not None else (-1.0, 1.0)
    assert (p >= lo).all() and (p <= hi).all() and (v >= 0).all()
    ag = np.abs(g[g != 0])
    assert ((ag >= np.float32(1e-6)) & (ag <= 1)).all()
    assert ((v[v != 0] >= np.float32(1e-14)) & (v[v != 0] <= np.float32(1e-2))).all()
    if t == 1:
        assert not m.any() and not v.any() and jump.size == 0
    if n >= 255:
        assert still.size >= 3 and (g == 0).sum() > still.size and (t == 1 or jump.size >= 2)
        assert (p[still] == lo).any() and (p[still] == hi).any()
    assert not (g[still].any() or m[still].any() or v[still].any())
    assert not (g[jump].any() or v[jump].any()) and (m[jump] != 0).all()
    if n >= 16:      # a step that skips the last sweep (one or three elements) leaves m and v wrong there
        assert g[-4:].all() and not np.isin(np.arange(n - 4, n), np.union1d(still, jump)).any()
        assert {0, 1} <= set(still.tolist()) and (t == 1 or 2 in jump)
    ref = R.adam_ref(p, g, m, v, *R.adam_scalars(R.BETAS[b], t), clamp)
    assert np.isfinite(ref["pre"]).all() and (ref["bar_p"] >= 0).all()
    assert (~ref["keep"]).sum() <= 0.01 * n
    assert ref["keep"][still].all() and np.array_equal(ref["p"][still], p[still].astype(np.float64))
    if clamp is not None:
        assert ref["keep"][jump].all() and np.isin(ref["p"][jump], clamp).all()
        assert np.array_equal(ref["p"][jump] == lo, m[jump] > 0)      # step_size < 0: m > 0 goes down


@pytest.mark.parametrize("b", range(len(R.BETAS)))
def test_adam_nonfinite_pattern_is_torchs(b):
    """What the GPU test expects at NaN / +inf gradients is what torch.optim.Adam + clamp_ leave: p NaN at
    both; m and v NaN at a NaN gradient and +inf (or, through lerp's other branch, NaN) at +inf."""
    n, t, clamp = R.MID, 10, (-1.0, 1.0)
    p, g, m, v, _, _ = R.adam_inputs(n, t, clamp)
    nan_at, inf_at = R.nonfinite_positions(n)
    assert nan_at.size >= 3 and inf_at.size >= 3 and not np.intersect1d(nan_at, inf_at).size
    g = g.copy()
    g[nan_at], g[inf_at] = np.nan, np.inf
    ref = R.adam_ref(p, g, m, v, *R.adam_scalars(R.BETAS[b], t), clamp)
    tp, tm, tv = torch_adam(p, g, m, v, R.BETAS[b], t, clamp)
    ep, em, ev = R.adam_emulate(p, g, m, v, *R.adam_scalars(R.BETAS[b], t), clamp)
    bad = np.zeros(n, bool)
    bad[nan_at] = bad[inf_at] = True
    for got in ((tp, tm, tv), (ep, em, ev)):
        for a, r in zip(got, (ref["p"], ref["m"], ref["v"])):
            assert np.array_equal(np.isnan(a), np.isnan(r)) and np.array_equal(np.isposinf(a), np.isposinf(r))
            assert np.array_equal(~np.isfinite(a), bad)
    assert np.isnan(ref["p"][bad]).all() and np.isnan(ref["m"][nan_at]).all() and np.isnan(ref["v"][nan_at]).all()
    assert np.isposinf(ref["v"][inf_at]).all()
    assert (np.isnan(ref["m"][inf_at]) if b == 1 else np.isposinf(ref["m"][inf_at])).all()


# ------------------------------------------------------------------------------------------- K12
def test_window_against_the_references():
    """The kernel's window (the taps over their sequential fp32 sum) against ssim.py:gaussian's (over
    torch's sum, the rounded exact sum, one ulp more): nine weights are one ulp above the reference's, none
    below.  On a smooth pair that alone moves the mixed SSIM by more than the 8u the two references may
    differ by, which is why the GPU test carries it as a named allowance."""
    ref, mine = R.reference_window(), R.window()
    assert (mine.view(np.int32) - ref.view(np.int32)).tolist() == [1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1]
    taps = np.array([math.exp(-(k - 5) ** 2 / 4.5) for k in range(11)], np.float32)
    assert np.array_equal(ref, taps / np.float32(taps.astype(np.float64).sum()))
    z, x = np.mgrid[:33, :45]
    tru = np.sin(0.1 * z + 0.07 * x)[None, None].astype(np.float32)
    pred = np.sin(0.1 * z + 0.07 * x + 0.3)[None, None].astype(np.float32)
    moved = R.window_allowance(pred, tru).max()
    print(f"K12 SSIM with the kernel's window: {moved / U:.1f} u from the reference window's")
    assert moved > 8 * U


@pytest.mark.parametrize("H,W,B,kind", R.metric_cases())
def test_metric_case_conditions_and_mixed_against_full(H, W, B, kind):
    """The inputs are what the table says, and the mixed reference with the reference's window is within 8u
    (absolute, SSIM) of the full one; MAE and RMSE within 2u relative (fl32(pv - tv): u on the mean of |d|,
    3u / 2 under the root).  With the kernel's window the mixed SSIM is further away by at most the window
    allowance, which is 0 for identical images."""
    pred, tru = R.metric_inputs(H, W, B, kind)
    assert pred.shape == tru.shape == (B, 1, H, W) and pred.dtype == tru.dtype == np.float32
    assert np.abs(pred).max() <= 1 and np.abs(tru).max() <= 1
    mae, rmse, ssim, map_abs = R.metrics_mixed(pred, tru, R.reference_window())
    fmae, frmse, fssim = R.metrics_full(pred, tru)
    assert (np.abs(ssim - fssim) <= 8 * U).all(), (ssim, fssim)
    kssim = R.metrics_mixed(pred, tru)[2]
    alw = R.window_allowance(pred, tru)
    assert (np.abs(kssim - fssim) <= 8 * U + alw).all()
    assert kind != "identical" or (not alw.any() and (kssim.astype(np.float32) == 1).all())
    assert (np.abs(mae - fmae) <= 2 * U * fmae).all() and (np.abs(rmse - frmse) <= 2 * U * frmse).all()
    assert (map_abs >= np.abs(ssim)).all() and (np.abs(ssim) <= 1 + 1e-12).all()
    if kind == "identical":
        assert np.array_equal(pred, tru) and not mae.any() and not rmse.any()
        assert (ssim.astype(np.float32) == 1).all()
    else:
        assert (mae > 0).all() and (ssim < 1 - 1e-5).all()
    if kind == "constants":
        assert (mae == 2).all() and (rmse == 2).all()
    if kind == "negated":
        assert np.array_equal(pred, -tru)
    if kind == "layered":
        assert (mae < 0.1).all() and (H * W < 64 or ((mae < 0.03) & (ssim > 0.5)).all())
    if B == 3 and H * W > 1 and kind not in ("constants",):
        assert len({float(x) for x in mae}) == (1 if kind == "identical" else 3)


@pytest.mark.parametrize("kind", ["near", "smooth"])
@pytest.mark.parametrize("H,W", [(70, 70), (33, 45), (7, 9), (1, 1)])
def test_mixed_against_full_on_close_and_smooth_pairs(H, W, kind):
    """Two more input kinds for the references alone: pairs that differ by 1e-4 (SSIM just under 1, where
    the variances cancel most) and smooth fields: within 8u."""
    rng = np.random.default_rng(R._seed("k12host", H, W, kind))
    z, x = np.mgrid[:H, :W]
    if kind == "near":
        tru = rng.uniform(-1, 1, (3, 1, H, W)).astype(np.float32)
        pred = np.clip(tru + rng.normal(0, 1e-4, tru.shape), -1, 1).astype(np.float32)
    else:
        tru = np.stack([np.sin(0.1 * (b + 1) * z + 0.07 * x) for b in range(3)])[:, None].astype(np.float32)
        pred = np.stack([np.sin(0.1 * (b + 1) * z + 0.07 * x + 0.3) for b in range(3)])[:, None].astype(np.float32)
    _, _, ssim, _ = R.metrics_mixed(pred, tru, R.reference_window())
    _, _, fssim = R.metrics_full(pred, tru)
    print(f"K12 mixed vs full {kind} {H}x{W}: {np.abs(ssim - fssim).max() / U:.2f} u; "
          f"window allowance {R.window_allowance(pred, tru).max() / U:.2f} u")
    assert (np.abs(ssim - fssim) <= 8 * U).all()


def test_seam_pixels_lie_where_they_are_named():
    mt, win, _, _, _ = R.kernel_constants()
    h = win // 2
    pts = R.seam_pixels(2 * mt, 2 * mt + 1)
    assert len(set(pts.values())) == len(pts) == 13
    # the window of a pixel at seam - HALO - 1 stays inside the first tile, at seam - HALO it reaches across
    assert pts["y_seam-halo-1"][0] + h == mt - 1 and pts["y_seam-halo"][0] + h == mt
    assert pts["y_seam+halo-1"][0] - h == mt - 1 and pts["y_seam+halo"][0] - h == mt
    assert pts["x_seam-halo-1"][1] + h == mt - 1 and pts["x_seam+halo"][1] - h == mt
    # a bump of 0.5 on the layered model moves the SSIM by more than a thousand times the GPU test's bar
    _, tru = R.metric_inputs(2 * mt, 2 * mt + 1, 1, "layered")
    for y, x in pts.values():
        q = tru.copy()
        q[0, 0, y, x] += np.float32(0.5)
        _, _, ssim, _ = R.metrics_mixed(q, tru)
        assert 1 - ssim[0] > 1e3 * U


# ------------------------------------------------------------------------------------------- CosineLR
@pytest.mark.parametrize("eta_min", [0.0, 0.003])
@pytest.mark.parametrize("T_max", [1, 2, 20, 300])
def test_cosine_lr_is_torchs(T_max, eta_min):
    """CosineLR against torch.optim.lr_scheduler.CosineAnnealingLR over 4 T_max + 3 steps, the restart
    branch ((epoch - 1 - T_max) % (2 T_max) == 0) included: the same doubles."""
    from red_diffeq.core.fused import CosineLR
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=0.03)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_max, eta_min=eta_min)
    mine = CosineLR(0.03, T_max=T_max, eta_min=eta_min)
    restarts = 0
    for e in range(1, 4 * T_max + 4):
        opt.step()
        sch.step()
        restarts += (e - 1 - T_max) % (2 * T_max) == 0
        assert mine.step() == opt.param_groups[0]["lr"], (e, mine.lr, opt.param_groups[0]["lr"])
    assert restarts >= 2
