"""Case tables, input builders and references of the serial-tail kernel tests (tests/test_loop_refs_host.py,
tests/test_gpu_loop_tail.py): K11, the fused Adam + clamp (k_adam), and K12, the fused MAE / RMSE / SSIM
(k_metrics_tile / k_metrics_final), of csrc/loop.hip.  Plain numpy and CPU torch, no GPU.

K11  one reference: torch's multi-tensor Adam (torch/optim/adam.py) in fp64 on the kernel's own fp32 state,
     every scalar first rounded to fp32 as the C ABI receives it:
         m' = lerp(m, g, c1)    (m + c1 (g - m), or g - (g - m)(1 - c1) when |c1| >= 0.5, as torch's lerp)
         v' = beta2 v + c2 g^2;  den = sqrt(v') / bc2_sqrt + eps;  upd = step_size m' / den
         p' = p + upd, then clip to [lo, hi]
     c1 and c2 are torch's constants fl32(1 - beta) with 1 - beta formed in double.  Per-element bars from
     counting roundings (u = 2^-24):
         bar_m = 2u (|m| + |g|)              the difference, the product, the sum
         bar_v = 3u v'                       both products, the sum
         bar_p = 2u |p'| + |step_size| bar_m / den + |upd| (4u + bar_v / (2 v'))
     m' can cancel, so its error enters the update as an absolute term, not relative to |upd|.
     The kernel forms 1 - beta in fp32 from the fp32 beta.  At non-dyadic betas that is another constant
     (default betas: c2 0.00099998713 against torch's 0.00100000005, 1.29e-5 relative; c1 2.2e-7 relative),
     and the bars widen by the exactly derived allowance |c2_k - c2_t| g^2 on v, |c1_k - c1_t| |g - m| on m,
     both carried into p by the same formula (adam_ref: alw_m, alw_v, alw_p).

K12  two references, both on the kernel's fp32 inputs:
     mixed  what the kernel is defined to compute: d = fl32(pv - tv); MAE the fp64 mean of |d|; RMSE the
            sqrt of the fp64 mean of fl32(d d); SSIM the fp64 separable 11-tap blur (zero padding) of the
            five moments of the fp32 images fl32((x + 1) / 2) with the fp32 1-D window of ssim.py:gaussian,
            C1 = fl32(0.01^2), C2 = fl32(0.03^2); each result then cast to fp32.  The kernel differs in the
            order of the fp64 sums only.
     full   the reference's formulas in torch fp64: means of |d| and d^2 of the widened inputs, and _ssim
            with its 2-D fp32 window product.
     The window.  ssim.py:gaussian divides the taps by torch's sum of them, the rounded exact sum; rdq_metrics
     adds them one by one in fp32 and lands one ulp lower, so nine of its weights are one ulp above the
     reference's.  mixed with the reference's window is within 8u of full on every case; mixed with the
     kernel's window (the default: what the kernel computes) is up to 81u from it on smooth pairs, because
     the variances E[x^2] - mu^2 lose 1.3e-7 mu^2 against C2 = 9e-4.  window_allowance is that distance,
     computed exactly per case; the kernel is held to mixed with its own window at the plain bars, and to
     mixed with the reference's window and to full with the allowance added (left as it is).

The sizes are computed from the kernels' constants, read from the source, so that each size keeps hitting
the branch it is listed for."""
import functools
import math
import os
import re

import numpy as np
import torch

from conftest import PKG

U = 2.0 ** -24            # fp32 unit roundoff


def f32(x):
    """A Python double rounded to fp32, as a double: what a float argument of the C ABI carries."""
    return float(np.float32(x))


def _seed(*key):
    return [int(x) for x in "".join(map(str, key)).encode()]


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """(MT, WIN, k_adam's block, rdq_adam_step's grid cap, k_metrics_final's block) as csrc/loop.hip has them."""
    src = open(os.path.join(PKG, "csrc", "loop.hip")).read()
    m = re.search(r"constexpr int MT = (\d+), WIN = (\d+), HALO = WIN / 2, IT = MT \+ 2 \* HALO;", src)
    mt, win = int(m.group(1)), int(m.group(2))
    blk = int(re.search(r"__launch_bounds__\((\d+)\) void k_adam\(", src).group(1))
    m = re.search(r"std::min<int64_t>\(\(n \+ (\d+)\) / (\d+), (\d+)\)", src)
    assert int(m.group(1)) + 1 == int(m.group(2)) == blk
    assert re.search(rf"k_adam, dim3\(\(unsigned\)blocks\), dim3\({blk}\)", src)
    cap = int(m.group(3))
    fin = src[src.index("void k_metrics_final("):]
    fblk = int(re.search(r"for \(int t = tid; t < a\.ntiles; t \+= (\d+)\)", fin).group(1))
    assert re.search(rf"__launch_bounds__\({fblk}\) void k_metrics_final\(", src)
    assert re.search(rf"k_metrics_final, dim3\(B\), dim3\({fblk}\)", src)
    return mt, win, blk, cap, fblk


# ------------------------------------------------------------------------------------------- K11
BETAS = ((0.875, 1 - 2.0 ** -10), (0.25, 0.75), (0.9, 0.999))   # dyadic; dyadic, lerp's other branch; default
STEPS = (1, 2, 10, 1000)                                        # t = 1 starts from the zero state
CLAMPS = ((-1.0, 1.0), (0.0, 0.5), None)
LR, EPS = 0.03, 1e-8
MID = 4099                # the size of the beta x t x clamp cases: 17 blocks, the last of three elements


def adam_sizes():
    """name -> n.  With a block of 256 and a cap of 2048 blocks: 1, 255, 256, 257, 524288 (every thread one
    element, one sweep), 524289 (one thread takes a second sweep), 1048579 (a third sweep of three)."""
    _, _, blk, cap, _ = kernel_constants()
    return {"1": 1, "blk-1": blk - 1, "blk": blk, "blk+1": blk + 1, "cap": cap * blk, "cap+1": cap * blk + 1,
            "2cap+3": 2 * cap * blk + 3}


def adam_sweeps(n):
    """Passes of k_adam's grid-stride loop that thread 0 of block 0 runs."""
    _, _, blk, cap, _ = kernel_constants()
    return -(-n // (min(-(-n // blk), cap) * blk))


def adam_cases():
    """(n, betas index, t, clamp index): every beta pair x t x clamp at MID, and every size x beta pair with
    t and the clamp rotating so that each appears at the multi-sweep sizes too."""
    cases = [(MID, b, t, c) for b in range(len(BETAS)) for t in STEPS for c in range(len(CLAMPS))]
    for i, n in enumerate(adam_sizes().values()):
        for b in range(len(BETAS)):
            cases.append((n, b, STEPS[(i + b) % len(STEPS)], (i + 2 * b) % len(CLAMPS)))
    return cases


def adam_scalars(betas, t, lr=LR, eps=EPS):
    """(beta1, beta2, eps, step_size, bc2_sqrt) as FusedAdamClamp.step hands them to the op: formed in
    double as torch/optim/adam.py does."""
    bc1 = 1 - betas[0] ** t
    bc2 = 1 - betas[1] ** t
    return betas[0], betas[1], eps, (lr / bc1) * -1, bc2 ** 0.5


def adam_constants(beta1, beta2):
    """(c1_t, c2_t, c1_k, c2_k): 1 - beta as torch forms it (in double, rounded to fp32 when it meets the
    tensor) and as loop.hip forms it (fp32 subtraction from the fp32 beta)."""
    one = np.float32(1)
    return (f32(1 - beta1), f32(1 - beta2), float(one - np.float32(beta1)), float(one - np.float32(beta2)))


def adam_inputs(n, t, clamp, key=""):
    """(p, g, m, v) fp32 (n,), and the index sets of the special rows.
      p   uniform over the clamp range ((-1, 1) with the clamp off)
      g   |g| log-uniform in [1e-6, 1] with a random sign, a tenth exactly 0
      v   log-uniform in [1e-14, 1e-2], a tenth exactly 0;  m = +-sqrt(v) r, r log-uniform in [1e-3, 3], or
          log-uniform in [1e-6, 1e-1] where v is 0.  t = 1: m = v = 0 (the zero state).
      still   rows with g = m = v = 0 (p must not move); every other one of them sits exactly on lo / hi
      jump    rows with g = v = 0 and |m| in [1e-4, 1e-1]: the update is m' step_size / eps, at least
              0.03 x 0.25e-4 / 1e-8 = 75, far past a clamp bound
    n >= 16: rows 0, 1 are still, row 2 jumps, and the last four rows are ordinary with g != 0."""
    rng = np.random.default_rng(_seed("k11", n, t, clamp, key))
    lo, hi = clamp if clamp is not None else (-1.0, 1.0)
    p = rng.uniform(lo, hi, n).astype(np.float32)
    g = (10.0 ** rng.uniform(-6, 0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rng.random(n) < 0.1] = 0
    if t == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        v = (10.0 ** rng.uniform(-14, -2, n)).astype(np.float32)
        v[rng.random(n) < 0.1] = 0
        m = np.sqrt(v.astype(np.float64)) * 10.0 ** rng.uniform(-3, math.log10(3), n)
        m = np.where(v == 0, 10.0 ** rng.uniform(-6, -1, n), m) * rng.choice([-1.0, 1.0], n)
        m = m.astype(np.float32)
    r = rng.random(n)
    still = np.flatnonzero(r < 0.03)
    jump = np.flatnonzero((r >= 0.03) & (r < 0.06)) if t > 1 else np.zeros(0, np.int64)
    if n >= 16:      # the first rows are special whatever the draw; the last four are ordinary rows with
        #              g != 0, so that a sweep that is not run (the last sweep is one or three elements) shows
        tail = np.arange(n - 4, n)
        still = np.setdiff1d(np.union1d(still, [0, 1]), np.append(tail, 2))
        jump = np.setdiff1d(np.union1d(jump, [2] if t > 1 else []), np.union1d(still, tail)).astype(np.int64)
        g[tail] = np.where(g[tail] == 0, np.float32(0.01), g[tail])
    g[still] = m[still] = v[still] = 0
    g[jump] = v[jump] = 0
    m[jump] = (10.0 ** rng.uniform(-4, -1, jump.size) * rng.choice([-1.0, 1.0], jump.size)).astype(np.float32)
    p[still[0::4]] = lo
    p[still[1::4]] = hi
    return p, g, m, v, still, jump


def adam_ref(p, g, m, v, beta1, beta2, eps, step_size, bc2_sqrt, clamp=None):
    """The fp64 reference of one step and its bars (module docstring).  Returns a dict of fp64 arrays:
    p, m, v (the new state), pre (p before the clamp), upd, bar_m, bar_v, bar_p (the allowance included),
    alw_m, alw_v, alw_p (the allowance alone), and keep: the elements whose p is compared, those whose fp64
    pre-clamp value is further than 4 bar_p from both bounds, or that do not move at all."""
    b2, e, ss, bc = f32(beta2), f32(eps), f32(step_size), f32(bc2_sqrt)
    c1t, c2t, c1k, c2k = adam_constants(beta1, beta2)
    P, G, M, V = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        m1 = M + c1t * (G - M) if abs(c1t) < 0.5 else G - (G - M) * (1 - c1t)
        v1 = b2 * V + c2t * G * G
        den = np.sqrt(v1) / bc + e
        upd = ss * m1 / den
        pre = P + upd
        out = pre if clamp is None else np.clip(pre, f32(clamp[0]), f32(clamp[1]))

        def into_p(bm, bv, rnd):
            rel_v = np.where(v1 > 0, bv / (2 * np.where(v1 > 0, v1, 1.0)), 0.0)
            return abs(ss) * bm / den + np.abs(upd) * (rnd + rel_v)
        alw_m = abs(c1k - c1t) * np.abs(G - M)
        alw_v = abs(c2k - c2t) * G * G
        alw_p = into_p(alw_m, alw_v, 0.0)
        bar_m = 2 * U * (np.abs(M) + np.abs(G)) + alw_m
        bar_v = 3 * U * v1 + alw_v
        bar_p = 2 * U * np.abs(pre) + into_p(bar_m, bar_v, 4 * U)
        keep = np.ones(P.shape, bool)
        if clamp is not None:
            keep = (np.abs(pre - f32(clamp[0])) > 4 * bar_p) & (np.abs(pre - f32(clamp[1])) > 4 * bar_p)
        keep |= (G == 0) & (M == 0) & (V == 0)
    return dict(p=out, m=m1, v=v1, pre=pre, upd=upd, bar_m=bar_m, bar_v=bar_v, bar_p=bar_p, alw_m=alw_m,
                alw_v=alw_v, alw_p=alw_p, keep=keep)


def adam_emulate(p, g, m, v, beta1, beta2, eps, step_size, bc2_sqrt, clamp=None):
    """k_adam statement by statement in numpy fp32, every operation rounded (no FMA): (p, m, v) fp32."""
    F = np.float32
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    b1, b2, e, ss, bc = F(beta1), F(beta2), F(eps), F(step_size), F(bc2_sqrt)
    w, omb2 = F(1) - b1, F(1) - b2
    with np.errstate(all="ignore"):
        mi = m + w * (g - m) if abs(w) < 0.5 else g - (g - m) * (F(1) - w)
        vi = v * b2
        vi = vi + omb2 * g * g
        denom = np.sqrt(vi) / bc + e
        pi = p + ss * (mi / denom)
        if clamp is not None:
            pi = np.where(pi != pi, pi, np.minimum(np.maximum(pi, F(clamp[0])), F(clamp[1])))
    assert pi.dtype == mi.dtype == vi.dtype == F
    return pi, mi, vi


def adam_errors(got_p, got_m, got_v, ref):
    """The largest err / bar of p (over ref['keep']), m and v; a zero bar asks for an exact value."""
    def ratio(got, want, bar, sel):
        err = np.abs(got.astype(np.float64) - want)[sel]
        bar = bar[sel]
        if err.size == 0:
            return 0.0
        return float(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)).max())
    every = np.ones(ref["keep"].shape, bool)
    return (ratio(got_p, ref["p"], ref["bar_p"], ref["keep"]), ratio(got_m, ref["m"], ref["bar_m"], every),
            ratio(got_v, ref["v"], ref["bar_v"], every))


def nonfinite_positions(n):
    """Where the NaN / +inf gradients go: the ends of the first block and of the first sweep, the middle and
    the last element; even entries of the list get NaN, odd ones +inf."""
    _, _, blk, cap, _ = kernel_constants()
    pos = sorted({i for i in (0, 1, blk - 1, blk, n // 2, cap * blk - 1, cap * blk, n - 2, n - 1) if 0 <= i < n})
    return np.array(pos[0::2], np.int64), np.array(pos[1::2], np.int64)


# ------------------------------------------------------------------------------------------- K12
METRIC_INPUTS = ("uniform", "layered", "negated", "constants", "identical")


def metric_shapes():
    """(H, W): a single pixel; smaller than the window; the window; one tile; a second tile of one row / one
    column; 2 x 3 tiles; the product's model; one row of exactly fblk tiles (k_metrics_final: one sweep) and
    of fblk + 1 tiles (thread 0 takes a second)."""
    mt, _, _, _, fblk = kernel_constants()
    return ((1, 1), (7, 9), (11, 11), (mt, mt), (mt + 1, mt), (mt, mt + 1), (2 * mt, 2 * mt + 1), (70, 70),
            (1, fblk * mt), (1, fblk * mt + 1))


def metric_tiles(H, W):
    mt = kernel_constants()[0]
    return -(-H // mt) * -(-W // mt)


def metric_cases():
    return [(H, W, B, kind) for H, W in metric_shapes() for B in (1, 3) for kind in METRIC_INPUTS]


def layered(B, H, W, shift=0):
    """Horizontal layers of 7 rows, the right part faulted down by 3 rows, another set of levels per model."""
    z, x = np.arange(H)[:, None], np.arange(W)[None, :]
    layer = (z + 6 + 3 * (x >= (W + 1) // 2)) // 7
    a = np.stack([-0.9 + 0.125 * ((5 * (layer + b + shift)) % 15) for b in range(B)])
    return a[:, None].astype(np.float32)


@functools.lru_cache(maxsize=4)
def metric_inputs(H, W, B, kind):
    """(pred, true_norm), fp32 (B, 1, H, W) in [-1, 1].
      uniform    both uniform random
      layered    a layered truth and the same model plus noise of 0.02: the workload's kind
      negated    pred = -truth, truth uniform          constants  pred = +1, truth = -1
      identical  pred = truth bit for bit, uniform"""
    rng = np.random.default_rng(_seed("k12", H, W, B, kind))
    tru = rng.uniform(-1, 1, (B, 1, H, W)).astype(np.float32)
    if kind == "uniform":
        return rng.uniform(-1, 1, (B, 1, H, W)).astype(np.float32), tru
    if kind == "layered":
        tru = layered(B, H, W)
        return np.clip(tru + rng.normal(0, 0.02, tru.shape).astype(np.float32), -1, 1).astype(np.float32), tru
    if kind == "negated":
        return -tru, tru
    if kind == "constants":
        return np.ones_like(tru), -np.ones_like(tru)
    assert kind == "identical"
    return tru.copy(), tru


def seam_pixels(H, W):
    """name -> (y, x) of the one bumped pixel: the image's corners, both sides of a tile corner, and HALO
    before / after a seam in each direction (the first / last pixel whose window reaches across it)."""
    mt, win, _, _, _ = kernel_constants()
    h = win // 2
    pts = {"origin": (0, 0), "tile_last": (mt - 1, mt - 1), "tile_first": (mt, mt), "across": (mt - 1, mt),
           "image_last": (H - 1, W - 1), "y_seam-halo-1": (mt - h - 1, 3), "y_seam-halo": (mt - h, 3),
           "y_seam+halo-1": (mt + h - 1, 3), "y_seam+halo": (mt + h, 3), "x_seam-halo-1": (3, mt - h - 1),
           "x_seam-halo": (3, mt - h), "x_seam+halo-1": (3, mt + h - 1), "x_seam+halo": (3, mt + h)}
    assert all(0 <= y < H and 0 <= x < W for y, x in pts.values())
    return pts


@functools.lru_cache(maxsize=None)
def window():
    """The fp32 1-D window as rdq_metrics builds it: the taps fl32(exp(-(k - 5)^2 / (2 1.5^2))) over their
    fp32 sum, added one by one in fp32 (3.7592325211)."""
    _, win, _, _, _ = kernel_constants()
    g = np.array([math.exp(-(k - win // 2) ** 2 / (2.0 * 1.5 * 1.5)) for k in range(win)], np.float32)
    s = np.float32(0)
    for x in g:
        s = np.float32(s + x)
    w = g / s
    assert w.dtype == np.float32
    return w


@functools.lru_cache(maxsize=None)
def reference_window():
    """ssim.py:gaussian in torch on the CPU, as the reference builds it: the same taps over torch's sum of
    them, 3.7592327595, the rounded exact sum, one ulp above the kernel's: nine of the kernel's eleven
    weights are one ulp above these."""
    _, win, _, _, _ = kernel_constants()
    g = torch.Tensor([math.exp(-(x - win // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(win)])
    return (g / g.sum()).numpy()


def _blur(a, w):
    """(..., H, W) fp64: the separable zero-padded blur, the horizontal pass first, taps added in order."""
    w = w.astype(np.float64)
    h = len(w) // 2
    H, W = a.shape[-2:]
    pad = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(h, h), (h, h)])
    hz = np.zeros(a.shape[:-2] + (H + 2 * h, W))
    for k in range(len(w)):
        hz += w[k] * pad[..., :, k:k + W]
    out = np.zeros(a.shape)
    for k in range(len(w)):
        out += w[k] * hz[..., k:k + H, :]
    return out


def metrics_mixed(pred, tru, w=None):
    """The kernel's definition.  Returns (mae, rmse, ssim, mean |map|), fp64 (B,) before the final cast; the
    kernel's fp32 results are within the cast (u relative) and the summation order of these.  w: another
    fp32 window than the kernel's window(), e.g. reference_window()."""
    w = window() if w is None else w
    assert pred.dtype == tru.dtype == np.float32 and pred.shape == tru.shape and pred.shape[1] == 1
    B = pred.shape[0]
    d = pred - tru
    sq = d * d
    assert d.dtype == sq.dtype == np.float32
    mae = np.abs(d).reshape(B, -1).astype(np.float64).mean(1)
    rmse = np.sqrt(sq.reshape(B, -1).astype(np.float64).mean(1))
    x = ((pred + np.float32(1)) / np.float32(2))
    y = ((tru + np.float32(1)) / np.float32(2))
    assert x.dtype == np.float32
    X, Y = x.astype(np.float64), y.astype(np.float64)
    m1, m2, e11, e22, e12 = (_blur(a, w) for a in (X, Y, X * X, Y * Y, X * Y))
    C1, C2 = float(np.float32(0.01) * np.float32(0.01)), float(np.float32(0.03) * np.float32(0.03))
    s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
    smap = ((2.0 * m1 * m2 + C1) * (2.0 * s12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2))
    smap = smap.reshape(B, -1)
    return mae, rmse, smap.mean(1), np.abs(smap).mean(1)


def metric_bars(mae, rmse, ssim, map_abs, n):
    """Bars of the kernel's fp32 results against metrics_mixed's fp64 ones: MAE and RMSE 2u relative (the
    cast; for RMSE the half-weight of the fp32 squares), SSIM the cast and the order of the n-term fp64 sum."""
    return 2 * U * np.abs(mae), 2 * U * np.abs(rmse), U * np.abs(ssim) + n * 2.0 ** -52 * map_abs


def window_allowance(pred, tru):
    """|SSIM with the kernel's window - SSIM with the reference's|, fp64 (B,), both by metrics_mixed: what
    the one-ulp difference of the two window sums moves the SSIM by, exactly, for this pair of images."""
    return np.abs(metrics_mixed(pred, tru)[2] - metrics_mixed(pred, tru, reference_window())[2])


def metrics_full(pred, tru):
    """(mae, rmse, ssim) fp64 (B,): MetricsCalculator.calculate's formulas in torch fp64 on the widened
    inputs, the SSIM on the fp32 images fl32((x + 1) / 2) with the 2-D fp32 window w w^T of create_window."""
    B = pred.shape[0]
    p, t = torch.from_numpy(np.ascontiguousarray(pred)), torch.from_numpy(np.ascontiguousarray(tru))
    d = p.double() - t.double()
    mae = d.abs().mean(dim=(1, 2, 3))
    rmse = (d ** 2).mean(dim=(1, 2, 3)).sqrt()
    a, b = ((p + 1) / 2).double(), ((t + 1) / 2).double()
    w1 = torch.from_numpy(reference_window()).unsqueeze(1)
    w2 = w1.mm(w1.t()).float().double()[None, None]
    pad = w2.shape[-1] // 2

    def conv(z):
        return torch.nn.functional.conv2d(z, w2, padding=pad)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 ** 2, conv(b * b) - mu2 ** 2, conv(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))
    return mae.numpy(), rmse.numpy(), smap.reshape(B, -1).mean(1).numpy()
