"""Case tables, input builders and references of the loss-side kernel tests (tests/test_loss_refs_host.py,
tests/test_gpu_losses.py): K5, the masked L1 misfit (k_l1_partial / k_l1_final / k_l1_backward), and K6,
TV / Tikhonov (k_smooth_fwd / k_smooth_bwd), of csrc/fwi.hip.  Plain numpy and CPU torch, no GPU.

Two references per operation, both on the kernels' own fp32 inputs:

mixed  what the kernel is defined to compute: its fp32 element operations in numpy fp32, its fp64 sums in
       fp64, its final roundings.  The kernel differs only in the order of the fp64 sums.
         K5   terms fl32(fl32(|y - pred|) mask) summed in fp64 to S; nobs = max(fl32(sum64 mask), 1);
              loss = fl32(S / nobs);  backward sign(pred - y) fl32(mask fl32(gout / nobs)).
         K6   e = fl32(r - c), terms |e| or fl32(e e) summed in fp64 to Sx, Sy;
              tx = fl32(Sx / (H (W - 1))), ty = fl32(Sy / ((H - 1) W)), loss = fl32(tx + ty).
full   the reference's formulas (core/losses.py:27-39, regularization/benchmark.py:4-37) in torch fp64 on
       the widened inputs, gradients by fp64 autograd.

The K5 sizes are computed from the kernel's two constants, read from the source, so that each size keeps
hitting the branch it is listed for (k5_branches)."""
import functools
import os
import re

import numpy as np
import torch

from conftest import PKG

U = 2.0 ** -24            # fp32 unit roundoff
MIN_DIFF = 1e-6           # a model difference the TV sign depends on is 0 or at least this


def ulps(a, b):
    """Distance in fp32 units in the last place between non-negative fp32 arrays."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape and (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------- K5
@functools.lru_cache(maxsize=None)
def kernel_constants():
    """(L1_BLOCK, L1_ITEMS, K6 loads per pass CH, K6 block) as csrc/fwi.hip has them."""
    src = open(os.path.join(PKG, "csrc", "fwi.hip")).read()
    blk, items = (int(re.search(rf"constexpr int {n} = (\d+);", src).group(1)) for n in ("L1_BLOCK", "L1_ITEMS"))
    k6 = src[src.index("void k_smooth_fwd("):src.index("void k_smooth_bwd(")]
    ch = int(re.search(r"constexpr int CH = (\d+);", k6).group(1))
    k6blk = int(re.search(r"__launch_bounds__\((\d+)\) void k_smooth_fwd\(", src).group(1))
    assert re.search(rf"k_smooth_fwd, dim3\(B\), dim3\({k6blk}\)", src)
    return blk, items, ch, k6blk


def k5_branches(n):
    """Which branches of k_l1_partial / k_l1_final a model of n elements runs, by walking k_l1_final's two
    loops for every thread: nchunk; clamped (the last chunk is partial: clamped loads, j < n guard);
    strided (some thread of k_l1_final adds more than one chunk); unrolled (threads that take the
    eight-loads loop at least once); unrolled_then_tail (of those, threads that go on into the tail loop);
    tail_only (threads that add chunks in the tail loop alone)."""
    blk, items, _, _ = kernel_constants()
    chunk = blk * items
    nchunk = -(-n // chunk)
    unrolled = then_tail = tail_only = 0
    most = 0
    for t in range(blk):
        c, u, k = t, 0, 0
        while c + 7 * blk < nchunk:
            u, c = u + 1, c + 8 * blk
        while c < nchunk:
            k, c = k + 1, c + blk
        unrolled += u > 0
        then_tail += u > 0 and k > 0
        tail_only += u == 0 and k > 0
        most = max(most, 8 * u + k)
    return dict(nchunk=nchunk, clamped=n % chunk != 0, strided=most > 1, unrolled=unrolled,
                unrolled_then_tail=then_tail, tail_only=tail_only)


def k5_sizes():
    """name -> (shape, the branches the size is in the table for).  With L1_BLOCK = 256 and L1_ITEMS = 16
    (chunk 4096) the sizes are n = 1, 255, 256, 257, 4095, 4096, 4097, 8193 at B = 3, the product's record
    (1, 5, 1000, 70), (2, 300 chunk + 5), (1, 1799 chunk + 1) and (1, 2050 chunk + 77)."""
    blk, items, _, _ = kernel_constants()
    ch = blk * items
    one = dict(nchunk=1, strided=False, unrolled=0, unrolled_then_tail=0, tail_only=1)
    t = {
        # one chunk: a single element; one row of threads short of / exactly / just over full (item k = 1 starts)
        "n=1": ((3, 1), dict(one, clamped=True)),
        f"n={blk - 1}": ((3, blk - 1), dict(one, clamped=True)),
        f"n={blk}": ((3, blk), dict(one, clamped=True)),
        f"n={blk + 1}": ((3, blk + 1), dict(one, clamped=True)),
        # a chunk one short of full; exactly full (no clamped load); a second chunk of one element; three chunks
        f"n={ch - 1}": ((3, ch - 1), dict(one, clamped=True)),
        f"n={ch}": ((3, ch), dict(one, clamped=False)),
        f"n={ch + 1}": ((3, ch + 1), dict(one, nchunk=2, clamped=True, tail_only=2)),
        f"n={2 * ch + 1}": ((3, 2 * ch + 1), dict(one, nchunk=3, clamped=True, tail_only=3)),
        # the product's record: 5 shots, 1000 samples, 70 receivers
        "record": ((1, 5, 1000, 70), dict(one, nchunk=-(-350000 // ch), clamped=350000 % ch != 0,
                                          tail_only=min(blk, -(-350000 // ch)))),
        # nchunk = L1_BLOCK + 45: the c += L1_BLOCK loop of k_l1_final goes round twice for 45 threads
        "strided": ((2, (blk + 44) * ch + 5), dict(nchunk=blk + 45, clamped=True, strided=True, unrolled=0,
                                                   unrolled_then_tail=0, tail_only=blk)),
        # nchunk = 7 L1_BLOCK + 8: eight threads take the unrolled loop, the rest the tail loop alone
        "unroll8": ((1, (7 * blk + 7) * ch + 1), dict(nchunk=7 * blk + 8, clamped=True, strided=True, unrolled=8,
                                                      unrolled_then_tail=0, tail_only=blk - 8)),
        # nchunk = 8 L1_BLOCK + 3: every thread takes the unrolled loop once, three go on into the tail
        "unroll_all": ((1, (8 * blk + 2) * ch + 77), dict(nchunk=8 * blk + 3, clamped=True, strided=True,
                                                          unrolled=blk, unrolled_then_tail=3, tail_only=0)),
    }
    return t


K5_MASKS = ("none", "rand01", "columns", "zero_model", "frac", "bool", "eq")
K5_GOUT = (-0.7, 0.0, 2.0)       # backward: a negative value, a zero, a power of two


def k5_shape(size):
    return k5_sizes()[size][0]


def k5_backward_shape(size):
    """The backward cases: the B = 3 sizes as they are and the product's record at B = 3."""
    shape = k5_shape(size)
    return (3,) + shape[1:] if size == "record" else shape


def k5_forward_cases():
    """(size, mask kind): every mask kind at every size; whole receiver columns need the 4-D record."""
    return [(s, m) for s, (shape, _) in k5_sizes().items() for m in K5_MASKS if m != "columns" or len(shape) == 4]


def k5_backward_cases():
    return [(s, m) for s, m in k5_forward_cases() if k5_backward_shape(s)[0] == 3]


def zero_model(B):
    """The model of the batch whose mask is all zero in the "zero_model" kind."""
    return B // 2


def _seed(*key):
    return [int(x) for x in "".join(map(str, key)).encode()]


@functools.lru_cache(maxsize=2)
def _k5_pair(shape):
    rng = np.random.default_rng(_seed("k5", shape))
    return rng.standard_normal(shape, dtype=np.float32), rng.standard_normal(shape, dtype=np.float32)


def k5_inputs(shape, kind):
    """(pred, y, mask) as numpy: random normal fp32 pred and y; mask None, fp32 or bool by kind.
      rand01      0 / 1, 30 % zero                      columns  whole receivers (last axis) zero per model
      zero_model  rand01 with model zero_model(B) all 0  frac     values in {0, 0.5, 1}
      bool        rand01 as a bool array                 eq       rand01, and a tenth of pred equal to y bit for bit"""
    pred, y = _k5_pair(tuple(shape))
    rng = np.random.default_rng(_seed("k5mask", shape, kind))
    B = shape[0]
    if kind == "none":
        return pred, y, None
    if kind == "columns":
        mask = np.ones(shape, np.float32)
        for b in range(B):
            mask[b, ..., rng.permutation(shape[-1])[:max(1, shape[-1] // 5)]] = 0
        return pred, y, mask
    if kind == "frac":
        return pred, y, rng.integers(0, 3, shape).astype(np.float32) / np.float32(2)
    mask = (rng.random(shape, dtype=np.float32) >= 0.3)
    if kind == "bool":
        return pred, y, mask
    mask = mask.astype(np.float32)
    if kind == "zero_model":
        mask[zero_model(B)] = 0
    if kind == "eq":
        same = rng.random(shape, dtype=np.float32) < 0.1
        if same.size < 20:
            same.reshape(-1)[0] = True
        pred = np.where(same, y, pred)
    return pred, y, mask


def l1_mixed(pred, y, mask):
    """(loss, nobs), fp32 (B,): the K5 forward as the kernel is defined."""
    B = pred.shape[0]
    t = np.abs(y - pred)
    assert t.dtype == np.float32
    if mask is not None:
        m = mask.astype(np.float32)
        t = t * m
        cnt = m.reshape(B, -1).astype(np.float64).sum(1)
    else:
        cnt = np.full(B, pred[0].size, np.float64)
    S = t.reshape(B, -1).astype(np.float64).sum(1)
    nobs = np.maximum(cnt.astype(np.float32), np.float32(1))
    return (S / nobs.astype(np.float64)).astype(np.float32), nobs


def l1_backward_mixed(pred, y, mask, nobs, gout):
    """dpred, fp32: sign(pred - y) fl32(mask fl32(gout / nobs)), nobs and gout fp32 (B,)."""
    B = pred.shape[0]
    bshape = (B,) + (1,) * (pred.ndim - 1)
    g = (np.asarray(gout, np.float32) / np.asarray(nobs, np.float32)).reshape(bshape)
    m = np.float32(1) if mask is None else mask.astype(np.float32)
    out = np.sign(pred - y) * (m * g)
    assert out.dtype == np.float32
    return out


def l1_full(pred, y, mask, gout=None):
    """(loss, nobs, dpred or None) in fp64: the reference's observation_loss on the widened inputs; the
    gradient of sum_b gout[b] loss[b] by autograd."""
    p = torch.from_numpy(np.ascontiguousarray(pred)).double().requires_grad_(gout is not None)
    t = torch.from_numpy(np.ascontiguousarray(y)).double()
    loss = torch.nn.L1Loss(reduction="none")(t, p)
    dims = tuple(range(1, p.dim()))
    if mask is not None:
        m = torch.from_numpy(np.ascontiguousarray(mask)).double()
        loss = loss * m
        nobs = m.sum(dim=dims).clamp(min=1.0)
        loss = loss.sum(dim=dims) / nobs
    else:
        nobs = torch.full((p.shape[0],), float(p[0].numel()), dtype=torch.float64)
        loss = loss.mean(dim=dims)
    grad = None
    if gout is not None:
        grad, = torch.autograd.grad((loss * torch.as_tensor(np.asarray(gout, np.float64))).sum(), p)
        grad = grad.numpy()
    return loss.detach().numpy(), nobs.numpy(), grad


# ------------------------------------------------------------------------------------------- K6
TV, L2 = 0, 1
K6_SHAPES = ((2, 2), (2, 9), (9, 2), (16, 16), (16, 17), (45, 46), (72, 72), (72, 192), (502, 3002))
K6_INPUTS = ("uniform", "layered", "constant", "checker", "spike")
LAYER, FAULT_SHIFT = 7, 3
LAYER_START = 6           # the first layer boundary lies under row 0, so that H = 2 models have one too


def k6_passes(H, W):
    """Passes of k_smooth_fwd's `base += CH * blockDim.x` loop that thread 0 runs."""
    _, _, ch, blk = kernel_constants()
    return -(-H * W // (ch * blk))


# (H, W) -> what the shape is in the table for; "passes" is asserted against k6_passes at CH = 8, block 256
K6_WHY = {
    (2, 2): dict(passes=1, why="n = 4 < 256: corners only, one difference per direction and row / column"),
    (2, 9): dict(passes=1, why="n < 256, H = 2: no interior, every cell lacks an up or a down term"),
    (9, 2): dict(passes=1, why="n < 256, W = 2: no interior, every cell lacks a left or a right term"),
    (16, 16): dict(passes=1, why="n = 256: one element per thread"),
    (16, 17): dict(passes=1, why="n = 272: just over one element per thread, odd W"),
    (45, 46): dict(passes=2, why="n = 2070, just over 2048: a second pass of 22 threads"),
    (72, 72): dict(passes=3, why="the product's padded model"),
    (72, 192): dict(passes=7, why="a wide model, H != W"),
    (502, 3002): dict(passes=736, why="the configs[4] padded model: 736 passes in one workgroup"),
}


def k6_batches(H, W):
    return (1, 3, 25) if (H, W) == (72, 72) else (1, 3)


def k6_cases():
    """(H, W, B, input kind): every input kind at every shape and batch size."""
    return [(H, W, B, inp) for H, W in K6_SHAPES for B in k6_batches(H, W) for inp in K6_INPUTS]


def cell_classes(H, W):
    """(H, W) int: 0 corner, 1 edge, 2 interior (how many of the four neighbour terms a cell has: 2, 3, 4)."""
    zb = np.zeros((H, 1), bool)
    xb = np.zeros((1, W), bool)
    zb[[0, H - 1]] = True
    xb[:, [0, W - 1]] = True
    return np.where(zb & xb, 0, np.where(zb | xb, 1, 2))


CLASS_NAMES = ("corner", "edge", "interior")


def classes_possible(H, W):
    """The classes an H x W model (H, W >= 2) can have."""
    return [0] + ([1] if H > 2 or W > 2 else []) + ([2] if H > 2 and W > 2 else [])


def spike_cells(H, W):
    """name -> (z, x): the four corners, the middle of every edge the shape has, an interior cell if any."""
    cells = {"corner00": (0, 0), "corner0W": (0, W - 1), "cornerH0": (H - 1, 0), "cornerHW": (H - 1, W - 1)}
    if W > 2:
        cells.update(top=(0, W // 2), bottom=(H - 1, W // 2))
    if H > 2:
        cells.update(left=(H // 2, 0), right=(H // 2, W - 1))
    if H > 2 and W > 2:
        cells["interior"] = (H // 2, W // 2)
    return cells


def bad_differences(a):
    """Cells of (B, 1, H, W) with a right or down difference strictly between 0 and MIN_DIFF in magnitude."""
    a64 = a.astype(np.float64)
    dx, dy = np.abs(np.diff(a64, axis=3)), np.abs(np.diff(a64, axis=2))
    bad = np.zeros(a.shape, bool)
    bad[..., 1:] |= (dx > 0) & (dx < MIN_DIFF)
    bad[:, :, 1:, :] |= (dy > 0) & (dy < MIN_DIFF)
    return bad


@functools.lru_cache(maxsize=2)
def k6_input(H, W, B, kind, spike=None):
    """(B, 1, H, W) fp32, values in about [-1, 1] (the normalised velocity range).
      uniform   uniform random; the few cells with a neighbour closer than MIN_DIFF are moved by 0.01
      layered   horizontal layers of LAYER rows, the right part shifted down by FAULT_SHIFT rows (one
                vertical fault), another set of levels per model: most differences are exactly 0
      constant  one value per model                  checker  (-1)^(z + x)
      spike     a flat model with one cell (spike = (z, x)) raised or lowered, another amount per model"""
    rng = np.random.default_rng(_seed("k6", H, W, B, kind))
    z, x = np.arange(H)[:, None], np.arange(W)[None, :]
    if kind == "uniform":
        a = rng.uniform(-1, 1, (B, 1, H, W)).astype(np.float32)
        for _ in range(8):
            bad = bad_differences(a)
            if not bad.any():
                break
            a[bad] += np.float32(0.01)
        return a
    if kind == "layered":
        layer = (z + LAYER_START + FAULT_SHIFT * (x >= (W + 1) // 2)) // LAYER
        a = np.stack([(-0.9 + 0.125 * ((5 * (layer + b)) % 15)) for b in range(B)])
        return a[:, None].astype(np.float32)
    if kind == "constant":
        return np.stack([np.full((1, H, W), v, np.float32) for v in _levels(B)])
    if kind == "checker":
        return np.broadcast_to((1 - 2 * ((z + x) % 2)).astype(np.float32), (B, 1, H, W)).copy()
    assert kind == "spike" and spike is not None
    a = np.full((B, 1, H, W), 0.25, np.float32)
    a[:, 0, spike[0], spike[1]] += np.array([(-1) ** b * (b + 8) / 16 for b in range(B)], np.float32)
    return a


def _levels(B):
    return [np.float32(0.37 - 0.11 * b) for b in range(B)]


def k6_gout(B):
    """Distinct upstream gradients per model, with a negative one and a power of two."""
    return np.array([(1.0, -0.75, 0.3)[b % 3] * (1 + b // 3) for b in range(B)], np.float32)


def k6_variants(H, W, B, kind):
    """(label, input) of a case, one at a time: the spike kind yields one input per cell of spike_cells."""
    if kind != "spike":
        yield "", k6_input(H, W, B, kind)
        return
    for name, cell in spike_cells(H, W).items():
        yield name, k6_input(H, W, B, kind, cell)


def smooth_mixed(mu, kind):
    """loss, fp32 (B,): the K6 forward as the kernel is defined."""
    assert mu.dtype == np.float32
    B, _, H, W = mu.shape
    ex, ey = mu[..., 1:] - mu[..., :-1], mu[:, :, 1:, :] - mu[:, :, :-1, :]
    tx, ty = (np.abs(ex), np.abs(ey)) if kind == TV else (ex * ex, ey * ey)
    assert tx.dtype == np.float32
    sx = tx.reshape(B, -1).astype(np.float64).sum(1) / (H * (W - 1))
    sy = ty.reshape(B, -1).astype(np.float64).sum(1) / ((H - 1) * W)
    out = sx.astype(np.float32) + sy.astype(np.float32)
    assert out.dtype == np.float32
    return out


def smooth_full(mu, kind, gout=None):
    """(loss, grad or None) in fp64: the reference's total_variation_loss / tikhonov_loss on the widened
    model; the gradient of sum_b gout[b] loss[b] by autograd."""
    m = torch.from_numpy(np.ascontiguousarray(mu)).double().requires_grad_(gout is not None)
    dx = m[:, :, :, 1:] - m[:, :, :, :-1]
    dy = m[:, :, 1:, :] - m[:, :, :-1, :]
    if kind == TV:
        dx, dy = torch.abs(dx), torch.abs(dy)
    else:
        dx, dy = dx ** 2, dy ** 2
    loss = dx.reshape(dx.shape[0], -1).mean(dim=1) + dy.reshape(dy.shape[0], -1).mean(dim=1)
    grad = None
    if gout is not None:
        grad, = torch.autograd.grad((loss * torch.as_tensor(np.asarray(gout, np.float64))).sum(), m)
        grad = grad.numpy()
    return loss.detach().numpy(), grad


def smooth_terms(mu, kind, gout):
    """(4, B, 1, H, W) fp64: the up to four signed terms of every cell's gradient (right, left, down, up
    neighbour; 0 where the cell has no such neighbour).  Their sum is the gradient, the sum of their
    absolute values the M of the per-cell bar."""
    B, _, H, W = mu.shape
    m = mu.astype(np.float64)
    g = np.asarray(gout, np.float64).reshape(B, 1, 1, 1)
    gx, gy = g / (H * (W - 1)), g / ((H - 1) * W)
    d = (lambda e: np.sign(e)) if kind == TV else (lambda e: 2.0 * e)
    tx, ty = d(np.diff(m, axis=3)) * gx, d(np.diff(m, axis=2)) * gy
    t = np.zeros((4,) + mu.shape)
    t[0][..., :-1] = -tx
    t[1][..., 1:] = tx
    t[2][:, :, :-1, :] = -ty
    t[3][:, :, 1:, :] = ty
    return t


def smooth_term_sum(mu, kind, gout):
    """M of the per-cell bar, (B, 1, H, W) fp64: the sum over smooth_terms of the absolute values, without
    building the four fields (the large shape)."""
    B, _, H, W = mu.shape
    g = np.abs(np.asarray(gout, np.float64)).reshape(B, 1, 1, 1)
    gx, gy = g / (H * (W - 1)), g / ((H - 1) * W)
    d = (lambda e: (e != 0).astype(np.float64)) if kind == TV else (lambda e: 2.0 * np.abs(e))
    tx = d(mu[..., 1:].astype(np.float64) - mu[..., :-1]) * gx
    ty = d(mu[:, :, 1:, :].astype(np.float64) - mu[:, :, :-1, :]) * gy
    M = np.zeros(mu.shape)
    M[..., :-1] += tx
    M[..., 1:] += tx
    M[:, :, :-1, :] += ty
    M[:, :, 1:, :] += ty
    return M
