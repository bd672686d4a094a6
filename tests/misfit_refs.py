"""Case tables, input builders and references of the K13 tests (tests/test_misfit_refs_host.py,
tests/test_gpu_misfit.py): the L2, Huber and trace-normalised correlation (NCC) misfits of csrc/misfit.hip.
Plain numpy and CPU torch, no GPU.

Two references per kind, both on the kernels' own fp32 inputs:

mixed  the definitions of include/red_diffeq_misfit.h in numpy, operation by operation: d = fl32(pred - y),
       everything after it in fp64 in the header's order, one final rounding to fp32 per output.  The kernels
       may differ from it only in the order of the fp64 sums (numpy adds pairwise, the kernels in their fixed
       thread / chunk order); an elementwise output (the backward) has no sum and is the kernel's bit for bit.
full   the textbook formulas in torch fp64 on the widened inputs, gradients by fp64 autograd.  The NCC
       reference takes sqrt of where(ok, a c, 1), never where(ok, sqrt(a c), 1): autograd differentiates
       both arguments of a where, and sqrt'(0) = inf times the zero cotangent is NaN for the whole tensor.

Sizes are computed from the kernels' constants, read from the source (kernel_constants), so that each keeps
hitting the branch it is listed for (mf_branches, ncc_branches)."""
import functools
import os
import re

import numpy as np
import torch

from conftest import PKG

U = 2.0 ** -24            # fp32 unit roundoff
E = 2.0 ** -53            # fp64 unit roundoff
KINDS = ("l2", "huber", "ncc")
DELTA = 0.25              # the Huber threshold of every case
GOUT = (-0.7, 0.0, 2.0)   # K5_GOUT: a negative value, a zero, a power of two
MASKS = ("none", "rand01", "columns", "frac", "zero_model")


def bar(k, k64=16):
    """Relative bound of k fp32 roundings and k64 fp64 roundings compounded: (1 + u)^k (1 + e)^k64 - 1."""
    return (1.0 + U) ** k * (1.0 + E) ** k64 - 1.0


def ulps(a, b):
    """Distance in fp32 units in the last place between non-negative fp32 arrays."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape and (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """dict of MF_BLOCK, MF_ITEMS, NCC_BLOCK, NCC_TC, NCC_UNROLL as csrc/misfit.hip has them."""
    src = open(os.path.join(PKG, "csrc", "misfit.hip")).read()
    return {n: int(re.search(rf"constexpr int {n} = (\d+);", src).group(1))
            for n in ("MF_BLOCK", "MF_ITEMS", "NCC_BLOCK", "NCC_TC", "NCC_UNROLL")}


def zero_model(B):
    """The model of the batch whose mask is all zero in the "zero_model" kind."""
    return B // 2


def _seed(*key):
    return [int(x) for x in "".join(map(str, key)).encode()]


def make_mask(shape, kind):
    """None, or fp32 of `shape`: rand01 0 / 1 with 30 % zero; columns whole receivers (last axis) zero per
    model, as missing_trace makes; frac values in {0, 0.5, 1}; zero_model rand01 with one model all zero."""
    rng = np.random.default_rng(_seed("mfmask", shape, kind))
    B = shape[0]
    if kind == "none":
        return None
    if kind == "columns":
        mask = np.ones(shape, np.float32)
        for b in range(B):
            mask[b, ..., rng.permutation(shape[-1])[:max(1, shape[-1] // 5)]] = 0
        return mask
    if kind == "frac":
        return rng.integers(0, 3, shape).astype(np.float32) / np.float32(2)
    mask = (rng.random(shape, dtype=np.float32) >= 0.3).astype(np.float32)
    if kind == "zero_model":
        mask[zero_model(B)] = 0
    return mask


# ------------------------------------------------------------------------------ L2 / Huber sizes
def mf_branches(n):
    """Which branches of k_mf_partial / k_mf_final a model of n elements runs, by walking k_mf_final's two
    loops for every thread (as loss_refs.k5_branches does for K5): nchunk; clamped (the last chunk is partial);
    strided (some thread of k_mf_final adds more than one pair); unrolled / tail_only thread counts."""
    c = kernel_constants()
    blk, chunk = c["MF_BLOCK"], c["MF_BLOCK"] * c["MF_ITEMS"]
    nchunk = -(-n // chunk)
    unrolled = tail_only = most = 0
    for t in range(blk):
        i, u, k = t, 0, 0
        while i + 7 * blk < nchunk:
            u, i = u + 1, i + 8 * blk
        while i < nchunk:
            k, i = k + 1, i + blk
        unrolled += u > 0
        tail_only += u == 0 and k > 0
        most = max(most, 8 * u + k)
    return dict(nchunk=nchunk, clamped=n % chunk != 0, strided=most > 1, unrolled=unrolled, tail_only=tail_only)


def mf_sizes():
    """name -> (shape, the branches the size is in the table for): K5's ladder from the new constants.  With
    MF_BLOCK = 256 and MF_ITEMS = 16: n = 1, 255, 256, 257, 4095, 4096, 4097, 8193 at B = 3, the product's
    record (1, 5, 1000, 70), and (2, 300 chunks + 5), where k_mf_final's loop goes round twice."""
    c = kernel_constants()
    blk, ch = c["MF_BLOCK"], c["MF_BLOCK"] * c["MF_ITEMS"]
    one = dict(nchunk=1, strided=False, unrolled=0, tail_only=1)
    return {
        "n=1": ((3, 1), dict(one, clamped=True)),
        f"n={blk - 1}": ((3, blk - 1), dict(one, clamped=True)),
        f"n={blk}": ((3, blk), dict(one, clamped=True)),
        f"n={blk + 1}": ((3, blk + 1), dict(one, clamped=True)),
        f"n={ch - 1}": ((3, ch - 1), dict(one, clamped=True)),
        f"n={ch}": ((3, ch), dict(one, clamped=False)),
        f"n={ch + 1}": ((3, ch + 1), dict(one, nchunk=2, clamped=True, tail_only=2)),
        f"n={2 * ch + 1}": ((3, 2 * ch + 1), dict(one, nchunk=3, clamped=True, tail_only=3)),
        "record": ((1, 5, 1000, 70), dict(one, nchunk=-(-350000 // ch), clamped=350000 % ch != 0,
                                          tail_only=min(blk, -(-350000 // ch)))),
        "strided": ((2, (blk + 44) * ch + 5), dict(nchunk=blk + 45, clamped=True, strided=True, unrolled=0,
                                                   tail_only=blk)),
    }


def mf_shape(size):
    return mf_sizes()[size][0]


def mf_backward_shape(size):
    """The backward cases: the B = 3 sizes as they are and the product's record at B = 3."""
    shape = mf_shape(size)
    return (3,) + shape[1:] if size == "record" else shape


def mf_forward_cases():
    """(size, mask kind): every mask kind at every size; whole receiver columns need the 4-D record."""
    return [(s, m) for s, (shape, _) in mf_sizes().items() for m in MASKS if m != "columns" or len(shape) == 4]


def mf_backward_cases():
    return [(s, m) for s, m in mf_forward_cases() if mf_backward_shape(s)[0] == 3]


# the Huber special elements, by flat index j of a model: j % HUBER_PERIOD < len(HUBER_SPECIALS)
HUBER_PERIOD = 41
HUBER_SPECIALS = ("+delta", "-delta", "+delta+ulp", "+delta-ulp", "-delta-ulp", "-delta+ulp", "zero")


def huber_special(shape):
    """int array of `shape`: the index into HUBER_SPECIALS of a special element, -1 elsewhere.  A model of
    fewer than HUBER_PERIOD elements starts the cycle at 2 b + 1, so that the n = 1 models are -delta,
    +delta-ulp and -delta+ulp."""
    B = shape[0]
    n = int(np.prod(shape[1:]))
    j = np.arange(n)[None, :] + (2 * np.arange(B)[:, None] + 1) * (n < HUBER_PERIOD)
    k = j % HUBER_PERIOD
    return np.where(k < len(HUBER_SPECIALS), k, -1).reshape(shape)


@functools.lru_cache(maxsize=2)
def mf_pair(kind, shape):
    """(pred, y) fp32.  l2: random normal.  huber: multiples of 2^-10 (so that d = pred - y is exact) with a
    spread of about 0.7 around DELTA = 0.25, and the special elements of huber_special: |d| == delta exactly,
    |d| one fp32 ulp above and below delta (y = 0 there, pred the neighbour of +-delta), and d == 0."""
    rng = np.random.default_rng(_seed("mf", kind, shape))
    if kind != "huber":
        return rng.standard_normal(shape, dtype=np.float32), rng.standard_normal(shape, dtype=np.float32)
    pred = (np.round(rng.standard_normal(shape) * 512) / 1024).astype(np.float32)
    y = (np.round(rng.standard_normal(shape) * 512) / 1024).astype(np.float32)
    sp = huber_special(shape)
    d = np.float32(DELTA)
    up, dn = np.nextafter(d, np.float32(1)), np.nextafter(d, np.float32(0))
    pred = np.where(sp == 0, y + d, np.where(sp == 1, y - d, pred))
    for k, v in ((2, up), (3, dn), (4, -up), (5, -dn)):
        y = np.where(sp == k, np.float32(0), y)
        pred = np.where(sp == k, v, pred)
    pred = np.where(sp == 6, y, pred)
    assert pred.dtype == y.dtype == np.float32
    assert np.array_equal((pred - y).astype(np.float64), pred.astype(np.float64) - y.astype(np.float64))
    return pred, y


def mf_inputs(kind, shape, mask_kind):
    pred, y = mf_pair(kind, tuple(shape))
    return pred, y, make_mask(tuple(shape), mask_kind)


# ------------------------------------------------------------------------------ L2 / Huber references
def _rho(kind, d32, delta):
    d = d32.astype(np.float64)
    if kind == "l2":
        return d * d
    dl = np.float64(np.float32(delta))
    return np.where(np.abs(d32) <= np.float32(delta), (d * d) / (2.0 * dl), np.abs(d) - 0.5 * dl)


def _psi(kind, d32, delta):
    d = d32.astype(np.float64)
    if kind == "l2":
        return 2.0 * d
    return np.clip(d / np.float64(np.float32(delta)), -1.0, 1.0)


def mf_mixed(kind, pred, y, mask, delta=DELTA):
    """(loss, nobs), fp32 (B,): the L2 / Huber forward as the header defines it."""
    B = pred.shape[0]
    d = pred - y
    assert d.dtype == np.float32
    m = np.ones(pred.shape, np.float64) if mask is None else mask.astype(np.float32).astype(np.float64)
    S = (m * _rho(kind, d, delta)).reshape(B, -1).sum(1)
    nobs = np.maximum(m.reshape(B, -1).sum(1).astype(np.float32), np.float32(1))
    return (S / nobs.astype(np.float64)).astype(np.float32), nobs


def mf_backward_mixed(kind, pred, y, mask, nobs, gout, delta=DELTA):
    """dpred fp32: fl32((m psi(d)) g), g = fl64(gout / nobs), nobs and gout fp32 (B,)."""
    B = pred.shape[0]
    g = (np.asarray(gout, np.float32).astype(np.float64) / np.asarray(nobs, np.float32).astype(np.float64))
    g = g.reshape((B,) + (1,) * (pred.ndim - 1))
    m = np.float64(1) if mask is None else mask.astype(np.float32).astype(np.float64)
    return ((m * _psi(kind, pred - y, delta)) * g).astype(np.float32)


def mf_full(kind, pred, y, mask, gout=None, delta=DELTA):
    """(loss, nobs, dpred or None) in fp64 on the widened inputs; the gradient of sum_b gout[b] loss[b]."""
    p = torch.from_numpy(np.ascontiguousarray(pred)).double().requires_grad_(gout is not None)
    t = torch.from_numpy(np.ascontiguousarray(y)).double()
    d = p - t
    if kind == "l2":
        rho = d * d
    else:
        dl = float(np.float32(delta))
        rho = torch.where(d.abs() <= dl, d * d / (2 * dl), d.abs() - dl / 2)
    dims = tuple(range(1, p.dim()))
    if mask is not None:
        m = torch.from_numpy(np.ascontiguousarray(mask)).double()
        nobs = m.sum(dim=dims).clamp(min=1.0)
        loss = (rho * m).sum(dim=dims) / nobs
    else:
        nobs = torch.full((p.shape[0],), float(p[0].numel()), dtype=torch.float64)
        loss = rho.sum(dim=dims) / nobs
    grad = None
    if gout is not None:
        grad, = torch.autograd.grad((loss * torch.as_tensor(np.asarray(gout, np.float64))).sum(), p)
        grad = grad.numpy()
    return loss.detach().numpy(), nobs.numpy(), grad


# ------------------------------------------------------------------------------ NCC shapes
def ncc_branches(nt, ng):
    """What k_ncc_partial does at (nt, ng), by walking its loops for every thread of every (column tile, time
    chunk): ntc time chunks, ctiles column tiles; per tile (wt, R, threads used); unrolled / tail: threads that
    take the unrolled loop / the one-row loop at least once; idle: threads with a phase < R and no row."""
    c = kernel_constants()
    blk, tc, un = c["NCC_BLOCK"], c["NCC_TC"], c["NCC_UNROLL"]
    ntc, ctiles = -(-nt // tc), -(-ng // blk)
    tiles, unrolled, tail, idle = [], 0, 0, 0
    for tile in range(ctiles):
        wt = min(blk, ng - tile * blk)
        R = blk // wt
        tiles.append((wt, R, R * wt))
        for ch in range(ntc):
            t1 = min(nt, (ch + 1) * tc)
            for phase in range(R):
                t, u, k = ch * tc + phase, 0, 0
                while t + (un - 1) * R < t1:
                    u, t = u + 1, t + un * R
                while t < t1:
                    k, t = k + 1, t + R
                unrolled += wt * (u > 0)
                tail += wt * (k > 0)
                idle += wt * (u == 0 and k == 0)
    return dict(ntc=ntc, ctiles=ctiles, tiles=tiles, unrolled=unrolled, tail=tail, idle=idle)


def ncc_ng():
    """ng -> why it is in the table, and what ncc_branches must say of its tiles (asserted on the host)."""
    blk = kernel_constants()["NCC_BLOCK"]
    return {
        1: dict(why="one column: R = 256 phases, more phases than rows in a chunk", tiles=[(1, blk, blk)]),
        3: dict(why="R wt = 255 != 256: the last thread has no column", tiles=[(3, blk // 3, blk // 3 * 3)]),
        64: dict(why="a divisor of the block: every thread used", tiles=[(64, blk // 64, blk)]),
        70: dict(why="the product's width: R = 3, 210 of 256 threads", tiles=[(70, blk // 70, blk // 70 * 70)]),
        blk + 1: dict(why="a second column tile of one column", tiles=[(blk, 1, blk), (1, blk, blk)]),
    }


def ncc_nt():
    """nt -> (why, time chunks)."""
    tc = kernel_constants()["NCC_TC"]
    return {1: ("a single sample", 1), 2: ("two samples", 1), tc - 1: ("one row short of a chunk", 1),
            tc: ("exactly one chunk", 1), tc + 1: ("a second chunk of one row", 2),
            2 * tc + 1: ("three chunks", 3)}


RECORD = (1, 5, 1000, 70)


def ncc_shapes():
    return [(3, ns, nt, ng) for ns in (1, 2) for ng in ncc_ng() for nt in ncc_nt()] + [RECORD]


@functools.lru_cache(maxsize=2)
def ncc_pair(shape):
    """(pred, y) fp32: a random normal pred and an observed record correlated with it (cosine about 0.85), so
    that J is neither near 0 nor near 1."""
    rng = np.random.default_rng(_seed("ncc", shape))
    pred = rng.standard_normal(shape, dtype=np.float32)
    y = (np.float32(0.8) * pred + np.float32(0.5) * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
    return pred, y


def ncc_inputs(shape, mask_kind):
    pred, y = ncc_pair(tuple(shape))
    return pred, y, make_mask(tuple(shape), mask_kind)


# ------------------------------------------------------------------------------ NCC references
def ncc_sums(pred, y, mask):
    """a, c, q, Q = sum |pt yt|, each fp64 (B, ns, ng): the header's per-trace sums, numpy's summation order."""
    m = np.float64(1) if mask is None else mask.astype(np.float32).astype(np.float64)
    pt, yt = m * pred.astype(np.float64), m * y.astype(np.float64)
    return (pt * pt).sum(2), (yt * yt).sum(2), (pt * yt).sum(2), np.abs(pt * yt).sum(2)


def ncc_coef(a, c, q):
    """(inv, r, J, live) fp64 from per-trace sums, in the header's operation order."""
    live = c > 0
    ok = live & (a > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        root = np.sqrt(a * c)
        inv = np.where(ok, 1.0 / root, 0.0)
        r = np.where(ok, q / a, 0.0)
        J = np.where(ok, 1.0 - q / root, np.where(live, 1.0, 0.0))
    return inv, r, J, live


def ncc_loss(J, live):
    """(loss, ntr) fp32 (B,) from per-trace J and the live flags."""
    B = J.shape[0]
    ntr = np.maximum(live.reshape(B, -1).sum(1).astype(np.float32), np.float32(1))
    return (J.reshape(B, -1).sum(1) / ntr.astype(np.float64)).astype(np.float32), ntr


def ncc_mixed(pred, y, mask):
    """dict(a, c, q, Q, inv, r, J, live, loss, ntr): the NCC forward as the header defines it."""
    a, c, q, Q = ncc_sums(pred, y, mask)
    inv, r, J, live = ncc_coef(a, c, q)
    loss, ntr = ncc_loss(J, live)
    return dict(a=a, c=c, q=q, Q=Q, inv=inv, r=r, J=J, live=live, loss=loss, ntr=ntr)


def ncc_backward_mixed(pred, y, mask, inv, r, ntr, gout):
    """(dpred fp32, M fp64): fl32((m g) ((r pt - yt) inv)) with g = fl64(gout / ntr), from per-trace (inv, r)
    fp64 (B, ns, ng), and the sum of the absolute values of the element's two terms,
    M = |m g| (|r pt| + |yt|) inv."""
    B = pred.shape[0]
    g = (np.asarray(gout, np.float32).astype(np.float64) / np.asarray(ntr, np.float32).astype(np.float64))
    g = g.reshape(B, 1, 1, 1)
    m = np.ones(pred.shape) if mask is None else mask.astype(np.float32).astype(np.float64)
    pt, yt = m * pred.astype(np.float64), m * y.astype(np.float64)
    rr, ii = r[:, :, None, :], inv[:, :, None, :]
    out = ((m * g) * ((rr * pt - yt) * ii)).astype(np.float32)
    return out, np.abs(m * g) * (np.abs(rr * pt) + np.abs(yt)) * ii


def ncc_full(pred, y, mask, gout=None, ntr=None):
    """dict(J, live, loss, ntr, grad) in torch fp64 on the widened inputs, grad of sum_b gout[b] loss[b] by
    autograd (None without gout).  ntr: a global live-trace count (B,) to normalise by instead of the own."""
    p = torch.from_numpy(np.ascontiguousarray(pred)).double().requires_grad_(gout is not None)
    t = torch.from_numpy(np.ascontiguousarray(y)).double()
    if mask is not None:
        m = torch.from_numpy(np.ascontiguousarray(mask)).double()
        pt, yt = m * p, m * t
    else:
        pt, yt = p, t
    a, c, q = (pt * pt).sum(2), (yt * yt).sum(2), (pt * yt).sum(2)
    live = c > 0
    ok = live & (a > 0)
    root = torch.sqrt(torch.where(ok, a * c, torch.ones_like(a)))      # never where(ok, sqrt(a c), 1)
    J = torch.where(ok, 1.0 - q / root, live.double())
    B = p.shape[0]
    n = live.reshape(B, -1).sum(1).double().clamp(min=1.0) if ntr is None else torch.as_tensor(np.asarray(ntr, np.float64))
    loss = J.reshape(B, -1).sum(1) / n
    grad = None
    if gout is not None:
        grad, = torch.autograd.grad((loss * torch.as_tensor(np.asarray(gout, np.float64))).sum(), p)
        grad = grad.numpy()
    return dict(J=J.detach().numpy(), live=live.numpy(), loss=loss.detach().numpy(), ntr=n.numpy(), grad=grad)


def ncc_exact_case():
    """(pred, y, mask) at (3, 2, 37, 7) for the exact cases: model 1 has every trace dead (y zero on shot 0,
    the mask zero on shot 1); in models 0 and 2 receiver 2 is masked out, the observed trace (shot 1,
    receiver 4) is zero, and the predicted trace (shot 0, receiver 5) is zero under a live observed one."""
    shape = (3, 2, 37, 7)
    rng = np.random.default_rng(_seed("nccexact"))
    pred = rng.standard_normal(shape, dtype=np.float32)
    y = (np.float32(0.8) * pred + np.float32(0.5) * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
    mask = np.ones(shape, np.float32)
    mask[:, :, :, 2] = 0
    y[:, 1, :, 4] = 0
    pred[:, 0, :, 5] = 0
    y[1, 0] = 0
    mask[1, 1] = 0
    dead = np.zeros((3, 2, 7), bool)
    dead[:, :, 2] = True
    dead[:, 1, 4] = True
    dead[1] = True
    zero_pred = np.zeros((3, 2, 7), bool)
    zero_pred[:, 0, 5] = True
    zero_pred &= ~dead
    return pred, y, mask, dead, zero_pred
