"""fp64 references of the illumination pass, written from the equations in include/red_diffeq_fwi.h.

  q_k  = C1X2 P_{k-1} + (C2 S1(P_{k-1}) + C3 S2(P_{k-1}))      S1 / S2: nearest / second neighbours, periodic wrap
  hA   = sum_{k = 1 .. nt} q_k^2                                  level k of the history (slot k = P_{k-1})
  H    = (dA/dv)^2 fold(sum_w hA),  dA/dv = 2 v (dt/dx)^2 scale   scale = 1500 for normalised input, else 1

The kernel's fp32 constants are taken as doubles (C2 = fp32(4/3), C3 = fp32(-1/12)), so a difference from these
references is the kernel's rounding alone.  Also an fp64 restatement of the forward itself (replicate pad, sponge,
step, source, record), whose history is the truth the end-to-end tests compare against.
"""
import numpy as np

U = 2.0 ** -24
C1X2 = -5.0
C2 = float(np.float32(4.0 / 3.0))
C3 = float(np.float32(-1.0 / 12.0))


def _nbr(P, d):
    return (np.roll(P, d, -2), np.roll(P, -d, -2), np.roll(P, d, -1), np.roll(P, -d, -1))


def q_of(P):
    """(q, Sq) of one or more levels P [..., Hp, Wp] in fp64; Sq = 5|P| + |C2| sum|n1| + |C3| sum|n2| bounds the
    magnitudes the fp32 evaluation rounds."""
    P = np.asarray(P, np.float64)
    n1, n2 = _nbr(P, 1), _nbr(P, 2)
    q = C1X2 * P + (C2 * sum(n1) + C3 * sum(n2))
    Sq = 5.0 * np.abs(P) + abs(C2) * sum(np.abs(a) for a in n1) + abs(C3) * sum(np.abs(a) for a in n2)
    return q, Sq


def hA_and_bar(hist, nt):
    """hA [..., Hp, Wp] in fp64 from a history [nt + 2, ..., Hp, Wp] (slot k = P_{k-1}), and the per-cell bar of the
    fp32 kernel, counted from k_illum_tb's text.  S1 = ((a + b) + c) + d is three roundings and C2 * S1 a fourth; the
    same for the C3 term; lap = (C2 S1) + (C3 S2) a fifth on both; C1X2 * P one rounding; d = that + lap one more on
    all three: at most 6 roundings on any term, |q^ - q| <= 7u Sq with the second-order terms.  t = q^ q^ then has
    |t - q^2| <= 14u |q| Sq + u q^2 (to first order), and the n - 1 adds of n non-negative terms from zero lose at
    most (n - 1) u of the sum:

        bar = sum_k (14u |q_k| Sq_k + u q_k^2) + (n - 1) u sum_k q_k^2."""
    acc = bar1 = None
    for k in range(1, nt + 1):
        q, Sq = q_of(hist[k])
        t = q * q
        e = 14.0 * U * np.abs(q) * Sq + U * t
        acc = t if acc is None else acc + t
        bar1 = e if bar1 is None else bar1 + e
    return acc, bar1 + (nt - 1) * U * acc


def fold(hA, nbc, nz, nx):
    """sum over the wavefields (axis 1, ascending), then the replicate fold of [B, Hp, Wp] onto [B, nz, nx]: padded
    cell (z, x) belongs to model cell (clip(z - nbc), clip(x - nbc))."""
    s = np.asarray(hA, np.float64).sum(axis=1) if hA.ndim == 4 else np.asarray(hA, np.float64)
    B, Hp, Wp = s.shape
    iz = np.clip(np.arange(Hp) - nbc, 0, nz - 1)
    ix = np.clip(np.arange(Wp) - nbc, 0, nx - 1)
    rows = np.zeros((B, nz, Wp))
    np.add.at(rows, (slice(None), iz), s)
    out = np.zeros((B, nz, nx))
    np.add.at(out, (slice(None), slice(None), ix), rows)
    return out


def H_of(hA, v_model, dt, dx, nbc, scale):
    """H [B, nz, nx] in fp64; v_model [B, nz, nx]: the model cells' velocity in m/s (the fp32 values the operator
    holds, as doubles); dt, dx: the plan's fp32 values."""
    v = np.asarray(v_model, np.float64)
    dt, dx = float(np.float32(dt)), float(np.float32(dx))
    d = 2.0 * v * (dt / dx) ** 2 * scale
    return d * d * fold(hA, nbc, v.shape[-2], v.shape[-1])


def denorm32(vn):
    """The operator's fused denormalisation of a normalised fp32 model, in fp32 (v_denormalize: min 1500, max 4500)."""
    vn = np.asarray(vn, np.float32)
    return ((vn + np.float32(1.0)) / np.float32(2.0) * np.float32(3000.0) + np.float32(1500.0)).astype(np.float32)


def ricker(f, dt, nt):
    nw = 2.2 / f / dt
    nw = 2 * np.floor(nw / 2) + 1
    nc = np.floor(nw / 2)
    al = (nc - np.arange(nw)) * f * dt * np.pi
    w0 = (1 - 2 * al ** 2) * np.exp(-al ** 2)
    w = np.zeros(nt)
    w[:len(w0)] = w0
    return w


def forward64(v, ctx, wavelet=None):
    """The forward in fp64 from the physics: v [B, nz, nx] m/s -> (seis [B, ns, nt, ng], history [nt + 2, B, ns, Hp,
    Wp]).  Replicate pad by nbc; sponge kappa = dt * k0 (d / a)^2 within nbc cells of an edge (d cells from the inner
    edge of the strip, a = (nbc - 1) dx, k0 = 3 vmin ln(1e7) / (2 a), columns overwrite rows); the 4th-order step
    with periodic wrap, P' = (2 - 5 alpha - kappa) P - (1 - kappa) P_old + alpha (4/3 S1 - 1/12 S2), alpha = (v dt /
    dx)^2; source: P'[src] += (v dt)^2 w[n]; record at the receivers after the source.  Sources and receivers
    linspace over the grid unless ctx carries sx / gx."""
    v = np.asarray(v, np.float64)
    B, nz, nx = v.shape
    nbc, nt, dx, dt = int(ctx["nbc"]), int(ctx["nt"]), float(ctx["dx"]), float(ctx["dt"])
    vp = np.pad(v, ((0, 0), (nbc, nbc), (nbc, nbc)), mode="edge")
    Hp, Wp = vp.shape[1:]
    a = (nbc - 1) * dx
    k0 = 3.0 * vp.reshape(B, -1).min(1) * np.log(1e7) / (2.0 * a)
    prof = (np.arange(nbc) * dx / a) ** 2                     # grows outwards
    damp = np.zeros_like(vp)
    damp[:, :nbc, :] = (k0[:, None] * prof[::-1])[:, :, None]
    damp[:, Hp - nbc:, :] = (k0[:, None] * prof)[:, :, None]
    damp[:, :, :nbc] = (k0[:, None] * prof[::-1])[:, None, :]
    damp[:, :, Wp - nbc:] = (k0[:, None] * prof)[:, None, :]
    kappa = damp * dt
    alpha = (vp * dt / dx) ** 2
    t1, t2 = 2.0 - 5.0 * alpha - kappa, 1.0 - kappa
    beta = (vp * dt) ** 2
    sx = np.asarray(ctx["sx"], np.float64) if "sx" in ctx else np.linspace(0, ctx["n_grid"] - 1, num=ctx["ns"])
    gx = np.asarray(ctx["gx"], np.float64) if "gx" in ctx else np.linspace(0, ctx["n_grid"] - 1, num=ctx["ng"])
    isx = (np.around(sx) + nbc).astype(int)
    igx = (np.around(gx) + nbc).astype(int)
    isz, igz = int(np.around(ctx["sz"] / dx) + nbc), int(np.around(ctx["gz"] / dx) + nbc)
    ns = len(isx)
    w = ricker(ctx["f"], dt, nt) if wavelet is None else np.asarray(wavelet, np.float64)
    hist = np.zeros((nt + 2, B, ns, Hp, Wp))
    seis = np.zeros((B, ns, nt, len(igx)))
    al, t1, t2 = alpha[:, None], t1[:, None], t2[:, None]
    for n in range(nt):
        P, Po = hist[n + 1], hist[n]
        Pn = t1 * P - t2 * Po + al * (4.0 / 3.0 * sum(_nbr(P, 1)) - 1.0 / 12.0 * sum(_nbr(P, 2)))
        for s in range(ns):
            Pn[:, s, isz, isx[s]] += beta[:, isz, isx[s]] * w[n]
        hist[n + 2] = Pn
        seis[:, :, n, :] = Pn[:, :, igz, igx]
    return seis, hist


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ax = tuple(range(1, a.ndim))
    return np.sqrt(((a - b) ** 2).sum(ax) / (b ** 2).sum(ax))
