"""TEST INFRASTRUCTURE: the time-embedding and linear edge cases (tests/test_gpu_linear_edges.py on the GPU,
tests/test_linear_cases_host.py on the CPU).  Every route of rdq_linear, rdq_sinusoidal_emb, rdq_time_mlp and
rdq_linear_silu_multi (csrc/unet.hip: k_linear, k_sinusoidal, k_time_mlp, k_time_mlp_b, k_linear_silu_multi,
k_linear_silu_multi_b, k_wdot_silu_b) at ragged sizes, compared PER ELEMENT with an fp64 evaluation of

    rdq_linear             y[b][o] = act_out(b[o] + sum_i w[o][i] act_in(x[b][i]))   act_in SiLU, act_out GELU (erf)
    rdq_sinusoidal_emb     y[b] = [sin(t_b f_i) | cos(t_b f_i)],  f_i = exp(i neg_emb),  i < dim / 2
    rdq_time_mlp           y[b] = b2 + W2 GELU(b1 + W1 emb(t_b))
    rdq_linear_silu_multi  y_j[b] = b_j + W_j SiLU(x[b])   (b_j nullable), n <= 32 linears

on the fp32 inputs.  neg_emb is the fp32 number the host hands the kernels, -(float)(ln(theta) / (dim / 2 - 1)) formed
in double, restated here from the formula (so a wrong step on the host is an error, not an input).

build(case_id) is a pure function of the id: CPU tensors, the fp64 reference and the bar, per element.

VALUES.  Weights randn / sqrt(in); inputs 3 randn, and from in >= 8 four entries per sample at +30, -30, +95, -95
(SiLU's tails: expf(95) overflows, so silu_exact(-95) = -95 / inf = -0 where the exact value is -5e-40).  Biases
0.5 randn + 2 (-1)^o, so neighbouring rows of one linear differ by about 4; some linears have no bias.  Time steps
of the time MLP are distinct values below 64 (with steps near 1000 the embedding's bar, which grows with the
argument, is too large for the condition below; rdq_sinusoidal_emb's own cases go to 999, and the bitwise tests of
the time MLP use steps up to 999).  The time MLP's bar is a worst case carried through two layers (up to 4e-3 at
dim 260 on outputs of size 2), and random outputs of neighbouring samples do not differ by 100 times that at every
element.  So hidden unit 0 codes the sample: its weight row is 3 on sin(t f_0) = sin t and 0 elsewhere, no bias,
the steps TM_T alternate between sin t > 0.65 and sin t < -0.65, so GELU(3 sin t) alternates between about 2.5 ... 3
and about 0; every output row reads it with weight +2 or -2.  All other weights are the random ones.

CONDITION.  In every linear, time-MLP and multi-linear case the reference outputs of adjacent rows (in the launch's
row order, across linear boundaries) and of adjacent samples differ by at least SEP = 100 times the larger of the
two bars, so a row or sample stored in the wrong slot, or a clamped duplicate, cannot pass.  build() draws again
(seed salt 0, 1, ...) until this holds; it depends on the reference alone.  The embedding cases are exempt: at
t = 0 every sine is 0, which the GPU test asserts exactly.

THE BAR is derived from the kernel text, never from a kernel's output.  u = 2^-24.
  A dot-product row on a wave (k_linear, wave_dot, lsm_rows, k_linear_silu_multi_b, k_wdot_silu_b):
  lane l sums the ceil(in / 64) terms i = l + 64 k in order (a product and an add each; two roundings where the
  compiler does not contract them), the 64 partials are summed by a six-level tree, then the bias is added:
      P(in) = 2 ceil(in / 64) + 6 + 1,   bar = g(P) S + sum_i |w_i| da_i + u |ref|,   S = |b| + sum |w_i| |a_i|,
  g(P) = P u / (1 - P u), da_i the error of the activation a_i = act(x_i):
      da = EPS_SILU |a| + 2^-126,  EPS_SILU = (2 ULP_EXPF + 1 + 2) u
  for silu_exact = v / (1 + expf(-v)): expf's error passes with a factor e / (1 + e) <= 1, one add, one division
  (taken as <= 1 ulp = 2 u); 2^-126, the least normal number, covers a flushed or overflowed tail.
  The time MLP's hidden rows are a thread's serial chain over dim: P1 = 2 dim + 1.
  GELU of a value v known to dv, gelu_exact = (0.5 v) (1 + erff(v c)), c = fp32(1 / sqrt 2):
      d = 1.13 dv + 0.5 |v| A_GELU u + u |gelu(v)|,   A_GELU = 1 + 2 ULP_ERFF + 2
  (|gelu'| <= 1.13; v c carries 2 u, which erf's slope turns into at most 0.97 u absolute since
  |t| erf'(t) <= 0.484; erff's own error is 2 ULP_ERFF u absolute because |erf| <= 1; the add of 1 rounds a value
  <= 2).  It is absolute in |v| because 1 + erff cancels for negative v.
  The embedding: arg = (float)t expf((float)i neg_emb); the product i neg_emb rounds (relative u, which expf turns
  into |i neg_emb| u), expf's own error, the product with t:
      darg = |arg| (|i neg_emb| + 2 ULP_EXPF + 1) u,   d sin = darg + 2 ULP_SINF u,   d cos = darg + 2 ULP_COSF u.
  The time MLP propagates these: layer 1 sum |w1| de, GELU, layer 2 sum |w2| dh.

ASSUMED, not derived: the library functions' errors in ulps (one ulp taken as 2 u relative): expf 1, erff 4,
sinf 2, cosf 2 over the whole argument range, and a division within 1 ulp.  A ROCm installation carries no
HIP math accuracy table to read them from; these are the figures recalled from the HIP math API documentation with
sinf / cosf doubled.  The GPU test records the measured worst ratio of every case next to its bar (record_margin);
the assumptions stand only while those ratios sit well under 1 (DESIGN.md section 4 lists them)."""
import math
import types

import torch
import torch.nn.functional as F

INVALID, PER_SAMPLE, BATCHED, WDOT = 0, 1, 2, 3                # RDQ_LINEAR_ROUTE_*
ROUTE_NAMES = {PER_SAMPLE: "per_sample", BATCHED: "batched", WDOT: "wdot"}
U = 2.0 ** -24
TINY = 2.0 ** -126
ULP_EXPF, ULP_ERFF, ULP_SINF, ULP_COSF = 1, 4, 2, 2            # assumed (module docstring)
EPS_SILU = (2 * ULP_EXPF + 1 + 2) * U
GELU_SLOPE = 1.13
A_GELU = 1 + 2 * ULP_ERFF + 2
SEP = 100.0
TMB, LSB, WD_B = 8, 32, 64                                     # samples per workgroup of the three batched kernels
SPECIALS = (30.0, -30.0, 95.0, -95.0)
# the time MLP's steps, sample by sample: distinct, below 64, sin t alternately > 0.65 and < -0.65 after the 0
TM_T = (0, 1, 5, 8, 17, 2, 11, 14, 30, 20, 24, 33, 36, 27, 4, 39, 42, 45, 49, 52, 55, 58, 61, 46, 23)

LIN = [  # (B, in, out, act_in, act_out, bias)
    (1, 1, 1, 1, 0, True), (3, 63, 5, 1, 1, True), (2, 64, 4, 0, 0, False), (2, 65, 7, 0, 1, True),
    (2, 200, 9, 1, 0, True), (1, 513, 3, 1, 1, True)]
EMB_DIMS, EMB_THETAS, EMB_T = (4, 6, 64, 2048), (10000.0, 100.0), (0, 1, 17, 999)
TM_SHAPES = [(4, 1, 1), (6, 257, 5), (64, 300, 33), (260, 255, 70)]       # (dim, hid, out)
TM_B = {1: PER_SAMPLE, 16: PER_SAMPLE, 17: BATCHED, 25: BATCHED}
# name -> (rows of each linear, which linears have a bias)
LSM_SETS = {
    "r1": ([1], [True]),
    "r5-1-11": ([5, 1, 11], [True, False, True]),               # 17 rows: a wave's 8 / 16 rows span three linears
    "r64-1": ([64, 1], [True, False]),                          # 65 rows: one past a workgroup's 64
    "n32": ([j % 3 + 1 for j in range(32)], [j % 3 != 1 for j in range(32)]),
}
FUSED_LSM_SETS = {"r16-5-1-11": ([16, 5, 1, 11], [True, True, False, True]), "r16-64-1": ([16, 64, 1], [True, False, True])}


def _spec(kind, **kw):
    return types.SimpleNamespace(kind=kind, **kw)


def _cases():
    out = {}
    for B, cin, cout, ai, ao, bias in LIN:
        out[f"lin-B{B}-in{cin}-out{cout}-ai{ai}-ao{ao}{'' if bias else '-nobias'}"] = _spec(
            "lin", B=B, cin=cin, rows=[cout], has_bias=[bias], act_in=ai, act_out=ao)
    for dim in EMB_DIMS:
        for theta in EMB_THETAS:
            out[f"emb-dim{dim}-theta{int(theta)}"] = _spec("emb", B=len(EMB_T), dim=dim, theta=theta)
    for B, route in TM_B.items():
        for dim, hid, cout in TM_SHAPES:
            out[f"tm-B{B}-dim{dim}-hid{hid}-out{cout}"] = _spec("tm", B=B, dim=dim, hid=hid, rows=[cout], theta=10000.0,
                                                                 route=route)
    lsm = [(cin, B, PER_SAMPLE) for cin in (1, 63, 100, 255) for B in (2, 16)]
    lsm += [(cin, B, BATCHED) for cin in (1, 63, 100, 255) for B in (17, 33, 35)]       # nb = 17, 1, 3
    lsm += [(256, B, WDOT) for B in (17, 65, 130)]
    lsm += [(cin, 20, PER_SAMPLE) for cin in (257, 600)]
    for cin, B, route in lsm:
        for name, (rows, has_bias) in LSM_SETS.items():
            out[f"lsm-B{B}-in{cin}-{name}"] = _spec("lsm", B=B, cin=cin, rows=list(rows), has_bias=list(has_bias),
                                                    route=route)
    return out


CASES = _cases()
CASE_IDS = list(CASES)
BATCHED_IDS = [c for c, s in CASES.items() if getattr(s, "route", PER_SAMPLE) != PER_SAMPLE]


def _gen(case_id, salt=0):
    g = torch.Generator()
    g.manual_seed(31000 + 7919 * salt + sum(ord(c) * (i + 1) for i, c in enumerate(case_id)) % 1000003)
    return g


def gamma(P):
    return P * U / (1.0 - P * U)


def p_wave(cin):
    """Longest rounding path of a wave's dot product over cin inputs plus the bias add (module docstring)."""
    return 2 * -(-cin // 64) + 6 + 1


def silu(x):
    return x / (1.0 + torch.exp(-x))


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def neg_emb_of(dim, theta):
    """The fp32 step the host passes: -(float)(ln(theta) / (dim / 2 - 1)), theta an fp32 argument."""
    th = float(torch.tensor(theta, dtype=torch.float32))
    return -float(torch.tensor(math.log(th) / (dim // 2 - 1), dtype=torch.float64).float())


def emb_arg(t, dim, neg_emb, dtype):
    """(B, dim / 2) arguments t f_i; fp32: the kernel's own operations, fp64: exact on the fp32 neg_emb."""
    i = torch.arange(dim // 2, dtype=dtype)
    if dtype == torch.float32:
        return t.to(dtype).view(-1, 1) * torch.exp(i * torch.tensor(neg_emb, dtype=dtype))
    return t.to(dtype).view(-1, 1) * torch.exp(i * neg_emb)


def embedding(case, dtype, mut=None):
    arg = emb_arg(case.t, case.spec.dim, case.neg_emb, dtype)
    halves = (torch.cos(arg), torch.sin(arg)) if mut == "swap_halves" else (torch.sin(arg), torch.cos(arg))
    return torch.cat(halves, dim=1)


def embedding_bar(case):
    dim = case.spec.dim
    arg = emb_arg(case.t, dim, case.neg_emb, torch.float64).abs()
    ine = (torch.arange(dim // 2, dtype=torch.float64) * case.neg_emb).abs()
    darg = arg * (ine + 2 * ULP_EXPF + 1) * U
    return torch.cat((darg + 2 * ULP_SINF * U, darg + 2 * ULP_COSF * U), dim=1)


def dot_rows(a, da, w, b, P, mut=None):
    """(ref, bar) of rows b + a W^T in a's dtype; a (B, in) known to da, w (R, in), b (R) or None."""
    if mut == "drop256":
        a, w = a[:, :256], w[:, :256]
    ref = a @ w.T
    if mut == "tail_twice":
        ref = ref + a[:, -1:] * w[:, -1].view(1, -1)
    if b is not None:
        ref = ref + b.view(1, -1)
    if da is None:
        return ref, None
    S = a.abs() @ w.abs().T + (b.abs().view(1, -1) if b is not None else 0.0)
    return ref, gamma(P) * S + da @ w.abs().T + U * ref.abs()


def gelu_bar(v, dv):
    return GELU_SLOPE * dv + 0.5 * v.abs() * A_GELU * U + U * gelu(v).abs()


def evaluate(case, dtype=torch.float64, mut=None, bars=False):
    """The case's operation in `dtype` -> list of outputs (one per linear; one tensor for emb / tm / lin), and
    with bars=True (fp64 only) the list of per-element bars.  mut: a kernel mistake restated on the reference
    (tests/test_linear_cases_host.py): drop256, tail_twice, no_silu, swap_halves."""
    s = case.spec
    c = lambda t: None if t is None else t.to(dtype)
    if s.kind == "emb":
        return [embedding(case, dtype, mut)], ([embedding_bar(case)] if bars else None)
    if s.kind == "tm":
        e = embedding(case, dtype, mut)
        de = embedding_bar(case) if bars else None
        pre, dpre = dot_rows(e, de, c(case.w1), c(case.b1), 2 * s.dim + 1)
        h = gelu(pre) if dtype == torch.float64 else F.gelu(pre)
        dh = gelu_bar(pre, dpre) if bars else None
        y, dy = dot_rows(h, dh, c(case.w[0]), c(case.b[0]), p_wave(s.hid), mut)
        return [y], ([dy] if bars else None)
    x = c(case.x)
    silu_on = (s.kind == "lsm" or s.act_in == 1) and mut != "no_silu"
    if silu_on:
        a = silu(x) if dtype == torch.float64 else F.silu(x)
    else:
        a = x
    da = None
    if bars:
        da = EPS_SILU * a.abs() + TINY if silu_on else torch.zeros_like(a)
    ys, dys = [], []
    for w, b in zip(case.w, case.b):
        y, dy = dot_rows(a, da, c(w), c(b), p_wave(s.cin), mut)
        if s.kind == "lin" and s.act_out == 1:
            dy = gelu_bar(y, dy) if bars else None
            y = gelu(y) if dtype == torch.float64 else F.gelu(y)
        ys.append(y)
        dys.append(dy)
    return ys, (dys if bars else None)


def _bias(rows, g):
    return 0.5 * torch.randn(rows, generator=g) + 2.0 * (1.0 - 2.0 * (torch.arange(rows) % 2))


def _inputs(B, cin, g):
    x = 3.0 * torch.randn(B, cin, generator=g)
    if cin >= 8:
        for b in range(B):
            for k, v in enumerate(SPECIALS):
                x[b, (5 * b + 17 * k + 3) % cin] = v
    return x


def _draw(case_id, salt):
    s = CASES[case_id]
    g = _gen(case_id, salt)
    case = types.SimpleNamespace(id=case_id, spec=s, salt=salt, route=getattr(s, "route", None))
    if s.kind == "emb":
        case.t = torch.tensor(EMB_T, dtype=torch.int64)
        case.neg_emb = neg_emb_of(s.dim, s.theta)
    elif s.kind == "tm":
        case.t = torch.tensor(TM_T[:s.B], dtype=torch.int64)
        case.neg_emb = neg_emb_of(s.dim, s.theta)
        case.w1 = torch.randn(s.hid, s.dim, generator=g) / math.sqrt(s.dim)
        case.b1 = 0.5 * torch.randn(s.hid, generator=g)
        case.w = [torch.randn(s.rows[0], s.hid, generator=g) / math.sqrt(s.hid)]
        case.b = [_bias(s.rows[0], g)]
        # hidden unit 0 codes the sample (module docstring): GELU(3 sin t), read by every output row with weight +-2
        case.w1[0] = 0.0
        case.w1[0, 0] = 3.0
        case.b1[0] = 0.0
        case.w[0][:, 0] = 2.0 * (1.0 - 2.0 * (torch.arange(s.rows[0]) % 2))
    else:
        case.x = _inputs(s.B, s.cin, g)
        case.w = [torch.randn(r, s.cin, generator=g) / math.sqrt(s.cin) for r in s.rows]
        case.b = [_bias(r, g) if hb else None for r, hb in zip(s.rows, s.has_bias)]
    case.ref64, case.bar = evaluate(case, torch.float64, bars=True)
    return case


def adjacent_gap(case):
    """min over adjacent rows (launch row order, across linears) and adjacent samples of |ref - ref'| / max(bar, bar');
    inf where the case has neither."""
    ref, bar = torch.cat(case.ref64, dim=1), torch.cat(case.bar, dim=1)
    worst = math.inf
    for d in (0, 1):
        if ref.shape[d] > 1:
            n = ref.shape[d] - 1
            diff = (ref.narrow(d, 1, n) - ref.narrow(d, 0, n)).abs()
            worst = min(worst, float((diff / torch.maximum(bar.narrow(d, 1, n), bar.narrow(d, 0, n))).min()))
    return worst


def build(case_id):
    for salt in range(200):
        case = _draw(case_id, salt)
        if case.spec.kind == "emb" or adjacent_gap(case) >= SEP:
            return case
    raise AssertionError(f"{case_id}: no draw meets the adjacent-difference condition")


def worst_ratio(got, case):
    """got: list of CPU fp32 outputs.  (max |got - ref64| / bar over every element, linear index, flat index); an
    element that is not finite counts as infinitely wrong."""
    worst = (0.0, 0, 0)
    for j, (y, ref, bar) in enumerate(zip(got, case.ref64, case.bar)):
        assert y.shape == ref.shape, (case.id, j, tuple(y.shape), tuple(ref.shape))
        r = (y.double() - ref).abs() / bar
        r = torch.where(torch.isfinite(y.double()), r, torch.full_like(r, math.inf))
        i = int(r.argmax())
        if float(r.flatten()[i]) > worst[0]:
            worst = (float(r.flatten()[i]), j, i)
    return worst


# ------------------------------------------------------------------- the fused forms (bitwise comparisons only)
def fused_lsm_ids():
    return [f"lsmconv-B{B}-in{cin}-{name}" for cin in (100, 256, 300) for B in (1, 2, 3) for name in FUSED_LSM_SETS]


def build_fused_lsm(fid):
    """rdq_conv2d_gn_silu_lsm: a 3x3 conv 8 -> 8 channels on 5 x 7 (pad 1, one GroupNorm group of 8 channels) whose
    scale/shift is linear 0 (16 = 2 cout rows) of the set, and the set on a (B, in) embedding."""
    _, Bs, ins, name = fid.split("-", 3)
    B, cin = int(Bs[1:]), int(ins[2:])
    rows, has_bias = FUSED_LSM_SETS[name]
    g = _gen(fid)
    f = types.SimpleNamespace(id=fid, B=B, cin=cin, rows=list(rows), geom=(B, 8, 5, 7), cout=8, G=1, eps=1e-5)
    f.x = torch.randn(B, 8, 5, 7, generator=g)
    f.cw = torch.randn(8, 8, 3, 3, generator=g) / math.sqrt(72.0)
    f.cb = torch.randn(8, generator=g)
    f.gamma = 1.0 + 0.3 * torch.randn(8, generator=g)
    f.beta = 0.3 * torch.randn(8, generator=g)
    f.temb = _inputs(B, cin, g)
    f.w = [torch.randn(r, cin, generator=g) / math.sqrt(cin) for r in rows]
    f.b = [_bias(r, g) if hb else None for r, hb in zip(rows, has_bias)]
    return f


HEAD_CONVS = {"k3": (8, 3, 1, 5, 7), "k7": (64, 7, 3, 9, 10)}            # cout, k, pad, H, W; one input channel
HEAD_MLPS = [(6, 257, 5), (64, 300, 33)]


def fused_head_ids():
    return [f"head-{k}-B{B}-dim{dim}-hid{hid}-out{out}" for k in HEAD_CONVS for B in (1, 3, 16)
            for dim, hid, out in HEAD_MLPS]


def build_fused_head(fid):
    """rdq_unet_head: the stem conv (3x3 1 -> 8 on 5 x 7, 7x7 1 -> 64 on 9 x 10) and a time MLP, steps up to 999."""
    _, k, Bs, dims, hids, outs = fid.split("-")
    cout, kk, pad, H, W = HEAD_CONVS[k]
    g = _gen(fid)
    f = types.SimpleNamespace(id=fid, B=int(Bs[1:]), dim=int(dims[3:]), hid=int(hids[3:]), out=int(outs[3:]), cout=cout,
                              k=kk, pad=pad, H=H, W=W, theta=10000.0)
    f.x = torch.randn(f.B, 1, H, W, generator=g)
    f.cw = torch.randn(cout, 1, kk, kk, generator=g) / kk
    f.cb = torch.randn(cout, generator=g)
    f.t = wide_steps(torch.tensor(TM_T[-f.B:], dtype=torch.int64))
    f.w1 = torch.randn(f.hid, f.dim, generator=g) / math.sqrt(f.dim)
    f.b1 = 0.5 * torch.randn(f.hid, generator=g)
    f.w2 = torch.randn(f.out, f.hid, generator=g) / math.sqrt(f.hid)
    f.b2 = _bias(f.out, g)
    return f


def wide_steps(t):
    """TM_T's steps spread over 0 ... 999 (0 stays 0, 61 becomes 999): the bitwise tests' time steps."""
    return torch.where(t == 0, t, t * 16 + 23)
