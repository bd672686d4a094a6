"""TEST INFRASTRUCTURE: inputs of the U-Net range / edge tests (tests/test_gpu_unet_range.py on the
GPU, tests/test_unet_range_inputs.py on the CPU): activations and weights at the value ranges of a
TRAINED network (softmax logits of tens to hundreds, GroupNorm inputs whose offset is many times their
spread, RMSNorm pixels at zero), where an unsubtracted exp overflows, a dropped chunk rescale or a
cancelled variance is an O(1) error, and every clamp / guard branch of csrc/unet.hip decides the result.

build(case_id) is a pure function of (case id, seed): CPU fp32 tensors in a Case whose `ref` is the
plain restatement of the operation (tests/unet_torch_ref.py), dtype-generic, so that
    ref64 = R.eval64(case.ref, **case.inputs)       the reference
    e32   = rel_err(R.eval32(case.ref, ...), ref64)  the reference's own fp32 error
and the bar of every fp32 case is max(1e-5, 4 e32) (bar()), with e32 <= 1e-4 required (E32_CAP)."""
import math
import types

import torch
import torch.nn.functional as F

import unet_torch_ref as R

E32_CAP = 1e-4
EXP_OVERFLOW = 89.0          # expf overflows above 88.72
CHUNK_GAP = 110.0            # exp(-110) is 0 in fp32 (below the smallest denormal, exp(-103.3))
LA_CH = 256                  # tokens per chunk of k_la_ctx


def bar(e32):
    """The one rule of every fp32 case: the project's per-op bar, or four times the reference's own
    fp32 error (two independent fp32 evaluations in different summation orders, each off by ~e32)."""
    return max(1e-5, 4.0 * e32)


def _gen(case_id, seed):
    g = torch.Generator()
    g.manual_seed(seed * 1000003 + sum(ord(c) * (i + 1) for i, c in enumerate(case_id)) % 1000003)
    return g


def _case(cid, kind, inputs, ref, **extra):
    return types.SimpleNamespace(id=cid, kind=kind, inputs=inputs, ref=ref, **extra)


# ------------------------------------------------------------------------------- A. attention
def _crafted_la_qkv(g, B, heads, dh, H, W, nmem=4):
    """q, k = 25 randn, v = randn, memory k = 25 randn.  Per (head, d) row of k one chunk of LA_CH tokens
    (memory tokens first) is dominant -- chunk (row mod nch) -- and every other chunk, its memory tokens
    included, is shifted to sit >= CHUNK_GAP + 5 below it: exp(m_c - M) is exactly 0 for whole chunks,
    in both directions (an earlier chunk under a later one and the reverse)."""
    n, C = H * W, heads * dh
    q = 25 * torch.randn(B, C, n, generator=g)
    k = 25 * torch.randn(B, C, n, generator=g)
    v = torch.randn(B, C, n, generator=g)
    mem = torch.randn(2, heads, dh, nmem, generator=g)
    mem[0] *= 25
    mk = mem[0].reshape(C, nmem)
    nch = (n + nmem + LA_CH - 1) // LA_CH
    lo = lambda c: max(c * LA_CH - nmem, 0)                     # noqa: E731  pixel range of chunk c
    hi = lambda c: min((c + 1) * LA_CH - nmem, n)               # noqa: E731
    for row in range(C):
        dom = row % nch
        top = k[:, row, lo(dom):hi(dom)].amax(dim=-1)           # (B,) the dominant chunk's pixel maximum
        if dom == 0:
            top = torch.maximum(top, mk[row].max())
        else:
            mk[row] += (top.min() - (CHUNK_GAP + 5)) - mk[row].max()
        for c in range(nch):
            if c != dom:
                seg = k[:, row, lo(c):hi(c)]
                seg += ((top - (CHUNK_GAP + 5)) - seg.amax(dim=-1))[:, None]
    qkv = torch.cat((q, k, v), dim=1).reshape(B, 3 * C, H, W).contiguous()
    return qkv, mem.contiguous()


def la_chunk_maxima(qkv, mem_kv, heads):
    """(B, heads * dh, nch) maxima of the k logits per chunk of LA_CH tokens, memory tokens first."""
    _, k = R.la_logits(qkv, mem_kv, heads)
    b, h, d, nk = k.shape
    nch = (nk + LA_CH - 1) // LA_CH
    k = F.pad(k, (0, nch * LA_CH - nk), value=-math.inf)
    return k.reshape(b, h * d, nch, LA_CH).amax(dim=-1)


LA_CORE = {"la_core-dh32-18x18": (2, 4, 32, 18, 18), "la_core-dh8-17x17": (2, 4, 8, 17, 17)}
LA_BLOCK = {f"la_block-dim{dim}-18x18-res{int(res)}-bias{int(bias)}": (2, dim, 18, 18, res, bias)
            for dim in (64, 128, 256) for res in (True, False) for bias in (True, False)}
LA_BLOCK["la_block-dim64-46x45-res1-bias1"] = (1, 64, 46, 45, True, True)      # 2074 tokens: 9 chunks


def _la_core(cid, seed):
    B, heads, dh, H, W = LA_CORE[cid]
    qkv, mem = _crafted_la_qkv(_gen(cid, seed), B, heads, dh, H, W)
    return _case(cid, "la_core", dict(qkv=qkv, mem_kv=mem, heads=heads, scale=dh ** -0.5), R.linear_attention_core)


def _la_block(cid, seed):
    B, dim, H, W, res, bias = LA_BLOCK[cid]
    g = _gen(cid, seed)
    qkv, mem = _crafted_la_qkv(g, B, 4, 32, H, W)
    inp = dict(qkv=qkv, mem_kv=mem, heads=4, scale=32 ** -0.5,
               w_out=torch.randn(dim, 128, 1, 1, generator=g) / 128 ** 0.5,
               b_out=0.1 * torch.randn(dim, generator=g) if bias else None,
               g_out=1 + 0.2 * torch.randn(1, dim, 1, 1, generator=g),
               res=torch.randn(B, dim, H, W, generator=g) if res else None)
    return _case(cid, "la_block", inp, R.linear_attention_block)


# the module form: to_qkv.weight x LA_W_SCALE, mem_kv x 20 (a fresh LinearAttention otherwise), one
# pixel of x all zeros (the RMSNorm clamp inside lb_store)
LA_W_SCALE = 50.0
LA_MODULE = {"la_module-C64-9x9": (2, 64, 9, 9), "la_module-C64-10x10": (2, 64, 10, 10),
             "la_module-C128-18x18": (2, 128, 18, 18)}


def _la_module(cid, seed):
    B, C, H, W = LA_MODULE[cid]
    g = _gen(cid, seed)
    hid = 128
    bound = 1 / C ** 0.5                                         # nn.Conv2d's default init range
    x = torch.randn(B, C, H, W, generator=g)
    x[B - 1, :, H // 2, W // 3] = 0.0
    inp = dict(x=x, g_in=1 + 0.2 * torch.randn(1, C, 1, 1, generator=g),
               w_qkv=LA_W_SCALE * (2 * torch.rand(3 * hid, C, 1, 1, generator=g) - 1) * bound,
               mem_kv=20 * torch.randn(2, 4, 32, 4, generator=g),
               w_out=(2 * torch.rand(C, hid, 1, 1, generator=g) - 1) / hid ** 0.5,
               b_out=0.1 * torch.randn(C, generator=g),
               g_out=1 + 0.2 * torch.randn(1, C, 1, 1, generator=g), heads=4, scale=32 ** -0.5)
    return _case(cid, "la_module", inp, R.linear_attention_fn, zero_pixel=(B - 1, H // 2, W // 3))


def la_module_qkv(inp):
    return F.conv2d(R.rmsnorm(inp["x"], inp["g_in"]), inp["w_qkv"])


ATTN = {"attn-9x9": (2, 9, 9, 4), "attn-3x11": (2, 3, 11, 4), "attn-1x3-nk7": (2, 1, 3, 4),
        "attn-dominant-last-pixel": (2, 9, 9, 4), "attn-dominant-mem0": (2, 9, 9, 4)}
ATTN_DOMINANCE = 200.0


def _attn(cid, seed):
    B, H, W, nmem = ATTN[cid]
    g = _gen(cid, seed)
    heads, dh, n = 4, 32, H * W
    C = heads * dh
    if "dominant" not in cid:
        q = 6 * torch.randn(B, heads, dh, n, generator=g)
        k = 6 * torch.randn(B, heads, dh, n, generator=g)
        mem = torch.randn(2, heads, nmem, dh, generator=g)
        mem[0] *= 6
    else:
        # O(1) scores everywhere but at ONE key, which every query scores ATTN_DOMINANCE higher: q carries
        # 10 along d = 0, the other keys 0, the dominant key 200 sqrt(32) / 10
        q = torch.randn(B, heads, dh, n, generator=g)
        k = torch.randn(B, heads, dh, n, generator=g)
        mem = torch.randn(2, heads, nmem, dh, generator=g)
        q[:, :, 0] = 10.0
        k[:, :, 0] = 0.0
        mem[0, :, :, 0] = 0.0
        big = ATTN_DOMINANCE * dh ** 0.5 / 10.0
        if cid.endswith("mem0"):
            mem[0, :, 0, 0] = big
        else:
            k[:, :, 0, n - 1] = big
    v = torch.randn(B, heads, dh, n, generator=g)
    qkv = torch.cat((q.reshape(B, C, n), k.reshape(B, C, n), v.reshape(B, C, n)), 1).reshape(B, 3 * C, H, W)
    return _case(cid, "attn", dict(qkv=qkv.contiguous(), mem_kv=mem.contiguous(), heads=heads), R.full_attention_core)


# ---------------------------------------------------------------------------------- B. RMSNorm
# (C, H, W) -> the kernel instance of rdq_rmsnorm / launch_rmsnorm_r (PX by HW: < 256 -> 16, < 2048 -> 32,
# else 64; NPT = smallest of 2, 4, 8, 16 with C <= NPT * 1024 / PX, else the fallback k_rmsnorm)
RMS_SHAPES = {(125, 9, 9): "PX16 NPT2", (509, 9, 9): "PX16 NPT8", (1030, 3, 3): "fallback",
              (61, 18, 18): "PX32 NPT2", (250, 13, 20): "PX32 NPT8", (600, 16, 16): "fallback",
              (29, 41, 50): "PX64 NPT2", (253, 46, 45): "PX64 NPT16"}
RMS = {f"rmsnorm-C{C}-{H}x{W}-res{r}": (C, H, W, bool(r)) for (C, H, W) in RMS_SHAPES for r in (1, 0)}
CONV_RMS = {"conv_rms-64to96-9x9": (64, 96, 9, 9), "conv_rms-512to64-5x7": (512, 64, 5, 7)}


def rms_instance(C, HW):
    """The instance rdq_rmsnorm dispatches (C, HW) to, restated from csrc/unet.hip."""
    px = 64 if HW >= 2048 else 32 if HW >= 256 else 16
    for npt in (2, 4, 8, 16):
        if C <= npt * (1024 // px):
            return f"PX{px} NPT{npt}"
    return "fallback"


def _rms_x(g, B, C, H, W):
    """randn with per-pixel magnitudes log-uniform over [1e-3, 1e3]; sample 1's first and last pixels 0."""
    mag = 10 ** (6 * torch.rand(B, 1, H, W, generator=g) - 3)
    x = torch.randn(B, C, H, W, generator=g) * mag
    x[1, :, 0, 0] = 0.0
    x[1, :, H - 1, W - 1] = 0.0
    return x


def _rms(cid, seed):
    C, H, W, res = RMS[cid]
    g = _gen(cid, seed)
    x = _rms_x(g, 2, C, H, W)
    inp = dict(x=x, g=1 + 0.3 * torch.randn(1, C, 1, 1, generator=g),
               res=torch.randn(2, C, H, W, generator=g) if res else None)
    return _case(cid, "rmsnorm", inp, lambda x, g, res: R.rmsnorm(x, g) + (res if res is not None else 0),
                 zero_pixels=[(1, 0, 0), (1, H - 1, W - 1)])


def _conv_rms(cid, seed):
    C, cout, H, W = CONV_RMS[cid]
    g = _gen(cid, seed)
    inp = dict(x=_rms_x(g, 2, C, H, W), g=1 + 0.3 * torch.randn(1, C, 1, 1, generator=g),
               w=torch.randn(cout, C, 1, 1, generator=g) / C ** 0.5, bias=torch.randn(cout, generator=g))
    return _case(cid, "conv_rms", inp, R.rms_conv, zero_pixels=[(1, 0, 0), (1, H - 1, W - 1)])


# ---------------------------------------------------------------------------- C. GroupNorm-SiLU
GN_SHAPES = [(64, 8, 35, 35, 2), (16, 8, 9, 9, 2), (512, 8, 9, 9, 17), (512, 8, 18, 18, 9)]
GN = {f"gn-C{C}-{H}x{W}-B{B}-ss{s}": (C, G, H, W, B, bool(s)) for (C, G, H, W, B) in GN_SHAPES for s in (1, 0)}
GN_REGIMES = [(0.0, 1.0), (30.0, 1.0), (-100.0, 0.05), (0.0, 1e-3)]      # (mean, std) per (sample, group), cycled
GN_CONST = 7.25
GN_EPS = 1e-5


def gn_form(C, G, HW, B):
    """The path rdq_group_norm_silu takes, restated from csrc/unet.hip (gn_grid, GN_CHUNK): (apply form,
    apply workgroups per (sample, group), separate k_gn_stats launch, statistics chunks per group)."""
    cpg = C // G
    if HW <= 512 and C * B > 8192:
        form, gx = "small", -(-cpg // (1024 // HW))
    else:
        form, gx = "channel", cpg * -(-HW // 1024)
    return form, gx, gx * B * G > 4096, -(-cpg * HW // 4096)


def gn_const_group(b, G):
    return (2 + b) % G


def _gn(cid, seed):
    C, G, H, W, B, ss = GN[cid]
    g = _gen(cid, seed)
    cpg = C // G
    x = torch.randn(B, G, cpg, H, W, generator=g)
    for b in range(B):
        for gr in range(G):
            mean, std = GN_REGIMES[(b * G + gr) % 4]
            x[b, gr] = x[b, gr] * std + mean
        x[b, gn_const_group(b, G)] = GN_CONST
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g) + 0.05
    sc = None
    if ss:
        sc = 0.5 * torch.randn(B, 2 * C, generator=g)
        # the constant group's value SiLU(beta (scale + 1) + shift) is checked to 1e-6 RELATIVE: its shift
        # takes the sign of beta (scale + 1), so the sum does not cancel (the bound counts roundings)
        for b in range(B):
            c0 = gn_const_group(b, G) * cpg
            prod = beta[c0:c0 + cpg] * (sc[b, c0:c0 + cpg] + 1)
            sc[b, C + c0:C + c0 + cpg] = sc[b, C + c0:C + c0 + cpg].abs() * torch.sign(prod)
    inp = dict(x=x.reshape(B, C, H, W).contiguous(), gamma=gamma, beta=beta, groups=G, eps=GN_EPS, scale_shift=sc)
    return _case(cid, "gn", inp, R.gn_silu)


def gn_const_expected(inp):
    """fp64 SiLU(beta (scale + 1) + shift) of the constant group's channels: [(b, channel slice, (cpg,) values)]."""
    B, C = inp["x"].shape[:2]
    G = inp["groups"]
    cpg = C // G
    out = []
    for b in range(B):
        c0 = gn_const_group(b, G) * cpg
        v = inp["beta"][c0:c0 + cpg].double()
        if inp["scale_shift"] is not None:
            s = inp["scale_shift"][b].double()
            v = v * (s[c0:c0 + cpg] + 1) + s[C + c0:C + c0 + cpg]
        out.append((b, slice(c0, c0 + cpg), v / (1 + torch.exp(-v))))
    return out


# ------------------------------------------------- D. GroupNorm statistics in the conv epilogue
# (cin1, cin2, cout, H, W, B); weights 0.05 randn, bias of output group g = 20 (g - 3), sample b's input
# scaled by (1 + b): |mean| / std of the conv output of order 10 - 100 per group, of either sign
CONV_GN_SHAPES = [(64, 0, 64, 5, 7, 7), (64, 0, 128, 9, 9, 3), (128, 64, 512, 9, 9, 1)]
CONV_GN = {f"conv_gn-{a}+{b2}to{co}-{H}x{W}-B{B}-{v}": (a, b2, co, H, W, B, v == "ss", v == "post", 0)
           for (a, b2, co, H, W, B) in CONV_GN_SHAPES for v in ("ss", "post")}
CONV_GN["conv_gn_out-64to64-9x9-B2-nf1"] = (64, 0, 64, 9, 9, 2, True, True, 1)
CONV_GN_WSCALE, CONV_GN_BIAS = 0.05, 20.0


def _conv_gn_inputs(g, cin1, cin2, cout, H, W, B, ss, post, nf, wscale=CONV_GN_WSCALE, bias_step=CONV_GN_BIAS):
    G = 8
    x = torch.randn(B, cin1 + cin2, H, W, generator=g) * (1 + torch.arange(B, dtype=torch.float32))[:, None, None, None]
    inp = dict(x=x, w=wscale * torch.randn(cout, cin1 + cin2, 3, 3, generator=g),
               b=bias_step * (torch.arange(cout) // (cout // G) - 3).float(),
               gamma=1 + 0.3 * torch.randn(cout, generator=g), beta=0.2 * torch.randn(cout, generator=g),
               groups=G, eps=GN_EPS,
               scale_shift=0.5 * torch.randn(B, 2 * cout, generator=g) if ss else None,
               post=torch.randn(B, cout, H, W, generator=g) if post else None)
    if nf:
        inp["w_out"] = torch.randn(nf, cout, 1, 1, generator=g) / cout ** 0.5
        inp["b_out"] = torch.randn(nf, generator=g)
    return inp


def _conv_gn(cid, seed):
    cin1, cin2, cout, H, W, B, ss, post, nf = CONV_GN[cid]
    inp = _conv_gn_inputs(_gen(cid, seed), cin1, cin2, cout, H, W, B, ss, post, nf)
    return _case(cid, "conv_gn_out" if nf else "conv_gn", inp, R.conv_gn_silu, cin1=cin1)


def conv_gn_offsets(inp):
    """|mean| / std per (sample, group) of the conv output (the GroupNorm's input), in inp's dtype."""
    y = F.conv2d(inp["x"], inp["w"], inp["b"], padding=1)
    B, C = y.shape[:2]
    y = y.reshape(B, inp["groups"], -1)
    return y.mean(-1) / y.std(-1)


# --------------------------------------------------------------- E. RED prologue and epilogue
RED_T = (0, 1, 500, 998, 999)
RED = {f"red-n{n}-s{s}": (shape, s) for n, shape in ((257, (5, 1, 1, 257)), (5184, (5, 1, 72, 72))) for s in (0.1, 3)}


def red_tables():
    """The fp32 schedule buffers of a real GaussianDiffusion (sigmoid schedule, 1000 steps)."""
    from red_diffeq.models.diffusion import GaussianDiffusion

    class _Model(torch.nn.Module):
        channels, out_dim, self_condition = 1, 1, False
    d = GaussianDiffusion(_Model(), image_size=72, timesteps=1000, objective="pred_noise")
    return {k: getattr(d, k).clone() for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                                               "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")}


def _red(cid, seed):
    """x0 in [-1, 1] (0.3 of the elements at each end, the rest uniform: at t = 0, where x0_hat is x0 to a
    few percent, the clamp still fires on both sides), eps = randn, eps_hat = eps + s r randn.  r is 1 on
    the even elements; on the odd ones r = min(1, 1 / (3 srm1[t])), which caps the perturbation of x0_hat
    there at s / 3: with r = 1 everywhere NO element is left unclamped at t = 998 / 999 (srm1 = 57.7 /
    1824.9: x0_hat = x0 - 173 z / 5475 z), so the regime 'every branch, at every t' would not be reached."""
    shape, s = RED[cid]
    g = _gen(cid, seed)
    tab = red_tables()
    t = torch.tensor(RED_T, dtype=torch.int64)
    u = torch.rand(shape, generator=g)
    x0 = torch.where(u < 0.3, torch.tensor(-1.0), torch.where(u > 0.7, torch.tensor(1.0), (u - 0.5) * 5))
    eps = torch.randn(shape, generator=g)
    r = torch.ones(shape)
    cap = (1 / (3 * tab["sqrt_recipm1_alphas_cumprod"][t])).clamp(max=1.0).reshape(-1, 1, 1, 1)
    odd = (torch.arange(x0[0].numel()) % 2 == 1).reshape((1,) + tuple(shape[1:]))
    r = torch.where(odd, cap.expand(shape), r)
    eps_hat = eps + s * r * torch.randn(shape, generator=g)
    xt = R.red_q_sample(x0, t, eps, tab["sqrt_alphas_cumprod"], tab["sqrt_one_minus_alphas_cumprod"])[0]
    return _case(cid, "red", dict(x0=x0, t=t, eps=eps, eps_hat=eps_hat, xt=xt, **tab), None, s=s)


# ------------------------------------------------------------------------------ F. bf16 forms
LA_BF16 = {"la_bf16-" + k.split("-", 1)[1]: v for k, v in LA_MODULE.items()}
# the smallest shape of test_conv_bf16_gn_silu_fused's parameters (tests/test_gpu_unet.py): 64 -> 64 at
# 72 x 72, B = 32; weights / bias scaled so that |mean| / std of the conv output is ~16 (larger offsets
# quantise away in the bf16 raw output, RDQ_UNET_OPT_BF16_RAW: a stated property of the form)
CONV_GN_BF16 = {"conv_gn_bf16-64to64-72x72-B32": (64, 0, 64, 72, 72, 32, True, True, 0)}


def _la_bf16(cid, seed):
    c = _la_module("la_module-" + cid.split("-", 1)[1], seed)      # the inputs of the fp32 module case
    return _case(cid, "la_bf16", c.inputs, R.linear_attention_bf16, zero_pixel=c.zero_pixel)


def conv_gn_bf16_ref(x, w, b, gamma, beta, groups, eps, scale_shift=None, post=None):
    """conv on bf16-rounded operands, the raw output rounded to bf16 before the statistics and the apply.
    Returns (ref, alt, ambiguous): where the exact raw value lies within the fp32 accumulation bound
    2^-23 (K + 2) (sum |x| |w| + |b|), K = 9 cin, of a bf16 rounding tie, an fp32 accumulation may
    legitimately round to the OTHER neighbour (one bf16 step, ~1e-2 of the output range, against a bar of
    1e-5); alt holds the output for that neighbour there (statistics of ref), ambiguous marks those elements."""
    xr, wr = R.bf16r(x), R.bf16r(w)
    raw = F.conv2d(xr, wr, b, padding=1)
    near = R.bf16r(raw)
    tol = 2.0 ** -23 * (w[0].numel() + 2) * (F.conv2d(xr.abs(), wr.abs(), b.abs(), padding=1))
    step = torch.exp2(torch.floor(torch.log2(raw.abs().clamp_min(1e-30))) - 7)      # bf16 spacing at raw
    other = near + torch.where(raw > near, step, -step)         # the bf16 neighbour on raw's other side
    amb = (raw - (near + other) / 2).abs() <= tol
    B, C = raw.shape[:2]
    g = near.reshape(B, groups, -1)
    mean, var = g.mean(-1, keepdim=True), g.var(-1, unbiased=False, keepdim=True)

    def apply(r):
        y = ((r.reshape(B, groups, -1) - mean) / torch.sqrt(var + eps)).reshape(r.shape)
        y = y * gamma[None, :, None, None] + beta[None, :, None, None]
        if scale_shift is not None:
            scale, shift = scale_shift[:, :, None, None].chunk(2, dim=1)
            y = y * (scale + 1) + shift
        y = F.silu(y)
        return y + post if post is not None else y
    return apply(near), apply(torch.where(amb, other, near)), amb


def _conv_gn_bf16(cid, seed):
    cin1, cin2, cout, H, W, B, ss, post, nf = CONV_GN_BF16[cid]
    g = _gen(cid, seed)
    inp = _conv_gn_inputs(g, cin1, cin2, cout, H, W, B, ss, post, nf)
    # every sample at unit scale: the conv output's std is sqrt(576) 0.05 = 1.2, the bias of group g
    # 16 x 1.2 x sign(g - 3): |mean| / std = 16 with either sign (0 for group 3)
    inp["x"] = torch.randn(B, cin1 + cin2, H, W, generator=g)
    inp["b"] = 16.0 * 1.2 * (torch.arange(cout) // (cout // 8) - 3).float().sign()
    return _case(cid, "conv_gn_bf16", inp, conv_gn_bf16_ref)


# ------------------------------------------------------------------------------------ registry
_BUILDERS = [(LA_CORE, _la_core), (LA_BLOCK, _la_block), (LA_MODULE, _la_module), (ATTN, _attn), (RMS, _rms),
             (CONV_RMS, _conv_rms), (GN, _gn), (CONV_GN, _conv_gn), (RED, _red), (LA_BF16, _la_bf16),
             (CONV_GN_BF16, _conv_gn_bf16)]
FP32_GROUPS = (LA_CORE, LA_BLOCK, LA_MODULE, ATTN, RMS, CONV_RMS, GN, CONV_GN)
FP32_CASES = [cid for grp in FP32_GROUPS for cid in grp]
SEED = 0
_CACHE = {}


def build(cid, seed=SEED):
    """The case's inputs (CPU fp32); cached per (id, seed), never modified by the tests."""
    if (cid, seed) not in _CACHE:
        for table, fn in _BUILDERS:
            if cid in table:
                _CACHE[(cid, seed)] = fn(cid, seed)
                break
        else:
            raise KeyError(cid)
    return _CACHE[(cid, seed)]


def reference(cid, seed=SEED):
    """(ref64, e32, bar) of an fp32 case, computed once per (id, seed)."""
    key = ("ref", cid, seed)
    if key not in _CACHE:
        c = build(cid, seed)
        ref64 = R.eval64(c.ref, **c.inputs)
        e32 = R.rel_err(R.eval32(c.ref, **c.inputs), ref64)
        _CACHE[key] = (ref64, e32, bar(e32))
    return _CACHE[key]
