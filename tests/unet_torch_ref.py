"""TEST INFRASTRUCTURE: plain PyTorch fp32 reference of the U-Net block arithmetic
(reference red_diffeq/models/diffusion.py:78-218), used by tests/test_gpu_unet.py to check
the HIP kernels op by op and the whole U-Net (unet_forward below) on the same device, and, in its
functional dtype-generic form with the fp64 wrappers (second half), by the range / edge tests
(tests/unet_range_cases.py, test_gpu_unet_range.py, test_unet_range_inputs.py)."""
import torch
import torch.nn.functional as F

def pixel_unshuffle2(x):
    """einops 'b c (h p1) (w p2) -> b (c p1 p2) h w' with p1 = p2 = 2 (diffusion.py:82)."""
    return F.pixel_unshuffle(x, 2)


def upsample_nearest2(x):
    """nn.Upsample(scale_factor=2, mode='nearest') (diffusion.py:79)."""
    return F.interpolate(x, scale_factor=2, mode="nearest")


def conv2d(x, conv):
    return F.conv2d(x, conv.weight, conv.bias, padding=conv.padding)


def linear(x, lin):
    return F.linear(x, lin.weight, lin.bias)


def group_norm_affine_silu(x, norm, scale_shift=None):
    """GroupNorm -> x*(scale+1)+shift -> SiLU (Block.forward, diffusion.py:142-149)."""
    x = F.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps)
    if scale_shift is not None:
        scale, shift = scale_shift
        x = x * (scale + 1) + shift
    return F.silu(x)


def rmsnorm(x, g):
    """F.normalize(x, dim=1) * g * sqrt(C) (diffusion.py:84-91)."""
    return F.normalize(x, dim=1) * g * x.shape[1] ** 0.5


def linear_attention(x, m):
    """LinearAttention.forward (diffusion.py:182-195): softmax-feature attention with memory kv."""
    b, c, h, w = x.shape
    heads = m.heads
    xn = rmsnorm(x, m.norm.g)
    qkv = F.conv2d(xn, m.to_qkv.weight).chunk(3, dim=1)
    q, k, v = (t.reshape(b, heads, -1, h * w) for t in qkv)
    mk, mv = (t.unsqueeze(0).expand(b, -1, -1, -1) for t in m.mem_kv)
    k = torch.cat((mk, k), dim=-1)
    v = torch.cat((mv, v), dim=-1)
    q = q.softmax(dim=-2) * m.scale
    k = k.softmax(dim=-1)
    context = torch.einsum("bhdn,bhen->bhde", k, v)
    out = torch.einsum("bhde,bhdn->bhen", context, q).reshape(b, -1, h, w)
    out = F.conv2d(out, m.to_out[0].weight, m.to_out[0].bias)
    return rmsnorm(out, m.to_out[1].g)


def full_attention(x, m):
    """Attention.forward (diffusion.py:209-218) with Attend(flash=False):
    softmax(q k^T / sqrt(d)) v over (memory kv + pixels)."""
    b, c, h, w = x.shape
    heads = m.heads
    xn = rmsnorm(x, m.norm.g)
    qkv = F.conv2d(xn, m.to_qkv.weight).chunk(3, dim=1)
    q, k, v = (t.reshape(b, heads, -1, h * w).transpose(-1, -2) for t in qkv)
    mk, mv = (t.unsqueeze(0).expand(b, -1, -1, -1) for t in m.mem_kv)
    k = torch.cat((mk, k), dim=-2)
    v = torch.cat((mv, v), dim=-2)
    scale = q.shape[-1] ** -0.5
    attn = (torch.einsum("bhid,bhjd->bhij", q, k) * scale).softmax(dim=-1)
    out = torch.einsum("bhij,bhjd->bhid", attn, v)
    out = out.transpose(-1, -2).reshape(b, -1, h, w)
    return F.conv2d(out, m.to_out.weight, m.to_out.bias)


def _block(x, blk, scale_shift=None):
    x = conv2d(x, blk.proj)
    return group_norm_affine_silu(x, blk.norm, scale_shift)


def _resnet(x, m, t):
    ss = None
    if m.mlp is not None:
        te = F.linear(F.silu(t), m.mlp[1].weight, m.mlp[1].bias)
        ss = te[:, :, None, None].chunk(2, dim=1)
    h = _block(x, m.block1, ss)
    h = _block(h, m.block2)
    res = conv2d(x, m.res_conv) if isinstance(m.res_conv, torch.nn.Conv2d) else x
    return h + res


def _attn(x, m):
    from red_diffeq.models.diffusion import Attention
    return full_attention(x, m) if isinstance(m, Attention) else linear_attention(x, m)


def _resample(x, m):
    if isinstance(m, torch.nn.Conv2d):
        return conv2d(x, m)
    if isinstance(m[0], torch.nn.Upsample):
        return conv2d(upsample_nearest2(x), m[1])
    return conv2d(pixel_unshuffle2(x), m[1])


def unet_forward(net, x, time):
    """Unet.forward (diffusion.py:273-301) in plain PyTorch, on net's parameters."""
    import math
    x = conv2d(x, net.init_conv)
    r = x.clone()
    sp = net.time_mlp[0]
    half = sp.dim // 2
    emb = math.log(sp.theta) / (half - 1)
    emb = torch.exp(torch.arange(half, device=x.device) * -emb)
    emb = time[:, None] * emb[None, :]
    t = torch.cat((emb.sin(), emb.cos()), dim=-1)
    t = F.linear(t, net.time_mlp[1].weight, net.time_mlp[1].bias)
    t = F.gelu(t)
    t = F.linear(t, net.time_mlp[3].weight, net.time_mlp[3].bias)
    h = []
    for b1, b2, attn, down in net.downs:
        x = _resnet(x, b1, t)
        h.append(x)
        x = _resnet(x, b2, t)
        x = _attn(x, attn) + x
        h.append(x)
        x = _resample(x, down)
    x = _resnet(x, net.mid_block1, t)
    x = _attn(x, net.mid_attn) + x
    x = _resnet(x, net.mid_block2, t)
    for b1, b2, attn, up in net.ups:
        x = torch.cat((x, h.pop()), dim=1)
        x = _resnet(x, b1, t)
        x = torch.cat((x, h.pop()), dim=1)
        x = _resnet(x, b2, t)
        x = _attn(x, attn) + x
        x = _resample(x, up)
    x = torch.cat((x, r), dim=1)
    x = _resnet(x, net.final_res_block, t)
    return conv2d(x, net.final_conv)


# ------------------------------------------------------------------------------------------------
# Functional, dtype-generic restatements (tensors in, tensor out: no module), so the same code runs
# on the CPU in fp32 and in fp64 (tests/unet_range_cases.py, test_gpu_unet_range.py: the fp64
# evaluation is the reference, the fp32 one measures the reference's own error e32).
def to_dtype(v, dtype):
    """v with every floating tensor (in dicts / lists / tuples too) cast to dtype on the CPU."""
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()
    if isinstance(v, dict):
        return {k: to_dtype(x, dtype) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(to_dtype(x, dtype) for x in v)
    return v


def eval64(fn, *args, **kw):
    """fn on the CPU in fp64, on the given (fp32) tensors cast to double."""
    with torch.no_grad():
        return fn(*to_dtype(args, torch.float64), **to_dtype(kw, torch.float64))


def eval32(fn, *args, **kw):
    with torch.no_grad():
        return fn(*to_dtype(args, torch.float32), **to_dtype(kw, torch.float32))


def rel_err(a, ref):
    """max |a - ref| / max |ref| (the measure of every range test), in fp64."""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def la_logits(qkv, mem_kv, heads):
    """(q, k) of the LinearAttention core as (b, heads, dh, n) / (b, heads, dh, nmem + n): the softmax
    logits (k with the memory tokens first, as the kernels order them)."""
    b, c3, h, w = qkv.shape
    q, k, _ = (t.reshape(b, heads, -1, h * w) for t in qkv.chunk(3, dim=1))
    return q, torch.cat((mem_kv[0].unsqueeze(0).expand(b, -1, -1, -1), k), dim=-1)


def linear_attention_core(qkv, mem_kv, heads, scale):
    """LinearAttention.forward from qkv to the hidden tensor (diffusion.py:186-194)."""
    b, c3, h, w = qkv.shape
    q, k, v = (t.reshape(b, heads, -1, h * w) for t in qkv.chunk(3, dim=1))
    mk, mv = (t.unsqueeze(0).expand(b, -1, -1, -1) for t in mem_kv)
    k = torch.cat((mk, k), dim=-1)
    v = torch.cat((mv, v), dim=-1)
    q = q.softmax(dim=-2) * scale
    k = k.softmax(dim=-1)
    context = torch.einsum("bhdn,bhen->bhde", k, v)
    return torch.einsum("bhde,bhdn->bhen", context, q).reshape(b, -1, h, w)


def linear_attention_block(qkv, mem_kv, heads, scale, w_out, b_out, g_out, res=None):
    """... then to_out = Conv2d(hidden, dim, 1) + RMSNorm(dim) and the block's residual."""
    y = rmsnorm(F.conv2d(linear_attention_core(qkv, mem_kv, heads, scale), w_out, b_out), g_out)
    return y + res if res is not None else y


def linear_attention_fn(x, g_in, w_qkv, mem_kv, w_out, b_out, g_out, heads, scale):
    """LinearAttention.forward(x) + x on the module's tensors."""
    qkv = F.conv2d(rmsnorm(x, g_in), w_qkv)
    return linear_attention_block(qkv, mem_kv, heads, scale, w_out, b_out, g_out, x)


def attn_scores(qkv, mem_kv, heads):
    """Scaled scores q k^T / sqrt(dh) of the Attention core, (b, heads, n, nmem + n)."""
    b, c3, h, w = qkv.shape
    q, k, _ = (t.reshape(b, heads, -1, h * w).transpose(-1, -2) for t in qkv.chunk(3, dim=1))
    k = torch.cat((mem_kv[0].unsqueeze(0).expand(b, -1, -1, -1), k), dim=-2)
    return torch.einsum("bhid,bhjd->bhij", q, k) * q.shape[-1] ** -0.5


def full_attention_core(qkv, mem_kv, heads):
    """Attention.forward from qkv to the tensor before to_out (diffusion.py:213-217)."""
    b, c3, h, w = qkv.shape
    v = qkv.chunk(3, dim=1)[2].reshape(b, heads, -1, h * w).transpose(-1, -2)
    v = torch.cat((mem_kv[1].unsqueeze(0).expand(b, -1, -1, -1), v), dim=-2)
    out = torch.einsum("bhij,bhjd->bhid", attn_scores(qkv, mem_kv, heads).softmax(dim=-1), v)
    return out.transpose(-1, -2).reshape(b, -1, h, w)


def rms_conv(x, g, w, bias=None):
    """1x1 conv of RMSNorm(x) (the attention blocks' to_qkv)."""
    return F.conv2d(rmsnorm(x, g), w, bias)


def gn_silu(x, gamma, beta, groups, eps, scale_shift=None, post=None):
    """GroupNorm -> x * (scale + 1) + shift -> SiLU [+ post]; scale_shift (B, 2C), scale first."""
    y = F.group_norm(x, groups, gamma, beta, eps)
    if scale_shift is not None:
        scale, shift = scale_shift[:, :, None, None].chunk(2, dim=1)
        y = y * (scale + 1) + shift
    y = F.silu(y)
    return y + post if post is not None else y


def conv_gn_silu(x, w, b, gamma, beta, groups, eps, scale_shift=None, post=None, w_out=None, b_out=None):
    """Block.forward on cat'ed input x: 3x3 conv, gn_silu [+ post], then an optional 1x1 out conv."""
    y = gn_silu(F.conv2d(x, w, b, padding=w.shape[-1] // 2), gamma, beta, groups, eps, scale_shift, post)
    return F.conv2d(y, w_out, b_out) if w_out is not None else y


def red_q_sample(x0, t, eps, sqrt_ac, sqrt_1mac):
    """x_t = sqrt(abar_t) x0 + sqrt(1 - abar_t) eps (include/red_diffeq_unet.h); also the two products."""
    sh = (-1,) + (1,) * (x0.dim() - 1)
    a1, a2 = sqrt_ac[t].reshape(sh) * x0, sqrt_1mac[t].reshape(sh) * eps
    return a1 + a2, a1, a2


def red_epilogue(xt, t, eps_hat, eps, sr, srm1):
    """g = eps' - eps with x0_hat = clamp(sr[t] x_t - srm1[t] eps_hat, -1, 1), eps' = (sr[t] x_t -
    x0_hat) / srm1[t] (include/red_diffeq_unet.h); returns (g, u, w, eps', unclamped x0_hat)."""
    sh = (-1,) + (1,) * (xt.dim() - 1)
    u, w = sr[t].reshape(sh) * xt, srm1[t].reshape(sh) * eps_hat
    x0 = u - w
    pn = (u - x0.clamp(-1.0, 1.0)) / srm1[t].reshape(sh)
    return pn - eps, u, w, pn, x0


def bf16r(t):
    """t rounded to bf16 (round to nearest even), in t's dtype: through fp32, as the kernels round
    fp32 values (a double first rounded to fp32 differs from the direct rounding only on ties of measure 0)."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def linear_attention_bf16(x, g_in, w_qkv, mem_kv, w_out, b_out, g_out, heads, scale, downstream=True):
    """R_b: LinearAttention.forward(x) + x in the arithmetic of the two-launch bf16 form (csrc/unet.hip
    k_lab_kv / k_lab_out), evaluated in x's dtype (fp64 in the tests) with every matrix operand rounded
    to bf16 where the kernels round it: RMSNorm(x) and the packed weights; exp(k - m) and v before the
    context product; the normalised, scaled context and softmax(q) before the hidden product; the
    hidden tensor and W_out before the projection.  The memory tokens enter the context unrounded, as
    in k_lab_out.  downstream=False rounds only the first-stage operands (xn and W_qkv).
    The kernel's exp(k - m) is taken against a running maximum; the weights' ratio is the same up to
    the bf16 rounding of exp(k - m_running), which this restatement takes at the final maximum."""
    r = bf16r if downstream else (lambda t: t)
    b, c, h, w = x.shape
    n = h * w
    xn = bf16r(rmsnorm(x, g_in))
    qkv = F.conv2d(xn, bf16r(w_qkv))
    q, k, v = (t.reshape(b, heads, -1, n) for t in qkv.chunk(3, dim=1))
    mk, mv = (t.unsqueeze(0).expand(b, -1, -1, -1) for t in mem_kv)
    m = torch.maximum(k.amax(dim=-1, keepdim=True), mk.amax(dim=-1, keepdim=True))
    pk, pm = torch.exp(k - m), torch.exp(mk - m)
    den = pk.sum(-1, keepdim=True) + pm.sum(-1, keepdim=True)
    ctx = torch.einsum("bhdn,bhen->bhde", r(pk), r(v)) + torch.einsum("bhdn,bhen->bhde", pm, mv)
    ctx = r(ctx * (scale / den))
    hid = r(torch.einsum("bhde,bhdn->bhen", ctx, r(q.softmax(dim=-2))).reshape(b, -1, h, w))
    return rmsnorm(F.conv2d(hid, r(w_out), b_out), g_out) + x
