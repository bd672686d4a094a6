"""U-Net HIP kernels (csrc/unet.hip) at the value ranges of a TRAINED network and at their edge
branches, against an fp64 reference (tests/unet_torch_ref.py evaluated on the CPU in double on the same
fp32 inputs; inputs from tests/unet_range_cases.py, whose regimes tests/test_unet_range_inputs.py
asserts on the CPU).  tests/test_gpu_unet.py and test_gpu_ops.py feed O(1) activations and fresh
initialisations, where a softmax without its max subtraction, a chunk rescale that is only approximately
right, or a cancelled variance still passes; here the logits reach tens to hundreds, whole chunks
rescale to exactly 0, GroupNorm offsets are up to 2000 x the spread, RMSNorm pixels are exactly zero.

One rule for every fp32 case: err = max |kernel - ref64| / max |ref64| <= max(1e-5, 4 e32), e32 the error
of the SAME restatement evaluated in fp32 on the CPU (<= 1e-4, asserted by the CPU module): 1e-5 is the
project's per-op bar, the factor 4 covers two independent fp32 evaluations with different summation
orders.  err, e32 and the bar go to margins.jsonl (record_margin).  Finite-ness is asserted on its own."""
import os

import pytest
import torch

import unet_range_cases as K
import unet_torch_ref as R
from conftest import record_margin

pytestmark = pytest.mark.gpu


def _test_id():
    return os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]


def _dev(inp, cuda):
    return {k: (v.to(cuda) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}


def check(got, cid, what=""):
    """The bar rule of the module docstring for an fp32 case; NaN / inf reported as such."""
    ref64, e32, bar = K.reference(cid)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert torch.isfinite(got).all(), f"{cid} {what}: {int((~torch.isfinite(got)).sum())} non-finite outputs"
    err = R.rel_err(got, ref64)
    print(f"{cid} {what}: err {err:.3g}  e32 {e32:.3g}  bar {bar:.3g}")
    record_margin(_test_id(), f"{cid} {what}".strip(), err, bar)
    record_margin(_test_id(), f"{cid} e32 (fp32 CPU restatement vs fp64)", e32, K.E32_CAP)
    assert err <= bar, (cid, what, err, e32, bar)
    return err


# ----------------------------------------------------------------- A. softmax range, attention
@pytest.mark.parametrize("cid", list(K.LA_CORE))
def test_linear_attn_core(cuda, cid):
    """k_la_ctx / k_la_reduce / k_la_out on crafted qkv: logits to +-100, whole chunks at exp(m_c - M) == 0
    in both directions; dh = 32 (MFMA context) and dh = 8 (scalar path), 2 chunks, ragged last chunk."""
    from red_diffeq import ops  # noqa: F401
    d = _dev(K.build(cid).inputs, cuda)
    check(torch.ops.red_diffeq.linear_attn(d["qkv"], d["mem_kv"], d["heads"], float(d["scale"])), cid)


@pytest.mark.parametrize("cid", list(K.LA_BLOCK))
def test_linear_attn_block(cuda, cid):
    """k_la_out_proj<64 / 128 / 256> on the same crafted qkv: the in-launch combine over 2 chunks, ragged
    pixel blocks (324 = 10 x 32 + 4 = 20 x 16 + 4), with / without residual and bias; 9 chunks (> LAO_MAXCH)
    combined by k_la_reduce's own launch."""
    from red_diffeq import ops  # noqa: F401
    d = _dev(K.build(cid).inputs, cuda)
    got = torch.ops.red_diffeq.linear_attn_block(d["qkv"], d["mem_kv"], d["heads"], float(d["scale"]), d["w_out"],
                                                 d["b_out"], d["g_out"], d["res"])
    check(got, cid)


def _la_module(cuda, inp):
    from red_diffeq.models.diffusion import LinearAttention
    m = LinearAttention(inp["x"].shape[1]).to(cuda)
    with torch.no_grad():
        m.norm.g.copy_(inp["g_in"])
        m.to_qkv.weight.copy_(inp["w_qkv"])
        m.mem_kv.copy_(inp["mem_kv"])
        m.to_out[0].weight.copy_(inp["w_out"])
        m.to_out[0].bias.copy_(inp["b_out"])
        m.to_out[1].g.copy_(inp["g_out"])
    assert m.heads == inp["heads"] and float(m.scale) == inp["scale"]
    return m


@pytest.mark.parametrize("cid", list(K.LA_MODULE))
def test_linear_attention_module(cuda, cid):
    """LinearAttention.forward(x) + x with to_qkv x 50 and mem_kv x 20 (q / k logits past 89), one all-zero
    pixel: the two-launch fp32 form (k_lab_kv / k_lab_out<D, true>: running-maximum rescale; at 9 x 9 the
    last tile's second 32-pixel block lies wholly past n, tmax = -inf) and the three-launch form."""
    from red_diffeq.models import unet_ops as ops
    c = K.build(cid)
    x = c.inputs["x"].to(cuda)
    m = _la_module(cuda, c.inputs)
    old = ops.FUSED_LA_F32
    with torch.no_grad():
        try:
            ops.FUSED_LA_F32 = True
            fused = ops.linear_attention(x, m)
            ops.FUSED_LA_F32 = False
            unfused = ops.linear_attention(x, m)
        finally:
            ops.FUSED_LA_F32 = old
    check(fused, cid, "two-launch fp32")
    check(unfused, cid, "three-launch fp32")


@pytest.mark.parametrize("cid", list(K.ATTN))
def test_full_attn_core(cuda, cid):
    """k_full_attn<32>: scores past +-89 (online-softmax rescale, FA_KS merge); a 32-query block with one
    query; nk = 7 < FA_KS (a key split without keys, m = -inf); a single key 200 above the rest, at the last
    pixel token and at memory token 0."""
    from red_diffeq import ops  # noqa: F401
    d = _dev(K.build(cid).inputs, cuda)
    check(torch.ops.red_diffeq.attn(d["qkv"], d["mem_kv"], d["heads"]), cid)


# ------------------------------------------------------------------------------ B. RMSNorm edges
@pytest.mark.parametrize("cid", list(K.RMS))
def test_rmsnorm_range_and_zero_pixels(cuda, cid):
    """k_rmsnorm_r<NPT, PX> in every PX and the smallest / largest NPT of each, and the fallback k_rmsnorm:
    per-pixel magnitudes over [1e-3, 1e3]; at an all-zero pixel (the 1e-12 clamp) the output is exactly the
    residual, or 0."""
    from red_diffeq.models import unet_ops as ops
    c = K.build(cid)
    d = _dev(c.inputs, cuda)
    got = ops.rmsnorm(d["x"], d["g"], residual=d["res"])
    check(got, cid)
    for b, i, j in c.zero_pixels:
        want = d["res"][b, :, i, j] if d["res"] is not None else torch.zeros_like(got[b, :, i, j])
        assert torch.equal(got[b, :, i, j], want), (cid, b, i, j)


@pytest.mark.parametrize("cid", list(K.CONV_RMS))
def test_conv_rms_range_and_zero_pixels(cuda, cid):
    """conv2d_rms (the normalisation in the 1x1 conv's gather) on the same inputs; at a zero pixel the output
    is exactly the bias."""
    from red_diffeq import ops as O
    c = K.build(cid)
    d = _dev(c.inputs, cuda)
    assert O.conv_rms_fusable(d["x"], d["w"])
    got = torch.ops.red_diffeq.conv2d_rms(d["x"], d["g"], d["w"], d["bias"], None)
    check(got, cid)
    for b, i, j in c.zero_pixels:
        assert torch.equal(got[b, :, i, j], d["bias"]), (cid, b, i, j)


# ----------------------------------------------------------------------------- C. GroupNorm-SiLU
@pytest.mark.parametrize("cid", list(K.GN))
def test_group_norm_silu_offsets(cuda, cid):
    """gn_silu (k_gn_partial, k_gn_stats / in-apply statistics, k_gn_apply<SMALL>): groups at (mean, std) =
    (0, 1), (30, 1), (-100, 0.05), (0, 1e-3), and one constant group per sample (variance exactly 0, the
    `var < 0 ? 0` site) whose output is SiLU(beta (scale + 1) + shift) to 1e-6 relative (three fp32 roundings
    and expf)."""
    from red_diffeq import ops  # noqa: F401
    inp = K.build(cid).inputs
    d = _dev(inp, cuda)
    got = torch.ops.red_diffeq.gn_silu(d["x"], d["gamma"], d["beta"], d["scale_shift"], d["groups"], d["eps"])
    check(got, cid)
    worst = 0.0
    for b, sl, want in K.gn_const_expected(inp):
        g = got[b, sl].double().cpu()
        rel = ((g - want[:, None, None]).abs() / want.abs()[:, None, None]).max().item()
        worst = max(worst, rel)
    record_margin(_test_id(), f"{cid} constant group, rel to fp64", worst, 1e-6)
    assert worst <= 1e-6, (cid, worst)


# ----------------------------------------------------- D. GroupNorm statistics in the conv epilogue
@pytest.mark.parametrize("cid", list(K.CONV_GN))
def test_conv_gn_silu_offsets(cuda, cid):
    """conv_group_norm_silu (rdq_conv2d_gn_silu) and conv2d_gn_silu_out: the conv output's |mean| / std is
    10 - 100 per group with either sign, sample b's input scaled by (1 + b); 32-pixel tiles straddle two
    samples at every phase (HW = 35), C / G = 8, 16 and 64, concatenated input."""
    import torch.nn as nn
    from red_diffeq import ops as O
    from red_diffeq.models import unet_ops as ops
    c = K.build(cid)
    d = _dev(c.inputs, cuda)
    cout = d["w"].shape[0]
    x, x2 = (d["x"][:, :c.cin1].contiguous(), d["x"][:, c.cin1:].contiguous()) if d["x"].shape[1] > c.cin1 \
        else (d["x"], None)
    assert O.conv_gn_fusable(x, x2, d["w"], 1, 0, d["groups"])
    with torch.no_grad():
        if c.kind == "conv_gn_out":
            got = torch.ops.red_diffeq.conv2d_gn_silu_out(x, d["w"], d["b"], 1, d["gamma"], d["beta"], d["scale_shift"],
                                                          d["groups"], d["eps"], d["post"], d["w_out"], d["b_out"])
        else:
            conv = nn.Conv2d(d["w"].shape[1], cout, 3, padding=1).to(cuda)
            norm = nn.GroupNorm(d["groups"], cout, eps=d["eps"]).to(cuda)
            conv.weight.copy_(d["w"])
            conv.bias.copy_(d["b"])
            norm.weight.copy_(d["gamma"])
            norm.bias.copy_(d["beta"])
            got = ops.conv_group_norm_silu(x, conv, norm, d["scale_shift"], skip=x2, post=d["post"])
    check(got, cid)
    assert int(O._TICKET_POOL[x.device]["pool"].abs().sum()) == 0


# ------------------------------------------------------------------ E. RED prologue and epilogue
@pytest.mark.parametrize("cid", list(K.RED))
def test_red_q_sample_and_epilogue_elementwise(cuda, cid):
    """k_red_q_sample(_t) and k_red_epilogue on a real 1000-step schedule at t = 0, 1, 500, 998, 999, n ragged
    over the 256-thread block; the clamp fires on both sides and not at all at every t (s = 3).  Reference:
    the formulas of include/red_diffeq_unet.h in fp64 on the fp32 tables.  Elementwise bounds, valid with
    or without FMA contraction (every rounding is 2^-24 relative):
      q_sample  x_t = fl(fl(a1) + fl(a2)), a1 = sa x0, a2 = s1a eps: |err| <= 2^-24 (|a1| + |a2| + |a1 + a2|)
                <= 2^-23 (|a1| + |a2|);
      epilogue  u = sr x_t, w = srm1 eps_hat: the clamp is 1-Lipschitz, so x0_hat carries <= 2^-24 (2 |u| + 2 |w|),
                the numerator u - x0_hat <= 2^-24 (4 |u| + 2 |w| + 1), the quotient and the final subtraction
                2^-24 (2 |eps'| + |eps|): |err| <= 2^-22 (|u| + |w| + 1) / srm1 + 2^-24 (2 |eps'| + |eps|), inside the
                asserted 2^-21 (|u| + |w| + 1) / srm1[t] + 2^-22 (|eps'| + |eps|)."""
    from red_diffeq import ops  # noqa: F401
    inp = K.build(cid).inputs
    d = _dev(inp, cuda)
    i64 = R.to_dtype(inp, torch.float64)
    sa, s1a = d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"]
    sr, srm1 = d["sqrt_recip_alphas_cumprod"], d["sqrt_recipm1_alphas_cumprod"]

    xt = torch.ops.red_diffeq.red_q_sample(d["x0"], d["t"], d["eps"], sa, s1a)
    ref, a1, a2 = R.red_q_sample(i64["x0"], i64["t"], i64["eps"], i64["sqrt_alphas_cumprod"],
                                 i64["sqrt_one_minus_alphas_cumprod"])
    assert torch.isfinite(xt).all()
    ratio = ((xt.double().cpu() - ref).abs() / (2.0 ** -23 * (a1.abs() + a2.abs())).clamp_min(1e-300)).max().item()
    record_margin(_test_id(), f"{cid} q_sample elementwise", ratio, 1.0)
    assert ratio <= 1.0, ratio

    xt2, t2 = torch.full_like(xt, float("nan")), torch.full_like(d["t"], -1)
    torch.ops.red_diffeq.red_q_sample_into(d["x0"], d["t"], d["eps"], sa, s1a, xt2, t2)
    assert torch.equal(xt2, xt) and torch.equal(t2, d["t"])

    # the epilogue on the builder's x_t (the fp32 q_sample of the CPU restatement): an input like any other
    got = torch.ops.red_diffeq.red_eps(d["xt"], d["t"], d["eps_hat"], d["eps"], sr, srm1)
    g64, u, w, pn, _ = R.red_epilogue(i64["xt"], i64["t"], i64["eps_hat"], i64["eps"], i64["sqrt_recip_alphas_cumprod"],
                                      i64["sqrt_recipm1_alphas_cumprod"])
    assert torch.isfinite(got).all()
    s = i64["sqrt_recipm1_alphas_cumprod"][i64["t"]].reshape(-1, 1, 1, 1)
    bound = 2.0 ** -21 * (u.abs() + w.abs() + 1) / s + 2.0 ** -22 * (pn.abs() + i64["eps"].abs())
    ratio = ((got.double().cpu() - g64).abs() / bound).max().item()
    record_margin(_test_id(), f"{cid} epilogue elementwise", ratio, 1.0)
    assert ratio <= 1.0, ratio


# ------------------------------------------------------------------------------- F. bf16 forms
@pytest.mark.parametrize("cid", list(K.LA_BF16))
def test_linear_attention_bf16_range(cuda, cid):
    """linear_attn_bf16 (k_lab_kv / k_lab_out<D, false>) on the module inputs of A (logits past 89): new
    behaviour, no reference counterpart.  Reference R_b (unet_torch_ref.linear_attention_bf16): fp64 with
    every matrix operand rounded to bf16 where the kernels round it, so the logits agree to fp32
    accumulation; bar: the op's existing bf16 bar, 3e-2 max |R_b|.  Recorded, not asserted: the distance of
    R_b from its variant that rounds only the first-stage operands (the downstream rounding noise)."""
    from red_diffeq import ops as O
    from red_diffeq.models import unet_ops as ops
    c = K.build(cid)
    x = c.inputs["x"].to(cuda)
    m = _la_module(cuda, c.inputs)
    assert O.linear_attn_bf16_fusable(x, m.to_qkv.weight, m.to_out[0].weight, m.heads)
    with torch.no_grad(), ops.precision("bf16"):
        got = ops.linear_attention(x, m)
    rb = R.eval64(c.ref, **c.inputs)
    first = R.eval64(c.ref, downstream=False, **c.inputs)
    assert torch.isfinite(got).all(), f"{cid}: {int((~torch.isfinite(got)).sum())} non-finite outputs"
    err = R.rel_err(got, rb)
    record_margin(_test_id(), f"{cid} R_b vs first-stage-only rounding (not asserted)", R.rel_err(first, rb), 3e-2)
    record_margin(_test_id(), f"{cid} bf16 kernel vs R_b", err, 3e-2)
    assert err <= 3e-2, (cid, err)


@pytest.mark.parametrize("cid", list(K.CONV_GN_BF16))
def test_conv_bf16_gn_silu_offsets(cuda, cid):
    """conv2d_bf16_gn_silu at |mean| / std = 16 of the conv output (larger offsets quantise away in the bf16
    raw output, a stated property of the form): fp64 on bf16-rounded operands, the raw output rounded to
    bf16 before the statistics; the bar of test_conv_bf16_gn_silu_fused (1e-5 of the output range).  That test
    takes the raw output from the kernel's own conv; against fp64 a raw value within the fp32 accumulation
    bound of a bf16 rounding tie may round to either neighbour, so at those elements (marked by the reference,
    their share recorded) the nearer of the two legitimate outputs is compared; every other element has one."""
    from red_diffeq import ops as O
    from red_diffeq.models import unet_ops as ops
    c = K.build(cid)
    d = _dev(c.inputs, cuda)
    assert O.conv_gn_bf16_fusable(d["x"], None, d["w"], 1, ops.PLAIN, d["groups"])
    with torch.no_grad(), ops.precision("bf16"):
        got = torch.ops.red_diffeq.conv2d_bf16_gn_silu(d["x"], None, d["w"], d["b"], 1, ops.PLAIN, d["gamma"], d["beta"],
                                                       d["scale_shift"], d["groups"], d["eps"], d["post"])
    ref, alt, amb = R.eval64(c.ref, **c.inputs)
    assert torch.isfinite(got).all()
    g = got.double().cpu()
    took_alt = amb & ((g - alt).abs() < (g - ref).abs())
    err = float(torch.minimum((g - ref).abs(), (g - alt).abs()).max() / ref.abs().max())
    print(f"{cid}: err {err:.3g}; {float(amb.double().mean()):.3g} of the elements near a bf16 tie, "
          f"{int(took_alt.sum())} of {amb.numel()} on the other neighbour")
    record_margin(_test_id(), f"{cid} share of elements near a bf16 rounding tie (not asserted)",
                  float(amb.double().mean()), 1.0)
    record_margin(_test_id(), cid, err, 1e-5)
    assert amb.double().mean() < 0.15              # (worst-case accumulation bound: ~0.11 here) the exception
    assert err <= 1e-5, (cid, err)
