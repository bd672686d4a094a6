"""The inputs of tests/test_gpu_unet_range.py (tests/unet_range_cases.py) reach the regimes they are
built for, checked on the CPU in fp64, and their reference is precise enough to judge a kernel: the
fp32 evaluation of every fp32 case is within E32_CAP = 1e-4 of the fp64 one (max-abs over max |ref64|), so
the bar max(1e-5, 4 e32) never exceeds 4e-4, far below the O(1) error of a wrong rescale, a dropped
chunk or a cancelled variance."""
import math

import pytest
import torch
import torch.nn.functional as F

import unet_range_cases as K
import unet_torch_ref as R


@pytest.mark.parametrize("cid", K.FP32_CASES)
def test_reference_fp32_error_within_cap(cid):
    ref64, e32, bar = K.reference(cid)
    print(f"{cid}: e32 = {e32:.3g}, bar = {bar:.3g}")
    assert torch.isfinite(ref64).all()
    assert e32 <= K.E32_CAP, (cid, e32)
    assert 1e-5 <= bar <= 4 * K.E32_CAP


def test_builders_are_pure():
    for cid in ("la_core-dh8-17x17", "gn-C16-9x9-B2-ss1", "red-n257-s3"):
        a = K.build(cid).inputs
        K._CACHE.pop((cid, K.SEED))                     # built again from (id, seed) alone
        b = K.build(cid).inputs
        for k in a:
            if isinstance(a[k], torch.Tensor):
                assert a[k].dtype in (torch.float32, torch.int64) and a[k].device.type == "cpu"
                assert torch.equal(a[k], b[k]), (cid, k)


# --------------------------------------------------------------------------------- A. softmax
@pytest.mark.parametrize("cid", list(K.LA_CORE) + list(K.LA_BLOCK))
def test_linear_attention_crafted_logits(cid):
    """Both softmaxes overflow without their max subtraction, and per (b, head, d) row one chunk's maximum
    sits >= 110 above every other chunk's (exp(m_c - M) == 0 in fp32), an earlier chunk under a later one
    for some rows and the reverse for others."""
    inp = R.to_dtype(K.build(cid).inputs, torch.float64)
    q, k = R.la_logits(inp["qkv"], inp["mem_kv"], inp["heads"])
    assert q.max() > K.EXP_OVERFLOW and k.max() > K.EXP_OVERFLOW, (float(q.max()), float(k.max()))
    cm = K.la_chunk_maxima(inp["qkv"], inp["mem_kv"], inp["heads"])          # (B, rows, nch)
    nch = cm.shape[-1]
    assert nch == (9 if "46x45" in cid else 2)
    top, dom = cm.max(dim=-1)
    others = cm.masked_fill(F.one_hot(dom, nch).bool(), -math.inf).amax(dim=-1)
    assert (top - others >= K.CHUNK_GAP).all(), float((top - others).min())
    assert float(torch.exp(torch.tensor(-K.CHUNK_GAP, dtype=torch.float32))) == 0.0
    assert set(dom.unique().tolist()) == set(range(nch))                     # every chunk dominates some row


@pytest.mark.parametrize("cid", list(K.LA_MODULE))
def test_linear_attention_module_logits(cid):
    c = K.build(cid)
    inp = R.to_dtype(c.inputs, torch.float64)
    qkv = K.la_module_qkv(inp)
    q, k = R.la_logits(qkv, inp["mem_kv"], inp["heads"])
    print(f"{cid}: max q logit {float(q.max()):.1f}, max k logit {float(k.max()):.1f}")
    assert q.max() > K.EXP_OVERFLOW and k.max() > K.EXP_OVERFLOW, (float(q.max()), float(k.max()))
    b, y, x = c.zero_pixel
    assert (c.inputs["x"][b, :, y, x] == 0).all() and (qkv[b, :, y, x] == 0).all()


@pytest.mark.parametrize("cid", list(K.ATTN))
def test_full_attention_scores(cid):
    inp = R.to_dtype(K.build(cid).inputs, torch.float64)
    s = R.attn_scores(inp["qkv"], inp["mem_kv"], inp["heads"])               # (B, heads, n, nk)
    print(f"{cid}: scores in [{float(s.min()):.1f}, {float(s.max()):.1f}]")
    assert s.max() > K.EXP_OVERFLOW
    if cid == "attn-1x3-nk7":
        assert s.shape[-1] == 7                                              # < FA_KS = 8: one split has no key
    if "dominant" in cid:
        j = 0 if cid.endswith("mem0") else s.shape[-1] - 1
        rest = torch.cat((s[..., :j], s[..., j + 1:]), dim=-1).amax(dim=-1)
        assert (s[..., j] - rest >= K.ATTN_DOMINANCE - 10).all(), float((s[..., j] - rest).min())
        v = inp["mem_kv"][1][:, 0] if cid.endswith("mem0") else \
            inp["qkv"].chunk(3, 1)[2].reshape(2, 4, 32, -1)[..., -1]
        out = R.full_attention_core(**inp).reshape(2, 4, 32, -1)
        assert (out - v.expand(2, 4, 32)[..., None]).abs().max() < 1e-12     # the output IS that key's value


# --------------------------------------------------------------------------------- B. RMSNorm
@pytest.mark.parametrize("shape,inst", list(K.RMS_SHAPES.items()))
def test_rmsnorm_shapes_land_in_their_instance(shape, inst):
    C, H, W = shape
    assert K.rms_instance(C, H * W) == inst


@pytest.mark.parametrize("cid", list(K.RMS) + list(K.CONV_RMS))
def test_rmsnorm_inputs(cid):
    c = K.build(cid)
    x = c.inputs["x"].double()
    norm = x.norm(dim=1)
    assert x.shape[0] == 2
    for b, i, j in c.zero_pixels:
        assert norm[b, i, j] == 0
    nz = norm[norm > 0] / x.shape[1] ** 0.5
    assert nz.min() < 1e-2 and nz.max() > 1e2, (float(nz.min()), float(nz.max()))   # per-pixel magnitudes spread
    assert nz.min() > 1e-4 and nz.max() < 1e4


# ------------------------------------------------------------------------------- C. GroupNorm
def test_group_norm_shapes_take_their_path():
    """(form, apply workgroups per (sample, group), separate statistics launch, statistics chunks)."""
    assert K.gn_form(64, 8, 35 * 35, 2) == ("channel", 16, False, 3)     # odd HW, two 1024-chunks, three 4096-chunks
    assert K.gn_form(16, 8, 81, 2) == ("channel", 2, False, 1)
    assert K.gn_form(512, 8, 81, 17) == ("small", 6, False, 2)           # 12 channels per workgroup, last one 4
    assert K.gn_form(512, 8, 324, 9) == ("channel", 64, True, 6)         # 4608 workgroups: k_gn_stats
    assert [s[:5] for s in K.GN_SHAPES] == [(64, 8, 35, 35, 2), (16, 8, 9, 9, 2), (512, 8, 9, 9, 17), (512, 8, 18, 18, 9)]


@pytest.mark.parametrize("cid", list(K.GN))
def test_group_norm_inputs(cid):
    inp = K.build(cid).inputs
    x = inp["x"].double()
    B, C = x.shape[:2]
    G = inp["groups"]
    xg = x.reshape(B, G, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    ratio = mean.abs() / var.sqrt()
    const = torch.zeros(B, G, dtype=torch.bool)
    for b in range(B):
        const[b, K.gn_const_group(b, G)] = True
        assert (xg[b, K.gn_const_group(b, G)] == K.GN_CONST).all()
    assert (var[const] == 0).all()
    assert ratio[~const].max() > 1000                  # mean -100 / std 0.05
    assert ((var < K.GN_EPS) & ~const).any()           # a variance below eps
    assert (ratio[~const] < 1).any()                   # and the O(1) regime next to them
    for b, sl, v in K.gn_const_expected(inp):
        assert torch.isfinite(v).all()
        if inp["scale_shift"] is not None:             # no cancellation in beta (scale + 1) + shift
            s = inp["scale_shift"][b].double()
            p = inp["beta"][sl].double() * (s[sl] + 1)
            assert (p * s[C + sl.start:C + sl.stop] >= 0).all()


# ------------------------------------------------------------------------ D. conv + GroupNorm
@pytest.mark.parametrize("cid", list(K.CONV_GN) + list(K.CONV_GN_BF16))
def test_conv_group_norm_offsets(cid):
    inp = R.to_dtype(K.build(cid).inputs, torch.float64)
    r = K.conv_gn_offsets(inp)                          # (B, G) mean / std, signed
    print(f"{cid}: |mean|/std in [{float(r.abs().min()):.2f}, {float(r.abs().max()):.1f}]")
    assert (r > 5).any() and (r < -5).any()             # offsets of either sign
    if cid in K.CONV_GN_BF16:
        big = r.abs()[:, [0, 1, 2, 4, 5, 6, 7]]
        assert big.min() > 12 and big.max() < 20        # |mean| / std ~ 16
    else:
        assert r.abs().max() > 10 and r.abs().max() < 100
        x = inp["x"]
        if x.shape[0] > 1:                              # sample b's input is (1 + b) x the unit scale
            s = x.reshape(x.shape[0], -1).std(-1)
            assert torch.allclose(s / s[0], torch.arange(1, x.shape[0] + 1, dtype=s.dtype), rtol=0.15)


# ----------------------------------------------------------------------------------- E. RED
@pytest.mark.parametrize("cid", list(K.RED))
def test_red_inputs_and_clamp_shares(cid):
    c = K.build(cid)
    inp = R.to_dtype(c.inputs, torch.float64)
    assert tuple(inp["t"].tolist()) == K.RED_T and inp["x0"].abs().max() <= 1
    assert inp["sqrt_alphas_cumprod"].shape == (1000,) and c.inputs["sqrt_alphas_cumprod"].dtype == torch.float32
    _, _, _, _, x0 = R.red_epilogue(inp["xt"], inp["t"], inp["eps_hat"], inp["eps"], inp["sqrt_recip_alphas_cumprod"],
                                    inp["sqrt_recipm1_alphas_cumprod"])
    x0 = x0.reshape(len(K.RED_T), -1)
    hi, lo = (x0 > 1).double().mean(-1), (x0 < -1).double().mean(-1)
    mid = 1 - hi - lo
    print(f"{cid}: clamped high {hi.tolist()}, low {lo.tolist()}, unclamped {mid.tolist()}")
    if c.s == 3:
        assert hi.min() >= 0.10 and lo.min() >= 0.10 and mid.min() >= 0.10, (hi, lo, mid)
