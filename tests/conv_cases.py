"""TEST INFRASTRUCTURE: the conv edge cases (tests/test_gpu_conv_edges.py on the GPU, tests/test_conv_cases_host.py
on the CPU).  Every kernel family of rdq_conv2d / rdq_conv2d_bf16 / rdq_conv2d_stem at ragged shapes, compared
PER ELEMENT with an fp64 evaluation of the contract of rdq_conv_desc (include/red_diffeq_unet.h):

    out[b,n,oh,ow] = bias[n] + res[b,n,oh,ow] + sum_{c,ky,kx} w[n,c,ky,kx] * in[b,c,oh+ky-pad,ow+kx-pad]

`in` zero outside the image, output H x W (conv_def).  `in` is the LOGICAL input (logical_input: concat, nearest
x2 upsample or 2x2 unshuffle by plain indexing).  For the bf16 routes `in` and `w` are first rounded to bf16 by
torch; bias and residual stay fp32.

build(case_id) is a pure function of the case id: CPU fp32 tensors.  Channel c of the input is scaled by
2^((c mod 7) - 3) and output channel n of the weights by 2^((n mod 5) - 4) / sqrt(K), so small-magnitude
channels exist and an error confined to one of them cannot hide under a global maximum.

The bar is derived, not measured (bar()).  With S = |bias| + |res| + sum |w| |in| (the same definition on absolute
values, fp64), an fp32 accumulation of K exact-product-then-round terms in ANY order, plus the split-K slab sum
(S_split adds), the bias add and the residual add, is within (K + S_split + 2) u S of the exact value, u = 2^-24
(the fp32 MFMA is a k-ordered fmaf chain, one rounding per product-and-add).  The bf16 routes use 2^-23: the
products of two bf16 values are exact in fp32, and one ulp per add (faithful rounding) is assumed for the
accumulation inside v_mfma_f32_32x32x16_bf16.  K <= 1300 in every case: beyond that the worst-case bound
approaches the size of one dropped term."""
import math
import types

import torch
import torch.nn.functional as F

INVALID, IG, CC, C3F, BF16_TAP, C3_BF16, STEM = 0, 1, 2, 3, 4, 5, 6      # RDQ_CONV_ROUTE_*; STEM: rdq_conv2d_stem
ROUTE_NAMES = {IG: "ig", CC: "cc", C3F: "c3f", BF16_TAP: "bf16tap", C3_BF16: "c3bf16", STEM: "stem"}
PLAIN, UPSAMPLE2, UNSHUFFLE2 = 0, 1, 2
OPT_BF16_PER_TAP, OPT_CONV3_MIN_TILES, OPT_CONV3F_MIN_TILES = 1, 2, 4   # RDQ_UNET_OPT_*
K_MAX = 1300
U32, U_BF16_ACC = 2.0 ** -24, 2.0 ** -23

GEOMS = {
    "3x5x7": (3, 5, 7),      # HW = 35: 32-pixel tiles straddle samples, last tile 9 pixels; 3 samples in a 256 tile
    "4x9x9": (4, 9, 9),      # the deepest product level; two halo tiles, the second ragged
    "2x3x72": (2, 3, 72),    # W = C3_WMAX; the halo is taller than the image
    "3x1x8": (3, 1, 8),      # H = 1
    "3x12x1": (3, 12, 1),    # W = 1
}
G_MODE = (2, 6, 10)          # upsample input (3, 5), unshuffle input (12, 20)
G_SPLIT = (1, 5, 7)
STEM_GEOMS = {"2x1x64": (2, 1, 64), "2x3x65": (2, 3, 65), "2x5x72": (2, 5, 72), "2x7x71": (2, 7, 71)}


def _spec(route, geom, cin1, cin2, cout, kh, kw, pad, mode=PLAIN, bias=True, res=True, ws="full", tickets=True,
          via="ops", opts=None):
    return types.SimpleNamespace(route=route, bf16=route in (BF16_TAP, C3_BF16), geom=geom, cin1=cin1, cin2=cin2,
                                 cout=cout, kh=kh, kw=kw, pad=pad, mode=mode, bias=bias, res=res, ws=ws,
                                 tickets=tickets, via=via, opts=dict(opts or {}))


def _name(s, extra=""):
    B, H, W = s.geom
    cin = f"{s.cin1}+{s.cin2}" if s.cin2 else f"{s.cin1}"
    mode = {PLAIN: "", UPSAMPLE2: "-up", UNSHUFFLE2: "-unsh"}[s.mode]
    return (f"{ROUTE_NAMES[s.route]}-{cin}to{s.cout}-{s.kh}x{s.kw}p{s.pad}{mode}-{B}x{H}x{W}"
            f"{'' if s.bias else '-nobias'}{'' if s.res else '-nores'}{extra}")


def _cases():
    out = {}

    def add(s, extra=""):
        cid = _name(s, extra)
        assert cid not in out, cid
        out[cid] = s

    g0 = GEOMS["3x5x7"]
    # ---------------------------------------------------------------------------------------------- IG
    # a workspace and tickets through the operator (split-K through k_conv_reduce where K allows), none via the C ABI
    ig = [(3, 0, 5, 3, 3, 1), (7, 0, 70, 3, 3, 1), (33, 0, 64, 3, 3, 1), (4, 0, 6, 3, 3, 1), (2, 0, 16, 7, 7, 3),
          (5, 6, 20, 3, 3, 1), (5, 0, 3, 1, 1, 0)]
    ig0 = [(5, 0, 9, 5, 5, 2), (6, 0, 4, 1, 3, 1), (6, 0, 4, 3, 1, 1), (40, 0, 5, 5, 5, 2)]   # launch_conv_ig<0>
    for i, f in enumerate(ig):
        add(_spec(IG, g0, *f, bias=i % 2 == 0, res=i % 3 != 1))
    for f in ig0:
        add(_spec(IG, g0, *f, via="abi"))          # not nn.Conv2d's (1x3 / 3x1 with one pad) or simply via the ABI
    for gname, g in GEOMS.items():
        if gname != "3x5x7":
            for f in ((3, 0, 5, 3, 3, 1), (33, 0, 64, 3, 3, 1)):
                add(_spec(IG, g, *f))
            add(_spec(IG, g, 5, 0, 9, 5, 5, 2, via="abi"))
    add(_spec(IG, g0, 33, 0, 64, 3, 3, 1, ws="none", via="abi"), "-nows")
    add(_spec(IG, g0, 40, 0, 5, 5, 5, 2, ws="none", via="abi"), "-nows")
    add(_spec(IG, G_MODE, 4, 0, 6, 3, 3, 1, mode=UPSAMPLE2))
    add(_spec(IG, G_MODE, 8, 0, 12, 3, 3, 1, mode=UNSHUFFLE2))
    add(_spec(IG, G_MODE, 12, 0, 7, 1, 1, 0, mode=UNSHUFFLE2, res=False))
    add(_spec(IG, G_MODE, 64, 0, 40, 1, 1, 0, mode=UPSAMPLE2))      # 1x1 on an upsampled input: not the CC form
    # ---------------------------------------------------------------------------------------------- CC
    for gname, g in GEOMS.items():
        add(_spec(CC, g, 8, 0, 8, 3, 3, 1, bias=gname != "4x9x9", res=gname != "3x1x8"))
        add(_spec(CC, g, 16, 0, 72, 3, 3, 1))
        add(_spec(CC, g, 24, 16, 64, 3, 3, 1))
        add(_spec(CC, g, 64, 0, 40, 1, 1, 0))
        add(_spec(CC, g, 64, 64, 130, 1, 1, 0, bias=gname != "3x12x1"))
    for g in (g0, GEOMS["4x9x9"]):
        for pad in (0, 2):
            add(_spec(CC, g, 8, 0, 8, 3, 3, pad, via="abi"))
    add(_spec(CC, G_MODE, 16, 0, 72, 3, 3, 1, mode=UPSAMPLE2))
    add(_spec(CC, G_MODE, 256, 0, 64, 1, 1, 0, mode=UNSHUFFLE2))
    for cin in (136, 128):        # 17 stages: 5 slabs, the last of one stage; 16 stages: 4 even slabs
        add(_spec(CC, G_SPLIT, cin, 0, 64, 3, 3, 1, via="abi", tickets=True), "-tickets")
        add(_spec(CC, G_SPLIT, cin, 0, 64, 3, 3, 1, via="abi", tickets=False), "-reduce")
        add(_spec(CC, G_SPLIT, cin, 0, 64, 3, 3, 1, via="abi", ws="half", tickets=True), "-halfws")
        add(_spec(CC, G_SPLIT, cin, 0, 64, 3, 3, 1), "-op")
    # ---------------------------------------------------------------------------------------------- C3F
    o3f = {OPT_CONV3F_MIN_TILES: 1}
    for gname, g in GEOMS.items():
        add(_spec(C3F, g, 8, 0, 64, 3, 3, 1, opts=o3f, bias=gname != "2x3x72", res=gname != "3x12x1"))
        add(_spec(C3F, g, 40, 0, 64, 3, 3, 1, opts=o3f))
        add(_spec(C3F, g, 24, 16, 128, 3, 3, 1, opts=o3f))
    add(_spec(C3F, G_MODE, 16, 0, 64, 3, 3, 1, mode=UPSAMPLE2, opts=o3f))
    # ------------------------------------------------------------------------------------------ C3_BF16
    o3 = {OPT_CONV3_MIN_TILES: 1}
    for gname, g in GEOMS.items():
        add(_spec(C3_BF16, g, 8, 0, 64, 3, 3, 1, opts=o3, bias=gname != "2x3x72", res=gname != "3x12x1"))
        add(_spec(C3_BF16, g, 40, 0, 128, 3, 3, 1, opts=o3))
        add(_spec(C3_BF16, g, 64, 8, 64, 3, 3, 1, opts=o3))
    add(_spec(C3_BF16, G_MODE, 16, 0, 64, 3, 3, 1, mode=UPSAMPLE2, opts=o3))
    # ----------------------------------------------------------------------------------------- BF16_TAP
    tap = [(8, 0, 16, 3, 3, 1), (24, 16, 40, 3, 3, 1), (16, 0, 130, 3, 3, 1), (64, 0, 40, 1, 1, 0), (3, 0, 32, 5, 5, 2),
           (2, 0, 16, 7, 7, 3)]
    for i, f in enumerate(tap):
        add(_spec(BF16_TAP, g0, *f, bias=i % 2 == 0, res=i % 3 != 1))
    for gname, g in GEOMS.items():
        if gname != "3x5x7":
            add(_spec(BF16_TAP, g, 24, 16, 40, 3, 3, 1))
            add(_spec(BF16_TAP, g, 16, 0, 130, 3, 3, 1))
    add(_spec(BF16_TAP, g0, 24, 16, 40, 3, 3, 1, ws="none", via="abi"), "-nows")
    add(_spec(BF16_TAP, G_MODE, 8, 0, 16, 3, 3, 1, mode=UPSAMPLE2))
    add(_spec(BF16_TAP, G_MODE, 64, 0, 40, 1, 1, 0, mode=UNSHUFFLE2))
    add(_spec(BF16_TAP, g0, 8, 0, 64, 3, 3, 1, opts={OPT_CONV3_MIN_TILES: 1, OPT_BF16_PER_TAP: 1}), "-pertap")
    # --------------------------------------------------------------------------------------------- stem
    for g in STEM_GEOMS.values():
        add(_spec(STEM, g, 1, 0, 64, 7, 7, 3, res=False, via="abi"))
    add(_spec(STEM, STEM_GEOMS["2x3x65"], 1, 0, 64, 7, 7, 3, bias=False, res=False, via="abi"))
    return out


CASES = _cases()
CASE_IDS = list(CASES)


def _gen(case_id):
    g = torch.Generator()
    g.manual_seed(20240 + sum(ord(c) * (i + 1) for i, c in enumerate(case_id)) % 1000003)
    return g


def in_shape(s):
    """Shape of the tensor x the kernel is given (the logical input has s.cin1 channels at H x W)."""
    B, H, W = s.geom
    if s.mode == UPSAMPLE2:
        return (B, s.cin1, H // 2, W // 2)
    if s.mode == UNSHUFFLE2:
        return (B, s.cin1 // 4, 2 * H, 2 * W)
    return (B, s.cin1, H, W)


def logical_input(x, x2, mode):
    """The (B, cin1 + cin2, H, W) tensor the conv sums over, by plain indexing."""
    if mode == UPSAMPLE2:
        B, C, h, w = x.shape
        ih = torch.arange(2 * h) // 2
        iw = torch.arange(2 * w) // 2
        x = x[:, :, ih][:, :, :, iw]
    elif mode == UNSHUFFLE2:                      # channel c*4 + p1*2 + p2 <- x[c][2h+p1][2w+p2]
        B, C, h2, w2 = x.shape
        out = x.new_zeros(B, 4 * C, h2 // 2, w2 // 2)
        for p1 in range(2):
            for p2 in range(2):
                out[:, p1 * 2 + p2::4] = x[:, :, p1::2, p2::2]
        x = out
    return torch.cat((x, x2), dim=1) if x2 is not None else x


def conv_def(inp, w, bias, res, pad):
    """The contract, dtype-generic: zero outside the image, output H x W, one pad for both axes (negative: crop)."""
    kh, kw = w.shape[2], w.shape[3]
    y = F.conv2d(F.pad(inp, (pad, kw - 1 - pad, pad, kh - 1 - pad)), w)
    if bias is not None:
        y = y + bias.to(y.dtype).view(1, -1, 1, 1)
    if res is not None:
        y = y + res.to(y.dtype)
    return y


def rne_bf16(t):
    return t.to(torch.bfloat16).float()


def trunc_bf16(t):
    """Truncation toward zero to bf16 (mutation 6): the low 16 bits cleared."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def ig_splits(M, cout, K):
    tiles = -(-M // 32) * -(-cout // 64)
    nsteps = -(-K // 32)
    S = max(1, min(-(-256 // tiles), nsteps // 4))
    per = -(-nsteps // S)
    return -(-nsteps // per)


def cc_splits(M, cout, cin, kh, min_stages=3, split2=12):
    tiles = -(-M // 32) * -(-cout // 64)
    nstages = cin // (8 if kh == 3 else 64)
    S = max(1, min(256 // tiles, nstages // min_stages, 16))
    if 128 <= tiles < 256 and nstages >= split2:
        S = 2
    per = -(-nstages // S)
    return -(-nstages // per)


def bf_splits(M, cout, cin, taps):
    nb = 128 if cout >= 128 else 64
    tiles = -(-M // 128) * -(-cout // nb)
    nsteps = taps * (-(-cin // 32))
    S = max(1, min(-(-512 // tiles), nsteps // 4))
    per = -(-nsteps // S)
    return -(-nsteps // per)


def max_slabs(s):
    """Most split-K slabs the route sums for this case (the documented split rules of csrc/unet.hip with an
    unbounded workspace; a smaller workspace only sums fewer), 0 where the route never splits."""
    B, H, W = s.geom
    M, cin = B * H * W, s.cin1 + s.cin2
    if s.ws == "none" or s.route in (C3F, C3_BF16, STEM):
        return 0
    if s.route == IG:
        S = ig_splits(M, s.cout, cin * s.kh * s.kw)
    elif s.route == CC:
        S = cc_splits(M, s.cout, cin, s.kh)
    else:
        S = bf_splits(M, s.cout, cin, s.kh * s.kw)
    return S if S > 1 else 0


def operands(case):
    """(logical input, weights) as the route's arithmetic sees them: bf16-rounded for the bf16 routes."""
    inp = logical_input(case.x, case.x2, case.spec.mode)
    w = case.w
    if case.spec.bf16:
        inp, w = rne_bf16(inp), rne_bf16(w)
    return inp, w


def ref(case, dtype, inp=None, w=None, bias=0, res=0):
    """The contract on the case's operands in `dtype` (overrides: the mutations of the host test)."""
    i0, w0 = operands(case)
    inp = i0 if inp is None else inp
    w = w0 if w is None else w
    bias = case.bias if isinstance(bias, int) else bias
    res = case.res if isinstance(res, int) else res
    return conv_def(inp.to(dtype), w.to(dtype), bias, res, case.spec.pad)


def bar(case):
    """(K + S_split + 2) u S per element, fp64; u = 2^-24, or 2^-23 on the bf16 routes (module docstring)."""
    inp, w = operands(case)
    S = conv_def(inp.double().abs(), w.double().abs(), None if case.bias is None else case.bias.abs(),
                 None if case.res is None else case.res.abs(), case.spec.pad)
    u = U_BF16_ACC if case.spec.bf16 else U32
    return (case.K + case.s_split + 2) * u * S


def worst_ratio(got, case):
    """max over elements of |got - ref64| / bar (got: CPU fp32), and the flat index where it occurs."""
    r = (got.double() - case.ref64).abs() / case.bar
    i = int(r.argmax())
    return float(r.flatten()[i]), i


def build(case_id):
    s = CASES[case_id]
    g = _gen(case_id)
    B, H, W = s.geom
    cin = s.cin1 + s.cin2
    K = cin * s.kh * s.kw
    assert K <= K_MAX, (case_id, K)
    logical = torch.randn(B, cin, H, W, generator=g) * (2.0 ** ((torch.arange(cin) % 7) - 3)).view(1, -1, 1, 1)
    # the kernel's x: the tensor whose logical image carries the channel scaling
    if s.mode == PLAIN:
        x = logical[:, :s.cin1].contiguous()
    else:
        x = torch.randn(in_shape(s), generator=g)
        c_of = torch.arange(x.shape[1]) if s.mode == UPSAMPLE2 else None
        if s.mode == UPSAMPLE2:
            x = x * (2.0 ** ((c_of % 7) - 3)).view(1, -1, 1, 1)
        else:                                                  # logical channel c*4 + p1*2 + p2
            for p1 in range(2):
                for p2 in range(2):
                    sc = 2.0 ** (((torch.arange(x.shape[1]) * 4 + p1 * 2 + p2) % 7) - 3)
                    x[:, :, p1::2, p2::2] *= sc.view(1, -1, 1, 1)
    x2 = logical[:, s.cin1:].contiguous() if s.cin2 else None
    w = torch.randn(s.cout, cin, s.kh, s.kw, generator=g) * \
        (2.0 ** ((torch.arange(s.cout) % 5) - 4) / math.sqrt(K)).view(-1, 1, 1, 1)
    bias = torch.randn(s.cout, generator=g) if s.bias else None
    res = torch.randn(B, s.cout, H, W, generator=g) if s.res else None
    case = types.SimpleNamespace(id=case_id, spec=s, x=x, x2=x2, w=w, bias=bias, res=res, K=K,
                                 s_split=max_slabs(s), shape=(B, s.cout, H, W))
    case.ref64 = ref(case, torch.float64)
    case.bar = bar(case)
    return case


def impulse(case_id):
    """The impulse form of a case: a single 1.0 at a corner pixel of the last sample, in the last input channel
    (of x2 where there is a concat), no bias, no residual.  Every product is w * 1 or w * 0 and every other
    addend an exact zero, so the output is BIT FOR BIT the weights (bf16-rounded on the bf16 routes) placed by
    the contract, whatever the summation order or split.  The corner is the last pixel, or the first where the
    last one's whole response falls outside the image (a 1 x 3 filter with pad 1 writes row ih + 1)."""
    case = build(case_id)
    case.bias = case.res = None
    if case.spec.mode == UPSAMPLE2:
        # one pixel of x is four logical pixels: an output sums up to four weights.  On a 2^-12 grid every
        # partial sum, in any order, is exact in fp32 (and the bf16 rounding keeps the grid)
        case.w = torch.round(case.w * 4096.0) / 4096.0
    for corner in (-1, 0):
        case.x = torch.zeros_like(case.x)
        case.x2 = torch.zeros_like(case.x2) if case.x2 is not None else None
        (case.x2 if case.x2 is not None else case.x)[-1, -1, corner, corner] = 1.0
        case.expect = ref(case, torch.float64).float()
        if int((case.expect != 0).sum()) > 0:
            break
    assert torch.equal(case.expect.double(), ref(case, torch.float64)), case_id     # exact in fp32
    assert int((case.expect != 0).sum()) > 0, case_id
    return case


# one or more per route, at the smallest geometry of the route (and of each split / mode variant)
IMPULSE = ["ig-33to64-3x3p1-3x5x7", "ig-40to5-5x5p2-3x5x7", "ig-6to4-1x3p1-3x5x7", "ig-8to12-3x3p1-unsh-2x6x10",
           "cc-24+16to64-3x3p1-3x5x7", "cc-64+64to130-1x1p0-3x5x7", "cc-136to64-3x3p1-1x5x7-tickets",
           "cc-136to64-3x3p1-1x5x7-reduce", "cc-136to64-3x3p1-1x5x7-halfws", "cc-16to72-3x3p1-up-2x6x10",
           "c3f-24+16to128-3x3p1-3x5x7", "c3f-16to64-3x3p1-up-2x6x10", "c3bf16-64+8to64-3x3p1-3x5x7",
           "c3bf16-16to64-3x3p1-up-2x6x10", "bf16tap-24+16to40-3x3p1-3x5x7", "bf16tap-24+16to40-3x3p1-3x5x7-nows",
           "bf16tap-16to130-3x3p1-3x5x7", "bf16tap-64to40-1x1p0-unsh-2x6x10", "stem-1to64-7x7p3-2x1x64",
           "stem-1to64-7x7p3-2x7x71"]


def resolve(prefix):
    """The case id of an IMPULSE entry (ids carry -nobias / -nores suffixes)."""
    if prefix in CASES:
        return prefix
    ids = [c for c in CASE_IDS if c.startswith(prefix + "-nobias") or c.startswith(prefix + "-nores")]
    assert len(ids) == 1, (prefix, ids)
    return ids[0]


def border_classes(H, W):
    """name -> boolean (H, W) mask of the nine border classes; empty ones left out (H or W < 3 merges some)."""
    oh = torch.arange(H).view(-1, 1).expand(H, W)
    ow = torch.arange(W).view(1, -1).expand(H, W)
    t, b, l, r = oh == 0, oh == H - 1, ow == 0, ow == W - 1
    cls = {"tl": t & l, "tr": t & r, "bl": b & l, "br": b & r, "top": t & ~l & ~r, "bottom": b & ~l & ~r,
           "left": l & ~t & ~b, "right": r & ~t & ~b, "interior": ~t & ~b & ~l & ~r}
    return {k: v for k, v in cls.items() if bool(v.any())}
