"""Every route of the conv kernels (csrc/unet.hip: k_conv_ig, k_conv_cc, k_conv3_f32, k_conv_bf16, k_conv3_bf16,
k_stem7 / k_stem7x2, k_conv_reduce, k_pack_w_bf16) at ragged shapes, compared PER ELEMENT with an fp64 evaluation
of the contract of rdq_conv_desc.  Cases, reference and the derived bar: tests/conv_cases.py (checked on the CPU
by tests/test_conv_cases_host.py, which also shows which kernel mistakes the comparison catches).  Each case
asserts the route it ran (rdq_conv2d_route), so a change of the routing cannot silently move a case to another
kernel.  tests/test_gpu_unet.py keeps the product's large-K shapes."""
import ctypes

import pytest
import torch
import torch.nn as nn

import conv_cases as C
from conftest import record_margin

pytestmark = pytest.mark.gpu


class options:
    """Set U-Net kernel options for a block and put the old values back, whatever happens inside."""

    def __init__(self, opts):
        self.opts, self.old = dict(opts), []

    def __enter__(self):
        from red_diffeq import _hip
        L = _hip.lib()
        for k, v in self.opts.items():
            old = L.rdq_unet_set_option(k, v)
            assert old >= 0, (k, v, old)
            self.old.append((k, old))
        return self

    def __exit__(self, *exc):
        from red_diffeq import _hip
        L = _hip.lib()
        for k, old in reversed(self.old):
            L.rdq_unet_set_option(k, old)


def _desc(s):
    from red_diffeq import _hip
    B, H, W = s.geom
    return _hip.ConvDesc(B=B, cin1=s.cin1, cin2=s.cin2, H=H, W=W, cout=s.cout, kh=s.kh, kw=s.kw, pad=s.pad,
                         in_mode=s.mode)


def _dev(t, cuda):
    return t.to(cuda).contiguous() if t is not None else None


def _module(case, cuda):
    s = case.spec
    conv = nn.Conv2d(s.cin1 + s.cin2, s.cout, (s.kh, s.kw), padding=s.pad, bias=case.bias is not None)
    with torch.no_grad():
        conv.weight.copy_(case.w)
        if case.bias is not None:
            conv.bias.copy_(case.bias)
    return conv.to(cuda)


def run(case, cuda, ws=None, tickets=None):
    """The case's op on the device under its options -> CPU fp32; the route is asserted first."""
    from red_diffeq import _hip, ops as O
    from red_diffeq.models import unet_ops as ops
    s = case.spec
    ws = s.ws if ws is None else ws
    tickets = s.tickets if tickets is None else tickets
    L = _hip.lib()
    d = _desc(s)
    x, x2, res = _dev(case.x, cuda), _dev(case.x2, cuda), _dev(case.res, cuda)
    w, bias = _dev(case.w, cuda), _dev(case.bias, cuda)
    st = _hip.stream_of(x)
    with options(s.opts), torch.no_grad():
        if s.route != C.STEM:
            assert L.rdq_conv2d_route(ctypes.byref(d), int(s.bf16)) == s.route, case.id
        if s.via == "ops":
            conv = _module(case, cuda)
            assert ws == "full"
            if s.bf16:
                assert O.bf16_eligible(conv.weight), case.id
                with ops.precision("bf16"):
                    y = ops.conv2d(x, conv, x2=x2, mode=s.mode, residual=res)
            else:
                y = ops.conv2d(x, conv, x2=x2, mode=s.mode, residual=res)
        else:
            y = torch.empty(case.shape, device=cuda)
            if s.route == C.STEM:
                _hip.check(L.rdq_conv2d_stem(ctypes.byref(d), _hip.ptr(x), _hip.ptr(w), _hip.ptr(bias), _hip.ptr(y), st),
                           "rdq_conv2d_stem")
            elif s.bf16:
                assert ws == "none"
                wp = O._bf16_pack(w, d, st)
                _hip.check(L.rdq_conv2d_bf16(ctypes.byref(d), _hip.ptr(x), _hip.ptr(x2), _hip.ptr(wp), _hip.ptr(bias),
                                             _hip.ptr(res), _hip.ptr(y), None, 0, st), "rdq_conv2d_bf16")
            else:
                full = int(L.rdq_conv2d_ws_bytes(ctypes.byref(d)))
                nws = {"full": full, "half": full // 2, "none": 0}[ws]
                wsb = torch.empty(nws, dtype=torch.uint8, device=cuda) if nws else None
                tk = O._tickets(x.device, int(L.rdq_conv2d_tickets(ctypes.byref(d)))) if tickets and nws else None
                _hip.check(L.rdq_conv2d(ctypes.byref(d), _hip.ptr(x), _hip.ptr(x2), _hip.ptr(w), _hip.ptr(bias),
                                        _hip.ptr(res), _hip.ptr(y), _hip.ptr(wsb), nws, tk, st), "rdq_conv2d")
        torch.cuda.synchronize()
    assert tuple(y.shape) == case.shape
    return y.cpu()


def tickets_are_zero(cuda):
    from red_diffeq import ops as O
    st = O._TICKET_POOL.get(torch.device(cuda))
    return st is None or int(st["pool"].abs().sum()) == 0


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_case_per_element(cuda, cid):
    case = C.build(cid)
    got = run(case, cuda)
    ratio, i = C.worst_ratio(got, case)
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), case.shape))
    print(f"{cid}: worst |got - ref64| / bar = {ratio:.4f} at (b, n, oh, ow) = {idx}")
    record_margin("conv_edges_per_element", cid, ratio, 1.0)
    assert ratio <= 1.0, (cid, ratio, idx, float(got[idx]), float(case.ref64[idx]))
    assert tickets_are_zero(cuda)


@pytest.mark.parametrize("cin", [136, 128])
def test_cc_split_tickets_bitwise(cuda, cin):
    """Split-K combined in the launch (arrival tickets) and by k_conv_reduce: the same slab order, bit for bit;
    the CASES spec splits 17 stages as 4 + 4 + 4 + 4 + 1 and 16 stages evenly."""
    from red_diffeq import _hip
    base = f"cc-{cin}to64-3x3p1-1x5x7"
    case = C.build(base + "-tickets")
    d = _desc(case.spec)
    slab = 2 * 32 * 64 * 4                       # 2 tiles of CC_BM x CC_BN floats
    assert int(_hip.lib().rdq_conv2d_ws_bytes(ctypes.byref(d))) == C.cc_splits(35, 64, cin, 3) * slab
    assert C.cc_splits(35, 64, cin, 3) == (5 if cin == 136 else 4)
    a = run(case, cuda, tickets=True)
    b = run(case, cuda, tickets=False)
    assert torch.equal(a, b)
    assert tickets_are_zero(cuda)


@pytest.mark.parametrize("prefix", C.IMPULSE)
def test_impulse_bitwise(cuda, prefix):
    """A single 1.0 in the last channel at a corner pixel of the last sample (conv_cases.impulse): the output is the
    weights placed by the contract, bit for bit (every other product and every other slab is an exact zero), and 0
    elsewhere."""
    case = C.impulse(C.resolve(prefix))
    got = run(case, cuda)
    bad = (got != case.expect).nonzero()
    assert bad.numel() == 0, (case.id, bad[:8].tolist())
    assert tickets_are_zero(cuda)


def test_pack_w_bf16_layout(cuda):
    """k_pack_w_bf16: [cout][tap][cinp] of torch's round-to-nearest-even bf16, zeros for ci >= cin (cin % 32 != 0)."""
    from red_diffeq import _hip
    L = _hip.lib()
    g = torch.Generator().manual_seed(11)
    for cout, cin, kh, kw in ((5, 40, 3, 3), (3, 7, 5, 5), (70, 33, 1, 1)):
        w = torch.randn(cout, cin, kh, kw, generator=g)
        w.view(-1)[::3] *= 2.0 ** -7                                   # ties and small values among them
        w.view(-1)[1] = 1.0 + 2.0 ** -8                                # an exact tie: rounds to even (1.0)
        w.view(-1)[2] = 1.0 + 2.0 ** -7 + 2.0 ** -8                    # a tie that rounds up to even
        d = _hip.ConvDesc(B=1, cin1=cin, cin2=0, H=4, W=4, cout=cout, kh=kh, kw=kw, pad=0, in_mode=0)
        cinp = (cin + 31) // 32 * 32
        n = int(L.rdq_conv2d_bf16_wpack_bytes(ctypes.byref(d)))
        assert n == cout * kh * kw * cinp * 2
        wp = torch.full((n,), 0xAB, dtype=torch.uint8, device=cuda)
        wd = w.to(cuda)
        _hip.check(L.rdq_conv2d_bf16_pack(ctypes.byref(d), _hip.ptr(wd), _hip.ptr(wp), _hip.stream_of(wd)), "pack")
        torch.cuda.synchronize()
        got = wp.cpu().view(torch.int16).view(cout, kh * kw, cinp)
        want = torch.zeros(cout, kh * kw, cinp, dtype=torch.bfloat16)
        want[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin).to(torch.bfloat16)
        assert torch.equal(got, want.view(torch.int16)), (cout, cin, kh, kw)
