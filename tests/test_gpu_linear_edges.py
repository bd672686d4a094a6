"""Every route of the time-embedding and linear kernels (csrc/unet.hip: k_linear, k_sinusoidal, k_time_mlp,
k_time_mlp_b, k_linear_silu_multi, k_linear_silu_multi_b, k_wdot_silu_b, lsm_rows of k_conv_cc_lsm, the time-MLP
role of k_unet_head) at ragged sizes through the C ABI.  Cases, fp64 reference and the derived per-element bar:
tests/linear_cases.py (checked on the CPU by tests/test_linear_cases_host.py, which also shows which kernel mistakes
the comparison catches).  Each case asserts the route it ran (rdq_time_mlp_route, rdq_linear_silu_multi_route).
Every output buffer is pre-filled with a NaN pattern and followed by a guard region of the same pattern: an
element left unwritten fails its bar, and a store past the output is seen in the guard.  The fused and batched
forms are compared bit for bit with the per-sample entry points, as the kernels' comments promise."""
import ctypes

import pytest
import torch

import linear_cases as C
from conftest import record_margin

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF          # a quiet NaN with a payload no kernel produces
GUARD = 64                     # floats after every output


class Out:
    """A device output of `shape` floats, pre-filled with NAN_BITS, GUARD more floats of it behind."""

    def __init__(self, shape, cuda):
        self.shape = tuple(shape)
        self.n = 1
        for v in self.shape:
            self.n *= v
        self.raw = torch.full((self.n + GUARD,), NAN_BITS, dtype=torch.int32, device=cuda)

    def at(self, floats=0):
        return ctypes.c_void_p(self.raw.data_ptr() + 4 * floats)

    def bits(self):
        """The output's bit patterns on the CPU, after checking the guard."""
        raw = self.raw.cpu()
        assert bool((raw[self.n:] == NAN_BITS).all()), "store past the output"
        return raw[:self.n].view(self.shape)

    def result(self):
        return self.bits().view(torch.float32)


def _dev(t, cuda):
    return t.to(cuda).contiguous() if t is not None else None


def _at(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + t.element_size() * elems) if t is not None else ctypes.c_void_p(0)


def _ptrs(ps):
    return (ctypes.c_void_p * len(ps))(*ps)


def _stream(cuda):
    return ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)


def _lib():
    from red_diffeq import _hip
    return _hip.lib()


def _ok(rc, what):
    assert rc == 0, (what, rc)


def launch_lsm(cuda, B, cin, x, w, b, rows, outs, sample=0):
    """rdq_linear_silu_multi on B samples starting at `sample` of x (device) into outs at the same rows."""
    n = len(w)
    _ok(_lib().rdq_linear_silu_multi(B, cin, _at(x, sample * cin), n, _ptrs([_at(t) for t in w]),
                                     _ptrs([_at(t) for t in b]), (ctypes.c_int32 * n)(*rows),
                                     _ptrs([o.at(sample * r) for o, r in zip(outs, rows)]), _stream(cuda)),
        "rdq_linear_silu_multi")


def launch_tm(cuda, B, s, t, w1, b1, w2, b2, out, sample=0):
    _ok(_lib().rdq_time_mlp(B, s.dim, s.theta, _at(t, sample), _at(w1), _at(b1), s.hid, _at(w2), _at(b2), s.rows[0],
                            out.at(sample * s.rows[0]), _stream(cuda)), "rdq_time_mlp")


def run(case, cuda):
    """The case through its entry point -> list of CPU fp32 outputs; the route is asserted first."""
    s, L = case.spec, _lib()
    if s.kind == "emb":
        t = _dev(case.t, cuda)
        y = Out((s.B, s.dim), cuda)
        _ok(L.rdq_sinusoidal_emb(s.B, s.dim, s.theta, _at(t), y.at(), _stream(cuda)), "rdq_sinusoidal_emb")
        outs = [y]
    elif s.kind == "tm":
        assert L.rdq_time_mlp_route(s.B) == s.route, case.id
        t, w1, b1, w2, b2 = (_dev(v, cuda) for v in (case.t, case.w1, case.b1, case.w[0], case.b[0]))
        outs = [Out((s.B, s.rows[0]), cuda)]
        launch_tm(cuda, s.B, s, t, w1, b1, w2, b2, outs[0])
    elif s.kind == "lin":
        x, w, b = _dev(case.x, cuda), _dev(case.w[0], cuda), _dev(case.b[0], cuda)
        outs = [Out((s.B, s.rows[0]), cuda)]
        _ok(L.rdq_linear(s.B, s.cin, s.rows[0], _at(x), _at(w), _at(b), s.act_in, s.act_out, outs[0].at(), _stream(cuda)),
            "rdq_linear")
    else:
        assert L.rdq_linear_silu_multi_route(s.B, s.cin) == s.route, case.id
        x, w, b = _dev(case.x, cuda), [_dev(v, cuda) for v in case.w], [_dev(v, cuda) for v in case.b]
        outs = [Out((s.B, r), cuda) for r in s.rows]
        launch_lsm(cuda, s.B, s.cin, x, w, b, s.rows, outs)
    torch.cuda.synchronize()
    return [o.result() for o in outs]


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_case_per_element(cuda, cid):
    case = C.build(cid)
    s = case.spec
    got = run(case, cuda)
    ratio, j, i = C.worst_ratio(got, case)
    b, o = divmod(i, got[j].shape[1])
    print(f"{cid}: worst |got - ref64| / bar = {ratio:.4f} at linear {j}, (sample, row) = ({b}, {o})")
    record_margin(f"linear_edges_{s.kind}_{C.ROUTE_NAMES.get(case.route, 'only')}", cid, ratio, 1.0)
    assert ratio <= 1.0, (cid, ratio, j, b, o, float(got[j][b, o]), float(case.ref64[j][b, o]))
    if s.kind == "emb":                     # t = 0: sin is exactly 0 and cos exactly 1
        assert int(case.t[0]) == 0
        assert bool((got[0][0, :s.dim // 2] == 0).all()) and bool((got[0][0, s.dim // 2:] == 1).all())


@pytest.mark.parametrize("cid", C.BATCHED_IDS)
def test_batched_equals_per_sample_bitwise(cuda, cid):
    """Every sample's row of a BATCHED / WDOT launch is bit for bit the PER_SAMPLE launch of that sample alone (the
    time MLP also at steps spread to 999)."""
    case = C.build(cid)
    s, L = case.spec, _lib()
    assert s.route != C.PER_SAMPLE
    if s.kind == "tm":
        assert L.rdq_time_mlp_route(s.B) == s.route and L.rdq_time_mlp_route(1) == C.PER_SAMPLE
        w1, b1, w2, b2 = (_dev(v, cuda) for v in (case.w1, case.b1, case.w[0], case.b[0]))
        for steps in (case.t, C.wide_steps(case.t)):
            t = _dev(steps, cuda)
            whole, single = Out((s.B, s.rows[0]), cuda), Out((s.B, s.rows[0]), cuda)
            launch_tm(cuda, s.B, s, t, w1, b1, w2, b2, whole)
            for b in range(s.B):
                launch_tm(cuda, 1, s, t, w1, b1, w2, b2, single, sample=b)
            torch.cuda.synchronize()
            assert torch.equal(whole.bits(), single.bits()), (cid, steps.tolist())
            assert bool(torch.isfinite(whole.result()).all())
    else:
        assert L.rdq_linear_silu_multi_route(s.B, s.cin) == s.route
        assert L.rdq_linear_silu_multi_route(1, s.cin) == C.PER_SAMPLE
        x, w, b = _dev(case.x, cuda), [_dev(v, cuda) for v in case.w], [_dev(v, cuda) for v in case.b]
        whole, single = ([Out((s.B, r), cuda) for r in s.rows] for _ in range(2))
        launch_lsm(cuda, s.B, s.cin, x, w, b, s.rows, whole)
        for i in range(s.B):
            launch_lsm(cuda, 1, s.cin, x, w, b, s.rows, single, sample=i)
        torch.cuda.synchronize()
        for j, (a, c) in enumerate(zip(whole, single)):
            assert torch.equal(a.bits(), c.bits()), (cid, j)
            assert bool(torch.isfinite(a.result()).all())


@pytest.mark.parametrize("fid", C.fused_lsm_ids())
def test_conv_lsm_equals_separate_calls_bitwise(cuda, fid):
    """rdq_conv2d_gn_silu_lsm: the conv output and every linear's output are bit for bit those of rdq_conv2d_gn_silu
    (scale/shift = linear 0) and of rdq_linear_silu_multi on its PER_SAMPLE route."""
    from red_diffeq import _hip
    f, L = C.build_fused_lsm(fid), _lib()
    B, cc, H, W = f.geom
    d = _hip.ConvDesc(B=B, cin1=cc, cin2=0, H=H, W=W, cout=f.cout, kh=3, kw=3, pad=1, in_mode=0)
    nws = int(L.rdq_conv2d_gn_ws_bytes(ctypes.byref(d), f.G))
    assert nws > 0
    assert L.rdq_linear_silu_multi_route(f.B, f.cin) == C.PER_SAMPLE
    x, cw, cb, ga, be, temb = (_dev(v, cuda) for v in (f.x, f.cw, f.cb, f.gamma, f.beta, f.temb))
    w, b = [_dev(v, cuda) for v in f.w], [_dev(v, cuda) for v in f.b]
    n, st = len(w), _stream(cuda)
    rows = (ctypes.c_int32 * n)(*f.rows)
    ws = [torch.zeros(nws, dtype=torch.uint8, device=cuda) for _ in range(2)]
    y_f, y_s = Out(f.geom, cuda), Out(f.geom, cuda)
    ly_f, ly_s = ([Out((B, r), cuda) for r in f.rows] for _ in range(2))
    _ok(L.rdq_conv2d_gn_silu_lsm(ctypes.byref(d), _at(x), None, _at(cw), _at(cb), f.G, f.eps, _at(ga), _at(be), None,
                                 y_f.at(), _at(ws[0]), nws, None, f.cin, _at(temb), n, _ptrs([_at(t) for t in w]),
                                 _ptrs([_at(t) for t in b]), rows, _ptrs([o.at() for o in ly_f]), 0, st),
        "rdq_conv2d_gn_silu_lsm")
    launch_lsm(cuda, B, f.cin, temb, w, b, f.rows, ly_s)
    _ok(L.rdq_conv2d_gn_silu(ctypes.byref(d), _at(x), None, _at(cw), _at(cb), f.G, f.eps, _at(ga), _at(be), ly_s[0].at(),
                             None, y_s.at(), _at(ws[1]), nws, None, st), "rdq_conv2d_gn_silu")
    torch.cuda.synchronize()
    for j, (a, c) in enumerate(zip(ly_f, ly_s)):
        assert torch.equal(a.bits(), c.bits()), (fid, j)
        assert bool(torch.isfinite(a.result()).all())
    assert torch.equal(y_f.bits(), y_s.bits()), fid
    assert bool(torch.isfinite(y_f.result()).all())


@pytest.mark.parametrize("fid", C.fused_head_ids())
def test_unet_head_equals_separate_calls_bitwise(cuda, fid):
    """rdq_unet_head: y and temb are bit for bit those of rdq_conv2d (no workspace: no K split) and of rdq_time_mlp on
    its PER_SAMPLE route."""
    from red_diffeq import _hip
    f, L = C.build_fused_head(fid), _lib()
    d = _hip.ConvDesc(B=f.B, cin1=1, cin2=0, H=f.H, W=f.W, cout=f.cout, kh=f.k, kw=f.k, pad=f.pad, in_mode=0)
    assert L.rdq_conv2d_route(ctypes.byref(d), 0) == 1             # RDQ_CONV_ROUTE_IG
    assert L.rdq_time_mlp_route(f.B) == C.PER_SAMPLE
    x, cw, cb, t, w1, b1, w2, b2 = (_dev(v, cuda) for v in (f.x, f.cw, f.cb, f.t, f.w1, f.b1, f.w2, f.b2))
    st = _stream(cuda)
    shape = (f.B, f.cout, f.H, f.W)
    y_f, y_s, te_f, te_s = Out(shape, cuda), Out(shape, cuda), Out((f.B, f.out), cuda), Out((f.B, f.out), cuda)
    _ok(L.rdq_unet_head(ctypes.byref(d), _at(x), _at(cw), _at(cb), y_f.at(), f.dim, f.theta, _at(t), _at(w1), _at(b1),
                        f.hid, _at(w2), _at(b2), f.out, te_f.at(), st), "rdq_unet_head")
    _ok(L.rdq_conv2d(ctypes.byref(d), _at(x), None, _at(cw), _at(cb), None, y_s.at(), None, 0, None, st), "rdq_conv2d")
    _ok(L.rdq_time_mlp(f.B, f.dim, f.theta, _at(t), _at(w1), _at(b1), f.hid, _at(w2), _at(b2), f.out, te_s.at(), st),
        "rdq_time_mlp")
    torch.cuda.synchronize()
    assert torch.equal(te_f.bits(), te_s.bits()), fid
    assert torch.equal(y_f.bits(), y_s.bits()), fid
    assert bool(torch.isfinite(te_f.result()).all()) and bool(torch.isfinite(y_f.result()).all())
