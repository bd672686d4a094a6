"""Host-side checks of caller-supplied source wavelets: the fixture's own consistency (tests/golden/wavelet.npz), the
argument checks of FWIForward(..., wavelet=) and forward(v, wavelet=), which run before any device work, the C
ABI's new symbols, and the yardstick the GPU tests use: the CPU oracle with its wavelet array overwritten in place
reproduces the reference's fp32 seismograms bit for bit, one shot's wavelet at a time."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from wavelet_cases import CASES, Fixture, WaveletOracle, bits_equal

NEW = ("rdq_fwi_forward_src", "rdq_fwi_adjoint_src", "rdq_fwi_forward_ckpt_src", "rdq_fwi_adjoint_ckpt_src")
INVALID = -10001


@pytest.mark.parametrize("tag", CASES)
def test_fixture_is_consistent(tag):
    c = Fixture(tag)
    assert c.W.dtype == np.float32 and c.W.shape == (c.B, c.ns, c.nt)
    assert len({c.W[b, s].tobytes() for b in range(c.B) for s in range(c.ns)}) == c.B * c.ns
    assert c.seis32.dtype == np.float32 and c.seis64.dtype == np.float64 and c.seis32.shape == c.r.shape
    assert c.gw64.dtype == np.float64 and c.gw32.dtype == np.float32 and c.gw64.shape == c.W.shape
    assert c.gv64.shape == c.v.shape
    assert c.eref_w.shape == (c.B,) and (c.eref_w > 0).all()
    eref = [np.linalg.norm(c.gw32[b].astype(np.float64) - c.gw64[b]) / np.linalg.norm(c.gw64[b]) for b in range(c.B)]
    np.testing.assert_allclose(eref, c.eref_w, rtol=1e-12)
    # <F(v, dW), r> = <dW, gw64>: as stored, and the right side again from the stored arrays
    lhs, rhs = c.ip
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs))
    again = float((c.dW.astype(np.float64) * c.gw64).sum())
    assert abs(again - rhs) <= 1e-10 * abs(rhs)
    # and by linearity <F(v, W), r> = <W, gw64>, with the stored fp64 seismograms
    lin = float((c.seis64 * c.r.astype(np.float64)).sum())
    assert abs(lin - float((c.W.astype(np.float64) * c.gw64).sum())) <= 1e-10 * abs(lin)
    if c.ns >= 3:   # the impulses at the first injected sample and the last
        imp = [(b, s) for b in range(c.B) for s in range(c.ns) if np.count_nonzero(c.W[b, s]) == 2]
        assert imp and all(c.W[b, s, 0] != 0 and c.W[b, s, c.nt - 1] != 0 for b, s in imp)


def test_short_is_shorter_than_the_ricker():
    from red_diffeq.solvers.pde import ricker
    c = Fixture("short")
    assert c.nt == 10
    with pytest.raises(ValueError):
        ricker(c.ctx["f"], c.ctx["dt"], c.nt)


def test_header_declares_and_library_exports_the_source_symbols():
    from red_diffeq import _hip
    hdr = open(os.path.join(ROOT, "include", "red_diffeq_fwi.h")).read()
    declared = set(re.findall(r"^int\s+(rdq_\w+)\(", hdr, flags=re.M))
    lib = _hip.load_library()
    for n in NEW:
        assert n in declared and n in _hip.SIGNATURES, n
        assert isinstance(getattr(lib, n), ctypes._CFuncPtr)
    assert "typedef struct rdq_fwi_source" in hdr
    # argument checks need no GPU: a null source, a null wav, a negative stride, each before anything else
    one = ctypes.c_void_p(8)
    for src in (None, _hip.FwiSource(wav=None, model_stride=0, shot_stride=0, gwav=None),
                _hip.FwiSource(wav=8, model_stride=-1, shot_stride=0, gwav=None),
                _hip.FwiSource(wav=8, model_stride=0, shot_stride=-4, gwav=None)):
        ref = ctypes.byref(src) if src is not None else None
        assert lib.rdq_fwi_forward_src(one, 1, one, ref, one, one, one, None) == INVALID
        assert lib.rdq_fwi_adjoint_src(one, 1, one, ref, one, one, one, one, one, one, None) == INVALID
        assert lib.rdq_fwi_forward_ckpt_src(one, 1, 4, one, ref, one, one, one, None) == INVALID
        assert lib.rdq_fwi_adjoint_ckpt_src(one, 1, 4, one, ref, one, one, one, one, one, one, one, None) == INVALID
    ok = _hip.FwiSource(wav=8, model_stride=0, shot_stride=0, gwav=None)
    assert lib.rdq_fwi_forward_src(None, 1, one, ctypes.byref(ok), one, one, one, None) == INVALID     # no plan
    assert lib.rdq_fwi_forward_src(None, 0, one, ctypes.byref(ok), one, one, one, None) == INVALID     # B < 1


def test_constructor_wavelet_is_checked_and_copied():
    from red_diffeq.solvers.pde import FWIForward
    ctx = dict(n_grid=8, nt=10, dx=10.0, dt=0.001, nbc=4, f=15.0, sz=10, gz=10, ng=8, ns=2)
    for bad in (np.zeros(9), np.zeros(11), np.zeros((1, 10)), np.zeros((2, 10)), torch.zeros(10, 1), 3.0):
        with pytest.raises(ValueError, match=r"shape \(nt,\)"):
            FWIForward(dict(ctx), "cpu", normalize=False, wavelet=bad)
    w = torch.arange(10, dtype=torch.float32)
    fwi = FWIForward(dict(ctx), "cpu", normalize=False, wavelet=w)      # nt = 10: no Ricker fits, none is built
    assert fwi.wavelet.dtype == np.float64 and fwi.wavelet.tolist() == list(range(10))
    w[0] = 5.0
    assert fwi.wavelet[0] == 0.0                                        # a copy
    assert FWIForward(dict(ctx, nt=200), "cpu", normalize=False).wavelet is None
    assert FWIForward(dict(ctx), "cpu", normalize=False, wavelet=list(range(10))).wavelet.shape == (10,)


def test_call_wavelet_checks_come_before_any_device_work():
    """CPU tensors: a bad wavelet is a ValueError; only a well-formed call reaches the device check."""
    from red_diffeq.solvers.pde import FWIForward
    ctx = dict(n_grid=8, nt=200, dx=10.0, dt=0.001, nbc=4, f=15.0, sz=10, gz=10, ng=8, ns=3)
    fwi = FWIForward(dict(ctx), "cpu", normalize=False)
    part = FWIForward(dict(ctx), "cpu", normalize=False, shots=(1, 3))
    v = torch.full((2, 1, 8, 8), 2000.0)
    for bad in (torch.zeros(199), torch.zeros(201), torch.zeros(2, 200), torch.zeros(4, 200), torch.zeros(3, 199),
                torch.zeros(1, 3, 200), torch.zeros(3, 3, 200), torch.zeros(2, 2, 200), torch.zeros(2, 3, 1, 200),
                torch.zeros(())):
        for op in (fwi, part):      # (with shots=, ns is still the survey's full shot count)
            with pytest.raises(ValueError, match="wavelet must have shape"):
                op(v, wavelet=bad)
    with pytest.raises(ValueError, match="float tensor"):
        fwi(v, wavelet=torch.zeros(200, dtype=torch.int32))
    with pytest.raises(ValueError, match="float tensor"):
        fwi(v, wavelet=np.zeros(200, np.float32))
    with pytest.raises(ValueError, match=r"\(B,1,H,W\)"):
        fwi(v[:, 0], wavelet=torch.zeros(200))
    with pytest.raises(ValueError, match="wavelet is on"):
        fwi(v, wavelet=torch.zeros(200, device="meta"))
    for good in (torch.zeros(200), torch.zeros(3, 200), torch.zeros(2, 3, 200), torch.zeros(200, dtype=torch.float64)):
        for op in (fwi, part):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                op(v, wavelet=good)
    # the view the kernels get: this operator's shots, shared axes as zero strides (no copy)
    w = torch.arange(3 * 200, dtype=torch.float32).view(3, 200)
    view = part._call_wavelet(v, w)
    assert view.shape == (2, 2, 200) and view.stride() == (0, 200, 1) and view.data_ptr() == w[1].data_ptr()
    assert fwi._call_wavelet(v, w[0]).stride() == (0, 0, 1)


@pytest.mark.parametrize("tag", CASES)
def test_oracle_with_the_fixture_wavelets_reproduces_the_reference_bitwise(tag):
    """The yardstick of the GPU tests: per (model, shot), the oracle with that pair's wavelet written into its
    wavelet array gives that pair's seis32, bit for bit."""
    c = Fixture(tag)
    for b in range(c.B):
        o = WaveletOracle(c, c.v[b:b + 1])
        for s in range(c.ns):
            o.set_wavelet(c.W[b, s])
            seis = o.forward()
            assert seis.shape[1:] == c.seis32.shape[1:]
            assert bits_equal(seis[0, s], c.seis32[b, s]), (tag, b, s)
            assert np.abs(c.seis32[b, s]).max() > 0


@pytest.mark.parametrize("tag", CASES)
def test_scaling_is_exact_only_outside_the_subnormal_range(tag):
    """The reference's fp32 arithmetic (the oracle, on IEEE hardware) under a wavelet scaled by 8: exact on wrap,
    geom and short.  On tiles it is not: the numerical precursor passes through fp32's subnormal range, the first
    cells to differ are subnormal, and the differences spread from there.  Pinned here because the GPU forward
    reproduces these bits, so its own linearity test asks exact homogeneity where the reference has it and the
    reference's scaled record where it has not."""
    c = Fixture(tag)
    o = WaveletOracle(c, c.v[:1])
    tiny = float(np.finfo(np.float32).tiny)
    exact = True
    for s in range(c.ns):
        o.set_wavelet(c.W[0, s])
        a = o.forward(keep_history=True)[0, s].copy()
        ha = o.c["hist"][:, 0, s].copy()
        o.set_wavelet(c.W[0, s] * np.float32(8))
        t = o.forward(keep_history=True)[0, s]
        ht = o.c["hist"][:, 0, s]
        differ = ht != np.float32(8) * ha                   # (times 8 is exact in fp32)
        if differ.any():
            first = int(np.argmax(differ.reshape(differ.shape[0], -1).any(1)))
            assert np.abs(ha[first][differ[first]]).max() < tiny, (tag, s, first)      # it starts with subnormals
        exact = exact and bits_equal(t, a * np.float32(8))
    assert exact == (tag != "tiles"), (tag, exact)
    # the fixture's flags, which the reference wrote, say the same, and where they say "not exact" the reference's
    # scaled record is stored and is what the oracle computes, bit for bit
    assert [j for j, _, _ in c.scales] == [3, -3]
    assert all(h == exact for _, h, _ in c.scales), (tag, c.scales)
    for j, h, ref_scaled in c.scales:
        if not h:
            for s in range(c.ns):
                o.set_wavelet(c.W[0, s] * np.float32(2.0 ** j))
                assert bits_equal(o.forward()[0, s], ref_scaled[0, s]), (tag, j, s)
