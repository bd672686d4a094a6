"""Host-side checks of the illumination pass (rdq_fwi_illum / _illum_ckpt / _illum_finalize, FWIForward.illumination,
red_diffeq.utils.precondition, InversionEngine's precondition arguments): the C ABI's symbols and the argument checks
that need no device, the Python argument checks that run before any device work, the two preconditioning helpers
against numpy and CPU autograd, and the references of tests/illum_refs.py against the oracle."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import illum_refs as R
from conftest import ROOT, vnorm

NEW = ("rdq_fwi_illum", "rdq_fwi_illum_ckpt", "rdq_fwi_illum_finalize")
INVALID = -10001
SMOKE = dict(n_grid=24, nt=200, dx=10.0, dt=0.001, nbc=10, f=15.0, sz=10, gz=10, ng=24, ns=3)


def test_header_declares_and_library_exports_the_illumination_symbols():
    from red_diffeq import _hip
    hdr = open(os.path.join(ROOT, "include", "red_diffeq_fwi.h")).read()
    declared = set(re.findall(r"^int\s+(rdq_\w+)\(", hdr, flags=re.M))
    lib = _hip.load_library()
    for n in NEW:
        assert n in declared and n in _hip.SIGNATURES, n
        assert isinstance(getattr(lib, n), ctypes._CFuncPtr)


def test_invalid_arguments_return_without_a_device():
    """Every call has exactly one thing wrong and returns RDQ_E_INVALID before the plan is read or anything is
    launched (the pointers are fakes).  (A missing ckpt with more than one segment needs a real plan's nt: it is
    checked in tests/test_gpu_illumination.py.)"""
    from red_diffeq import _hip
    lib = _hip.load_library()
    one = ctypes.c_void_p(8)
    assert lib.rdq_fwi_illum(None, 1, 0, one, one, None) == INVALID
    assert lib.rdq_fwi_illum(one, 1, 0, None, one, None) == INVALID
    assert lib.rdq_fwi_illum(one, 1, 0, one, None, None) == INVALID
    for B in (0, -2):
        assert lib.rdq_fwi_illum(one, B, 0, one, one, None) == INVALID
    assert lib.rdq_fwi_illum(one, 1, -1, one, one, None) == INVALID

    def ckpt(plan=one, B=1, K=4, coeffs=one, src=None, enc=None, ck=one, seg=one, ring=one, hA=one):
        return lib.rdq_fwi_illum_ckpt(plan, B, K, coeffs, src, enc, ck, seg, ring, hA, None)
    src = _hip.FwiSource(wav=8, model_stride=0, shot_stride=0, gwav=None)
    enc = _hip.FwiEncoding(ne=2, wav=8, model_stride=0, enc_stride=0, source_stride=0, gwav=None)
    for kw in (dict(plan=None), dict(coeffs=None), dict(seg=None), dict(ring=None), dict(hA=None), dict(B=0), dict(B=-1),
               dict(K=0), dict(K=-5), dict(src=ctypes.byref(src), enc=ctypes.byref(enc)),
               dict(src=ctypes.byref(_hip.FwiSource(wav=None, model_stride=0, shot_stride=0, gwav=None))),
               dict(src=ctypes.byref(_hip.FwiSource(wav=8, model_stride=-1, shot_stride=0, gwav=None))),
               dict(enc=ctypes.byref(_hip.FwiEncoding(ne=0, wav=8, model_stride=0, enc_stride=0, source_stride=0,
                                                      gwav=None)))):
        assert ckpt(**kw) == INVALID, kw

    def fin(plan=one, B=1, nwf=0, coeffs=one, hA=one, vel_mode=0, colsum=one, H=one):
        return lib.rdq_fwi_illum_finalize(plan, B, nwf, coeffs, hA, vel_mode, colsum, H, None)
    for kw in (dict(plan=None), dict(coeffs=None), dict(hA=None), dict(colsum=None), dict(H=None), dict(B=0), dict(nwf=-1),
               dict(vel_mode=2), dict(vel_mode=-1)):
        assert fin(**kw) == INVALID, kw


def test_illumination_ops_are_registered():
    """(Named illum_fwi*: the set of fwi* operators is pinned by tests/test_host.py.)"""
    import red_diffeq.ops  # noqa: F401
    ns = torch.ops.red_diffeq
    want = {
        "illum_fwi": "red_diffeq::illum_fwi(Tensor history, SymInt plan, SymInt B, SymInt nwf) -> Tensor",
        "illum_fwi_ckpt": "red_diffeq::illum_fwi_ckpt(Tensor coeffs, Tensor ckpt, Tensor(a2!) seg, SymInt plan, SymInt B, "
                          "SymInt K) -> Tensor",
        "illum_fwi_ckpt_src": "red_diffeq::illum_fwi_ckpt_src(Tensor coeffs, Tensor w, Tensor ckpt, Tensor(a3!) seg, "
                              "SymInt plan, SymInt B, SymInt K) -> Tensor",
        "illum_fwi_ckpt_enc": "red_diffeq::illum_fwi_ckpt_enc(Tensor coeffs, Tensor weff, Tensor ckpt, Tensor(a3!) seg, "
                              "SymInt plan, SymInt B, SymInt K) -> Tensor",
        "illum_fwi_finalize": "red_diffeq::illum_fwi_finalize(Tensor coeffs, Tensor hA, SymInt plan, SymInt B, SymInt nwf, "
                              "SymInt vel_mode) -> Tensor",
    }
    for name, schema in want.items():
        assert str(getattr(ns, name).default._schema) == schema, name


def _fwi(**kw):
    from red_diffeq.solvers.pde import FWIForward
    from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize
    kw.setdefault("v_denorm_func", v_denormalize)
    return FWIForward(dict(SMOKE), "cuda", normalize=True, s_norm_func=s_normalize_none, **kw)


def test_illumination_argument_checks_run_before_device_work():
    """CPU tensors: the ValueErrors come before the operator would refuse the device."""
    v = torch.zeros(2, 1, 24, 24)
    with pytest.raises(ValueError, match="custom v_denorm_func"):
        _fwi(v_denorm_func=lambda x: x * 3000.0).illumination(v)
    f = _fwi()
    for bad in (torch.zeros(2, 24, 24), torch.zeros(2, 2, 24, 24)):
        with pytest.raises(ValueError, match="expected v of shape"):
            f.illumination(bad)
    with pytest.raises(ValueError, match="wavelet must have shape"):
        f.illumination(v, wavelet=torch.zeros(199))
    with pytest.raises(ValueError, match="encoding must have shape"):
        f.illumination(v, encoding=torch.zeros(2, 4))
    with pytest.raises(ValueError, match="shots="):
        _fwi(shots=(0, 2)).illumination(v, encoding=torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # every check passed: only now the device
        f.illumination(v)


def test_engine_argument_checks():
    """The settings are the engine's (constructor keywords / attributes: optimize()'s signature is pinned); a bad one
    raises at construction and, set afterwards, at the next optimize(), before the operator runs."""
    from red_diffeq.core.inversion import InversionEngine
    dm = types.SimpleNamespace(device=torch.device("cpu"))
    mu, y = torch.zeros(1, 1, 26, 26), torch.zeros(1, 3, 200, 24)

    class NoIllum:
        def __call__(self, v):
            raise AssertionError("the operator must not run")
    with pytest.raises(ValueError, match="Unknown precondition"):
        InversionEngine(dm, None, None, show_progress=False, precondition="hessian")
    with pytest.raises(ValueError, match="precondition_every"):
        InversionEngine(dm, None, None, show_progress=False, precondition="illumination", precondition_every=-1)
    with pytest.raises(ValueError, match="precondition_eps"):
        InversionEngine(dm, None, None, show_progress=False, precondition="illumination", precondition_eps=0.0)
    eng = InversionEngine(dm, None, None, show_progress=False)
    assert eng.precondition is None and (eng.precondition_eps, eng.precondition_power, eng.precondition_every) == (1e-2, 1.0, 0)
    eng.precondition = "hessian"
    with pytest.raises(ValueError, match="Unknown precondition"):
        eng.optimize(mu, mu[:, :, 1:-1, 1:-1], y, NoIllum(), ts=1)
    eng.precondition = "illumination"
    with pytest.raises(ValueError, match="illumination"):          # an operator without the method
        eng.optimize(mu, mu[:, :, 1:-1, 1:-1], y, NoIllum(), ts=1)


def _weights_np(H, eps, power):
    H = H.astype(np.float32)
    m = np.maximum(H.mean(axis=(1, 2, 3), keepdims=True, dtype=np.float64).astype(np.float32), np.finfo(np.float32).tiny)
    W = ((H / m + np.float32(eps)) ** np.float32(-power)).astype(np.float32)
    return W / W.mean(axis=(1, 2, 3), keepdims=True, dtype=np.float64).astype(np.float32)


@pytest.mark.parametrize("eps,power", [(1e-2, 1.0), (1e-3, 0.5), (0.3, 2.0)])
def test_illumination_weights_match_numpy(eps, power):
    from red_diffeq.utils.precondition import illumination_weights
    rng = np.random.default_rng(5)
    H = np.abs(rng.standard_normal((3, 1, 9, 11))).astype(np.float32) ** 4      # a wide dynamic range
    H[1] = 0.0                                                                   # an all-zero model
    H[2] = 0.0
    H[2, 0, 4, 5] = 7.0                                                          # one bright cell
    W = illumination_weights(torch.from_numpy(H), eps, power).numpy()
    assert W.shape == H.shape and W.dtype == np.float32
    np.testing.assert_allclose(W, _weights_np(H, eps, power), rtol=2e-5)       # (pow and the mean's order: a few ulp)
    np.testing.assert_allclose(W.reshape(3, -1).mean(1, dtype=np.float64), 1.0, rtol=1e-5)
    assert np.array_equal(W[1], np.ones_like(W[1]))                              # all-zero H: W = 1 exactly
    dark = W[2, 0, 0, 0]
    assert W[2, 0, 4, 5] < dark and np.all(W[2][H[2] == 0] == dark)              # the bright cell is damped, the rest equal
    np.testing.assert_allclose(W[2, 0, 4, 5] / dark, (eps / (99.0 + eps)) ** power, rtol=1e-4)   # Hn = 99 there
    assert (W > 0).all() and np.isfinite(W).all()
    with pytest.raises(ValueError):
        illumination_weights(torch.zeros(3, 9, 11))
    with pytest.raises(ValueError):
        illumination_weights(torch.zeros(1, 1, 3, 3), eps=0.0)


def test_precondition_grad_under_cpu_autograd():
    from red_diffeq.utils.precondition import precondition_grad
    g = torch.Generator().manual_seed(3)
    mu = torch.randn(2, 1, 6, 6, generator=g, requires_grad=True)
    W = torch.rand(2, 1, 4, 4, generator=g) + 0.5
    c = torch.randn(2, 1, 4, 4, generator=g)
    v = mu[:, :, 1:-1, 1:-1]
    out = precondition_grad(v, W)
    assert torch.equal(out, v)                                                   # identity forward
    ((out * c).sum() + 3.0 * (mu ** 2).sum()).backward()                         # "data" term + an unscaled "prior"
    want = 6.0 * mu.detach()
    want[:, :, 1:-1, 1:-1] += c * W
    assert torch.equal(mu.grad, want)                                            # the data term scaled, the prior not
    assert W.grad is None and not W.requires_grad


@pytest.fixture(scope="module")
def smoke_refs():
    from oracle import oracle as O
    from red_diffeq.utils.synthetic import make_model
    vn = vnorm(make_model("curvefault", 24, 24, seed=1, batch=2))
    seis32, c = O.OracleFWI(dict(SMOKE), 2).forward(vn, keep_history=True)
    v32 = R.denorm32(vn)[:, 0]
    seis64, hist64 = R.forward64(v32.astype(np.float64), SMOKE)
    return dict(vn=vn, v32=v32, seis32=seis32, hist32=c["hist"], seis64=seis64, hist64=hist64)


def test_restatement_agrees_with_the_oracle(smoke_refs):
    """The fp64 restatement and the oracle model the same physics: seismograms to fp32 level (fp32 rounding grows
    about linearly over the 200 steps, 200 u = 1.2e-5; measured 3.6e-6), and the fp64 illumination formula on the
    oracle's fp32 history against the same formula on the restatement's fp64 history, rel-L2 per model below 1e-3 (a
    condition that both are the same model, not a tolerance; measured 6.3e-7 and 7.8e-7)."""
    s = smoke_refs
    e_seis = R.rel_l2(s["seis32"], s["seis64"])
    assert (e_seis < 1e-4).all(), e_seis
    nt, nbc = SMOKE["nt"], SMOKE["nbc"]
    h32 = R.hA_and_bar(s["hist32"].astype(np.float64), nt)[0]
    h64 = R.hA_and_bar(s["hist64"], nt)[0]
    e_ref = R.rel_l2(h32.sum(1), h64.sum(1))
    print("e_seis", e_seis, "e_ref(hA)", e_ref)
    assert (e_ref < 1e-3).all(), e_ref
    H32 = R.H_of(h32, s["v32"], SMOKE["dt"], SMOKE["dx"], nbc, 1500.0)
    H64 = R.H_of(h64, s["v32"], SMOKE["dt"], SMOKE["dx"], nbc, 1500.0)
    assert (R.rel_l2(H32, H64) < 1e-3).all()
    # the spread the preconditioner is for comes from the physics: max / mean and min / mean of the model cells
    r = H64 / H64.mean(axis=(1, 2), keepdims=True)
    assert r.max() > 20 and r.min() < 0.05, (r.max(), r.min())


def test_fold_and_bar_helpers():
    rng = np.random.default_rng(0)
    hA = rng.random((2, 3, 9, 8))
    out = R.fold(hA, 2, 5, 4)
    s = hA.sum(1)
    assert out.shape == (2, 5, 4)
    np.testing.assert_allclose(out.sum((1, 2)), s.sum((1, 2)), rtol=1e-13)        # every padded cell lands once
    np.testing.assert_allclose(out[:, 0, 0], s[:, :3, :3].sum((1, 2)), rtol=1e-13)  # corner: (nbc + 1)^2 cells
    np.testing.assert_allclose(out[:, 2, 1], s[:, 4, 3], rtol=1e-13)              # interior: its own cell
    np.testing.assert_allclose(out[:, 4, 2], s[:, 6:, 4].sum(1), rtol=1e-13)      # bottom edge: nbc + 1 rows
    hist = rng.standard_normal((6, 1, 1, 7, 7))
    h, bar = R.hA_and_bar(hist, 4)
    q1 = R.q_of(hist[1])[0]
    P = hist[1][0, 0]
    want = -5.0 * P[3, 3] + R.C2 * (P[2, 3] + P[4, 3] + P[3, 2] + P[3, 4]) + R.C3 * (P[1, 3] + P[5, 3] + P[3, 1] + P[3, 5])
    assert abs(q1[0, 0, 3, 3] - want) < 1e-13
    want0 = -5.0 * P[0, 0] + R.C2 * (P[6, 0] + P[1, 0] + P[0, 6] + P[0, 1]) + R.C3 * (P[5, 0] + P[2, 0] + P[0, 5] + P[0, 2])
    assert abs(q1[0, 0, 0, 0] - want0) < 1e-13                                    # periodic wrap
    assert (bar > 0).all() and (bar < 1e-4 * h).all()
