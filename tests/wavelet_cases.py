"""Shared by tests/test_wavelet_host.py and tests/test_gpu_wavelet.py: the cases of tests/golden/wavelet.npz
(tests/golden/make_wavelet.py) and the CPU oracle driven with a wavelet of the test's choosing.

The oracle (oracle/oracle.py, left as it is) has one fp64 wavelet array for every shot and model, built as the Ricker
wavelet of ctx, and takes normalised velocities only.  Here its array is overwritten in place (the C side reads it
through a pointer at every call), a record shorter than the Ricker is had by building the oracle for a long record
and shortening nt afterwards, and a physical model goes through the same coefficient routine from a replicate pad
made here."""
import ctypes

import numpy as np

from conftest import load_golden

CASES = ("wrap", "tiles", "geom", "short")
SCALES = (3, -3)         # tests/golden/make_wavelet.py
RICKER_NT = 160          # long enough for the f = 15, dt = 1e-3 Ricker (147 samples)


class Fixture:
    def __init__(self, tag):
        z = load_golden("wavelet")
        pre = f"{tag}_ctx_"
        self.ctx = {k[len(pre):]: (z[k].item() if z[k].ndim == 0 else z[k].tolist()) for k in z.files
                    if k.startswith(pre)}
        self.tag, self.normalize, self.st = tag, bool(z[f"{tag}_normalize"]), int(z[f"{tag}_st"])
        for name in ("v", "W", "r", "seis32", "seis64", "gw64", "gw32", "gv64", "eref_w", "dW", "ip"):
            setattr(self, name, z[f"{tag}_{name}"])
        self.B, self.ns, self.nt = self.W.shape
        # per power-of-two scale 2^j of the wavelets: (j, is the reference's own fp32 record exactly 2^j seis32?,
        # the reference's fp32 record for 2^j W where it is not)
        self.scales = [(j, bool(h), None if h else z[f"{tag}_seis32_scaled_{i}"])
                       for i, (j, h) in enumerate(zip(SCALES, z[f"{tag}_homogeneous"]))]

    def fwi(self, device="cuda", **kw):
        from red_diffeq.solvers.pde import FWIForward
        from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize
        if self.normalize:
            kw = dict(dict(v_denorm_func=v_denormalize, s_norm_func=s_normalize_none), **kw)
        return FWIForward(dict(self.ctx), device, sample_temporal=self.st, normalize=self.normalize, **kw)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


class WaveletOracle:
    """The CPU oracle for models v (B, 1, nz, nx) of a fixture case, with a settable wavelet."""

    def __init__(self, case, v):
        from oracle import oracle as O
        self.O, self.case = O, case
        nt = int(case.ctx["nt"])
        self.f = O.OracleFWI(dict(case.ctx, nt=max(nt, RICKER_NT)), v.shape[0], sample_temporal=case.st)
        self.f.g.nt = nt                       # (the wavelet array stays RICKER_NT long: the first nt are read)
        self.nt = nt
        self.c = self._coeffs(np.ascontiguousarray(v, np.float32))

    def _coeffs(self, v):
        f, O = self.f, self.O
        if self.case.normalize:
            return f.coeffs(v)
        B, Hp, Wp = f._shape(v)
        nbc = f.g.nbc
        vpad = np.ascontiguousarray(np.pad(v[:, 0], ((0, 0), (nbc, nbc), (nbc, nbc)), mode="edge"))
        c = {k: np.empty((B, Hp, Wp), np.float32) for k in ("alpha", "temp1", "temp2", "kappa", "beta")}
        vmin, amin = np.empty(B, np.float32), np.empty(B, np.int64)
        O.lib().oracle_coeffs(ctypes.byref(f.g), O._p(vpad), O._p(c["alpha"]), O._p(c["temp1"]), O._p(c["temp2"]),
                              O._p(c["kappa"]), O._p(c["beta"]), O._p(vmin), O._p(amin, ctypes.c_int64))
        c.update(vpad=vpad, vmin=vmin, argmin=amin)
        return c

    def set_wavelet(self, w):
        self.f.wav[:self.nt] = np.asarray(w, np.float64)      # in place: the C struct points at this array

    def forward(self, keep_history=False):
        f, O, c = self.f, self.O, self.c
        B, Hp, Wp = c["vpad"].shape
        seis = np.zeros((B, f.g.ns, f.nrec, f.g.ng), np.float32)
        hist = np.empty((f.g.nt + 2, B, f.g.ns, Hp, Wp), np.float32) if keep_history else None
        O.lib().oracle_forward(ctypes.byref(f.g), O._p(c["alpha"]), O._p(c["temp1"]), O._p(c["temp2"]),
                               O._p(c["beta"]), O._p(seis), O._p(hist) if keep_history else None)
        if keep_history:
            c["hist"] = hist
        return seis

    def source_adjoint_field(self, dseis, j):
        """L_{j+1} at every (model, shot)'s source cell, (B, ns) fp32: the oracle's gbeta = sum_k L_k(src) w[k-1]
        with w a unit impulse at j (every other term is L * 0 = a signed zero, added exactly).  L does not depend on
        the forward field, so any stored history serves."""
        if "hist" not in self.c:
            self.forward(keep_history=True)
        w = np.zeros(self.nt)
        w[j] = 1.0
        self.set_wavelet(w)
        return self.f.adjoint(self.c, dseis)[2]

    def source_beta(self):
        """beta[b, isz, isx[s]], (B, ns) fp32."""
        return self.c["beta"][:, self.f.g.isz, :][:, self.f.isx]
