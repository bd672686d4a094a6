"""Host-side checks of the linearised (Born) forward: the C ABI's new symbols, the argument checks of
FWIForward.born / gauss_newton (which run before any device work) and the fixtures' own consistency, the
per-trace yardstick of tests/born_traces.py included."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import born_traces as T
from conftest import ROOT, load_golden

NEW = ("rdq_fwi_born_sizes", "rdq_fwi_dcoeffs", "rdq_fwi_born")
CASES = ("wrap", "tiles", "geom")


def test_header_declares_and_library_exports_the_born_symbols():
    from red_diffeq import _hip
    hdr = open(os.path.join(ROOT, "include", "red_diffeq_fwi.h")).read()
    declared = set(re.findall(r"^int\s+(rdq_\w+)\(", hdr, flags=re.M))
    lib = _hip.load_library()
    for n in NEW:
        assert n in declared and n in _hip.SIGNATURES, n
        assert isinstance(getattr(lib, n), ctypes._CFuncPtr)
    # argument checks need no GPU
    nbytes = ctypes.c_size_t()
    assert lib.rdq_fwi_born_sizes(None, 1, ctypes.byref(nbytes)) == -10001
    assert lib.rdq_fwi_born(None, 1, None, None, None, None, None, None) == -10001
    assert lib.rdq_fwi_dcoeffs(None, 1, None, None, 0, None, None, None, None) == -10001


@pytest.mark.parametrize("method", ["born", "gauss_newton"])
def test_shape_checks_come_before_any_device_work(method):
    """CPU tensors: a shape error is a ValueError; only well-formed arguments reach the device check."""
    from red_diffeq.solvers.pde import FWIForward
    ctx = dict(n_grid=8, nt=200, dx=10.0, dt=0.001, nbc=4, f=15.0, sz=10, gz=10, ng=8, ns=1)
    call = getattr(FWIForward(ctx, "cpu", normalize=False), method)
    v = torch.full((2, 1, 8, 8), 2000.0)
    with pytest.raises(ValueError, match="dv has shape"):
        call(v, torch.zeros(2, 1, 8, 7))
    with pytest.raises(ValueError, match="dv has shape"):
        call(v, torch.zeros(1, 1, 8, 8))
    with pytest.raises(ValueError, match=r"\(B,1,H,W\)"):
        call(v[:, 0], torch.zeros(2, 8, 8))
    with pytest.raises(ValueError, match=r"\(B,1,H,W\)"):
        call(v.expand(2, 3, 8, 8), torch.zeros(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(v, torch.zeros_like(v))


@pytest.mark.parametrize("tag", CASES)
def test_fixture_inner_products_agree(tag):
    """<J dv, w> = <dv, J^T w> in the reference's fp64, from the stored arrays and as stored."""
    z = load_golden("born")
    lhs = float((z[f"{tag}_jdv64"] * z[f"{tag}_w"].astype(np.float64)).sum())
    rhs = float((z[f"{tag}_dv"].astype(np.float64) * z[f"{tag}_jtw64"]).sum())
    scale = max(abs(lhs), abs(rhs))
    assert abs(lhs - rhs) <= 1e-10 * scale, (lhs, rhs)
    ip = z[f"{tag}_ip"]
    assert abs(ip[0] - ip[1]) <= 1e-10 * scale and abs(ip[0] - lhs) <= 1e-10 * scale
    assert (z[f"{tag}_eref"] > 0).all() and z[f"{tag}_eref"].shape == (z[f"{tag}_v"].shape[0],)
    assert z[f"{tag}_jdv64"].dtype == np.float64 and z[f"{tag}_jdv32"].dtype == np.float32


@pytest.mark.parametrize("case", T.ALL)
def test_per_trace_yardstick_is_usable_on_every_trace(case):
    """No trace of a fixture's J dv is empty, every per-trace bar is finite and positive, and the reference's own
    fp32 record meets the per-trace criterion with factor 1 (by construction: pinned here, so that a change of
    the yardstick that loses it is seen without a GPU)."""
    jdv64, jdv32, eref = T.records(case)
    n64, e_ref, bar = T.trace_yardstick(jdv64, jdv32, eref)
    assert n64.shape == jdv64.shape[:2] + jdv64.shape[3:] and (n64 > 0).all()
    assert np.isfinite(e_ref).all() and np.isfinite(bar).all() and (bar > 0).all()
    assert (T.trace_ratio(jdv32, jdv64, jdv32, eref) <= 1).all()
    # and the criterion can fail: a record that is off by 10 E_ref on one weak trace alone
    b, s, g = np.unravel_index(np.argmin(n64), n64.shape)
    off = jdv32.astype(np.float64)
    off[b, s, :, g] += 10 * max(e_ref[b, s, g], eref[b]) * max(n64[b, s, g], T.FLOOR * n64[b].max()) \
        * jdv64[b, s, :, g] / n64[b, s, g]
    assert T.trace_ratio(off, jdv64, jdv32, eref)[b, s, g] > 4


def test_terms_fixture_directions_are_single_cells():
    """Each direction of born_terms.npz is 0.04 at one cell per model, at the cell its name says: the argmins of
    the stored model, a source cell, the far corner, the top / left edge, an interior cell."""
    z = load_golden("born_terms")
    v = z["terms_v"]
    nz, nx = v.shape[2:]
    argmins = [divmod(int(v[b].argmin()), nx) for b in range(v.shape[0])]
    assert argmins == [(11, 6), (0, 0)]
    want = {"argmin": argmins, "source": [(1, 14)] * 2, "corner": [(nz - 1, nx - 1)] * 2,
            "edge": [(0, 17), (12, 0)], "interior": [(10, 20)] * 2}
    assert set(want) == set(T.DIRECTIONS)
    for name, cells in want.items():
        dv = z[f"terms_{name}_dv"]
        assert dv.dtype == np.float32 and dv.shape == v.shape
        for b, (iz, ix) in enumerate(cells):
            assert np.count_nonzero(dv[b]) == 1 and dv[b, 0, iz, ix] == np.float32(0.04), (name, b)
        ip = z[f"terms_{name}_ip"]
        lhs = float((z[f"terms_{name}_jdv64"] * z["terms_w"].astype(np.float64)).sum())
        rhs = float((dv.astype(np.float64) * z["terms_jtw64"]).sum())
        assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)) and abs(ip[0] - lhs) <= 1e-10 * abs(lhs)
        assert (z[f"terms_{name}_eref"] > 0).all()


def test_wavelet_prefix_does_not_depend_on_the_record_length():
    """ricker(15, 1e-3, nt)[:157] is the same bits for nt = 157 .. 161 (a 147-sample wavelet, zero-padded): what
    lets tests/test_gpu_born_terms.py compare records of different lengths sample by sample."""
    from red_diffeq.solvers.pde import ricker
    ref = ricker(15.0, 1e-3, 160)
    assert np.count_nonzero(ref) <= 147 and not ref[147:].any()
    for nt in range(157, 162):
        w = ricker(15.0, 1e-3, nt)
        assert w.shape == (nt,) and w[:157].tobytes() == ref[:157].tobytes(), nt
