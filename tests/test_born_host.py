"""Host-side checks of the linearised (Born) forward: the C ABI's new symbols, the argument checks of
FWIForward.born / gauss_newton (which run before any device work) and the fixture's own consistency."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

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
