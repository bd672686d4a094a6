"""Host-side checks of the fused forward + Born pass (rdq_fwi_born_fused; born / gauss_newton with
history=False): the C ABI's new symbol and its argument checks, and the Python argument checks, which run before
any device work."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

CTX = dict(n_grid=8, nt=200, dx=10.0, dt=0.001, nbc=4, f=15.0, sz=10, gz=10, ng=8, ns=1)


def test_header_declares_and_library_exports_the_fused_symbol():
    from red_diffeq import _hip
    hdr = open(os.path.join(ROOT, "include", "red_diffeq_fwi.h")).read()
    declared = set(re.findall(r"^int\s+(rdq_\w+)\(", hdr, flags=re.M))
    lib = _hip.load_library()
    assert "rdq_fwi_born_fused" in declared and "rdq_fwi_born_fused" in _hip.SIGNATURES
    assert isinstance(lib.rdq_fwi_born_fused, ctypes._CFuncPtr)
    assert len(_hip.SIGNATURES["rdq_fwi_born_fused"][1]) == 10


def test_null_arguments_are_invalid():
    """The argument checks need no GPU: a null plan or buffer, with and without a checkpoint interval."""
    from red_diffeq import _hip
    lib = _hip.load_library()
    for K in (0, 7):
        assert lib.rdq_fwi_born_fused(None, 1, K, None, None, None, None, None, None, None) == -10001
    assert lib.rdq_fwi_born_fused(None, 0, 7, None, None, None, None, None, None, None) == -10001


@pytest.mark.parametrize("method", ["born", "gauss_newton"])
def test_shape_checks_come_before_any_device_work(method):
    """CPU tensors and history=False: a shape error is the ValueError history=True raises; only well-formed
    arguments reach the device check."""
    from red_diffeq.solvers.pde import FWIForward
    call = getattr(FWIForward(dict(CTX), "cpu", normalize=False, checkpoint=40), method)
    v = torch.full((2, 1, 8, 8), 2000.0)
    with pytest.raises(ValueError, match="dv has shape"):
        call(v, torch.zeros(2, 1, 8, 7), history=False)
    with pytest.raises(ValueError, match="dv has shape"):
        call(v, torch.zeros(1, 1, 8, 8), history=False)
    with pytest.raises(ValueError, match=r"\(B,1,H,W\)"):
        call(v[:, 0], torch.zeros(2, 8, 8), history=False)
    with pytest.raises(ValueError, match=r"\(B,1,H,W\)"):
        call(v.expand(2, 3, 8, 8), torch.zeros(2, 3, 8, 8), history=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(v, torch.zeros_like(v), history=False)


def test_gauss_newton_without_history_needs_a_checkpoint_setting():
    """Neither checkpoint nor history_budget_gb: a ValueError that says so, on CPU tensors (before the device
    check); born(history=False) needs neither and goes on to the device check; either setting is enough."""
    from red_diffeq.solvers.pde import FWIForward
    v = torch.full((2, 1, 8, 8), 2000.0)
    fwi = FWIForward(dict(CTX), "cpu", normalize=False)
    with pytest.raises(ValueError, match=r"checkpoint.*history_budget_gb"):
        fwi.gauss_newton(v, torch.zeros_like(v), history=False)
    with pytest.raises(ValueError, match="dv has shape"):          # the shape checks still come first
        fwi.gauss_newton(v, torch.zeros(2, 1, 8, 7), history=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fwi.born(v, torch.zeros_like(v), history=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # the default path asks for no setting
        fwi.gauss_newton(v, torch.zeros_like(v))
    for kw in (dict(checkpoint=40), dict(history_budget_gb=1.0), dict(checkpoint="auto", history_budget_gb=1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FWIForward(dict(CTX), "cpu", normalize=False, **kw).gauss_newton(v, torch.zeros_like(v), history=False)
