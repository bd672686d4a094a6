"""Host-side checks of encoded simultaneous-source supershots: the fixture's own consistency
(tests/golden/encoding.npz), the C ABI's new symbols and their argument checks (which need no device), the argument
checks of FWIForward.forward(v, encoding=), which run before any device work, and the two helpers of
red_diffeq.utils.encoding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from encoding_cases import CASES, Fixture

NEW = ("rdq_fwi_forward_enc", "rdq_fwi_adjoint_enc", "rdq_fwi_forward_ckpt_enc", "rdq_fwi_adjoint_ckpt_enc",
       "rdq_fwi_grad_finalize_enc", "rdq_fwi_sizes_enc", "rdq_fwi_ckpt_sizes_enc")
INVALID = -10001


@pytest.mark.parametrize("tag", CASES)
def test_fixture_is_consistent(tag):
    c = Fixture(tag)
    assert c.E.dtype == np.float32 and c.E.shape == (c.ns + 2, c.ns) and c.ne > c.ns
    assert set(np.unique(c.E[:2])) <= {-1.0, 1.0}                       # sign rows
    assert c.E[2, c.ns - 1] == 0.0 and np.count_nonzero(c.E[2:]) == c.ns * c.ns - 1     # Gaussian, one exact zero
    assert c.seis64.dtype == np.float64 and c.seis64.shape == c.r.shape and c.seis64.shape[:2] == (c.B, c.ne)
    assert c.eref.shape == (c.B, c.ne) and (c.eref > 0).all()
    assert c.gv64.shape == c.v.shape and c.gW64.shape == c.W.shape and c.gE64.shape == (c.B, c.ne, c.ns)
    for y in (c.eref_v, c.eref_w, c.eref_E):
        assert y.shape == (c.B,) and (y > 0).all()
    lhs, rhs = c.ip
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs))
    assert abs(float((c.dW.astype(np.float64) * c.gW64).sum()) - rhs) <= 1e-10 * abs(rhs)
    # linear in W and in E: <seis_enc, r> = <W, gW64> = <E, gE64>
    lin = float((c.seis64 * c.r.astype(np.float64)).sum())
    assert abs(lin - float((c.W.astype(np.float64) * c.gW64).sum())) <= 1e-10 * abs(lin)
    assert abs(lin - float((c.E.astype(np.float64)[None] * c.gE64).sum())) <= 1e-10 * abs(lin)


def test_shared_has_two_sources_on_one_cell():
    from red_diffeq.solvers.pde import adj_sr
    c = Fixture("shared")
    x = c.ctx
    isx = adj_sr(np.asarray(x["sx"]) * x["dx"], x["sz"], np.arange(x["ng"]) * x["dx"], x["gz"], x["dx"], x["nbc"])[0]
    assert c.ns == 3 and isx[1] == isx[2] != isx[0]


def test_header_declares_and_library_exports_the_encoding_symbols():
    from red_diffeq import _hip
    hdr = open(os.path.join(ROOT, "include", "red_diffeq_fwi.h")).read()
    declared = set(re.findall(r"^int\s+(rdq_\w+)\(", hdr, flags=re.M))
    lib = _hip.load_library()
    for n in NEW:
        assert n in declared and n in _hip.SIGNATURES, n
        assert isinstance(getattr(lib, n), ctypes._CFuncPtr)
    assert "typedef struct rdq_fwi_encoding" in hdr
    # argument checks need no GPU: a null struct, a null wav, ne < 1, a negative stride, each before anything else
    one = ctypes.c_void_p(8)

    def enc(**kw):
        return _hip.FwiEncoding(**dict(dict(ne=2, wav=8, model_stride=0, enc_stride=0, source_stride=0, gwav=None), **kw))
    for e in (None, enc(wav=None), enc(ne=0), enc(ne=-3), enc(model_stride=-1), enc(enc_stride=-4),
              enc(source_stride=-1)):
        ref = ctypes.byref(e) if e is not None else None
        assert lib.rdq_fwi_forward_enc(one, 1, one, ref, one, one, one, None) == INVALID
        assert lib.rdq_fwi_adjoint_enc(one, 1, one, ref, one, one, one, one, one, one, None) == INVALID
        assert lib.rdq_fwi_forward_ckpt_enc(one, 1, 4, one, ref, one, one, one, None) == INVALID
        assert lib.rdq_fwi_adjoint_ckpt_enc(one, 1, 4, one, ref, one, one, one, one, one, one, one, None) == INVALID
    ok = enc()
    assert lib.rdq_fwi_forward_enc(None, 1, one, ctypes.byref(ok), one, one, one, None) == INVALID     # no plan
    for B in (0, -2):                                                                                   # B < 1
        assert lib.rdq_fwi_forward_enc(one, B, one, ctypes.byref(ok), one, one, one, None) == INVALID
        assert lib.rdq_fwi_adjoint_enc(one, B, one, ctypes.byref(ok), one, one, one, one, one, one, None) == INVALID
        assert lib.rdq_fwi_forward_ckpt_enc(one, B, 4, one, ctypes.byref(ok), one, one, one, None) == INVALID
        assert lib.rdq_fwi_adjoint_ckpt_enc(one, B, 4, one, ctypes.byref(ok), one, one, one, one, one, one, one,
                                            None) == INVALID
    sz, cs = _hip.FwiSizes(), _hip.FwiCkptSizes()
    for B, ne in ((0, 1), (1, 0), (1, -1)):
        assert lib.rdq_fwi_sizes_enc(one, B, ne, ctypes.byref(sz)) == INVALID
        assert lib.rdq_fwi_ckpt_sizes_enc(one, B, ne, 4, ctypes.byref(cs)) == INVALID
        assert lib.rdq_fwi_grad_finalize_enc(one, B, ne, one, one, one, one, one, 0, one, one, None) == INVALID
    assert lib.rdq_fwi_sizes_enc(None, 1, 1, ctypes.byref(sz)) == INVALID
    assert lib.rdq_fwi_grad_finalize_enc(None, 1, 1, one, one, one, one, one, 0, one, one, None) == INVALID


def test_encoded_ops_are_registered():
    import red_diffeq.ops  # noqa: F401
    ns = torch.ops.red_diffeq
    want = {
        "enc_fwi": "red_diffeq::enc_fwi(Tensor v, Tensor weff, SymInt plan, SymInt vel_mode, bool keep_history) -> (Tensor, Tensor, Tensor, Tensor)",
        "enc_fwi_ckpt": "red_diffeq::enc_fwi_ckpt(Tensor v, Tensor weff, SymInt plan, SymInt vel_mode, SymInt K) -> (Tensor, Tensor, Tensor, Tensor)",
        "enc_fwi_forward": "red_diffeq::enc_fwi_forward(Tensor coeffs, Tensor weff, SymInt plan, SymInt B, bool keep_history) -> (Tensor, Tensor)",
        "enc_fwi_adjoint": "red_diffeq::enc_fwi_adjoint(Tensor coeffs, Tensor weff, Tensor history, Tensor dseis, SymInt plan, SymInt B, bool want_gw) -> (Tensor, Tensor, Tensor, Tensor)",
        "enc_fwi_forward_ckpt": "red_diffeq::enc_fwi_forward_ckpt(Tensor coeffs, Tensor weff, SymInt plan, SymInt B, SymInt K) -> (Tensor, Tensor)",
        "enc_fwi_adjoint_ckpt": "red_diffeq::enc_fwi_adjoint_ckpt(Tensor coeffs, Tensor weff, Tensor ckpt, Tensor(a7!) seg, Tensor dseis, SymInt plan, SymInt B, SymInt K, bool want_gw) -> (Tensor, Tensor, Tensor, Tensor)",
        "enc_fwi_grad_finalize": "red_diffeq::enc_fwi_grad_finalize(Tensor coeffs, Tensor vstat, Tensor gA, Tensor gk, Tensor gbeta, SymInt plan, SymInt B, SymInt ne, SymInt vel_mode) -> Tensor",
    }
    assert sorted(n for n in dir(ns) if n.startswith("enc_fwi")) == sorted(want)
    for name, schema in want.items():
        got = str(getattr(ns, name).default._schema)
        assert re.sub(r"\(a\d+!\)", "(a!)", got) == re.sub(r"\(a\d+!\)", "(a!)", schema), name


def test_encoding_checks_come_before_any_device_work():
    """CPU tensors: a bad encoding is a ValueError; only a well-formed call reaches the device check."""
    from red_diffeq.solvers.pde import FWIForward
    ctx = dict(n_grid=8, nt=200, dx=10.0, dt=0.001, nbc=4, f=15.0, sz=10, gz=10, ng=8, ns=3)
    fwi = FWIForward(dict(ctx), "cpu", normalize=False)
    v = torch.full((2, 1, 8, 8), 2000.0)
    for bad in (torch.zeros(3), torch.zeros(2, 4), torch.zeros(2, 2), torch.zeros(1, 2, 3), torch.zeros(3, 2, 3),
                torch.zeros(2, 2, 4), torch.zeros(2, 2, 3, 1), torch.zeros(())):
        with pytest.raises(ValueError, match="encoding must have shape"):
            fwi(v, encoding=bad)
    for empty in (torch.zeros(0, 3), torch.zeros(2, 0, 3)):                  # ne < 1
        with pytest.raises(ValueError, match="ne >= 1"):
            fwi(v, encoding=empty)
    with pytest.raises(ValueError, match="float tensor"):
        fwi(v, encoding=torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="float tensor"):
        fwi(v, encoding=np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match=r"\(B,1,H,W\)"):
        fwi(v[:, 0], encoding=torch.zeros(2, 3))
    with pytest.raises(ValueError, match="encoding is on"):
        fwi(v, encoding=torch.zeros(2, 3, device="meta"))
    with pytest.raises(ValueError, match="wavelet must have shape"):          # the wavelet's own checks still run
        fwi(v, wavelet=torch.zeros(199), encoding=torch.zeros(2, 3))
    part = FWIForward(dict(ctx), "cpu", normalize=False, shots=(1, 3))
    with pytest.raises(ValueError, match="shots="):
        part(v, encoding=torch.zeros(2, 3))
    dv = torch.zeros_like(v)
    with pytest.raises(ValueError, match="takes no encoding"):
        fwi.born(v, dv, encoding=torch.zeros(2, 3))
    with pytest.raises(ValueError, match="takes no encoding"):
        fwi.gauss_newton(v, dv, encoding=torch.zeros(2, 3))
    for good in (torch.zeros(2, 3), torch.zeros(1, 3), torch.zeros(5, 3), torch.zeros(2, 4, 3),
                 torch.zeros(2, 3, dtype=torch.float64)):
        for w in (None, torch.zeros(200), torch.zeros(3, 200), torch.zeros(2, 3, 200)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                fwi(v, wavelet=w, encoding=good)
    # the codes the kernels' effective wavelets are formed from: (B, ne, ns), a shared model axis as a zero stride
    E = torch.arange(6, dtype=torch.float32).view(2, 3)
    view = fwi._call_encoding(v, E)
    assert view.shape == (2, 2, 3) and view.stride() == (0, 3, 1) and view.data_ptr() == E.data_ptr()


# ---------------------------------------------------------------------------- red_diffeq.utils.encoding
@pytest.mark.parametrize("kind", ["sign", "gaussian", "partition"])
def test_random_encoding_shapes_and_determinism(kind):
    from red_diffeq.utils.encoding import random_encoding
    for ne, ns in ((1, 1), (1, 5), (3, 8), (8, 8), (11, 4)):
        g = torch.Generator().manual_seed(5)
        a = random_encoding(ne, ns, kind, generator=g)
        b = random_encoding(ne, ns, kind, generator=g)                      # the generator moved on
        again = random_encoding(ne, ns, kind, generator=torch.Generator().manual_seed(5))
        assert a.shape == (ne, ns) and a.dtype == torch.float32 and a.device.type == "cpu"
        assert torch.equal(a, again)
        if ne * ns >= 8:
            assert not torch.equal(a, b)
        if kind == "sign":
            assert set(a.unique().tolist()) <= {-1.0, 1.0}
        if kind == "gaussian":
            assert torch.count_nonzero(a) == ne * ns
    big = random_encoding(64, 64, kind, generator=torch.Generator().manual_seed(1))
    if kind == "sign":
        assert 0.4 < float((big > 0).float().mean()) < 0.6
    if kind == "gaussian":
        assert abs(float(big.mean())) < 0.1 and 0.9 < float(big.std()) < 1.1


def test_random_encoding_partition_properties():
    from red_diffeq.utils.encoding import random_encoding
    seen = set()
    for seed in range(20):
        for ne, ns in ((1, 6), (2, 7), (4, 16), (5, 5), (7, 3)):
            E = random_encoding(ne, ns, "partition", generator=torch.Generator().manual_seed(seed))
            assert set(E.unique().tolist()) <= {-1.0, 0.0, 1.0}
            assert (E != 0).sum(0).tolist() == [1] * ns                     # every source in exactly one supershot
            sizes = (E != 0).sum(1)
            if ne <= ns:
                assert int(sizes.min()) >= 1 and int(sizes.max() - sizes.min()) <= 1      # none empty, balanced
            else:
                assert int(sizes.max()) == 1 and int(sizes.sum()) == ns
            if (ne, ns) == (4, 16):
                seen.add(tuple(E.flatten().tolist()))
    assert len(seen) > 15                                                   # the draws differ with the seed
    both = torch.stack([random_encoding(4, 16, "partition", generator=torch.Generator().manual_seed(s)).sum(0)
                        for s in range(20)])
    assert (both > 0).any() and (both < 0).any()                            # random signs
    for bad in ((0, 3, "sign"), (2, 0, "sign"), (2, 3, "signs")):
        with pytest.raises(ValueError):
            random_encoding(*bad)


def test_encode_agrees_with_an_fp64_einsum():
    from red_diffeq.utils.encoding import encode, random_encoding
    g = torch.Generator().manual_seed(3)
    data = torch.randn(2, 5, 7, 4, generator=g)
    for E in (random_encoding(3, 5, "gaussian", generator=g), random_encoding(2, 5, "sign", generator=g),
              random_encoding(2, 5, "partition", generator=g), torch.randn(2, 6, 5, generator=g)):
        out = encode(data, E)
        Eb = E.expand(2, E.shape[-2], 5)
        want = torch.einsum("bes,bsrg->berg", Eb.double(), data.double())
        assert out.shape == (2, E.shape[-2], 7, 4) and out.dtype == torch.float32
        # five fp32 products and adds per element: a few ulp of the largest partial sum
        scale = torch.einsum("bes,bsrg->berg", Eb.double().abs(), data.double().abs())
        assert float(((out.double() - want).abs() / scale).max()) <= 5 * 2.0 ** -24
        # the documented order, bit for bit: ascending s, one product and one add each
        ref = torch.zeros_like(out)
        for s in range(5):
            ref = ref + Eb[:, :, s, None, None] * data[:, s, None]
        assert torch.equal(out, ref)
    onehot = torch.eye(5)[[3, 0]]
    assert torch.equal(encode(data, onehot), data[:, [3, 0]])               # zero codes contribute exact zeros
    for bad_data, bad_E in ((data[0], torch.zeros(2, 5)), (data, torch.zeros(2, 4)), (data, torch.zeros(3, 2, 5)),
                            (data, torch.zeros(5))):
        with pytest.raises(ValueError):
            encode(bad_data, bad_E)
