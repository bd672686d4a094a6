"""PyTorch custom operators over the C ABI (torch.ops.red_diffeq.*).

Every HIP entry point the product path uses is registered with torch.library: a schema, the
ROCm implementation (the ctypes call into libred_diffeq_hip.so on the tensor's current stream), a
fake (meta) implementation giving output shapes without running anything, and for the FWI
operator an autograd formula whose backward is the hand-written adjoint.  The ops are
functional (fresh outputs, no input mutation), so torch.library.opcheck, FakeTensor tracing and
torch.compile see them as ordinary operators instead of opaque ctypes calls.

  FWI (include/red_diffeq_fwi.h; a plan is referred to by an integer handle, FwiPlan.op_id)
    red_diffeq::fwi_coeffs(v, plan, vel_mode) -> (coeffs, vstat)                   K3
    red_diffeq::fwi_forward(coeffs, plan, B, keep_history) -> (seis, history)      K1
    red_diffeq::fwi_adjoint(coeffs, history, dseis, plan, B) -> (gA, gk, gbeta)    K2
    red_diffeq::fwi_grad_finalize(coeffs, vstat, gA, gk, gbeta, plan, B, vel_mode) -> grad   K4
    red_diffeq::fwi(v, plan, vel_mode, keep_history) -> (seis, coeffs, vstat, history)
        differentiable in v (register_autograd: adjoint + finalize), what FWIForward calls
    red_diffeq::fwi_born(coeffs, vstat, history, dv, plan, B, vel_mode) -> dseis
        the linearised forward J dv over a stored history (FWIForward.born / gauss_newton; no autograd formula)
    red_diffeq::fwi_born_fused(coeffs, vstat, dv, plan, B, vel_mode, K) -> (seis, dseis, ckpt)
        the forward and J dv in one time loop with no history (born / gauss_newton with history=False); K = 0: no
        checkpoints, K >= 1: also fwi_forward_ckpt's store, for fwi_adjoint_ckpt
    red_diffeq::fwi_forward_ckpt(coeffs, plan, B, K) -> (seis, ckpt)               K1, checkpoints every K steps
    red_diffeq::fwi_adjoint_ckpt(coeffs, ckpt, seg, dseis, plan, B, K) -> (gA, gk, gbeta)
        K2 over segments recomputed into the scratch `seg` (the one mutated argument)
    red_diffeq::fwi_ckpt(v, plan, vel_mode, K) -> (seis, coeffs, vstat, ckpt)
        differentiable in v with the history bounded by recomputation (FWIForward(checkpoint=...))
    red_diffeq::fwi_src(v, w, plan, vel_mode, keep_history) / fwi_ckpt_src(v, w, plan, vel_mode, K)
        fwi / fwi_ckpt with the call's own wavelets w (B, ns, nt), differentiable in v and in w
        (FWIForward.forward(v, wavelet=...)); built on fwi_forward_src / fwi_adjoint_src /
        fwi_forward_ckpt_src / fwi_adjoint_ckpt_src (rdq_fwi_*_src), whose adjoints also return gw = d loss / d w
    red_diffeq::enc_fwi(v, weff, plan, vel_mode, keep_history) / enc_fwi_ckpt(v, weff, plan, vel_mode, K)
        encoded supershots: ne wavefields per model, each fired by all ns sources with the effective wavelets
        weff (B, ne, ns, nt); seis (B, ne, nrec, ng), differentiable in v and in weff
        (FWIForward.forward(v, encoding=E)); built on enc_fwi_forward / enc_fwi_adjoint / enc_fwi_forward_ckpt /
        enc_fwi_adjoint_ckpt / enc_fwi_grad_finalize (rdq_fwi_*_enc).  (Named enc_fwi*, not fwi*_enc: the set of
        fwi* operators is pinned by the host tests.)
    red_diffeq::illum_fwi(history, plan, B, nwf) -> hA / illum_fwi_ckpt(coeffs, ckpt, seg, plan, B, K) -> hA (and
        illum_fwi_ckpt_src(coeffs, w, ...), illum_fwi_ckpt_enc(coeffs, weff, ...)) /
        illum_fwi_finalize(coeffs, hA, plan, B, nwf, vel_mode) -> H
        the source illumination / pseudo-Hessian diagonal (rdq_fwi_illum*; FWIForward.illumination; no autograd
        formula).  (Named illum_fwi*, as enc_fwi*.)
  U-Net (include/red_diffeq_unet.h)
    conv2d_mfma, conv2d_rms, conv2d_gn_silu, conv2d_bf16_gn_silu, conv2d_bf16_gn_silu_out, conv2d_gn_silu_sc, conv2d_gn_silu_lsm, conv2d_gn_silu_out, unet_head,
    gn_silu, rmsnorm, linear, time_mlp, linear_silu_multi, sinusoidal_emb, linear_attn, linear_attn_block, attn,
    red_q_sample, red_q_sample_into, red_eps
  prior sampling (include/red_diffeq_sampling.h)
    sample_step(x_t, t, out, noise, tables, ...) writes x_next (and x_start_out / t_out): the fused reverse step
  loop(include/red_diffeq_loop.h)
    l1_misfit / l1_misfit_backward, smooth_reg / smooth_reg_backward, metrics, adam_clamp_
  misfits beyond L1 (include/red_diffeq_misfit.h)
    misfit(pred, y, mask, kind, delta) -> (loss, norm, coef), misfit_backward(..., norm, coef, gout, kind, delta)

No CPU implementation is registered: a CPU tensor reaching an op raises (no fallback).
"""
import ctypes
import weakref
from typing import List, Optional, Tuple

import torch
from torch import Tensor
from torch.utils.weak import WeakIdKeyDictionary

from . import _hip

LIB = "red_diffeq"
_PLANS = {}           # op handle -> weakref(FwiPlan); FwiPlan.__del__ unregisters


def register_plan(plan):
    h = id(plan)
    _PLANS[h] = weakref.ref(plan)
    return h


def unregister_plan(h):
    _PLANS.pop(h, None)


def _plan(h):
    ref = _PLANS.get(int(h))
    p = ref() if ref is not None else None
    if p is None:
        raise RuntimeError(f"red_diffeq: unknown FWI plan handle {h}")
    return p


def _f32(n, dev):
    return torch.empty(int(n) // 4, dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------ FWI
@torch.library.custom_op(f"{LIB}::fwi_coeffs", mutates_args=())
def fwi_coeffs(v: Tensor, plan: int, vel_mode: int) -> Tuple[Tensor, Tensor]:
    p = _plan(plan)
    _hip.require_device(v)
    B = v.shape[0]
    sz = p.sizes(B)
    coeffs = _f32(sz.coeffs, v.device)
    vstat = torch.empty(int(sz.vstat), dtype=torch.uint8, device=v.device)
    strides = (ctypes.c_int64 * 4)(*v.stride())
    _hip.check(p.lib.rdq_fwi_coeffs(p.handle, B, _hip.ptr(v), strides, vel_mode, _hip.ptr(coeffs), _hip.ptr(vstat),
                                    _hip.stream_of(v)), "rdq_fwi_coeffs")
    return coeffs, vstat


@fwi_coeffs.register_fake
def _(v, plan, vel_mode):
    sz = _plan(plan).sizes(v.shape[0])
    return (v.new_empty(int(sz.coeffs) // 4, dtype=torch.float32),
            v.new_empty(int(sz.vstat), dtype=torch.uint8))


def _seis_shape(p, B, ne=None):
    return (B, p.ns if ne is None else ne, p.sizes(B).nrec, p.ng)


def _sizes(p, B, ne=None):
    """rdq_fwi_sizes, or (ne: an encoded call's supershots per model) rdq_fwi_sizes_enc."""
    return p.sizes(B) if ne is None else p.sizes_enc(B, ne)


def _ckpt_sizes(p, B, K, ne=None):
    return p.ckpt_sizes(B, K) if ne is None else p.ckpt_sizes_enc(B, ne, K)


def _fake_coeffs(v, plan):
    sz = _plan(plan).sizes(v.shape[0])
    return v.new_empty(int(sz.coeffs) // 4, dtype=torch.float32), v.new_empty(int(sz.vstat), dtype=torch.uint8)


def _fake_forward(coeffs, plan, B, keep_history=False, K=None, ne=None):
    """(seis, store): store = the history (K None; empty unless keep_history) or the checkpoint store for K."""
    p = _plan(plan)
    nbytes = _ckpt_sizes(p, B, K, ne).ckpt if K is not None else (_sizes(p, B, ne).history if keep_history else 0)
    return coeffs.new_empty(_seis_shape(p, B, ne)), coeffs.new_empty(int(nbytes) // 4)


def _gw_shape(p, B, ne=None):
    return (B, p.ns, p.nt) if ne is None else (B, ne, p.ns, p.nt)


def _fake_adjoint(coeffs, plan, B, want_gw=None, ne=None):
    """The accumulators (gA, gk, gbeta), and with want_gw given (the _src and enc_ ops) also gw."""
    p = _plan(plan)
    sz = _sizes(p, B, ne)
    acc = (coeffs.new_empty(int(sz.gA) // 4), coeffs.new_empty(int(sz.gk_part) // 8, dtype=torch.float64),
           coeffs.new_empty(int(sz.gbeta) // 4))
    return acc if want_gw is None else acc + (coeffs.new_empty(_gw_shape(p, B, ne) if want_gw else (0,)),)


# Caller-supplied wavelets, per model and per shot, differentiable (rdq_fwi_*_src): always the narrow chunked
# kernels.  `w` is (B, ns, nt) fp32 with a unit last stride; a zero stride on the first or second axis (an
# expand() of a shared wavelet) is passed on as "shared", so nothing is materialised and autograd's own expand
# backward sums the gradient over the shared axes.
def _source(p, w, B, gw=None):
    if w.dim() != 3 or tuple(w.shape) != (B, p.ns, p.nt) or w.dtype != torch.float32:
        raise ValueError(f"fwi wavelet: expected fp32 of shape {(B, p.ns, p.nt)}, got {w.dtype} {tuple(w.shape)}")
    if w.stride(2) != 1 or w.stride(0) < 0 or w.stride(1) < 0:
        w = w.contiguous()
    # (the tensor is returned too: it owns the memory the struct points to)
    return w, _hip.FwiSource(wav=w.data_ptr(), model_stride=w.stride(0), shot_stride=w.stride(1),
                             gwav=gw.data_ptr() if gw is not None else None)


# Encoded supershots (rdq_fwi_*_enc): `weff` is (B, ne, ns, nt) fp32 with a unit last stride; zero strides (expanded
# axes) are passed on as "shared", as _source does.
def _encoding(p, weff, B, gw=None):
    if weff.dim() != 4 or weff.shape[0] != B or weff.shape[1] < 1 or tuple(weff.shape[2:]) != (p.ns, p.nt) \
            or weff.dtype != torch.float32:
        raise ValueError(f"fwi encoding: expected fp32 effective wavelets of shape {(B, 'ne', p.ns, p.nt)}, got "
                         f"{weff.dtype} {tuple(weff.shape)}")
    if weff.stride(3) != 1 or min(weff.stride()[:3]) < 0:
        weff = weff.contiguous()
    return weff, _hip.FwiEncoding(ne=weff.shape[1], wav=weff.data_ptr(), model_stride=weff.stride(0),
                                  enc_stride=weff.stride(1), source_stride=weff.stride(2),
                                  gwav=gw.data_ptr() if gw is not None else None)


def _run_forward(coeffs, plan, B, keep_history=False, K=None, w=None, enc=False):
    """The one forward behind fwi_forward{,_ckpt}{,_src} and enc_fwi_forward{,_ckpt}: rdq_fwi_forward{,_ckpt}{,_src,
    _enc}.  K: checkpoints every K steps instead of a history; w: the call's own wavelets, or (enc) its effective
    wavelets (B, ne, ns, nt).  Returns (seis, history | ckpt)."""
    p = _plan(plan)
    _hip.require_device(coeffs, w)
    ne = None
    if enc:
        w, src = _encoding(p, w, B)
        ne = w.shape[1]
    sz = _sizes(p, B, ne)
    nstore = _ckpt_sizes(p, B, K, ne).ckpt if K is not None else (sz.history if keep_history else 0)   # (K < 1 raises here)
    entry = "rdq_fwi_forward" + ("_ckpt" if K is not None else "") + ("_enc" if enc else "_src" if w is not None else "")
    if w is not None and not enc:
        w, src = _source(p, w, B)
    seis = torch.empty(_seis_shape(p, B, ne), dtype=torch.float32, device=coeffs.device)
    store = _f32(nstore, coeffs.device)
    ring = _f32(sz.ring, coeffs.device)
    args = [p.handle, B] + ([K] if K is not None else []) + [_hip.ptr(coeffs)]
    args += [ctypes.byref(src)] if w is not None else []
    args += [_hip.ptr(seis), _hip.ptr(store) if K is not None or keep_history else ctypes.c_void_p(0), _hip.ptr(ring),
             _hip.stream_of(coeffs)]
    _hip.check(getattr(p.lib, entry)(*args), entry)
    return seis, store


def _run_adjoint(op, coeffs, dseis, plan, B, history=None, ckpt=None, seg=None, K=None, w=None, want_gw=False,
                 enc=False):
    """The one adjoint behind fwi_adjoint{,_ckpt}{,_src} and enc_fwi_adjoint{,_ckpt}: rdq_fwi_adjoint{,_ckpt}{,_src,
    _enc} over a stored `history`, or (K) over the checkpoint store `ckpt` with every segment recomputed into the
    scratch `seg`.  `op` names the public op in error messages.  Returns (gA, gk, gbeta, gw); gw is empty unless
    want_gw."""
    p = _plan(plan)
    _hip.require_device(coeffs, w, history, ckpt, seg, dseis)
    ne = w.shape[1] if enc and w.dim() == 4 else None
    sz = _sizes(p, B, ne)
    if K is None:
        if dseis.shape != _seis_shape(p, B, ne) or history.numel() * 4 != sz.history:
            raise ValueError(f"{op}: dseis / history do not match the plan")
        stores = [_hip.ptr(history)]
    else:
        cs = _ckpt_sizes(p, B, K, ne)
        if dseis.shape != _seis_shape(p, B, ne):
            raise ValueError(f"{op}: dseis does not match the plan")
        if ckpt.dtype != torch.float32 or seg.dtype != torch.float32 or ckpt.numel() * 4 != cs.ckpt \
                or seg.numel() * 4 != cs.seg or not ckpt.is_contiguous() or not seg.is_contiguous():
            raise ValueError(f"{op}: ckpt / seg must be contiguous fp32 of {cs.ckpt} / {cs.seg} bytes "
                             f"(K = {K}), got {ckpt.numel() * ckpt.element_size()} / {seg.numel() * seg.element_size()}")
        stores = [_hip.ptr(ckpt), _hip.ptr(seg)]
    dseis = dseis.float().contiguous()
    gw = torch.empty(_gw_shape(p, B, ne) if want_gw else (0,), dtype=torch.float32, device=coeffs.device)
    entry = "rdq_fwi_adjoint" + ("_ckpt" if K is not None else "") + ("_enc" if enc else "_src" if w is not None else "")
    if enc:
        w, src = _encoding(p, w, B, gw if want_gw else None)
    elif w is not None:
        w, src = _source(p, w, B, gw if want_gw else None)
    ring = _f32(sz.ring, coeffs.device)
    gA = _f32(sz.gA, coeffs.device)
    gk = torch.empty(int(sz.gk_part) // 8, dtype=torch.float64, device=coeffs.device)
    gb = _f32(sz.gbeta, coeffs.device)
    args = [p.handle, B] + ([K] if K is not None else []) + [_hip.ptr(coeffs)]
    args += [ctypes.byref(src)] if w is not None else []
    args += stores + [_hip.ptr(dseis), _hip.ptr(ring), _hip.ptr(gA), _hip.ptr(gk), _hip.ptr(gb), _hip.stream_of(coeffs)]
    _hip.check(getattr(p.lib, entry)(*args), entry)
    return gA, gk, gb, gw


@torch.library.custom_op(f"{LIB}::fwi_forward", mutates_args=())
def fwi_forward(coeffs: Tensor, plan: int, B: int, keep_history: bool) -> Tuple[Tensor, Tensor]:
    return _run_forward(coeffs, plan, B, keep_history)


@fwi_forward.register_fake
def _(coeffs, plan, B, keep_history):
    return _fake_forward(coeffs, plan, B, keep_history)


@torch.library.custom_op(f"{LIB}::fwi_adjoint", mutates_args=())
def fwi_adjoint(coeffs: Tensor, history: Tensor, dseis: Tensor, plan: int, B: int) -> Tuple[Tensor, Tensor, Tensor]:
    return _run_adjoint("fwi_adjoint", coeffs, dseis, plan, B, history=history)[:3]


@fwi_adjoint.register_fake
def _(coeffs, history, dseis, plan, B):
    return _fake_adjoint(coeffs, plan, B)


@torch.library.custom_op(f"{LIB}::fwi_grad_finalize", mutates_args=())
def fwi_grad_finalize(coeffs: Tensor, vstat: Tensor, gA: Tensor, gk: Tensor, gbeta: Tensor, plan: int, B: int,
                      vel_mode: int) -> Tensor:
    p = _plan(plan)
    _hip.require_device(coeffs, gA)
    sz = p.sizes(B)
    colsum = torch.empty(int(sz.colsum) // 8, dtype=torch.float64, device=coeffs.device)
    out = torch.empty(B, 1, p.nz, p.nx, dtype=torch.float32, device=coeffs.device)
    _hip.check(p.lib.rdq_fwi_grad_finalize(p.handle, B, _hip.ptr(coeffs), _hip.ptr(vstat), _hip.ptr(gA), _hip.ptr(gk),
                                           _hip.ptr(gbeta), vel_mode, _hip.ptr(colsum), _hip.ptr(out),
                                           _hip.stream_of(coeffs)), "rdq_fwi_grad_finalize")
    return out


@fwi_grad_finalize.register_fake
def _(coeffs, vstat, gA, gk, gbeta, plan, B, vel_mode):
    p = _plan(plan)
    return coeffs.new_empty(B, 1, p.nz, p.nx)


# ---- linearised (Born) forward: J dv over the stored history (rdq_fwi_dcoeffs + rdq_fwi_born)
@torch.library.custom_op(f"{LIB}::fwi_born", mutates_args=())
def fwi_born(coeffs: Tensor, vstat: Tensor, history: Tensor, dv: Tensor, plan: int, B: int, vel_mode: int) -> Tensor:
    """dseis = J dv at the model `coeffs` / `vstat` / `history` (fwi_coeffs, fwi_forward with history) belong to."""
    p = _plan(plan)
    _hip.require_device(coeffs, vstat, history, dv)
    sz = p.sizes(B)
    if tuple(dv.shape) != (B, 1, p.nz, p.nx) or history.numel() * 4 != sz.history:
        raise ValueError("fwi_born: dv / history do not match the plan")
    dv = dv.float()
    nbytes = ctypes.c_size_t()
    _hip.check(p.lib.rdq_fwi_born_sizes(p.handle, B, ctypes.byref(nbytes)), "rdq_fwi_born_sizes")
    dwork = _f32(nbytes.value, coeffs.device)
    ring = _f32(sz.ring, coeffs.device)
    dseis = torch.empty(_seis_shape(p, B), dtype=torch.float32, device=coeffs.device)
    strides = (ctypes.c_int64 * 4)(*dv.stride())
    st = _hip.stream_of(coeffs)
    _hip.check(p.lib.rdq_fwi_dcoeffs(p.handle, B, _hip.ptr(dv), strides, vel_mode, _hip.ptr(coeffs), _hip.ptr(vstat),
                                     _hip.ptr(dwork), st), "rdq_fwi_dcoeffs")
    _hip.check(p.lib.rdq_fwi_born(p.handle, B, _hip.ptr(coeffs), _hip.ptr(dwork), _hip.ptr(history), _hip.ptr(dseis),
                                  _hip.ptr(ring), st), "rdq_fwi_born")
    return dseis


@fwi_born.register_fake
def _(coeffs, vstat, history, dv, plan, B, vel_mode):
    return coeffs.new_empty(_seis_shape(_plan(plan), B))


# ---- fused forward + Born pass: seis and J dv in one time loop with no history (rdq_fwi_dcoeffs + rdq_fwi_born_fused)
def _fused_ckpt_bytes(p, B, K):
    if K < 0:
        raise ValueError(f"fwi_born_fused: K must be 0 (no checkpoints) or >= 1, got {K}")
    return int(p.ckpt_sizes(B, K).ckpt) if K >= 1 else 0


@torch.library.custom_op(f"{LIB}::fwi_born_fused", mutates_args=())
def fwi_born_fused(coeffs: Tensor, vstat: Tensor, dv: Tensor, plan: int, B: int, vel_mode: int,
                   K: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(seis, dseis = J dv, ckpt) at the model `coeffs` / `vstat` (fwi_coeffs) belong to.  K = 0: no checkpoints
    (ckpt is empty); K >= 1: ckpt is fwi_forward_ckpt's store for K steps per segment, for fwi_adjoint_ckpt."""
    p = _plan(plan)
    _hip.require_device(coeffs, vstat, dv)
    sz = p.sizes(B)
    if tuple(dv.shape) != (B, 1, p.nz, p.nx):
        raise ValueError("fwi_born_fused: dv does not match the plan")
    dv = dv.float()
    nbytes = ctypes.c_size_t()
    _hip.check(p.lib.rdq_fwi_born_sizes(p.handle, B, ctypes.byref(nbytes)), "rdq_fwi_born_sizes")
    dwork = _f32(nbytes.value, coeffs.device)
    ring = _f32(sz.ring, coeffs.device)
    ckpt = _f32(_fused_ckpt_bytes(p, B, K), coeffs.device)
    seis = torch.empty(_seis_shape(p, B), dtype=torch.float32, device=coeffs.device)
    dseis = torch.empty(_seis_shape(p, B), dtype=torch.float32, device=coeffs.device)
    strides = (ctypes.c_int64 * 4)(*dv.stride())
    st = _hip.stream_of(coeffs)
    _hip.check(p.lib.rdq_fwi_dcoeffs(p.handle, B, _hip.ptr(dv), strides, vel_mode, _hip.ptr(coeffs), _hip.ptr(vstat),
                                     _hip.ptr(dwork), st), "rdq_fwi_dcoeffs")
    _hip.check(p.lib.rdq_fwi_born_fused(p.handle, B, max(K, 1), _hip.ptr(coeffs), _hip.ptr(dwork), _hip.ptr(seis),
                                        _hip.ptr(dseis), _hip.ptr(ckpt) if ckpt.numel() else ctypes.c_void_p(0),
                                        _hip.ptr(ring), st), "rdq_fwi_born_fused")
    return seis, dseis, ckpt


@fwi_born_fused.register_fake
def _(coeffs, vstat, dv, plan, B, vel_mode, K):
    p = _plan(plan)
    return (coeffs.new_empty(_seis_shape(p, B)), coeffs.new_empty(_seis_shape(p, B)),
            coeffs.new_empty(_fused_ckpt_bytes(p, B, K) // 4))


# ---- checkpointed gradient: the history bounded by recomputation (rdq_fwi_forward_ckpt / _adjoint_ckpt)
@torch.library.custom_op(f"{LIB}::fwi_forward_ckpt", mutates_args=())
def fwi_forward_ckpt(coeffs: Tensor, plan: int, B: int, K: int) -> Tuple[Tensor, Tensor]:
    """First pass: (seis, ckpt), ckpt = two wavefield levels per interior segment boundary."""
    return _run_forward(coeffs, plan, B, K=K)


@fwi_forward_ckpt.register_fake
def _(coeffs, plan, B, K):
    return _fake_forward(coeffs, plan, B, K=K)


@torch.library.custom_op(f"{LIB}::fwi_adjoint_ckpt", mutates_args=("seg",))
def fwi_adjoint_ckpt(coeffs: Tensor, ckpt: Tensor, seg: Tensor, dseis: Tensor, plan: int, B: int,
                     K: int) -> Tuple[Tensor, Tensor, Tensor]:
    """Backward: every segment recomputed into the scratch `seg`, then its adjoint; (gA, gk, gbeta)."""
    return _run_adjoint("fwi_adjoint_ckpt", coeffs, dseis, plan, B, ckpt=ckpt, seg=seg, K=K)[:3]


@fwi_adjoint_ckpt.register_fake
def _(coeffs, ckpt, seg, dseis, plan, B, K):
    return _fake_adjoint(coeffs, plan, B)


# ---- the call's own wavelets (rdq_fwi_*_src; _source above)
@torch.library.custom_op(f"{LIB}::fwi_forward_src", mutates_args=())
def fwi_forward_src(coeffs: Tensor, w: Tensor, plan: int, B: int, keep_history: bool) -> Tuple[Tensor, Tensor]:
    """fwi_forward with the source samples w[b, s, n] instead of the plan's wavelet."""
    return _run_forward(coeffs, plan, B, keep_history, w=w)


@fwi_forward_src.register_fake
def _(coeffs, w, plan, B, keep_history):
    return _fake_forward(coeffs, plan, B, keep_history)


@torch.library.custom_op(f"{LIB}::fwi_adjoint_src", mutates_args=())
def fwi_adjoint_src(coeffs: Tensor, w: Tensor, history: Tensor, dseis: Tensor, plan: int, B: int,
                    want_gw: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(gA, gk, gbeta, gw): fwi_adjoint with the source samples w, and gw = d(loss)/d(w) (B, ns, nt) where
    want_gw (else empty: the kernel is given no gwav and nothing is allocated)."""
    return _run_adjoint("fwi_adjoint_src", coeffs, dseis, plan, B, history=history, w=w, want_gw=want_gw)


@fwi_adjoint_src.register_fake
def _(coeffs, w, history, dseis, plan, B, want_gw):
    return _fake_adjoint(coeffs, plan, B, want_gw)


@torch.library.custom_op(f"{LIB}::fwi_forward_ckpt_src", mutates_args=())
def fwi_forward_ckpt_src(coeffs: Tensor, w: Tensor, plan: int, B: int, K: int) -> Tuple[Tensor, Tensor]:
    """fwi_forward_ckpt with the source samples w."""
    return _run_forward(coeffs, plan, B, K=K, w=w)


@fwi_forward_ckpt_src.register_fake
def _(coeffs, w, plan, B, K):
    return _fake_forward(coeffs, plan, B, K=K)


@torch.library.custom_op(f"{LIB}::fwi_adjoint_ckpt_src", mutates_args=("seg",))
def fwi_adjoint_ckpt_src(coeffs: Tensor, w: Tensor, ckpt: Tensor, seg: Tensor, dseis: Tensor, plan: int, B: int,
                         K: int, want_gw: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(gA, gk, gbeta, gw): fwi_adjoint_ckpt with the source samples w (the recompute reads them again)."""
    return _run_adjoint("fwi_adjoint_ckpt_src", coeffs, dseis, plan, B, ckpt=ckpt, seg=seg, K=K, w=w, want_gw=want_gw)


@fwi_adjoint_ckpt_src.register_fake
def _(coeffs, w, ckpt, seg, dseis, plan, B, K, want_gw):
    return _fake_adjoint(coeffs, plan, B, want_gw)


# ---- encoded supershots (rdq_fwi_*_enc; _encoding above): every per-shot axis holds the ne supershots
@torch.library.custom_op(f"{LIB}::enc_fwi_forward", mutates_args=())
def enc_fwi_forward(coeffs: Tensor, weff: Tensor, plan: int, B: int, keep_history: bool) -> Tuple[Tensor, Tensor]:
    """fwi_forward of ne supershots: wavefield (b, e) takes every source s with the samples weff[b, e, s, n]."""
    return _run_forward(coeffs, plan, B, keep_history, w=weff, enc=True)


@enc_fwi_forward.register_fake
def _(coeffs, weff, plan, B, keep_history):
    return _fake_forward(coeffs, plan, B, keep_history, ne=weff.shape[1])


@torch.library.custom_op(f"{LIB}::enc_fwi_adjoint", mutates_args=())
def enc_fwi_adjoint(coeffs: Tensor, weff: Tensor, history: Tensor, dseis: Tensor, plan: int, B: int,
                    want_gw: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(gA, gk, gbeta (B * ne * ns), gw): the adjoint of enc_fwi_forward, and gw = d(loss)/d(weff) (B, ne, ns, nt)
    where want_gw (else empty: the kernel is given no gwav and nothing is allocated)."""
    return _run_adjoint("enc_fwi_adjoint", coeffs, dseis, plan, B, history=history, w=weff, want_gw=want_gw, enc=True)


@enc_fwi_adjoint.register_fake
def _(coeffs, weff, history, dseis, plan, B, want_gw):
    return _fake_adjoint(coeffs, plan, B, want_gw, ne=weff.shape[1])


@torch.library.custom_op(f"{LIB}::enc_fwi_forward_ckpt", mutates_args=())
def enc_fwi_forward_ckpt(coeffs: Tensor, weff: Tensor, plan: int, B: int, K: int) -> Tuple[Tensor, Tensor]:
    """fwi_forward_ckpt of ne supershots."""
    return _run_forward(coeffs, plan, B, K=K, w=weff, enc=True)


@enc_fwi_forward_ckpt.register_fake
def _(coeffs, weff, plan, B, K):
    return _fake_forward(coeffs, plan, B, K=K, ne=weff.shape[1])


@torch.library.custom_op(f"{LIB}::enc_fwi_adjoint_ckpt", mutates_args=("seg",))
def enc_fwi_adjoint_ckpt(coeffs: Tensor, weff: Tensor, ckpt: Tensor, seg: Tensor, dseis: Tensor, plan: int, B: int,
                         K: int, want_gw: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(gA, gk, gbeta, gw): fwi_adjoint_ckpt of ne supershots (the recompute reads weff again)."""
    return _run_adjoint("enc_fwi_adjoint_ckpt", coeffs, dseis, plan, B, ckpt=ckpt, seg=seg, K=K, w=weff,
                        want_gw=want_gw, enc=True)


@enc_fwi_adjoint_ckpt.register_fake
def _(coeffs, weff, ckpt, seg, dseis, plan, B, K, want_gw):
    return _fake_adjoint(coeffs, plan, B, want_gw, ne=weff.shape[1])


@torch.library.custom_op(f"{LIB}::enc_fwi_grad_finalize", mutates_args=())
def enc_fwi_grad_finalize(coeffs: Tensor, vstat: Tensor, gA: Tensor, gk: Tensor, gbeta: Tensor, plan: int, B: int,
                          ne: int, vel_mode: int) -> Tensor:
    """K4 over the accumulators of an encoded adjoint: the ne planes summed in order, gbeta summed over e per source."""
    p = _plan(plan)
    _hip.require_device(coeffs, gA)
    sz = p.sizes_enc(B, ne)
    if gA.numel() * 4 != sz.gA or gk.numel() * 8 != sz.gk_part or gbeta.numel() * 4 != sz.gbeta:
        raise ValueError("enc_fwi_grad_finalize: gA / gk / gbeta do not match the plan and ne")
    colsum = torch.empty(int(sz.colsum) // 8, dtype=torch.float64, device=coeffs.device)
    out = torch.empty(B, 1, p.nz, p.nx, dtype=torch.float32, device=coeffs.device)
    _hip.check(p.lib.rdq_fwi_grad_finalize_enc(p.handle, B, ne, _hip.ptr(coeffs), _hip.ptr(vstat), _hip.ptr(gA),
                                               _hip.ptr(gk), _hip.ptr(gbeta), vel_mode, _hip.ptr(colsum), _hip.ptr(out),
                                               _hip.stream_of(coeffs)), "rdq_fwi_grad_finalize_enc")
    return out


@enc_fwi_grad_finalize.register_fake
def _(coeffs, vstat, gA, gk, gbeta, plan, B, ne, vel_mode):
    p = _plan(plan)
    return coeffs.new_empty(B, 1, p.nz, p.nx)


# ---- source illumination / pseudo-Hessian diagonal (rdq_fwi_illum / _illum_ckpt / _illum_finalize).  Functional, no
# autograd formula.  (Named illum_fwi*, not fwi_illum*: the set of fwi* operators is pinned by the host tests.)
def _illum_nwf(p, nwf):
    if nwf < 0:
        raise ValueError(f"illum_fwi: nwf must be 0 (the plan's shots) or >= 1, got {nwf}")
    return p.ns if nwf == 0 else int(nwf)


def _illum_sizes(p, B, nwf):
    return p.sizes(B) if nwf == p.ns else p.sizes_enc(B, nwf)


@torch.library.custom_op(f"{LIB}::illum_fwi", mutates_args=())
def illum_fwi(history: Tensor, plan: int, B: int, nwf: int) -> Tensor:
    """hA (B * nwf * Hp * ld,) = sum over the steps of q_k^2 from a stored history of nwf wavefields per model
    (nwf = 0: the plan's shots)."""
    p = _plan(plan)
    _hip.require_device(history)
    nw = _illum_nwf(p, nwf)
    sz = _illum_sizes(p, B, nw)
    if history.dtype != torch.float32 or history.numel() * 4 != sz.history or not history.is_contiguous():
        raise ValueError(f"illum_fwi: history must be contiguous fp32 of {sz.history} bytes")
    hA = _f32(sz.gA, history.device)
    _hip.check(p.lib.rdq_fwi_illum(p.handle, B, nw, _hip.ptr(history), _hip.ptr(hA), _hip.stream_of(history)),
               "rdq_fwi_illum")
    return hA


@illum_fwi.register_fake
def _(history, plan, B, nwf):
    p = _plan(plan)
    return history.new_empty(int(_illum_sizes(p, B, _illum_nwf(p, nwf)).gA) // 4)


def _run_illum_ckpt(op, coeffs, ckpt, seg, plan, B, K, w=None, enc=False):
    """The one checkpointed illumination pass behind illum_fwi_ckpt{,_src,_enc}."""
    p = _plan(plan)
    _hip.require_device(coeffs, w, ckpt, seg)
    ne = None
    src = enc_s = None
    if enc:
        w, enc_s = _encoding(p, w, B)
        ne = w.shape[1]
    elif w is not None:
        w, src = _source(p, w, B)
    sz, cs = _sizes(p, B, ne), _ckpt_sizes(p, B, K, ne)
    if ckpt.dtype != torch.float32 or seg.dtype != torch.float32 or ckpt.numel() * 4 != cs.ckpt \
            or seg.numel() * 4 != cs.seg or not ckpt.is_contiguous() or not seg.is_contiguous():
        raise ValueError(f"{op}: ckpt / seg must be contiguous fp32 of {cs.ckpt} / {cs.seg} bytes (K = {K})")
    ring = _f32(sz.ring, coeffs.device)
    hA = _f32(sz.gA, coeffs.device)
    _hip.check(p.lib.rdq_fwi_illum_ckpt(p.handle, B, K, _hip.ptr(coeffs), ctypes.byref(src) if src is not None else None,
                                        ctypes.byref(enc_s) if enc_s is not None else None,
                                        _hip.ptr(ckpt) if ckpt.numel() else ctypes.c_void_p(0), _hip.ptr(seg),
                                        _hip.ptr(ring), _hip.ptr(hA), _hip.stream_of(coeffs)), "rdq_fwi_illum_ckpt")
    return hA


def _fake_illum_ckpt(coeffs, plan, B, ne=None):
    return coeffs.new_empty(int(_sizes(_plan(plan), B, ne).gA) // 4)


@torch.library.custom_op(f"{LIB}::illum_fwi_ckpt", mutates_args=("seg",))
def illum_fwi_ckpt(coeffs: Tensor, ckpt: Tensor, seg: Tensor, plan: int, B: int, K: int) -> Tensor:
    """hA from fwi_forward_ckpt's store: every segment recomputed into the scratch `seg`, then accumulated."""
    return _run_illum_ckpt("illum_fwi_ckpt", coeffs, ckpt, seg, plan, B, K)


@illum_fwi_ckpt.register_fake
def _(coeffs, ckpt, seg, plan, B, K):
    return _fake_illum_ckpt(coeffs, plan, B)


@torch.library.custom_op(f"{LIB}::illum_fwi_ckpt_src", mutates_args=("seg",))
def illum_fwi_ckpt_src(coeffs: Tensor, w: Tensor, ckpt: Tensor, seg: Tensor, plan: int, B: int, K: int) -> Tensor:
    """illum_fwi_ckpt over fwi_forward_ckpt_src's store (the recompute reads the source samples w again)."""
    return _run_illum_ckpt("illum_fwi_ckpt_src", coeffs, ckpt, seg, plan, B, K, w=w)


@illum_fwi_ckpt_src.register_fake
def _(coeffs, w, ckpt, seg, plan, B, K):
    return _fake_illum_ckpt(coeffs, plan, B)


@torch.library.custom_op(f"{LIB}::illum_fwi_ckpt_enc", mutates_args=("seg",))
def illum_fwi_ckpt_enc(coeffs: Tensor, weff: Tensor, ckpt: Tensor, seg: Tensor, plan: int, B: int, K: int) -> Tensor:
    """illum_fwi_ckpt over enc_fwi_forward_ckpt's store of ne supershots (the recompute reads weff again)."""
    return _run_illum_ckpt("illum_fwi_ckpt_enc", coeffs, ckpt, seg, plan, B, K, w=weff, enc=True)


@illum_fwi_ckpt_enc.register_fake
def _(coeffs, weff, ckpt, seg, plan, B, K):
    return _fake_illum_ckpt(coeffs, plan, B, ne=weff.shape[1])


@torch.library.custom_op(f"{LIB}::illum_fwi_finalize", mutates_args=())
def illum_fwi_finalize(coeffs: Tensor, hA: Tensor, plan: int, B: int, nwf: int, vel_mode: int) -> Tensor:
    """H (B, 1, nz, nx) = (dA/dv)^2 x the replicate fold of the nwf planes of hA (fp64 sums, one cast)."""
    p = _plan(plan)
    _hip.require_device(coeffs, hA)
    nw = _illum_nwf(p, nwf)
    sz = _illum_sizes(p, B, nw)
    if hA.dtype != torch.float32 or hA.numel() * 4 != sz.gA or not hA.is_contiguous():
        raise ValueError("illum_fwi_finalize: hA does not match the plan and nwf")
    colsum = torch.empty(int(sz.colsum) // 8, dtype=torch.float64, device=coeffs.device)
    out = torch.empty(B, 1, p.nz, p.nx, dtype=torch.float32, device=coeffs.device)
    _hip.check(p.lib.rdq_fwi_illum_finalize(p.handle, B, nw, _hip.ptr(coeffs), _hip.ptr(hA), vel_mode, _hip.ptr(colsum),
                                            _hip.ptr(out), _hip.stream_of(coeffs)), "rdq_fwi_illum_finalize")
    return out


@illum_fwi_finalize.register_fake
def _(coeffs, hA, plan, B, nwf, vel_mode):
    p = _plan(plan)
    return coeffs.new_empty(B, 1, p.nz, p.nx)


# ---- the differentiable operators FWIForward calls: K3 + a forward, with the adjoint + K4 as the backward.
# Outputs (seis, coeffs, vstat, store): only seis is differentiable; coeffs / vstat / the history or checkpoint
# store are returned for the backward.
def _fake_fwi(v, plan, keep_history=False, K=None, ne=None):
    coeffs, vstat = _fake_coeffs(v, plan)
    seis, store = _fake_forward(coeffs, plan, v.shape[0], keep_history, K, ne)
    return seis, coeffs, vstat, store


@torch.library.custom_op(f"{LIB}::fwi", mutates_args=())
def fwi(v: Tensor, plan: int, vel_mode: int, keep_history: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """seis = FWM(v) (K3 + K1); coeffs / vstat / history are returned for the backward."""
    coeffs, vstat = fwi_coeffs(v, plan, vel_mode)
    seis, hist = fwi_forward(coeffs, plan, v.shape[0], keep_history)
    return seis, coeffs, vstat, hist


@fwi.register_fake
def _(v, plan, vel_mode, keep_history):
    return _fake_fwi(v, plan, keep_history)


@torch.library.custom_op(f"{LIB}::fwi_ckpt", mutates_args=())
def fwi_ckpt(v: Tensor, plan: int, vel_mode: int, K: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """seis = FWM(v) (K3 + the checkpointed first pass); coeffs / vstat / ckpt are returned for the backward."""
    coeffs, vstat = fwi_coeffs(v, plan, vel_mode)
    seis, ckpt = fwi_forward_ckpt(coeffs, plan, v.shape[0], K)
    return seis, coeffs, vstat, ckpt


@fwi_ckpt.register_fake
def _(v, plan, vel_mode, K):
    return _fake_fwi(v, plan, K=K)


@torch.library.custom_op(f"{LIB}::fwi_src", mutates_args=())
def fwi_src(v: Tensor, w: Tensor, plan: int, vel_mode: int, keep_history: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """seis = FWM(v; w) (K3 + K1 with the call's own wavelets); coeffs / vstat / history are for the backward."""
    coeffs, vstat = fwi_coeffs(v, plan, vel_mode)
    seis, hist = fwi_forward_src(coeffs, w, plan, v.shape[0], keep_history)
    return seis, coeffs, vstat, hist


@fwi_src.register_fake
def _(v, w, plan, vel_mode, keep_history):
    return _fake_fwi(v, plan, keep_history)


@torch.library.custom_op(f"{LIB}::fwi_ckpt_src", mutates_args=())
def fwi_ckpt_src(v: Tensor, w: Tensor, plan: int, vel_mode: int, K: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """fwi_src with the history bounded by recomputation (K steps per segment), as fwi_ckpt."""
    coeffs, vstat = fwi_coeffs(v, plan, vel_mode)
    seis, ckpt = fwi_forward_ckpt_src(coeffs, w, plan, v.shape[0], K)
    return seis, coeffs, vstat, ckpt


@fwi_ckpt_src.register_fake
def _(v, w, plan, vel_mode, K):
    return _fake_fwi(v, plan, K=K)


@torch.library.custom_op(f"{LIB}::enc_fwi", mutates_args=())
def enc_fwi(v: Tensor, weff: Tensor, plan: int, vel_mode: int, keep_history: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """seis (B, ne, nrec, ng) = the ne supershots of weff (B, ne, ns, nt) (K3 + the encoded K1); coeffs / vstat /
    history are for the backward."""
    coeffs, vstat = fwi_coeffs(v, plan, vel_mode)
    seis, hist = enc_fwi_forward(coeffs, weff, plan, v.shape[0], keep_history)
    return seis, coeffs, vstat, hist


@enc_fwi.register_fake
def _(v, weff, plan, vel_mode, keep_history):
    return _fake_fwi(v, plan, keep_history, ne=weff.shape[1])


@torch.library.custom_op(f"{LIB}::enc_fwi_ckpt", mutates_args=())
def enc_fwi_ckpt(v: Tensor, weff: Tensor, plan: int, vel_mode: int, K: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """enc_fwi with the history bounded by recomputation (K steps per segment), as fwi_ckpt."""
    coeffs, vstat = fwi_coeffs(v, plan, vel_mode)
    seis, ckpt = enc_fwi_forward_ckpt(coeffs, weff, plan, v.shape[0], K)
    return seis, coeffs, vstat, ckpt


@enc_fwi_ckpt.register_fake
def _(v, weff, plan, vel_mode, K):
    return _fake_fwi(v, plan, K=K, ne=weff.shape[1])


def _register_gradient(op, name, ckpt, src, enc=False):
    """The autograd formula of fwi{,_ckpt}{,_src} and enc_fwi{,_ckpt}: inputs (v, [w,] plan, vel_mode, keep_history |
    K).  The backward is the adjoint op of the same variant (looked up by name when it runs), then K4 for v (enc: the
    encoded K4); w.grad is the adjoint's gw."""
    adjoint = ("enc_" if enc else "") + "fwi_adjoint" + ("_ckpt" if ckpt else "") + ("_src" if src and not enc else "")

    def setup(ctx, inputs, output):
        v, (plan, vel_mode, last) = inputs[0], inputs[-3:]
        _, coeffs, vstat, store = output
        # only seis is differentiable: no zero "gradients" are materialised for the saved buffers
        # (a zeros_like of the history would be a multi-GB fill per backward)
        ctx.mark_non_differentiable(coeffs, vstat, store)
        ctx.set_materialize_grads(False)
        ctx.plan = None
        if not ckpt and not last:           # keep_history=False
            return
        ctx.plan, ctx.vel_mode, ctx.B, ctx.K = plan, vel_mode, v.shape[0], last
        ctx.coeffs, ctx.vstat, ctx.store = coeffs, vstat, store
        if src:
            ctx.save_for_backward(inputs[1])

    def backward(ctx, gseis, _gc, _gv, _gs):
        if ctx.plan is None:
            raise RuntimeError(f"red_diffeq::{name} was called with keep_history=False; no gradient is available")
        if gseis is None:                   # seis took no part in the loss: no gradient, for every variant
            return (None,) * (5 if src else 4)
        want_v, want_w = ctx.needs_input_grad[0], src and ctx.needs_input_grad[1]
        args = [ctx.coeffs, *ctx.saved_tensors, ctx.store]
        if ckpt:
            ne = ctx.saved_tensors[0].shape[1] if enc else None
            args.append(_f32(_ckpt_sizes(_plan(ctx.plan), ctx.B, ctx.K, ne).seg, ctx.coeffs.device))
        args += [gseis.contiguous(), ctx.plan, ctx.B] + ([ctx.K] if ckpt else []) + ([want_w] if src else [])
        gA, gk, gb, *gw = globals()[adjoint](*args)
        ctx.store = None                    # the history / the checkpoint store, and the segment buffer: released as
        del args                            # soon as the adjoint has run
        if not want_v:
            g = None
        elif enc:
            g = enc_fwi_grad_finalize(ctx.coeffs, ctx.vstat, gA, gk, gb, ctx.plan, ctx.B, ctx.saved_tensors[0].shape[1],
                                      ctx.vel_mode)
        else:
            g = fwi_grad_finalize(ctx.coeffs, ctx.vstat, gA, gk, gb, ctx.plan, ctx.B, ctx.vel_mode)
        return (g, gw[0] if want_w else None, None, None, None) if src else (g, None, None, None)

    op.register_autograd(backward, setup_context=setup)


_register_gradient(fwi, "fwi", ckpt=False, src=False)
_register_gradient(fwi_ckpt, "fwi_ckpt", ckpt=True, src=False)
_register_gradient(fwi_src, "fwi_src", ckpt=False, src=True)
_register_gradient(fwi_ckpt_src, "fwi_ckpt_src", ckpt=True, src=True)
_register_gradient(enc_fwi, "enc_fwi", ckpt=False, src=True, enc=True)
_register_gradient(enc_fwi_ckpt, "enc_fwi_ckpt", ckpt=True, src=True, enc=True)


# ---------------------------------------------------------------------------------------- U-Net
# bf16 weight packs, cached per weight TENSOR (weak keys: an entry dies with its tensor, so a new
# tensor at a recycled address never sees a stale pack) and per (version, input split)
_BF16_PACKS = WeakIdKeyDictionary()


def _conv_desc(x, x2, weight, pad, mode):
    cout, cin, kh, kw = weight.shape
    if mode == 1:
        H, W = x.shape[2] * 2, x.shape[3] * 2
    elif mode == 2:
        H, W = x.shape[2] // 2, x.shape[3] // 2
    else:
        H, W = x.shape[2], x.shape[3]
    cin1 = x.shape[1] * (4 if mode == 2 else 1)
    cin2 = x2.shape[1] if x2 is not None else 0
    if cin1 + cin2 != cin:
        raise ValueError(f"conv expects {cin} input channels, got {cin1}+{cin2}")
    return _hip.ConvDesc(B=x.shape[0], cin1=cin1, cin2=cin2, H=H, W=W, cout=cout, kh=kh, kw=kw, pad=pad,
                         in_mode=mode), (x.shape[0], cout, H, W)


def _bf16_pack(weight, d, stream):
    per = _BF16_PACKS.setdefault(weight, {})
    key = (weight._version, weight.data_ptr(), d.cin1, d.cin2)   # data_ptr: `p.data = t` replaces storage
    wp = per.get(key)
    if wp is None:
        per.clear()                      # older versions of this tensor are dead
        L = _hip.lib()
        wp = torch.empty(int(L.rdq_conv2d_bf16_wpack_bytes(ctypes.byref(d))), dtype=torch.uint8, device=weight.device)
        _hip.check(L.rdq_conv2d_bf16_pack(ctypes.byref(d), _hip.ptr(weight.contiguous()), _hip.ptr(wp), stream),
                   "rdq_conv2d_bf16_pack")
        per[key] = wp
    return wp


def clear_bf16_packs():
    """Drop the cached bf16 weight packs: needed after in-place updates through `.data`, which do
    not bump a tensor's version counter."""
    _BF16_PACKS.clear()


def check_same_conv(kh, kw, pad):
    """The conv kernels write an H x W output with one `pad` for both axes (include/red_diffeq_unet.h, the contract
    of rdq_conv_desc): nn.Conv2d's result exactly when 2 pad = k - 1 on both axes.  Anything else is refused
    here, before any device work, instead of computing something that is not the module's convolution."""
    if 2 * pad != kh - 1 or 2 * pad != kw - 1:
        raise ValueError(f"conv kernels implement 'same' convolutions only: a {kh} x {kw} filter with padding {pad} "
                         f"is not nn.Conv2d's H x W result (need kh = kw = 2 * pad + 1)")


def bf16_eligible(weight):
    cout, cin, kh, kw = weight.shape
    return cin * kh * kw >= 64 and cout >= 16


@torch.library.custom_op(f"{LIB}::conv2d_mfma", mutates_args=())
def conv2d_mfma(x: Tensor, x2: Optional[Tensor], weight: Tensor, bias: Optional[Tensor], residual: Optional[Tensor],
                pad: int, mode: int, bf16: bool) -> Tensor:
    """nn.Conv2d (stride 1) of the logical input cat(x', x2), x' = x | upsample2(x) | unshuffle2(x)
    (mode 0 / 1 / 2), + bias + residual; fp32 MFMA, or bf16 operands with fp32 accumulation.
    ValueError unless kh = kw = 2 pad + 1 (check_same_conv)."""
    check_same_conv(weight.shape[2], weight.shape[3], pad)
    _hip.require_device(x)
    x = x.contiguous()
    x2 = x2.contiguous() if x2 is not None else None
    d, shape = _conv_desc(x, x2, weight, pad, mode)
    y = torch.empty(shape, device=x.device, dtype=torch.float32)
    res = residual.contiguous() if residual is not None else None
    L = _hip.lib()
    st = _hip.stream_of(x)
    if bf16 and tuple(weight.shape) == (64, 1, 7, 7) and pad == 3 and mode == 0 and x2 is None and residual is None \
            and 64 <= x.shape[3] <= 72:
        # the batched bf16 U-Net's stem (an fp32 conv: K = 49 is below the bf16 floor) as a direct conv
        _hip.check(L.rdq_conv2d_stem(ctypes.byref(d), _hip.ptr(x), _hip.ptr(weight.contiguous()), _hip.ptr(bias),
                                     _hip.ptr(y), st), "rdq_conv2d_stem")
        return y
    if bf16 and bf16_eligible(weight):
        wp = _bf16_pack(weight, d, st)
        nws = int(L.rdq_conv2d_bf16_ws_bytes(ctypes.byref(d)))
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws else None
        _hip.check(L.rdq_conv2d_bf16(ctypes.byref(d), _hip.ptr(x), _hip.ptr(x2), _hip.ptr(wp), _hip.ptr(bias),
                                     _hip.ptr(res), _hip.ptr(y), _hip.ptr(ws), nws, st), "rdq_conv2d_bf16")
        return y
    nws = int(L.rdq_conv2d_ws_bytes(ctypes.byref(d)))
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws else None
    tk = _tickets(x.device, int(L.rdq_conv2d_tickets(ctypes.byref(d)))) if nws else None
    _hip.check(L.rdq_conv2d(ctypes.byref(d), _hip.ptr(x), _hip.ptr(x2), _hip.ptr(weight.contiguous()), _hip.ptr(bias),
                            _hip.ptr(res), _hip.ptr(y), _hip.ptr(ws), nws, tk, st), "rdq_conv2d")
    return y


# Split-K arrival tickets of rdq_conv2d (include/red_diffeq_unet.h): one zeroed pool per device,
# every launch leaves its words zero again.  Eager calls take consecutive windows of a ring (a window
# comes round again only thousands of launches later); calls captured into a hipGraph get windows
# that no later call reuses, since a graph replays with the same words, possibly beside eager work
# on another stream.  No pool yet (first call inside a capture) or the graph region used up: no
# tickets, and the slabs are combined by a second launch instead (same result).
_TICKET_POOL = {}
_TICKET_EAGER, _TICKET_GRAPH = 1 << 18, 1 << 19


def _tickets(device, n):
    capturing = torch.cuda.is_current_stream_capturing()
    st = _TICKET_POOL.get(device)
    if st is None:
        if capturing:
            return None
        st = _TICKET_POOL[device] = {"pool": torch.zeros(_TICKET_EAGER + _TICKET_GRAPH, dtype=torch.int32,
                                                         device=device), "eager": 0, "graph": 0}
    if capturing:
        if st["graph"] + n > _TICKET_GRAPH:
            return None
        off = _TICKET_EAGER + st["graph"]
        st["graph"] += n
    else:
        if st["eager"] + n > _TICKET_EAGER:
            st["eager"] = 0
        off = st["eager"]
        st["eager"] += n
    return st["pool"].data_ptr() + 4 * off


@conv2d_mfma.register_fake
def _(x, x2, weight, bias, residual, pad, mode, bf16):
    _, shape = _conv_desc(x, x2, weight, pad, mode)
    return x.new_empty(shape)


@torch.library.custom_op(f"{LIB}::gn_silu", mutates_args=())
def gn_silu(x: Tensor, weight: Tensor, bias: Tensor, scale_shift: Optional[Tensor], groups: int, eps: float) -> Tensor:
    """GroupNorm(groups) -> x * (scale + 1) + shift -> SiLU; scale_shift (B, 2C), scale first."""
    _hip.require_device(x)
    x = x.contiguous()
    B, C, H, W = x.shape
    L = _hip.lib()
    ws = torch.empty(max(8, int(L.rdq_group_norm_ws_bytes(B, C, H * W, groups))), dtype=torch.uint8, device=x.device)
    y = torch.empty_like(x)
    ss = scale_shift.contiguous() if scale_shift is not None else None
    _hip.check(L.rdq_group_norm_silu(B, C, H * W, groups, float(eps), _hip.ptr(x), _hip.ptr(weight), _hip.ptr(bias),
                                     _hip.ptr(ss), _hip.ptr(y), _hip.ptr(ws), _hip.stream_of(x)), "rdq_group_norm_silu")
    return y


@gn_silu.register_fake
def _(x, weight, bias, scale_shift, groups, eps):
    return torch.empty_like(x)


def conv_rms_fusable(x, weight):
    """rdq_conv2d_rms applies: 1x1 conv, channel counts multiples of 64 (<= 2048), fp32 extents."""
    cout, cin, kh, kw = weight.shape
    return kh == 1 and kw == 1 and cin % 64 == 0 and cin <= 2048 and x.shape[1] == cin and \
        x.numel() * 4 < 2 ** 31 and x.shape[0] * cout * x.shape[2] * x.shape[3] * 4 < 2 ** 31


@torch.library.custom_op(f"{LIB}::conv2d_rms", mutates_args=())
def conv2d_rms(x: Tensor, g: Tensor, weight: Tensor, bias: Optional[Tensor], residual: Optional[Tensor]) -> Tensor:
    """1x1 conv of RMSNorm(x) = F.normalize(x, dim=1) * g * sqrt(C) (the attention blocks' to_qkv,
    diffusion.py:184-186, 211-213), the normalisation formed in the conv's operand gather."""
    _hip.require_device(x)
    x = x.contiguous()
    d, shape = _conv_desc(x, None, weight, 0, 0)
    L = _hip.lib()
    nws = int(L.rdq_conv2d_ws_bytes(ctypes.byref(d)))
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws else None
    tk = _tickets(x.device, int(L.rdq_conv2d_tickets(ctypes.byref(d)))) if nws else None
    y = torch.empty(shape, device=x.device, dtype=torch.float32)
    res = residual.contiguous() if residual is not None else None
    _hip.check(L.rdq_conv2d_rms(ctypes.byref(d), _hip.ptr(x), _hip.ptr(g.contiguous()), _hip.ptr(weight.contiguous()),
                                _hip.ptr(bias), _hip.ptr(res), _hip.ptr(y), _hip.ptr(ws), nws, tk,
                                _hip.stream_of(x)), "rdq_conv2d_rms")
    return y


@conv2d_rms.register_fake
def _(x, g, weight, bias, residual):
    _, shape = _conv_desc(x, None, weight, 0, 0)
    return x.new_empty(shape)


def conv_gn_fusable(x, x2, weight, pad, mode, groups):
    """rdq_conv2d_gn_silu applies to this conv + GroupNorm (fp32 channel-chunk conv, H*W >= 32,
    C / G in {8, 16, 32, 64})."""
    d, _ = _conv_desc(x, x2, weight, pad, mode)
    return int(_hip.lib().rdq_conv2d_gn_ws_bytes(ctypes.byref(d), int(groups))) > 0


@torch.library.custom_op(f"{LIB}::conv2d_gn_silu", mutates_args=())
def conv2d_gn_silu(x: Tensor, x2: Optional[Tensor], weight: Tensor, bias: Optional[Tensor], pad: int, mode: int,
                   gamma: Tensor, beta: Tensor, scale_shift: Optional[Tensor], groups: int, eps: float,
                   post: Optional[Tensor]) -> Tensor:
    """Block.forward (diffusion.py:142-149): SiLU(GroupNorm(conv(x')) * (scale + 1) + shift) [+ post],
    the GroupNorm statistics accumulated by the conv's epilogue (two launches)."""
    _hip.require_device(x)
    x = x.contiguous()
    x2 = x2.contiguous() if x2 is not None else None
    d, shape = _conv_desc(x, x2, weight, pad, mode)
    L = _hip.lib()
    nws = int(L.rdq_conv2d_gn_ws_bytes(ctypes.byref(d), int(groups)))
    if nws == 0:
        raise ValueError("conv2d_gn_silu: shape not supported by the fused form (see conv_gn_fusable)")
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    tk = _tickets(x.device, int(L.rdq_conv2d_tickets(ctypes.byref(d))))
    y = torch.empty(shape, device=x.device, dtype=torch.float32)
    ss = scale_shift.contiguous() if scale_shift is not None else None
    pr = post.contiguous() if post is not None else None
    _hip.check(L.rdq_conv2d_gn_silu(ctypes.byref(d), _hip.ptr(x), _hip.ptr(x2), _hip.ptr(weight.contiguous()),
                                    _hip.ptr(bias), int(groups), float(eps), _hip.ptr(gamma), _hip.ptr(beta),
                                    _hip.ptr(ss), _hip.ptr(pr), _hip.ptr(y), _hip.ptr(ws), nws, tk,
                                    _hip.stream_of(x)), "rdq_conv2d_gn_silu")
    return y


@conv2d_gn_silu.register_fake
def _(x, x2, weight, bias, pad, mode, gamma, beta, scale_shift, groups, eps, post):
    _, shape = _conv_desc(x, x2, weight, pad, mode)
    return x.new_empty(shape)


def conv_gn_bf16_fusable(x, x2, weight, pad, mode, groups):
    """rdq_conv2d_bf16_gn_silu applies (the bf16 halo-staged conv, H*W >= 256, C / G in {8, 16, 32, 64})."""
    d, _ = _conv_desc(x, x2, weight, pad, mode)
    return bf16_eligible(weight) and int(_hip.lib().rdq_conv2d_bf16_gn_ws_bytes(ctypes.byref(d), int(groups))) > 0


@torch.library.custom_op(f"{LIB}::conv2d_bf16_gn_silu", mutates_args=())
def conv2d_bf16_gn_silu(x: Tensor, x2: Optional[Tensor], weight: Tensor, bias: Optional[Tensor], pad: int, mode: int,
                        gamma: Tensor, beta: Tensor, scale_shift: Optional[Tensor], groups: int, eps: float,
                        post: Optional[Tensor]) -> Tensor:
    """conv2d_gn_silu with bf16 conv operands (fp32 accumulation): the configs[4] batched U-Net's Block, the
    GroupNorm statistics reduced in the halo-staged conv's epilogue (two launches)."""
    _hip.require_device(x)
    x = x.contiguous()
    x2 = x2.contiguous() if x2 is not None else None
    d, shape = _conv_desc(x, x2, weight, pad, mode)
    L = _hip.lib()
    nws = int(L.rdq_conv2d_bf16_gn_ws_bytes(ctypes.byref(d), int(groups)))
    if nws == 0 or not bf16_eligible(weight):
        raise ValueError("conv2d_bf16_gn_silu: shape not supported by the fused form (see conv_gn_bf16_fusable)")
    st = _hip.stream_of(x)
    wp = _bf16_pack(weight, d, st)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    y = torch.empty(shape, device=x.device, dtype=torch.float32)
    ss = scale_shift.contiguous() if scale_shift is not None else None
    pr = post.contiguous() if post is not None else None
    _hip.check(L.rdq_conv2d_bf16_gn_silu(ctypes.byref(d), _hip.ptr(x), _hip.ptr(x2), _hip.ptr(wp), _hip.ptr(bias),
                                         int(groups), float(eps), _hip.ptr(gamma), _hip.ptr(beta), _hip.ptr(ss),
                                         _hip.ptr(pr), _hip.ptr(y), _hip.ptr(ws), nws, st), "rdq_conv2d_bf16_gn_silu")
    return y


@conv2d_bf16_gn_silu.register_fake
def _(x, x2, weight, bias, pad, mode, gamma, beta, scale_shift, groups, eps, post):
    _, shape = _conv_desc(x, x2, weight, pad, mode)
    return x.new_empty(shape)


@torch.library.custom_op(f"{LIB}::conv2d_bf16_block_pair", mutates_args=())
def conv2d_bf16_block_pair(x: Tensor, x2: Optional[Tensor], w1: Tensor, b1: Optional[Tensor], gamma1: Tensor, beta1: Tensor,
                           scale_shift: Optional[Tensor], eps1: float, w2: Tensor, b2: Optional[Tensor], gamma2: Tensor,
                           beta2: Tensor, eps2: float, groups: int, post: Optional[Tensor]) -> Tensor:
    """ResnetBlock's block2(block1(cat(x, x2), scale_shift)) [+ post] on the bf16 halo-staged conv
    (diffusion.py:160-168): block1's normalised output is written as bf16 channel octets, the rounding
    block2's conv applies to its operands anyway (rdq_conv2d_bf16_gn_silu8 / _x8): bit-identical to two
    conv2d_bf16_gn_silu calls, half the bytes between them."""
    _hip.require_device(x)
    x = x.contiguous()
    x2 = x2.contiguous() if x2 is not None else None
    d1, shape1 = _conv_desc(x, x2, w1, 1, 0)
    d2, shape2 = _conv_desc(torch.empty(shape1, device="meta"), None, w2, 1, 0)
    L = _hip.lib()
    n1 = int(L.rdq_conv2d_bf16_gn_ws_bytes(ctypes.byref(d1), int(groups)))
    n2 = int(L.rdq_conv2d_bf16_gn_ws_bytes(ctypes.byref(d2), int(groups)))
    if n1 == 0 or n2 == 0 or not bf16_eligible(w1) or not bf16_eligible(w2) or shape1[1] % 32:
        raise ValueError("conv2d_bf16_block_pair: shapes not supported (see unet_ops.block_pair)")
    st = _hip.stream_of(x)
    wp1, wp2 = _bf16_pack(w1, d1, st), _bf16_pack(w2, d2, st)
    ws = torch.empty(max(n1, n2), dtype=torch.uint8, device=x.device)
    B, C1, H, W = shape1
    h8 = torch.empty((B, C1 // 8, H, W, 8), device=x.device, dtype=torch.bfloat16)
    y = torch.empty(shape2, device=x.device, dtype=torch.float32)
    ss = scale_shift.contiguous() if scale_shift is not None else None
    pr = post.contiguous() if post is not None else None
    _hip.check(L.rdq_conv2d_bf16_gn_silu8(ctypes.byref(d1), _hip.ptr(x), _hip.ptr(x2), _hip.ptr(wp1), _hip.ptr(b1),
                                          int(groups), float(eps1), _hip.ptr(gamma1), _hip.ptr(beta1), _hip.ptr(ss),
                                          _hip.ptr(h8), _hip.ptr(ws), n1, st), "rdq_conv2d_bf16_gn_silu8")
    _hip.check(L.rdq_conv2d_bf16_gn_silu_x8(ctypes.byref(d2), _hip.ptr(h8), _hip.ptr(wp2), _hip.ptr(b2), int(groups),
                                            float(eps2), _hip.ptr(gamma2), _hip.ptr(beta2), None, _hip.ptr(pr),
                                            _hip.ptr(y), _hip.ptr(ws), n2, st), "rdq_conv2d_bf16_gn_silu_x8")
    return y


@conv2d_bf16_block_pair.register_fake
def _(x, x2, w1, b1, gamma1, beta1, scale_shift, eps1, w2, b2, gamma2, beta2, eps2, groups, post):
    return x.new_empty((x.shape[0], w2.shape[0], x.shape[2], x.shape[3]))


@torch.library.custom_op(f"{LIB}::conv2d_bf16_gn_silu_out", mutates_args=())
def conv2d_bf16_gn_silu_out(x: Tensor, weight: Tensor, bias: Optional[Tensor], pad: int, gamma: Tensor, beta: Tensor,
                            scale_shift: Optional[Tensor], groups: int, eps: float, post: Optional[Tensor],
                            w_out: Tensor, b_out: Optional[Tensor]) -> Tensor:
    """conv2d_gn_silu_out on the bf16 halo-staged conv (the configs[4] batched U-Net's tail)."""
    _hip.require_device(x)
    x = x.contiguous()
    d, shape = _conv_desc(x, None, weight, pad, 0)
    L = _hip.lib()
    nws = int(L.rdq_conv2d_bf16_gn_ws_bytes(ctypes.byref(d), int(groups)))
    if nws == 0 or not bf16_eligible(weight):
        raise ValueError("conv2d_bf16_gn_silu_out: shape not supported by the fused form (see conv_gn_bf16_fusable)")
    st = _hip.stream_of(x)
    wp = _bf16_pack(weight, d, st)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    nf = int(w_out.shape[0])
    yf = torch.empty(shape[0], nf, shape[2], shape[3], device=x.device, dtype=torch.float32)
    ss = scale_shift.contiguous() if scale_shift is not None else None
    pr = post.contiguous() if post is not None else None
    _hip.check(L.rdq_conv2d_bf16_gn_silu_out(ctypes.byref(d), _hip.ptr(x), None, _hip.ptr(wp), _hip.ptr(bias),
                                             int(groups), float(eps), _hip.ptr(gamma), _hip.ptr(beta), _hip.ptr(ss),
                                             _hip.ptr(pr), nf, _hip.ptr(w_out.contiguous()), _hip.ptr(b_out),
                                             _hip.ptr(yf), _hip.ptr(ws), nws, st), "rdq_conv2d_bf16_gn_silu_out")
    return yf


@conv2d_bf16_gn_silu_out.register_fake
def _(x, weight, bias, pad, gamma, beta, scale_shift, groups, eps, post, w_out, b_out):
    _, shape = _conv_desc(x, None, weight, pad, 0)
    return x.new_empty(shape[0], w_out.shape[0], shape[2], shape[3])


def conv_gn_sc_fusable(x, x2, weight, weight_s, groups):
    """rdq_conv2d_gn_silu_sc applies: block1's 3x3 conv + GroupNorm (conv_gn_fusable) and a 1x1
    shortcut of the same input in the channel-chunk form (channel counts multiples of 64)."""
    d, _ = _conv_desc(x, x2, weight, 1, 0)
    return weight.shape[-1] == 3 and weight_s.shape[-1] == 1 and \
        int(_hip.lib().rdq_conv2d_gn_sc_ws_bytes(ctypes.byref(d), int(groups), int(weight_s.shape[0]))) > 0


@torch.library.custom_op(f"{LIB}::conv2d_gn_silu_sc", mutates_args=())
def conv2d_gn_silu_sc(x: Tensor, x2: Optional[Tensor], weight: Tensor, bias: Optional[Tensor], gamma: Tensor,
                      beta: Tensor, scale_shift: Optional[Tensor], groups: int, eps: float, weight_s: Tensor,
                      bias_s: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """ResnetBlock with a 1x1 shortcut (diffusion.py:160-168): (block1(cat(x, x2)), res_conv(cat(x, x2)))
    with both convs in one launch, then block1's normalise pass."""
    _hip.require_device(x)
    x = x.contiguous()
    x2 = x2.contiguous() if x2 is not None else None
    d, shape = _conv_desc(x, x2, weight, 1, 0)
    cs = int(weight_s.shape[0])
    L = _hip.lib()
    nws = int(L.rdq_conv2d_gn_sc_ws_bytes(ctypes.byref(d), int(groups), cs))
    if nws == 0:
        raise ValueError("conv2d_gn_silu_sc: shape not supported by the fused form (see conv_gn_sc_fusable)")
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    tk = _tickets(x.device, int(L.rdq_conv2d_gn_sc_tickets(ctypes.byref(d), cs)))
    y = torch.empty(shape, device=x.device, dtype=torch.float32)
    ys = torch.empty(shape[0], cs, shape[2], shape[3], device=x.device, dtype=torch.float32)
    ss = scale_shift.contiguous() if scale_shift is not None else None
    _hip.check(L.rdq_conv2d_gn_silu_sc(ctypes.byref(d), _hip.ptr(x), _hip.ptr(x2), _hip.ptr(weight.contiguous()),
                                       _hip.ptr(bias), int(groups), float(eps), _hip.ptr(gamma), _hip.ptr(beta),
                                       _hip.ptr(ss), _hip.ptr(y), cs, _hip.ptr(weight_s.contiguous()), _hip.ptr(bias_s),
                                       _hip.ptr(ys), _hip.ptr(ws), nws, tk, _hip.stream_of(x)),
               "rdq_conv2d_gn_silu_sc")
    return y, ys


@conv2d_gn_silu_sc.register_fake
def _(x, x2, weight, bias, gamma, beta, scale_shift, groups, eps, weight_s, bias_s):
    _, shape = _conv_desc(x, x2, weight, 1, 0)
    return x.new_empty(shape), x.new_empty(shape[0], weight_s.shape[0], shape[2], shape[3])


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[_hip.ptr(t) for t in ts])


@torch.library.custom_op(f"{LIB}::conv2d_gn_silu_lsm", mutates_args=())
def conv2d_gn_silu_lsm(x: Tensor, weight: Tensor, bias: Optional[Tensor], pad: int, gamma: Tensor, beta: Tensor,
                       groups: int, eps: float, post: Optional[Tensor], temb: Tensor, weights: List[Tensor],
                       biases: List[Tensor], ss_index: int) -> Tuple[Tensor, List[Tensor]]:
    """(conv2d_gn_silu(x, ..., scale_shift = ys[ss_index], post), ys = linear_silu_multi(temb, weights,
    biases)): the first ResnetBlock's block1 with every block's Linear(SiLU(t)) computed as a side job of
    its conv launch (diffusion.py:280-283, 160-165)."""
    _hip.require_device(x)
    x = x.contiguous()
    temb = temb.contiguous()
    d, shape = _conv_desc(x, None, weight, pad, 0)
    L = _hip.lib()
    nws = int(L.rdq_conv2d_gn_ws_bytes(ctypes.byref(d), int(groups)))
    if nws == 0 or len(weights) > 32:
        raise ValueError("conv2d_gn_silu_lsm: shape not supported by the fused form")
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    tk = _tickets(x.device, int(L.rdq_conv2d_tickets(ctypes.byref(d))))
    y = torch.empty(shape, device=x.device, dtype=torch.float32)
    B, fin = temb.shape
    wl = [w.contiguous() for w in weights]
    ys = [torch.empty(B, w.shape[0], device=x.device, dtype=torch.float32) for w in wl]
    O = (ctypes.c_int32 * len(wl))(*[w.shape[0] for w in wl])
    pr = post.contiguous() if post is not None else None
    _hip.check(L.rdq_conv2d_gn_silu_lsm(ctypes.byref(d), _hip.ptr(x), None, _hip.ptr(weight.contiguous()),
                                        _hip.ptr(bias), int(groups), float(eps), _hip.ptr(gamma), _hip.ptr(beta),
                                        _hip.ptr(pr), _hip.ptr(y), _hip.ptr(ws), nws, tk, fin, _hip.ptr(temb), len(wl),
                                        _ptr_array(wl), _ptr_array(biases), O, _ptr_array(ys), int(ss_index),
                                        _hip.stream_of(x)), "rdq_conv2d_gn_silu_lsm")
    return y, ys


@conv2d_gn_silu_lsm.register_fake
def _(x, weight, bias, pad, gamma, beta, groups, eps, post, temb, weights, biases, ss_index):
    _, shape = _conv_desc(x, None, weight, pad, 0)
    return x.new_empty(shape), [temb.new_empty(temb.shape[0], w.shape[0]) for w in weights]


@torch.library.custom_op(f"{LIB}::conv2d_gn_silu_out", mutates_args=())
def conv2d_gn_silu_out(x: Tensor, weight: Tensor, bias: Optional[Tensor], pad: int, gamma: Tensor, beta: Tensor,
                       scale_shift: Optional[Tensor], groups: int, eps: float, post: Optional[Tensor],
                       w_out: Tensor, b_out: Optional[Tensor]) -> Tensor:
    """conv1x1(conv2d_gn_silu(x, ..., post), w_out) + b_out: final_res_block's block2 and final_conv
    (diffusion.py:299-301), the block output never written (w_out: (nf <= 4, cout, 1, 1))."""
    _hip.require_device(x)
    x = x.contiguous()
    d, shape = _conv_desc(x, None, weight, pad, 0)
    L = _hip.lib()
    nws = int(L.rdq_conv2d_gn_ws_bytes(ctypes.byref(d), int(groups)))
    if nws == 0:
        raise ValueError("conv2d_gn_silu_out: shape not supported by the fused form")
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    tk = _tickets(x.device, int(L.rdq_conv2d_tickets(ctypes.byref(d))))
    nf = int(w_out.shape[0])
    yf = torch.empty(shape[0], nf, shape[2], shape[3], device=x.device, dtype=torch.float32)
    ss = scale_shift.contiguous() if scale_shift is not None else None
    pr = post.contiguous() if post is not None else None
    _hip.check(L.rdq_conv2d_gn_silu_out(ctypes.byref(d), _hip.ptr(x), None, _hip.ptr(weight.contiguous()),
                                        _hip.ptr(bias), int(groups), float(eps), _hip.ptr(gamma), _hip.ptr(beta),
                                        _hip.ptr(ss), _hip.ptr(pr), nf, _hip.ptr(w_out.contiguous()), _hip.ptr(b_out),
                                        _hip.ptr(yf), _hip.ptr(ws), nws, tk, _hip.stream_of(x)),
               "rdq_conv2d_gn_silu_out")
    return yf


@conv2d_gn_silu_out.register_fake
def _(x, weight, bias, pad, gamma, beta, scale_shift, groups, eps, post, w_out, b_out):
    _, shape = _conv_desc(x, None, weight, pad, 0)
    return x.new_empty(shape[0], w_out.shape[0], shape[2], shape[3])


def unet_head_fusable(x, weight, time_mlp):
    """rdq_unet_head applies: init_conv outside the channel-chunk form (7x7 / 3x3, cout <= 64, no K split), B <= 16
    (beyond, the time MLP's batched kernel reads its weights once per sample block instead)."""
    cout, cin, kh, kw = weight.shape
    dim, hid = time_mlp[1].weight.shape[1], time_mlp[1].weight.shape[0]
    return x.shape[0] <= 16 and kh == kw and kh in (3, 7) and cout <= 64 and cin * kh * kw <= 224 and \
        x.shape[1] == cin and \
        (kh == 7 or cin % 8 != 0) and dim + hid <= 7680


@torch.library.custom_op(f"{LIB}::unet_head", mutates_args=())
def unet_head(x: Tensor, weight: Tensor, bias: Optional[Tensor], pad: int, t: Tensor, dim: int, theta: float,
              w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor) -> Tuple[Tensor, Tensor]:
    """(init_conv(x), time_mlp(t)) in one launch (diffusion.py:276-279)."""
    _hip.require_device(x)
    x = x.contiguous()
    t = t.to(torch.int64).contiguous()
    d, shape = _conv_desc(x, None, weight, pad, 0)
    y = torch.empty(shape, device=x.device, dtype=torch.float32)
    hid, out = w1.shape[0], w2.shape[0]
    temb = torch.empty(t.shape[0], out, device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().rdq_unet_head(ctypes.byref(d), _hip.ptr(x), _hip.ptr(weight.contiguous()), _hip.ptr(bias),
                                        _hip.ptr(y), dim, float(theta), _hip.ptr(t), _hip.ptr(w1.contiguous()),
                                        _hip.ptr(b1), hid, _hip.ptr(w2.contiguous()), _hip.ptr(b2), out,
                                        _hip.ptr(temb), _hip.stream_of(x)), "rdq_unet_head")
    return y, temb


@unet_head.register_fake
def _(x, weight, bias, pad, t, dim, theta, w1, b1, w2, b2):
    _, shape = _conv_desc(x, None, weight, pad, 0)
    return x.new_empty(shape), x.new_empty(t.shape[0], w2.shape[0])


@torch.library.custom_op(f"{LIB}::rmsnorm", mutates_args=())
def rmsnorm(x: Tensor, g: Tensor, residual: Optional[Tensor]) -> Tensor:
    """F.normalize(x, dim=1) * g * sqrt(C) [+ residual]."""
    _hip.require_device(x)
    x = x.contiguous()
    B, C, H, W = x.shape
    y = torch.empty_like(x)
    res = residual.contiguous() if residual is not None else None
    _hip.check(_hip.lib().rdq_rmsnorm(B, C, H * W, _hip.ptr(x), _hip.ptr(g), _hip.ptr(res), _hip.ptr(y),
                                      _hip.stream_of(x)), "rdq_rmsnorm")
    return y


@rmsnorm.register_fake
def _(x, g, residual):
    return torch.empty_like(x)


@torch.library.custom_op(f"{LIB}::linear", mutates_args=())
def linear(x: Tensor, weight: Tensor, bias: Tensor, act_in: int, act_out: int) -> Tensor:
    """act_out(Linear(act_in(x))); act 1 = SiLU on the input / GELU(erf) on the output."""
    _hip.require_device(x)
    x = x.contiguous()
    B, fin = x.shape
    fout = weight.shape[0]
    y = torch.empty(B, fout, device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().rdq_linear(B, fin, fout, _hip.ptr(x), _hip.ptr(weight), _hip.ptr(bias), act_in, act_out,
                                     _hip.ptr(y), _hip.stream_of(x)), "rdq_linear")
    return y


@linear.register_fake
def _(x, weight, bias, act_in, act_out):
    return x.new_empty(x.shape[0], weight.shape[0])


@torch.library.custom_op(f"{LIB}::time_mlp", mutates_args=())
def time_mlp(t: Tensor, dim: int, theta: float, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor) -> Tensor:
    """Unet.time_mlp (diffusion.py:255-258): Linear(GELU(Linear(SinusoidalPosEmb(t)))), one launch."""
    _hip.require_device(t)
    t = t.to(torch.int64).contiguous()
    hid, out = w1.shape[0], w2.shape[0]
    y = torch.empty(t.shape[0], out, device=t.device, dtype=torch.float32)
    _hip.check(_hip.lib().rdq_time_mlp(t.shape[0], dim, float(theta), _hip.ptr(t), _hip.ptr(w1.contiguous()),
                                       _hip.ptr(b1), hid, _hip.ptr(w2.contiguous()), _hip.ptr(b2), out, _hip.ptr(y),
                                       _hip.stream_of(t)), "rdq_time_mlp")
    return y


@time_mlp.register_fake
def _(t, dim, theta, w1, b1, w2, b2):
    return t.new_empty(t.shape[0], w2.shape[0], dtype=torch.float32)


@torch.library.custom_op(f"{LIB}::linear_silu_multi", mutates_args=())
def linear_silu_multi(x: Tensor, weights: List[Tensor], biases: List[Tensor]) -> List[Tensor]:
    """[Linear_j(SiLU(x)) for j]: every ResnetBlock's time MLP (diffusion.py:157-165), one launch
    (at most 32 linears sharing x)."""
    _hip.require_device(x)
    x = x.contiguous()
    n = len(weights)
    B, fin = x.shape
    ys = [torch.empty(B, w.shape[0], device=x.device, dtype=torch.float32) for w in weights]
    ws = [w.contiguous() for w in weights]
    W = (ctypes.c_void_p * n)(*[_hip.ptr(w) for w in ws])
    Bs = (ctypes.c_void_p * n)(*[_hip.ptr(b) for b in biases])
    O = (ctypes.c_int32 * n)(*[w.shape[0] for w in ws])
    Y = (ctypes.c_void_p * n)(*[_hip.ptr(y) for y in ys])
    _hip.check(_hip.lib().rdq_linear_silu_multi(B, fin, _hip.ptr(x), n, W, Bs, O, Y, _hip.stream_of(x)),
               "rdq_linear_silu_multi")
    return ys


@linear_silu_multi.register_fake
def _(x, weights, biases):
    return [x.new_empty(x.shape[0], w.shape[0]) for w in weights]


@torch.library.custom_op(f"{LIB}::sinusoidal_emb", mutates_args=())
def sinusoidal_emb(t: Tensor, dim: int, theta: float) -> Tensor:
    _hip.require_device(t)
    t = t.to(torch.int64).contiguous()
    y = torch.empty(t.shape[0], dim, device=t.device, dtype=torch.float32)
    _hip.check(_hip.lib().rdq_sinusoidal_emb(t.shape[0], dim, float(theta), _hip.ptr(t), _hip.ptr(y),
                                             _hip.stream_of(t)), "rdq_sinusoidal_emb")
    return y


@sinusoidal_emb.register_fake
def _(t, dim, theta):
    return t.new_empty(t.shape[0], dim, dtype=torch.float32)


@torch.library.custom_op(f"{LIB}::linear_attn", mutates_args=())
def linear_attn(qkv: Tensor, mem_kv: Tensor, heads: int, scale: float) -> Tensor:
    """LinearAttention core (diffusion.py:182-195): softmax(q) over d, softmax(k) over n with the
    memory key/values, context, out = context^T q; qkv (B, 3*heads*dh, H, W) -> (B, heads*dh, H, W)."""
    _hip.require_device(qkv)
    qkv = qkv.contiguous()
    B, C3, H, W = qkv.shape
    dh = C3 // (3 * heads)
    L = _hip.lib()
    ws = torch.empty(int(L.rdq_linear_attention_ws_bytes(B, heads, dh, H * W, mem_kv.shape[-1])), dtype=torch.uint8,
                     device=qkv.device)
    out = torch.empty(B, heads * dh, H, W, device=qkv.device, dtype=torch.float32)
    _hip.check(L.rdq_linear_attention(B, heads, dh, H * W, mem_kv.shape[-1], float(scale), _hip.ptr(qkv),
                                      _hip.ptr(mem_kv.contiguous()), _hip.ptr(out), _hip.ptr(ws), _hip.stream_of(qkv)),
               "rdq_linear_attention")
    return out


@linear_attn.register_fake
def _(qkv, mem_kv, heads, scale):
    B, C3, H, W = qkv.shape
    return qkv.new_empty(B, C3 // 3, H, W)


def linear_attn_block_fusable(qkv_channels, heads, dim):
    return heads == 4 and qkv_channels == 3 * heads * 32 and dim in (64, 128, 256)


@torch.library.custom_op(f"{LIB}::linear_attn_block", mutates_args=())
def linear_attn_block(qkv: Tensor, mem_kv: Tensor, heads: int, scale: float, w_out: Tensor,
                      b_out: Optional[Tensor], g_out: Tensor, residual: Optional[Tensor]) -> Tensor:
    """LinearAttention.forward(x) + x from qkv = to_qkv(RMSNorm(x)) (diffusion.py:182-195, residual
    286/297): context, softmax(q) x context, to_out = Conv2d(hidden, dim, 1) + RMSNorm(dim) and the
    residual, the last four in one launch (rdq_linear_attention_block).  dh = 32, dim 64/128/256."""
    _hip.require_device(qkv)
    qkv = qkv.contiguous()
    B, C3, H, W = qkv.shape
    dh = C3 // (3 * heads)
    dim = w_out.shape[0]
    L = _hip.lib()
    ws = torch.empty(int(L.rdq_linear_attention_ws_bytes(B, heads, dh, H * W, mem_kv.shape[-1])), dtype=torch.uint8,
                     device=qkv.device)
    y = torch.empty(B, dim, H, W, device=qkv.device, dtype=torch.float32)
    res = residual.contiguous() if residual is not None else None
    _hip.check(L.rdq_linear_attention_block(B, heads, dh, H * W, mem_kv.shape[-1], float(scale), _hip.ptr(qkv),
                                            _hip.ptr(mem_kv.contiguous()), dim, _hip.ptr(w_out.contiguous()),
                                            _hip.ptr(b_out) if b_out is not None else None,
                                            _hip.ptr(g_out.contiguous()), _hip.ptr(res) if res is not None else None,
                                            _hip.ptr(y), _hip.ptr(ws), _hip.stream_of(qkv)),
               "rdq_linear_attention_block")
    return y


@linear_attn_block.register_fake
def _(qkv, mem_kv, heads, scale, w_out, b_out, g_out, residual):
    B, C3, H, W = qkv.shape
    return qkv.new_empty(B, w_out.shape[0], H, W)


def linear_attn_bf16_fusable(x, w_qkv, w_out, heads):
    """rdq_linear_attention_bf16 applies: 4 heads of 32, dim 64 / 128 (the U-Net's 72 / 36 / 18 levels), 1x1 projections."""
    return (heads == 4 and x.dim() == 4 and x.shape[1] in (64, 128) and tuple(w_qkv.shape) == (384, x.shape[1], 1, 1)
            and tuple(w_out.shape) == (x.shape[1], 128, 1, 1))


@torch.library.custom_op(f"{LIB}::linear_attn_bf16", mutates_args=())
def linear_attn_bf16(x: Tensor, g_in: Tensor, w_qkv: Tensor, mem_kv: Tensor, w_out: Tensor, b_out: Optional[Tensor],
                     g_out: Tensor, heads: int, scale: float) -> Tensor:
    """LinearAttention.forward(x) + x (diffusion.py:182-195, residual 286/297) with bf16 operands and fp32
    accumulation, two launches (rdq_linear_attention_bf16): the configs[4] batched U-Net."""
    _hip.require_device(x)
    if not linear_attn_bf16_fusable(x, w_qkv, w_out, heads):
        raise ValueError("linear_attn_bf16: shape not supported (see linear_attn_bf16_fusable)")
    x = x.contiguous()
    B, D, H, W = x.shape
    L = _hip.lib()
    st = _hip.stream_of(x)
    dq, _ = _conv_desc(x, None, w_qkv, 0, 0)
    h = torch.empty(B, 128, H, W, device="meta")
    do, _ = _conv_desc(h, None, w_out, 0, 0)
    wq = _bf16_pack(w_qkv, dq, st)
    wo = _bf16_pack(w_out, do, st)
    nws = int(L.rdq_linear_attention_bf16_ws_bytes(B, D, H * W))
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    y = torch.empty_like(x)
    _hip.check(L.rdq_linear_attention_bf16(B, D, H * W, mem_kv.shape[-1], float(scale), _hip.ptr(x),
                                           _hip.ptr(g_in.contiguous()), _hip.ptr(wq), _hip.ptr(mem_kv.contiguous()),
                                           _hip.ptr(wo), _hip.ptr(b_out) if b_out is not None else None,
                                           _hip.ptr(g_out.contiguous()), _hip.ptr(y), _hip.ptr(ws), nws, st),
               "rdq_linear_attention_bf16")
    return y


@linear_attn_bf16.register_fake
def _(x, g_in, w_qkv, mem_kv, w_out, b_out, g_out, heads, scale):
    return torch.empty_like(x)


@torch.library.custom_op(f"{LIB}::linear_attn_f32", mutates_args=())
def linear_attn_f32(x: Tensor, g_in: Tensor, w_qkv: Tensor, mem_kv: Tensor, w_out: Tensor, b_out: Optional[Tensor],
                    g_out: Tensor, heads: int, scale: float) -> Tensor:
    """LinearAttention.forward(x) + x (diffusion.py:182-195, residual 286/297) in fp32, two launches
    (rdq_linear_attention_f32: qkv and the hidden tensor never written)."""
    _hip.require_device(x)
    if not linear_attn_bf16_fusable(x, w_qkv, w_out, heads):
        raise ValueError("linear_attn_f32: shape not supported (see linear_attn_bf16_fusable)")
    x = x.contiguous()
    B, D, H, W = x.shape
    L = _hip.lib()
    nws = int(L.rdq_linear_attention_f32_ws_bytes(B, D, H * W))
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    y = torch.empty_like(x)
    _hip.check(L.rdq_linear_attention_f32(B, D, H * W, mem_kv.shape[-1], float(scale), _hip.ptr(x),
                                          _hip.ptr(g_in.contiguous()), _hip.ptr(w_qkv.contiguous()),
                                          _hip.ptr(mem_kv.contiguous()), _hip.ptr(w_out.contiguous()),
                                          _hip.ptr(b_out) if b_out is not None else None, _hip.ptr(g_out.contiguous()),
                                          _hip.ptr(y), _hip.ptr(ws), nws, _hip.stream_of(x)), "rdq_linear_attention_f32")
    return y


@linear_attn_f32.register_fake
def _(x, g_in, w_qkv, mem_kv, w_out, b_out, g_out, heads, scale):
    return torch.empty_like(x)


@torch.library.custom_op(f"{LIB}::attn", mutates_args=())
def attn(qkv: Tensor, mem_kv: Tensor, heads: int) -> Tensor:
    """Attention core with Attend(flash=False) (diffusion.py:209-218): softmax(q k^T d^-1/2) v over
    the memory + image keys; qkv (B, 3*heads*dh, H, W) -> (B, heads*dh, H, W)."""
    _hip.require_device(qkv)
    qkv = qkv.contiguous()
    B, C3, H, W = qkv.shape
    dh = C3 // (3 * heads)
    out = torch.empty(B, heads * dh, H, W, device=qkv.device, dtype=torch.float32)
    _hip.check(_hip.lib().rdq_full_attention(B, heads, dh, H * W, mem_kv.shape[-2], _hip.ptr(qkv),
                                             _hip.ptr(mem_kv.contiguous()), _hip.ptr(out), _hip.stream_of(qkv)),
               "rdq_full_attention")
    return out


@attn.register_fake
def _(qkv, mem_kv, heads):
    B, C3, H, W = qkv.shape
    return qkv.new_empty(B, C3 // 3, H, W)


@torch.library.custom_op(f"{LIB}::red_q_sample", mutates_args=())
def red_q_sample(x0: Tensor, t: Tensor, eps: Tensor, sqrt_ac: Tensor, sqrt_1mac: Tensor) -> Tensor:
    """q_sample (diffusion.py:516-519) on the fp32 schedule buffers."""
    _hip.require_device(x0)
    x0, eps = x0.contiguous(), eps.contiguous()
    xt = torch.empty_like(x0)
    _hip.check(_hip.lib().rdq_red_q_sample(x0.shape[0], x0[0].numel(), _hip.ptr(sqrt_ac), _hip.ptr(sqrt_1mac),
                                           _hip.ptr(t), _hip.ptr(x0), _hip.ptr(eps), _hip.ptr(xt),
                                           _hip.stream_of(x0)), "rdq_red_q_sample")
    return xt


@torch.library.custom_op(f"{LIB}::red_q_sample_into", mutates_args=("xt", "t_out"))
def red_q_sample_into(x0: Tensor, t: Tensor, eps: Tensor, sqrt_ac: Tensor, sqrt_1mac: Tensor, xt: Tensor,
                      t_out: Tensor) -> None:
    """red_q_sample written into xt (contiguous, x0's shape), t copied into t_out (int64 [B]) by the same
    launch: the static inputs of a captured U-Net forward (Unet.graph_io)."""
    _hip.require_device(x0)
    x0, eps = x0.contiguous(), eps.contiguous()
    if xt.shape != x0.shape or not xt.is_contiguous() or t_out.dtype != torch.int64 or t_out.numel() != x0.shape[0]:
        raise ValueError("red_q_sample_into: xt / t_out do not match x0")
    _hip.check(_hip.lib().rdq_red_q_sample_t(x0.shape[0], x0[0].numel(), _hip.ptr(sqrt_ac), _hip.ptr(sqrt_1mac),
                                             _hip.ptr(t.to(torch.int64).contiguous()), _hip.ptr(x0), _hip.ptr(eps),
                                             _hip.ptr(xt), _hip.ptr(t_out), _hip.stream_of(x0)), "rdq_red_q_sample_t")


@red_q_sample_into.register_fake
def _(x0, t, eps, sqrt_ac, sqrt_1mac, xt, t_out):
    return None


@red_q_sample.register_fake
def _(x0, t, eps, sqrt_ac, sqrt_1mac):
    return torch.empty_like(x0)


@torch.library.custom_op(f"{LIB}::red_eps", mutates_args=())
def red_eps(xt: Tensor, t: Tensor, eps_hat: Tensor, eps: Tensor, sqrt_recip_ac: Tensor,
            sqrt_recipm1_ac: Tensor) -> Tensor:
    """RED residual (eps' - eps): eps' re-derived from the clipped x0 (diffusion.py:393-419)."""
    _hip.require_device(xt)
    xt, eps_hat, eps = xt.contiguous(), eps_hat.contiguous(), eps.contiguous()
    g = torch.empty_like(xt)
    _hip.check(_hip.lib().rdq_red_epilogue(xt.shape[0], xt[0].numel(), _hip.ptr(sqrt_recip_ac),
                                           _hip.ptr(sqrt_recipm1_ac), _hip.ptr(t), _hip.ptr(xt), _hip.ptr(eps_hat),
                                           _hip.ptr(eps), _hip.ptr(g), _hip.stream_of(xt)), "rdq_red_epilogue")
    return g


@red_eps.register_fake
def _(xt, t, eps_hat, eps, sqrt_recip_ac, sqrt_recipm1_ac):
    return torch.empty_like(xt)


SAMPLE_OBJECTIVES = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}       # RDQ_OBJ_*
SAMPLE_ANCESTRAL, SAMPLE_DDIM, SAMPLE_DDIM_LAST = 0, 1, 2              # RDQ_STEP_*


@torch.library.custom_op(f"{LIB}::sample_step", mutates_args=("x_next", "x_start_out", "t_out"))
def sample_step(x_t: Tensor, t: Tensor, out: Tensor, noise: Optional[Tensor], tables: List[Tensor], objective: int,
                step: int, a_next: float, c: float, sigma: float, t_next: int, x_next: Tensor,
                x_start_out: Optional[Tensor], t_out: Optional[Tensor]) -> None:
    """One reverse step of p_sample / ddim_sample (diffusion.py:411-446, 469-494; include/red_diffeq_sampling.h)
    written into x_next (contiguous, x_t's shape; may be x_t itself).  t int64 [B]; tables = the seven fp32
    schedule buffers (sqrt_recip_ac, sqrt_recipm1_ac, sqrt_ac, sqrt_1mac, posterior_mean_coef1, posterior_mean_coef2,
    posterior_log_variance_clipped), all of one length; step = SAMPLE_ANCESTRAL / _DDIM / _DDIM_LAST.  noise None: the ancestral t = 0 step, or DDIM with
    sigma == 0.  x_start_out (x_t's shape) receives the clamped x0, t_out (int64 [B]) t_next when t_next >= 0."""
    _hip.require_device(x_t, t, out, noise, x_next, x_start_out, t_out, *tables)
    B = x_t.shape[0]
    if x_t.dtype != torch.float32 or not x_t.is_contiguous() or x_t.dim() < 1 or x_t.numel() == 0:
        raise ValueError("sample_step: x_t must be a contiguous, non-empty fp32 tensor")
    for name, v in (("out", out), ("noise", noise), ("x_next", x_next), ("x_start_out", x_start_out)):
        if v is not None and (v.shape != x_t.shape or v.dtype != torch.float32 or not v.is_contiguous()):
            raise ValueError(f"sample_step: {name} does not match x_t (shape, fp32, contiguous)")
    for name, v in (("t", t), ("t_out", t_out)):
        if v is not None and (v.dtype != torch.int64 or v.shape != (B,) or not v.is_contiguous()):
            raise ValueError(f"sample_step: {name} must be a contiguous int64 [B]")
    if t_out is not None and t_out.data_ptr() == t.data_ptr():
        raise ValueError("sample_step: t_out must not be t")
    if len(tables) != 7 or any(v.dtype != torch.float32 or v.dim() != 1 or v.shape != tables[0].shape
                               or not v.is_contiguous() for v in tables):
        raise ValueError("sample_step: tables must be seven contiguous fp32 vectors of one length")
    T = tables[0].shape[0]
    if objective not in (0, 1, 2) or step not in (0, 1, 2) or T < 1 or t_next >= T:
        raise ValueError("sample_step: bad objective / step / t_next")
    if step == SAMPLE_DDIM and noise is None and sigma != 0.0:
        raise ValueError("sample_step: DDIM with sigma != 0 needs noise")
    tab = _hip.SampleTables(*(t_.data_ptr() for t_ in tables))
    _hip.check(_hip.lib().rdq_sample_step(B, x_t[0].numel(), objective, step, T, tab, _hip.ptr(t), _hip.ptr(x_t),
                                          _hip.ptr(out), _hip.ptr(noise), a_next, c, sigma, t_next, _hip.ptr(x_next),
                                          _hip.ptr(x_start_out), _hip.ptr(t_out), _hip.stream_of(x_t)),
               "rdq_sample_step")


@sample_step.register_fake
def _(x_t, t, out, noise, tables, objective, step, a_next, c, sigma, t_next, x_next, x_start_out, t_out):
    return None


# ----------------------------------------------------------------------------------------- loop
@torch.library.custom_op(f"{LIB}::l1_misfit", mutates_args=())
def l1_misfit(pred: Tensor, y: Tensor, mask: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """K5: per-model sum(|y - pred| * mask) / max(#observed, 1) (losses.py:14-41) -> (loss, nobs)."""
    _hip.require_device(pred, y, mask)
    pred, y = pred.float().contiguous(), y.float().contiguous()
    mask = mask.float().contiguous() if mask is not None else None
    B = pred.shape[0]
    n = pred.numel() // B
    L = _hip.lib()
    loss = torch.empty(B, dtype=torch.float32, device=pred.device)
    nobs = torch.empty(B, dtype=torch.float32, device=pred.device)
    part = torch.empty(int(L.rdq_l1_partial_bytes(B, n)), dtype=torch.uint8, device=pred.device)
    _hip.check(L.rdq_l1_forward(B, n, _hip.ptr(pred), _hip.ptr(y), _hip.ptr(mask), _hip.ptr(loss), _hip.ptr(nobs),
                                _hip.ptr(part), _hip.stream_of(pred)), "rdq_l1_forward")
    return loss, nobs


@l1_misfit.register_fake
def _(pred, y, mask):
    return pred.new_empty(pred.shape[0]), pred.new_empty(pred.shape[0])


@torch.library.custom_op(f"{LIB}::l1_misfit_backward", mutates_args=())
def l1_misfit_backward(pred: Tensor, y: Tensor, mask: Optional[Tensor], nobs: Tensor, gout: Tensor) -> Tensor:
    """dL/dpred = sign(pred - y) * mask * gout / nobs (the autograd of losses.py:27-39)."""
    _hip.require_device(pred, y)
    pred, y = pred.float().contiguous(), y.float().contiguous()
    mask = mask.float().contiguous() if mask is not None else None
    B = pred.shape[0]
    dpred = torch.empty_like(pred)
    # named, so that the copy of an expanded (stride-0) gout lives until the launch is enqueued
    nobs, gout = nobs.float().contiguous(), gout.float().contiguous()
    _hip.check(_hip.lib().rdq_l1_backward(B, pred.numel() // B, _hip.ptr(pred), _hip.ptr(y), _hip.ptr(mask),
                                          _hip.ptr(nobs), _hip.ptr(gout),
                                          _hip.ptr(dpred), _hip.stream_of(pred)), "rdq_l1_backward")
    return dpred


@l1_misfit_backward.register_fake
def _(pred, y, mask, nobs, gout):
    return torch.empty_like(pred, dtype=torch.float32)


MISFIT_KINDS = {"l2": 1, "huber": 2, "ncc": 3}                           # RDQ_MISFIT_*


def _misfit_dims(pred: Tensor, kind: int):
    """(B, ns, nt, ng) of a misfit call: the record's own for NCC (4-D), and for the elementwise kinds any
    [B, ...] shape as one row of n elements per model."""
    if kind not in MISFIT_KINDS.values():
        raise ValueError(f"misfit: unknown kind {kind}")
    if pred.dim() < 2 or pred.numel() == 0:
        raise ValueError("misfit: pred must be a non-empty [B, ...] tensor")
    if kind == MISFIT_KINDS["ncc"]:
        if pred.dim() != 4:
            raise ValueError("misfit: the ncc misfit needs a (B, ns, nt, ng) record")
        return tuple(pred.shape)
    return pred.shape[0], 1, 1, pred.numel() // pred.shape[0]


@torch.library.custom_op(f"{LIB}::misfit", mutates_args=())
def misfit(pred: Tensor, y: Tensor, mask: Optional[Tensor], kind: int, delta: float) -> Tuple[Tensor, Tensor, Tensor]:
    """K13 forward (include/red_diffeq_misfit.h): kind 1 L2, 2 Huber (delta), 3 NCC -> (loss, norm, coef);
    norm is nobs (L2, Huber) or the live-trace count (NCC), coef the NCC's (inv, r, J) per trace, float64
    (B, ns, ng, 3) (empty for the other kinds)."""
    _hip.require_device(pred, y, mask)
    B, ns, nt, ng = _misfit_dims(pred, kind)
    if y.shape != pred.shape or (mask is not None and mask.shape != pred.shape):
        raise ValueError("misfit: y and mask must have pred's shape")
    pred, y = pred.float().contiguous(), y.float().contiguous()
    mask = mask.float().contiguous() if mask is not None else None
    L = _hip.lib()
    loss = torch.empty(B, dtype=torch.float32, device=pred.device)
    norm = torch.empty(B, dtype=torch.float32, device=pred.device)
    coef = torch.empty((B, ns, ng, 3) if kind == MISFIT_KINDS["ncc"] else (0,), dtype=torch.float64, device=pred.device)
    ws = torch.empty(int(L.rdq_misfit_workspace_bytes(kind, B, ns, nt, ng)), dtype=torch.uint8, device=pred.device)
    _hip.check(L.rdq_misfit_forward(kind, B, ns, nt, ng, delta, _hip.ptr(pred), _hip.ptr(y), _hip.ptr(mask),
                                    _hip.ptr(loss), _hip.ptr(norm), _hip.ptr(coef), _hip.ptr(ws), _hip.stream_of(pred)), "rdq_misfit_forward")
    return loss, norm, coef


@misfit.register_fake
def _(pred, y, mask, kind, delta):
    B = pred.shape[0]
    shape = (B, pred.shape[1], pred.shape[3], 3) if kind == MISFIT_KINDS["ncc"] else (0,)
    return pred.new_empty(B, dtype=torch.float32), pred.new_empty(B, dtype=torch.float32), \
        pred.new_empty(shape, dtype=torch.float64)


@torch.library.custom_op(f"{LIB}::misfit_backward", mutates_args=())
def misfit_backward(pred: Tensor, y: Tensor, mask: Optional[Tensor], norm: Tensor, coef: Tensor, gout: Tensor,
                    kind: int, delta: float) -> Tensor:
    """K13 backward: dloss / dpred for the upstream gout (B,), with the forward's norm (or a sharded survey's
    global one) and, for NCC, the forward's coef."""
    _hip.require_device(pred, y, mask, norm, coef, gout)
    B, ns, nt, ng = _misfit_dims(pred, kind)
    pred, y = pred.float().contiguous(), y.float().contiguous()
    mask = mask.float().contiguous() if mask is not None else None
    if kind == MISFIT_KINDS["ncc"] and (coef.dtype != torch.float64 or coef.shape != (B, ns, ng, 3)):
        raise ValueError("misfit_backward: coef must be the forward's float64 (B, ns, ng, 3)")
    if norm.numel() != B or gout.numel() != B:
        raise ValueError("misfit_backward: norm and gout must have B elements")
    dpred = torch.empty_like(pred)
    # named, so that the copy of an expanded (stride-0) gout lives until the launch is enqueued
    norm, gout, coef = norm.float().contiguous(), gout.float().contiguous(), coef.contiguous()
    _hip.check(_hip.lib().rdq_misfit_backward(kind, B, ns, nt, ng, delta, _hip.ptr(pred), _hip.ptr(y), _hip.ptr(mask),
                                              _hip.ptr(norm), _hip.ptr(coef), _hip.ptr(gout),
                                              _hip.ptr(dpred), _hip.stream_of(pred)), "rdq_misfit_backward")
    return dpred


@misfit_backward.register_fake
def _(pred, y, mask, norm, coef, gout, kind, delta):
    return torch.empty_like(pred, dtype=torch.float32, memory_format=torch.contiguous_format)


@torch.library.custom_op(f"{LIB}::smooth_reg", mutates_args=())
def smooth_reg(mu: Tensor, kind: int) -> Tensor:
    """K6: TV (kind 0) / Tikhonov (kind 1) per model on the padded model (benchmark.py:4-37)."""
    _hip.require_device(mu)
    m = mu.float().contiguous()
    B, _, H, W = m.shape
    loss = torch.empty(B, dtype=torch.float32, device=m.device)
    _hip.check(_hip.lib().rdq_smooth_reg_forward(kind, B, H, W, _hip.ptr(m), _hip.ptr(loss), _hip.stream_of(m)),
               "rdq_smooth_reg_forward")
    return loss


@smooth_reg.register_fake
def _(mu, kind):
    return mu.new_empty(mu.shape[0], dtype=torch.float32)


@torch.library.custom_op(f"{LIB}::smooth_reg_backward", mutates_args=())
def smooth_reg_backward(mu: Tensor, gout: Tensor, kind: int) -> Tensor:
    _hip.require_device(mu)
    m = mu.float().contiguous()
    B, _, H, W = m.shape
    grad = torch.empty_like(m)
    gout = gout.float().contiguous()   # named: the copy of an expanded gout lives until the launch is enqueued
    _hip.check(_hip.lib().rdq_smooth_reg_backward(kind, B, H, W, _hip.ptr(m), _hip.ptr(gout),
                                                  _hip.ptr(grad), _hip.stream_of(m)), "rdq_smooth_reg_backward")
    return grad


@smooth_reg_backward.register_fake
def _(mu, gout, kind):
    return torch.empty_like(mu, dtype=torch.float32)


@torch.library.custom_op(f"{LIB}::metrics", mutates_args=())
def metrics(pred: Tensor, true_norm: Tensor) -> Tensor:
    """K12: (mae, rmse, ssim) per model as a (3, B) device tensor (metrics.py:13-46)."""
    _hip.require_device(pred, true_norm)
    if pred.dtype != torch.float32 or true_norm.dtype != torch.float32:
        raise ValueError("metrics: pred and true_norm must be fp32")
    if pred.dim() != 4 or pred.shape[1] != 1:
        raise ValueError("metrics: pred must be (B, 1, H, W)")
    if true_norm.device != pred.device:
        raise ValueError("metrics: pred and true_norm must be on the same device")
    if true_norm.numel() != pred.numel():
        raise ValueError("metrics: true_norm must have the elements of pred, (B, 1, H, W)")
    B, _, H, W = pred.shape
    t = true_norm.contiguous()
    L = _hip.lib()
    ws = torch.empty(int(L.rdq_metrics_ws_bytes(B, H, W)), dtype=torch.uint8, device=pred.device)
    out = torch.empty(3, B, dtype=torch.float32, device=pred.device)
    strides = (ctypes.c_int64 * 4)(*pred.stride())
    _hip.check(L.rdq_metrics(B, H, W, _hip.ptr(pred), strides, _hip.ptr(t), _hip.ptr(out), _hip.ptr(ws),
                             _hip.stream_of(pred)), "rdq_metrics")
    return out


@metrics.register_fake
def _(pred, true_norm):
    return pred.new_empty(3, pred.shape[0], dtype=torch.float32)


@torch.library.custom_op(f"{LIB}::adam_clamp_", mutates_args=("param", "exp_avg", "exp_avg_sq"))
def adam_clamp_(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, beta1: float, beta2: float,
                eps: float, step_size: float, bias_correction2_sqrt: float, clamp: bool, lo: float, hi: float,
                guard: Optional[Tensor] = None) -> None:
    """K11: one torch.optim.Adam step (step_size = -lr / (1 - beta1^t), bias_correction2_sqrt =
    sqrt(1 - beta2^t); torch/optim/adam.py's multi-tensor formula) then param.clamp_(lo, hi) when
    `clamp`, in one launch (reference inversion.py:87-91).  guard: optional int32 device word; the
    step is a no-op on the device while it is non-zero (the FWI status word of a failed persistent
    launch)."""
    _hip.require_device(param)
    for t in (grad, exp_avg, exp_avg_sq):
        if t.shape != param.shape or not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError("adam_clamp_: grad / exp_avg / exp_avg_sq must be contiguous fp32 like param")
    if not param.is_contiguous() or param.dtype != torch.float32:
        raise ValueError("adam_clamp_: param must be contiguous fp32")
    if guard is not None and (guard.dtype != torch.int32 or guard.numel() < 1):
        raise ValueError("adam_clamp_: guard must be an int32 device word")
    _hip.check(_hip.lib().rdq_adam_step(param.numel(), _hip.ptr(param), _hip.ptr(grad), _hip.ptr(exp_avg),
                                        _hip.ptr(exp_avg_sq), beta1, beta2, eps, step_size, bias_correction2_sqrt,
                                        int(clamp), lo, hi, _hip.ptr(guard), _hip.stream_of(param)),
               "rdq_adam_step")


@adam_clamp_.register_fake
def _(param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, step_size, bias_correction2_sqrt, clamp, lo, hi,
      guard=None):
    return None


# ------------------------------------------------------------------ forward-only operators
def _forward_only(op, name):
    """The U-Net / regulariser operators are inference kernels (the RED gradient is
    (eps_hat - eps).detach(), regularization/diffusion.py:75): they run with grad-requiring inputs
    (module parameters) but have no backward; differentiating through one raises."""
    def backward(ctx, *grads):
        raise RuntimeError(f"red_diffeq::{name} has no backward (forward-only HIP kernel)")

    def setup(ctx, inputs, output):
        pass
    op.register_autograd(backward, setup_context=setup)


for _op, _name in ((conv2d_mfma, "conv2d_mfma"), (conv2d_rms, "conv2d_rms"), (conv2d_gn_silu, "conv2d_gn_silu"), (conv2d_gn_silu_sc, "conv2d_gn_silu_sc"),
                   (conv2d_bf16_gn_silu, "conv2d_bf16_gn_silu"), (conv2d_bf16_gn_silu_out, "conv2d_bf16_gn_silu_out"),
                   (conv2d_bf16_block_pair, "conv2d_bf16_block_pair"),
                   (conv2d_gn_silu_lsm, "conv2d_gn_silu_lsm"), (conv2d_gn_silu_out, "conv2d_gn_silu_out"), (unet_head, "unet_head"),
                   (gn_silu, "gn_silu"),
                   (rmsnorm, "rmsnorm"), (linear, "linear"), (time_mlp, "time_mlp"),
                   (linear_silu_multi, "linear_silu_multi"),
                   (sinusoidal_emb, "sinusoidal_emb"), (linear_attn, "linear_attn"), (linear_attn_block, "linear_attn_block"), (linear_attn_bf16, "linear_attn_bf16"), (linear_attn_f32, "linear_attn_f32"), (attn, "attn"),
                   (red_q_sample, "red_q_sample"), (red_eps, "red_eps"), (metrics, "metrics")):
    _forward_only(_op, _name)
