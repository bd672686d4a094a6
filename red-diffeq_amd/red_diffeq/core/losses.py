"""LossCalculator (reference red_diffeq/core/losses.py:8-66) on the HIP L1 kernel (K5), and the misfits
beyond L1 (K13, include/red_diffeq_misfit.h): L2, Huber and trace-normalised correlation."""
import math
from typing import Optional

import torch

from .. import _hip
from .. import ops  # noqa: F401  (registers torch.ops.red_diffeq.*)
from ..regularization.base import RegularizationMethod


class _L1Misfit(torch.autograd.Function):
    """Per-model masked L1 misfit: forward torch.ops.red_diffeq.l1_misfit (K5), backward
    l1_misfit_backward (dpred = sign(pred - y) * mask * gout / nobs, exactly the autograd of
    losses.py:27-39).  nobs_override: the global observation count of a shot-sharded survey."""

    @staticmethod
    def forward(ctx, pred, y, mask, nobs_override):
        _hip.require_device(pred, y, mask)
        loss, nobs = torch.ops.red_diffeq.l1_misfit(pred, y, mask)
        if nobs_override is not None:          # shot-parallel: normalise by the global count
            loss = loss * (nobs / nobs_override)
            nobs = nobs_override.float().contiguous()
        ctx.save_for_backward(pred, y, mask, nobs)
        return loss

    @staticmethod
    def backward(ctx, gout):
        pred, y, mask, nobs = ctx.saved_tensors
        return torch.ops.red_diffeq.l1_misfit_backward(pred, y, mask, nobs, gout), None, None, None


def l1_misfit(predicted, target, mask=None, nobs=None):
    return _L1Misfit.apply(predicted, target, mask, nobs)


MISFITS = ("l1", "l2", "huber", "ncc")


def check_misfit(kind, delta=None):
    """The delta a misfit kind runs with (0.0 where it has none); ValueError for an unknown kind, or for
    "huber" without a finite delta > 0.  Host only: called before any GPU work."""
    if kind not in MISFITS:
        raise ValueError(f"Unknown misfit: {kind!r} (one of {MISFITS})")
    if kind != "huber":
        return 0.0
    try:
        ok = delta is not None and not isinstance(delta, bool) and math.isfinite(float(delta)) and float(delta) > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"the huber misfit needs a finite huber_delta > 0, got {delta!r}")
    return float(delta)


class _Misfit(torch.autograd.Function):
    """Per-model L2 / Huber / NCC misfit: forward torch.ops.red_diffeq.misfit (K13), backward misfit_backward.
    norm_override: the global normaliser of a shot-sharded survey (the observation count for L2 and Huber,
    the live-trace count for NCC), as _L1Misfit's nobs_override."""

    @staticmethod
    def forward(ctx, pred, y, mask, kind, delta, norm_override):
        _hip.require_device(pred, y, mask)
        loss, norm, coef = torch.ops.red_diffeq.misfit(pred, y, mask, kind, delta)
        if norm_override is not None:
            loss = loss * (norm / norm_override)
            norm = norm_override.float().contiguous()
        ctx.kind, ctx.delta = kind, delta
        ctx.save_for_backward(pred, y, mask, norm, coef)
        return loss

    @staticmethod
    def backward(ctx, gout):
        pred, y, mask, norm, coef = ctx.saved_tensors
        return (torch.ops.red_diffeq.misfit_backward(pred, y, mask, norm, coef, gout, ctx.kind, ctx.delta),
                None, None, None, None, None)


def misfit(predicted, target, mask=None, kind="l2", delta=None, norm=None):
    """Per-model data misfit of `kind` (MISFITS); "l1" is l1_misfit, bit for bit.  delta: Huber's threshold;
    norm: the survey's global normaliser when `predicted` holds a shard of the shots."""
    delta = check_misfit(kind, delta)
    if kind == "l1":
        return l1_misfit(predicted, target, mask, norm)
    return _Misfit.apply(predicted, target, mask, ops.MISFIT_KINDS[kind], delta, norm)


def global_norm(kind, y, mask):
    """The normaliser of the full survey, fp32 (B,), from the replicated record and mask (no communication):
    the observation count (K5's nobs) or, for "ncc", the number of live traces: those with a non-zero
    masked observed sample, the kernel's predicate c > 0."""
    B = y.shape[0]
    if kind == "ncc":
        live = (y != 0) if mask is None else ((mask != 0) & (y != 0))
        return live.any(dim=2).reshape(B, -1).sum(1).float().clamp(min=1.0)
    if mask is None:
        return torch.full((B,), float(y[0].numel()), dtype=torch.float32, device=y.device)
    return mask.reshape(B, -1).sum(1).clamp(min=1.0)


class LossCalculator:
    """Observation + regularisation losses (losses.py:8-66)."""

    def __init__(self, regularization_method: RegularizationMethod, misfit: str = "l1",
                 huber_delta: Optional[float] = None):
        check_misfit(misfit, huber_delta)
        self.regularization_method = regularization_method
        self.misfit = misfit
        self.huber_delta = huber_delta
        self.global_nobs = None   # set by the engine when shots are sharded across ranks

    def observation_loss(self, predicted: torch.Tensor, target: torch.Tensor,
                         mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-model misfit; L1 by default: with a mask, the mean over observed samples (losses.py:14-41)."""
        if self.misfit == "l1":
            return l1_misfit(predicted, target, mask, self.global_nobs)
        return misfit(predicted, target, mask, self.misfit, self.huber_delta, self.global_nobs)

    def regularization_loss(self, mu: torch.Tensor, generator: Optional[torch.Generator] = None):
        return self.regularization_method.get_reg_loss(mu, generator=generator)

    def total_loss(self, obs_loss: torch.Tensor, reg_loss: torch.Tensor, reg_lambda: float) -> torch.Tensor:
        return obs_loss + reg_lambda * reg_loss
