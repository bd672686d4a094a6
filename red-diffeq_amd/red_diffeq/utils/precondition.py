"""Diagonal preconditioning of the data term by the source illumination (FWIForward.illumination).

InversionEngine takes Adam steps on d(misfit)/d mu + reg_lambda d(reg)/d mu, and Adam normalises every coordinate, so
the size of the data term relative to the regulariser decides, cell by cell, which of the two sets the step's sign.
Where the survey does not light the model the data term is weak and the prior wins by default.  Scaling the DATA
gradient alone by W ~ 1 / illumination corrects that balance (Adam cannot undo it: the regulariser's term is not
scaled).  Both functions are torch elementwise ops on an nz x nx tensor, run once per refresh: not a hot path.
"""
import torch


def _mean(x):
    # per model, summed in fp64 and rounded once: the mean of equal values is that value, so a flat H gives W = 1 exactly
    return x.double().mean(dim=(1, 2, 3), keepdim=True).float()


def illumination_weights(H, eps=1e-2, power=1.0):
    """Weights W, H's shape (B, 1, nz, nx), from an illumination H >= 0, per model:

        Hn = H / max(mean(H), tiny);   W = (Hn + eps) ** (-power);   W = W / mean(W)

    so mean(W) = 1 and reg_lambda keeps its scale.  eps bounds the boost of a dark cell at about 1 / eps of a cell of
    mean illumination; power = 0.5 is the milder square-root compensation.  An all-zero H gives W = 1."""
    if H.dim() != 4 or H.shape[1] != 1:
        raise ValueError(f"illumination_weights: expected H of shape (B,1,nz,nx), got {tuple(H.shape)}")
    if not eps > 0:
        raise ValueError(f"illumination_weights: eps must be > 0, got {eps}")
    H = H.detach().float()
    tiny = torch.finfo(torch.float32).tiny
    Hn = H / _mean(H).clamp_min(tiny)
    W = (Hn + float(eps)) ** (-float(power))
    return W / _mean(W)


class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, W):
        ctx.save_for_backward(W)
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        (W,) = ctx.saved_tensors
        return g * W, None


def precondition_grad(v, W):
    """v, unchanged; the gradient that flows back through it is multiplied by W (elementwise, broadcast)."""
    return _ScaleGrad.apply(v, W)
