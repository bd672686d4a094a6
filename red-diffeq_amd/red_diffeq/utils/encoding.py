"""Source encoding for simultaneous-source ("supershot") inversion.

FWIForward.forward(v, encoding=E) models ne supershots per model, each fired by all ns sources at once, source s of
supershot e scaled by the code E[e, s].  The modelling is linear in the sources, so supershot e equals the sum over s
of E[e, s] times the record of shot s, and observed data are encoded with the same codes (encode) before the misfit
is taken.  A caller redraws the codes from iteration to iteration (random_encoding) so that the cross-talk between the
shots of one supershot averages out.
"""
import torch

KINDS = ("sign", "gaussian", "partition")


def random_encoding(ne, ns, kind, generator=None, device=None):
    """Codes E of shape (ne, ns), fp32 on `device`, drawn with `generator` (a torch.Generator on that device's type:
    the same generator state gives the same codes).

    kind = "sign":      every entry +1 or -1 with equal probability;
           "gaussian":  every entry standard normal;
           "partition": every source belongs to exactly one supershot, with a random sign there and 0 elsewhere
                        (each column has one non-zero entry, +1 or -1).  The sources are dealt in a random order to
                        the supershots in turn, so for ne <= ns no supershot is empty and their sizes differ by at
                        most one."""
    ne, ns = int(ne), int(ns)
    if ne < 1 or ns < 1:
        raise ValueError(f"random_encoding: ne and ns must be >= 1, got ne = {ne}, ns = {ns}")
    if kind not in KINDS:
        raise ValueError(f"random_encoding: kind must be one of {KINDS}, got {kind!r}")
    if kind == "gaussian":
        return torch.randn(ne, ns, generator=generator, device=device, dtype=torch.float32)
    sign = torch.randint(0, 2, (ne, ns) if kind == "sign" else (ns,), generator=generator, device=device)
    sign = (2 * sign - 1).to(torch.float32)
    if kind == "sign":
        return sign
    order = torch.randperm(ns, generator=generator, device=device)
    E = torch.zeros(ne, ns, dtype=torch.float32, device=device)
    E[torch.arange(ns, device=device) % ne, order] = sign
    return E


def encode(data, E):
    """Observed data (B, ns, nrec, ng) -> encoded data (B, ne, nrec, ng) with the codes E, (ne, ns) or (B, ne, ns):
    out[b, e] = sum_s E[b, e, s] * data[b, s].  The sum is taken in fp32 in ascending s, one product and one add per
    source (out = out + E[..., s] * data[:, s]), whatever the device: a fixed order, so the same data and codes give
    the same bits everywhere, and a zero code contributes an exact zero."""
    if data.dim() != 4:
        raise ValueError(f"encode: data must have shape (B, ns, nrec, ng), got {tuple(data.shape)}")
    B, ns = data.shape[0], data.shape[1]
    if E.dim() not in (2, 3) or E.shape[-1] != ns or (E.dim() == 3 and E.shape[0] != B):
        raise ValueError(f"encode: E must have shape (ne, {ns}) or ({B}, ne, {ns}), got {tuple(E.shape)}")
    E = E.to(device=data.device, dtype=torch.float32).expand(B, E.shape[-2], ns)
    data = data.to(torch.float32)
    out = torch.zeros(B, E.shape[1], data.shape[2], data.shape[3], dtype=torch.float32, device=data.device)
    for s in range(ns):
        out = out + E[:, :, s, None, None] * data[:, s, None]
    return out
