#!/usr/bin/env python
"""Generate tests/golden/wavelet.npz: the REFERENCE's FWIForward (solvers/pde.py) run on the CPU with caller-supplied
source wavelets, per model and per shot, and its autograd gradient with respect to them, for
FWIForward(..., wavelet=) and FWIForward.forward(v, wavelet=).

Run:  python tests/golden/make_wavelet.py          writes wavelet.npz

How.  The reference builds its wavelet in FWIForward.ricker and injects src[i] at every shot's source cell.  A
subclass that overrides only `ricker` to return a torch tensor makes FWM inject that tensor, and autograd then
differentiates through it, in fp32 and in fp64.  The reference has ONE wavelet for all shots and sums a loss over
models, so every (model, shot) pair is run on its own (a one-element `sx`, B = 1) and the results are stacked.

Cases: the Born fixtures' geometries (make_born.py; nt = 160, dt = 1e-3, dx = 10), the smallest at which the narrow
chunked kernels can go wrong:
  wrap   nz 12, nx 14, nbc 6, 2 shots, 7 receivers, B = 2, physical velocities: the region wraps the padded grid
         and holds the source row twice.
  tiles  nz 40, nx 70, nbc 24, 3 shots, 24 receivers, B = 2, normalised: 2 x 3 tiles at depth 4 with partial edge
         tiles; shots 0 and 2 have a receiver on the source cell.
  geom   nz 20, nx 30, nbc 24, sample_temporal = 3, sz != gz, one repeated gx, B = 1, normalised.
  short  the wrap geometry with nt = 10: shorter than any Ricker, fewer than three launches at depth 4.

Wavelets W (B, ns, nt) fp32, different for every model and shot; the kinds rotate with the model:
  noise     Gaussian noise smoothed with a 5-tap box
  ricker    half the Ricker wavelet of f = 15, delayed by 7 samples (cut at nt); sign flipped for odd models
  impulses  (where there is a third shot) 1 at n = 0 and +-1 (odd models: -1) at n = nt - 1: the first injected
            sample and the last

Per case <tag>:
  <tag>_ctx_*, <tag>_normalize, <tag>_st    the operator's ctx and constructor flags
  <tag>_v, <tag>_W, <tag>_r (float32)       model, wavelets, a random residual of the seismograms' shape
  <tag>_seis32, <tag>_seis64                the reference's seismograms in fp32 and fp64
  <tag>_gw64, <tag>_gw32, <tag>_gv64        autograd of <seis, r> with respect to W (fp64, fp32) and v (fp64)
  <tag>_eref_w                              per model, rel-L2 over (ns, nt) of gw32 against gw64: the reference's
                                            own fp32 error, the tests' yardstick
  <tag>_dW, <tag>_ip                        a random direction dW and (<F(v, dW), r>, <dW, gw64>) in fp64
  <tag>_homogeneous                         per j in SCALES = (3, -3): is the reference's own fp32 record for the
                                            wavelets 2^j W equal to 2^j seis32, bit for bit?  A power of two scales
                                            an fp32 recurrence exactly unless a value leaves the normal range; where
                                            the scheme's numerical precursor runs through the subnormal range (the
                                            large grid of `tiles`) products are rounded on an absolute grid and the
                                            scaled run rounds differently.  The tests ask exact homogeneity of the
                                            HIP path exactly where the reference has it,
  <tag>_seis32_scaled_<i>                   and where it has not, the reference's fp32 record for 2^SCALES[i] W,
                                            which the HIP path must then reproduce instead.
Asserted here: every eref_w > 0, the two inner products agree to 1e-10, and a central difference of <seis, r> along
a random direction in v agrees with <dv, gv64> to 1e-6.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_born as MB  # noqa: E402  (its models; loads the reference through make_golden)

G = MB.G
ref = G.ref


class WaveletOperator(ref.pde.FWIForward):
    """The reference operator with `ricker` returning the tensor in self.wavelet (nothing else overridden)."""
    wavelet = None

    def ricker(self, f, dt, nt):
        assert self.wavelet is not None and self.wavelet.shape == (nt,)
        return self.wavelet


def operators(ctx, normalize, st):
    """One single-shot operator per shot of ctx (sx in grid units, as ctx takes it)."""
    kw = dict(v_denorm_func=ref.data_trans.v_denormalize, s_norm_func=ref.data_trans.s_normalize_none) \
        if normalize else {}
    sx = np.linspace(0, ctx["n_grid"] - 1, num=ctx["ns"])
    return [WaveletOperator(dict(copy.deepcopy(ctx), sx=[float(x)], ns=1), "cpu", sample_temporal=st,
                            normalize=normalize, **kw) for x in sx]


def forward(ops, v, W):
    """(B, ns, nrec, ng) from one run per (model, shot); differentiable in v and W."""
    rows = []
    for b in range(v.shape[0]):
        shots = []
        for s, op in enumerate(ops):
            op.wavelet = W[b, s]
            shots.append(op(v[b:b + 1]))
        rows.append(torch.cat(shots, dim=1))
    return torch.cat(rows, dim=0)


def wavelets(B, ns, nt, seed):
    g = torch.Generator().manual_seed(seed)
    rick = ref.pde.FWIForward.ricker(None, 15.0, 1e-3, max(nt, 160))
    W = np.zeros((B, ns, nt), np.float32)
    kinds = ("noise", "ricker", "impulses")[:min(ns, 3)]
    for b in range(B):
        for s in range(ns):
            kind = kinds[(s + b) % len(kinds)]
            if kind == "noise":
                x = torch.randn(nt + 4, generator=g, dtype=torch.float64).numpy()
                W[b, s] = np.convolve(x, np.ones(5) / 5, mode="valid")
            elif kind == "ricker":
                W[b, s, 7:] = (-0.5 if b % 2 else 0.5) * rick[:nt - 7]
            else:
                W[b, s, 0], W[b, s, nt - 1] = 1.0, (-1.0 if b % 2 else 1.0)
    return W


SCALES = (3, -3)


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def run_case(tag, ctx, normalize, st, v, seed, dv_scale, out):
    ops = operators(ctx, normalize, st)
    B, ns, nt = v.shape[0], ctx["ns"], ctx["nt"]
    W = wavelets(B, ns, nt, seed)
    assert len({W[b, s].tobytes() for b in range(B) for s in range(ns)}) == B * ns      # all different
    v32, W32 = torch.from_numpy(v), torch.from_numpy(W)
    v64, W64 = v32.double(), W32.double()
    MB.unique_minimum(tag, v64)
    with torch.no_grad():
        seis32, seis64 = forward(ops, v32, W32), forward(ops, v64, W64)
    assert seis32.dtype == torch.float32 and seis64.dtype == torch.float64
    homogeneous = []
    for i, j in enumerate(SCALES):          # the reference itself under a power-of-two scale of the wavelets
        with torch.no_grad():
            scaled = forward(ops, v32, W32 * 2.0 ** j)
        homogeneous.append(bool(torch.equal(scaled, seis32 * 2.0 ** j)))
        if not homogeneous[-1]:
            out[f"{tag}_seis32_scaled_{i}"] = scaled.numpy()
    out[f"{tag}_homogeneous"] = np.array(homogeneous)
    g = torch.Generator().manual_seed(seed + 1)
    r32 = torch.randn(seis64.shape, generator=g)
    r64 = r32.double()

    def grads(vv, WW, rr):
        vv, WW = vv.clone().requires_grad_(True), WW.clone().requires_grad_(True)
        (forward(ops, vv, WW) * rr).sum().backward()
        return vv.grad, WW.grad
    gv64, gw64 = grads(v64, W64, r64)
    _, gw32 = grads(v32, W32, r32)
    assert gw32.dtype == torch.float32 and gw64.dtype == torch.float64
    eref = np.array([rel_l2(gw32[b].double(), gw64[b]) for b in range(B)])
    assert (eref > 0).all(), (tag, eref)
    # the seismograms are linear in the wavelet: <F(v, dW), r> = <dW, gw>
    dW32 = torch.randn(W.shape, generator=g)
    with torch.no_grad():
        lhs = float((forward(ops, v64, dW32.double()) * r64).sum())
    rhs = float((dW32.double() * gw64).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (tag, lhs, rhs)
    # gv64 against a central difference of the same functional
    dv = dv_scale * torch.randn(v.shape, generator=g, dtype=torch.float64)
    h = 1e-3
    with torch.no_grad():
        cd = float(((forward(ops, v64 + h * dv, W64) - forward(ops, v64 - h * dv, W64)) * r64).sum()) / (2 * h)
    dd = float((dv * gv64).sum())
    assert abs(cd - dd) <= 1e-6 * abs(dd), (tag, cd, dd)
    out.update({f"{tag}_ctx_{k}": np.asarray(x) for k, x in ctx.items()})
    out.update({f"{tag}_normalize": np.array(normalize), f"{tag}_st": np.array(st), f"{tag}_v": v, f"{tag}_W": W,
                f"{tag}_r": r32.numpy(), f"{tag}_seis32": seis32.numpy(), f"{tag}_seis64": seis64.numpy(),
                f"{tag}_gw64": gw64.numpy(), f"{tag}_gw32": gw32.numpy(), f"{tag}_gv64": gv64.numpy(),
                f"{tag}_eref_w": eref, f"{tag}_dW": dW32.numpy(), f"{tag}_ip": np.array([lhs, rhs])})
    print(f"{tag}: homogeneous under 2^{SCALES}: {homogeneous}")
    print(f"{tag}: seis {tuple(seis64.shape)}, E_ref(w) {eref}, <F dW, r> {lhs:.15e}, <dW, gw> {rhs:.15e}, "
          f"gv vs central difference {abs(cd - dd) / abs(dd):.2e}, seis32 vs seis64 {rel_l2(seis32.double(), seis64):.2e}")


def main():
    torch.set_num_threads(8)
    out = {}
    base = MB.BASE
    ctx = dict(base, n_grid=14, nbc=6, sz=10, gz=10, ng=7, ns=2)
    v = MB.model("curvevel", 12, 14, 21, 2, [(5, 8), (9, 3)], False)
    run_case("wrap", ctx, False, 1, v, 61, 60.0, out)
    run_case("short", dict(ctx, nt=10), False, 1, v, 91, 60.0, out)

    ctx = dict(base, n_grid=70, nbc=24, sz=10, gz=10, ng=24, ns=3)
    v = MB.model("curvevel", 40, 70, 31, 2, [(17, 33), (0, 0)], True)
    run_case("tiles", ctx, True, 1, v, 71, 0.04, out)

    ctx = dict(base, n_grid=30, nbc=24, sz=20, gz=10, ng=7, ns=2, gx=[1, 5, 9, 9, 14, 20, 27])
    v = MB.model("flatvel", 20, 30, 41, 1, [(11, 6)], True)
    run_case("geom", ctx, True, 3, v, 81, 0.04, out)

    G.save("wavelet", **out)
    assert os.path.getsize(os.path.join(HERE, "wavelet.npz")) <= 1 << 20


if __name__ == "__main__":
    main()
