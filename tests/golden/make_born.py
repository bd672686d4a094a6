#!/usr/bin/env python
"""Generate tests/golden/born.npz: the REFERENCE's FWIForward (solvers/pde.py) linearised on the CPU with
torch.func.jvp, in fp64 and in fp32, and its fp64 autograd adjoint, for FWIForward.born / gauss_newton.

Run:  python tests/golden/make_born.py          writes born.npz
      python tests/golden/make_born.py terms    writes born_terms.npz (below) and leaves born.npz alone

Cases (nt = 160, dt = 1e-3, f = 15: a 147-sample wavelet; dx = 10), the smallest shapes at which the Born
kernel can go wrong:
  wrap   nz 12, nx 14, nbc 6 (padded 24 x 26), 2 shots, 7 receivers, B = 2, physical velocities
         (normalize=False): a 64 x 64 region is larger than the padded grid, so it wraps and holds the source
         row more than once.
  tiles  nz 40, nx 70, nbc 24 (padded 88 x 118), 3 shots, 24 receivers, B = 2, normalised velocities: two tile
         rows and three tile columns at depth 4, with partial edge tiles.  Model 0 has its unique minimum in the
         interior, model 1 at cell (0, 0), so the sponge's tangent and the replicated pad's both come from a
         corner.  dv is dense, non-zero at both argmins and under every source.
  geom   nz 20, nx 30, nbc 24 (padded 68 x 78), sample_temporal = 3, source row != receiver row (sz = 20,
         gz = 10), explicit gx with one repeated column, B = 1, normalised.

Per case <tag>:
  <tag>_ctx_*, <tag>_normalize, <tag>_st    the operator's ctx and constructor flags
  <tag>_v, <tag>_dv (float32)               model and direction, in the operator's input units
  <tag>_w (float32)                         a random residual of the seismograms' shape
  <tag>_seis64, <tag>_jdv64, <tag>_jtw64    the reference in fp64: forward(v), J dv (jvp), J^T w (autograd)
  <tag>_jdv32                               the reference's fp32 J dv (jvp)
  <tag>_eref                                per model, rel-L2 of the fp32 jvp against the fp64 one: the
                                            reference's own fp32 error, the tests' yardstick
  <tag>_ip                                  (<J dv, w>, <dv, J^T w>) in fp64
Asserted here in fp64: the jvp agrees with a central difference (h = 1e-3) to 1e-6, the two inner products
agree to 1e-10, every E_ref > 0.

born_terms.npz, one case `terms`: the tangent has four sources (dA in the model, dA replicated into the pad, dK =
K dv[argmin] / vmin in the sponge, dbeta at the source cells) and a dense direction lets the interior dA drown
the other three.  Here every direction is 0.04 at ONE cell per model and zero elsewhere.
  nz 20, nx 30, nbc 24 (padded 68 x 78: two tile rows and two tile columns at depth 4), 3 shots (source cells
  (1, 0), (1, 14), (1, 29)), 7 receivers, sz = gz = 10, B = 2, normalised; model 0 has its unique minimum at
  (11, 6), model 1 at the corner (0, 0).
  direction   model 0    model 1    isolates
  argmin      (11, 6)    (0, 0)     dK through the sponge, plus the corner's replicated dA for model 1
  source      (1, 14)    (1, 14)    dbeta
  corner      (19, 29)   (19, 29)   dA replicated into an nbc x nbc pad block
  edge        (0, 17)    (12, 0)    dA replicated into a pad strip, top and left
  interior    (10, 20)   (10, 20)   a single interior dA cell, the baseline
  terms_ctx_*, terms_normalize, terms_st, terms_v, terms_w, terms_jtw64      once, as above
  terms_<direction>_dv / _jdv64 / _jdv32 / _eref / _ip                       per direction, as above
with the same assertions per direction.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (loads the reference through _refimport)

ref = G.ref
BASE = dict(nt=160, dx=10.0, dt=0.001, f=15.0)


def operator(ctx, normalize, st):
    kw = dict(v_denorm_func=ref.data_trans.v_denormalize, s_norm_func=ref.data_trans.s_normalize_none) \
        if normalize else {}
    return ref.pde.FWIForward(copy.deepcopy(ctx), "cpu", sample_temporal=st, normalize=normalize, **kw)


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def unique_minimum(tag, v64):
    flat = v64.flatten(1)
    for b in range(v64.shape[0]):
        assert int((flat[b] == flat[b].min()).sum()) == 1, (tag, b)


def linearise(tag, fw, v32, dv32):
    """(forward, J dv) in fp64, J dv in fp32, E_ref per model and the jvp's distance from a central difference."""
    v64, dv64 = v32.double(), dv32.double()
    seis64, jdv64 = torch.func.jvp(fw, (v64,), (dv64,))
    assert seis64.dtype == torch.float64
    _, jdv32 = torch.func.jvp(fw, (v32,), (dv32,))
    assert jdv32.dtype == torch.float32
    h = 1e-3
    with torch.no_grad():
        cd = (fw(v64 + h * dv64) - fw(v64 - h * dv64)) / (2 * h)
    assert rel_l2(cd, jdv64) < 1e-6, (tag, rel_l2(cd, jdv64))
    eref = np.array([rel_l2(jdv32[b].double(), jdv64[b]) for b in range(v32.shape[0])])
    assert (eref > 0).all(), (tag, eref)
    return seis64, jdv64, jdv32, eref, rel_l2(cd, jdv64)


def adjoint(fw, v64, w64):
    vg = v64.clone().requires_grad_(True)
    (fw(vg) * w64).sum().backward()
    return vg.grad


def run_case(tag, ctx, normalize, st, v, dv, seed, out):
    fw = operator(ctx, normalize, st)
    v32, dv32 = torch.from_numpy(v), torch.from_numpy(dv)
    v64, dv64 = v32.double(), dv32.double()
    unique_minimum(tag, v64)                                       # a unique minimum per model
    seis64, jdv64, jdv32, eref, cderr = linearise(tag, fw, v32, dv32)
    w32 = torch.randn(seis64.shape, generator=torch.Generator().manual_seed(seed))
    w64 = w32.double()
    jtw64 = adjoint(fw, v64, w64)
    lhs, rhs = float((jdv64 * w64).sum()), float((dv64 * jtw64).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (tag, lhs, rhs)
    out.update({f"{tag}_ctx_{k}": np.asarray(x) for k, x in ctx.items()})
    out.update({f"{tag}_normalize": np.array(normalize), f"{tag}_st": np.array(st), f"{tag}_v": v, f"{tag}_dv": dv,
                f"{tag}_w": w32.numpy(), f"{tag}_seis64": seis64.numpy(), f"{tag}_jdv64": jdv64.numpy(),
                f"{tag}_jtw64": jtw64.numpy(), f"{tag}_jdv32": jdv32.numpy(), f"{tag}_eref": eref,
                f"{tag}_ip": np.array([lhs, rhs])})
    print(f"{tag}: seis {tuple(seis64.shape)}, E_ref {eref}, <Jdv,w> {lhs:.15e}, <dv,JTw> {rhs:.15e}, "
          f"jvp vs central difference {cderr:.2e}")


def model(kind, nz, nx, seed, batch, argmins, normalised):
    """A synthetic model with a little noise and one cell per model pushed below the rest (the unique minimum)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.from_numpy(G.synthetic.make_model(kind, nz, nx, seed=seed, batch=batch)).double()
    if normalised:
        v = torch.from_numpy(np.asarray(G.vnorm(v.float().numpy()))).double()
    scale = 1.0 if normalised else 1500.0
    v = v + 0.02 * scale * torch.rand(v.shape, generator=g, dtype=torch.float64)
    for b, (iz, ix) in enumerate(argmins):
        v[b, 0, iz, ix] = v[b].min() - 0.05 * scale
    return v.float().numpy()


def direction(shape, seed, scale):
    dv = scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return dv.numpy()


def main():
    torch.set_num_threads(8)
    out = {}
    ctx = dict(BASE, n_grid=14, nbc=6, sz=10, gz=10, ng=7, ns=2)
    v = model("curvevel", 12, 14, 21, 2, [(5, 8), (9, 3)], False)
    run_case("wrap", ctx, False, 1, v, direction(v.shape, 22, 60.0), 23, out)

    ctx = dict(BASE, n_grid=70, nbc=24, sz=10, gz=10, ng=24, ns=3)
    v = model("curvevel", 40, 70, 31, 2, [(17, 33), (0, 0)], True)
    dv = direction(v.shape, 32, 0.04)
    fw = operator(ctx, True, 1)
    isx = fw.adj_sr(fw.ctx["sx"], ctx["sz"], fw.ctx["gx"], ctx["gz"], ctx["dx"], ctx["nbc"])[0] - ctx["nbc"]
    assert dv[0, 0, 17, 33] != 0 and dv[1, 0, 0, 0] != 0 and (dv[:, 0, 1, isx] != 0).all()
    run_case("tiles", ctx, True, 1, v, dv, 33, out)

    ctx = dict(BASE, n_grid=30, nbc=24, sz=20, gz=10, ng=7, ns=2, gx=[1, 5, 9, 9, 14, 20, 27])
    v = model("flatvel", 20, 30, 41, 1, [(11, 6)], True)
    run_case("geom", ctx, True, 3, v, direction(v.shape, 42, 0.04), 43, out)

    G.save("born", **out)
    assert os.path.getsize(os.path.join(HERE, "born.npz")) <= 1 << 20


TERMS = {"argmin": ((11, 6), (0, 0)), "source": ((1, 14), (1, 14)), "corner": ((19, 29), (19, 29)),
         "edge": ((0, 17), (12, 0)), "interior": ((10, 20), (10, 20))}


def main_terms():
    torch.set_num_threads(8)
    ctx = dict(BASE, n_grid=30, nbc=24, sz=10, gz=10, ng=7, ns=3)
    v = model("curvevel", 20, 30, 51, 2, [(11, 6), (0, 0)], True)
    fw = operator(ctx, True, 1)
    isx, isz = fw.adj_sr(fw.ctx["sx"], ctx["sz"], fw.ctx["gx"], ctx["gz"], ctx["dx"], ctx["nbc"])[:2]
    assert isz - ctx["nbc"] == 1 and list(isx - ctx["nbc"]) == [0, 14, 29], (isz, isx)
    v32 = torch.from_numpy(v)
    v64 = v32.double()
    unique_minimum("terms", v64)
    assert [divmod(int(v64[b].argmin()), 30) for b in range(2)] == [(11, 6), (0, 0)]
    out = {f"terms_ctx_{k}": np.asarray(x) for k, x in ctx.items()}
    w32 = None
    for name, cells in TERMS.items():
        dv = np.zeros_like(v)
        for b, (iz, ix) in enumerate(cells):
            dv[b, 0, iz, ix] = 0.04
        dv32 = torch.from_numpy(dv)
        seis64, jdv64, jdv32, eref, cderr = linearise(name, fw, v32, dv32)
        if w32 is None:
            w32 = torch.randn(seis64.shape, generator=torch.Generator().manual_seed(53))
            jtw64 = adjoint(fw, v64, w32.double())
        lhs, rhs = float((jdv64 * w32.double()).sum()), float((dv32.double() * jtw64).sum())
        assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (name, lhs, rhs)
        out.update({f"terms_{name}_dv": dv, f"terms_{name}_jdv64": jdv64.numpy(), f"terms_{name}_jdv32": jdv32.numpy(),
                    f"terms_{name}_eref": eref, f"terms_{name}_ip": np.array([lhs, rhs])})
        print(f"terms/{name}: record {tuple(jdv64.shape)}, E_ref {eref}, <Jdv,w> {lhs:.15e}, <dv,JTw> {rhs:.15e}, "
              f"jvp vs central difference {cderr:.2e}, max |J dv| / max |dv| {float(jdv64.abs().max()) / 0.04:.3e}")
    out.update({"terms_normalize": np.array(True), "terms_st": np.array(1), "terms_v": v, "terms_w": w32.numpy(),
                "terms_jtw64": jtw64.numpy()})
    G.save("born_terms", **out)
    assert os.path.getsize(os.path.join(HERE, "born_terms.npz")) <= 1 << 20


if __name__ == "__main__":
    if sys.argv[1:] == ["terms"]:
        main_terms()
    elif sys.argv[1:]:
        sys.exit(f"usage: {sys.argv[0]} [terms]")
    else:
        main()
