#!/usr/bin/env python
"""Generate tests/golden/encoding.npz: fp64 truth and fp32 yardsticks for encoded simultaneous-source supershots,
FWIForward.forward(v, wavelet=W, encoding=E), built from per-shot runs of the REFERENCE's FWIForward by linearity.

Run:  python tests/golden/make_encoding.py          writes encoding.npz

How.  The reference has one source cell per wavefield, so it cannot fire a supershot directly.  The wave equation is
linear in its sources: supershot e of the codes E (ne, ns) is sum_s E[e, s] * (the record of shot s with wavelet
W[b, s]).  make_wavelet's WaveletOperator (the reference with only `ricker` overridden) gives the per-(model, shot)
records in fp32 and fp64, differentiable in v and W; the combination is an einsum over s, differentiable in E.
  truth      seis64_enc = sum_s E[e, s] seis64[s]                                   (all in fp64)
  yardstick  E_ref[b, e] = rel-L2 of sum_s E[e, s] seis32[s] (fp32 records, summed in fp64) against the truth
  gradients  of <seis_enc, r> in v, W and E (E as a full (B, ne, ns) tensor) by the reference's autograd through the
             same combination, all-fp64 and all-fp32: gv64, gW64, gE64 and eref_v, eref_w, eref_E per model
             (rel-L2 of the fp32 gradient against the fp64 one)

Cases: the wavelet fixture's geometries and models (make_wavelet.py) and
  shared   the wrap geometry with three sources at grid columns 2, 9, 9: sources 1 and 2 share a padded cell.

Codes, one matrix E of ns + 2 rows per case (so ne > ns when used whole; the supershots of a call are independent
of each other, so the tests also run row subsets against the matching rows of the truth):
  rows 0, 1        random signs
  rows 2 ..        Gaussian, with E[2, ns - 1] set to exactly 0
  row 0 alone      the ne = 1 call

Per case <tag>:
  <tag>_ctx_*, <tag>_normalize, <tag>_st    the operator's ctx (with `sx` in grid units where it is not the
                                            default) and constructor flags
  <tag>_v, <tag>_W, <tag>_E, <tag>_r        model, wavelets, codes, a random residual of the encoded record's shape
  <tag>_seis64                              the truth (B, ne, nrec, ng), fp64
  <tag>_eref                                E_ref (B, ne)
  <tag>_gv64, <tag>_gW64, <tag>_gE64        the fp64 gradients ((B, 1, nz, nx), (B, ns, nt), (B, ne, ns))
  <tag>_eref_v, <tag>_eref_w, <tag>_eref_E  per model
  <tag>_dW, <tag>_ip                        a random direction dW and (<F_E(v, dW), r>, <dW, gW64>) in fp64
Asserted here: every yardstick > 0, the two inner products agree to 1e-10, and a central difference of
<seis_enc, r> along a random direction in v agrees with <dv, gv64> to 1e-6.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_wavelet as MW  # noqa: E402  (WaveletOperator, forward, wavelets; loads the reference)

MB, G, ref = MW.MB, MW.G, MW.ref


def operators(ctx, normalize, st):
    """One single-shot operator per source of ctx (its `sx` in grid units, or the default linspace)."""
    kw = dict(v_denorm_func=ref.data_trans.v_denormalize, s_norm_func=ref.data_trans.s_normalize_none) \
        if normalize else {}
    sx = ctx["sx"] if "sx" in ctx else np.linspace(0, ctx["n_grid"] - 1, num=ctx["ns"])
    return [MW.WaveletOperator(dict(copy.deepcopy(ctx), sx=[float(x)], ns=1), "cpu", sample_temporal=st,
                               normalize=normalize, **kw) for x in sx]


def codes(ns, seed):
    g = torch.Generator().manual_seed(seed)
    E = torch.empty(ns + 2, ns)
    E[:2] = 2.0 * torch.randint(0, 2, (2, ns), generator=g) - 1.0
    E[2:] = torch.randn(ns, ns, generator=g)
    E[2, ns - 1] = 0.0
    return E


def encoded(ops, v, W, E):
    """(B, ne, nrec, ng): the per-shot records combined with E (B, ne, ns), in the dtype of the operands."""
    return torch.einsum("bes,bsrg->berg", E, MW.forward(ops, v, W))


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def run_case(tag, ctx, normalize, st, v, seed, dv_scale, out):
    ops = operators(ctx, normalize, st)
    B, ns, nt = v.shape[0], ctx["ns"], ctx["nt"]
    W = MW.wavelets(B, ns, nt, seed)
    E = codes(ns, seed + 7)
    ne = E.shape[0]
    v32, W32 = torch.from_numpy(v), torch.from_numpy(W)
    E32 = E.expand(B, ne, ns).contiguous()
    v64, W64, E64 = v32.double(), W32.double(), E32.double()
    MB.unique_minimum(tag, v64)
    with torch.no_grad():
        seis64 = encoded(ops, v64, W64, E64)
        comb32 = torch.einsum("bes,bsrg->berg", E64, MW.forward(ops, v32, W32).double())   # fp32 records, fp64 sum
    eref = np.array([[rel_l2(comb32[b, e], seis64[b, e]) for e in range(ne)] for b in range(B)])
    assert (eref > 0).all(), (tag, eref)
    g = torch.Generator().manual_seed(seed + 1)
    r32 = torch.randn(seis64.shape, generator=g)
    r64 = r32.double()

    def grads(vv, WW, EE, rr):
        vv, WW, EE = (t.clone().requires_grad_(True) for t in (vv, WW, EE))
        (encoded(ops, vv, WW, EE) * rr).sum().backward()
        return vv.grad, WW.grad, EE.grad
    gv64, gW64, gE64 = grads(v64, W64, E64, r64)
    gv32, gW32, gE32 = grads(v32, W32, E32, r32)
    assert gW32.dtype == torch.float32 and gW64.dtype == torch.float64
    yard = {n: np.array([rel_l2(a[b].double(), t[b]) for b in range(B)])
            for n, a, t in (("v", gv32, gv64), ("w", gW32, gW64), ("E", gE32, gE64))}
    assert all((y > 0).all() for y in yard.values()), (tag, yard)
    # linear in the wavelets: <F_E(v, dW), r> = <dW, gW>
    dW32 = torch.randn(W.shape, generator=g)
    with torch.no_grad():
        lhs = float((encoded(ops, v64, dW32.double(), E64) * r64).sum())
    rhs = float((dW32.double() * gW64).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (tag, lhs, rhs)
    dv = dv_scale * torch.randn(v.shape, generator=g, dtype=torch.float64)
    h = 1e-3
    with torch.no_grad():
        cd = float(((encoded(ops, v64 + h * dv, W64, E64) - encoded(ops, v64 - h * dv, W64, E64)) * r64).sum()) / (2 * h)
    dd = float((dv * gv64).sum())
    assert abs(cd - dd) <= 1e-6 * abs(dd), (tag, cd, dd)
    out.update({f"{tag}_ctx_{k}": np.asarray(x) for k, x in ctx.items()})
    out.update({f"{tag}_normalize": np.array(normalize), f"{tag}_st": np.array(st), f"{tag}_v": v, f"{tag}_W": W,
                f"{tag}_E": E.numpy(), f"{tag}_r": r32.numpy(), f"{tag}_seis64": seis64.numpy(), f"{tag}_eref": eref,
                f"{tag}_gv64": gv64.numpy(), f"{tag}_gW64": gW64.numpy(), f"{tag}_gE64": gE64.numpy(),
                f"{tag}_eref_v": yard["v"], f"{tag}_eref_w": yard["w"], f"{tag}_eref_E": yard["E"],
                f"{tag}_dW": dW32.numpy(), f"{tag}_ip": np.array([lhs, rhs])})
    print(f"{tag}: seis {tuple(seis64.shape)}, E_ref {eref.min():.2e} .. {eref.max():.2e}, eref_v {yard['v']}, "
          f"eref_w {yard['w']}, eref_E {yard['E']}, <F dW, r> {lhs:.15e}, <dW, gW> {rhs:.15e}, "
          f"gv vs central difference {abs(cd - dd) / abs(dd):.2e}", flush=True)


def main():
    torch.set_num_threads(8)
    out = {}
    base = MB.BASE
    ctx = dict(base, n_grid=14, nbc=6, sz=10, gz=10, ng=7, ns=2)
    v = MB.model("curvevel", 12, 14, 21, 2, [(5, 8), (9, 3)], False)
    run_case("wrap", ctx, False, 1, v, 61, 60.0, out)
    run_case("short", dict(ctx, nt=10), False, 1, v, 91, 60.0, out)
    run_case("shared", dict(ctx, ns=3, sx=[2.0, 9.0, 9.0]), False, 1, v, 101, 60.0, out)

    ctx = dict(base, n_grid=70, nbc=24, sz=10, gz=10, ng=24, ns=3)
    v = MB.model("curvevel", 40, 70, 31, 2, [(17, 33), (0, 0)], True)
    run_case("tiles", ctx, True, 1, v, 71, 0.04, out)

    ctx = dict(base, n_grid=30, nbc=24, sz=20, gz=10, ng=7, ns=2, gx=[1, 5, 9, 9, 14, 20, 27])
    v = MB.model("flatvel", 20, 30, 41, 1, [(11, 6)], True)
    run_case("geom", ctx, True, 3, v, 81, 0.04, out)

    G.save("encoding", **out)
    assert os.path.getsize(os.path.join(HERE, "encoding.npz")) <= 1 << 20


if __name__ == "__main__":
    main()
