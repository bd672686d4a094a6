"""Cross-family contracts of the narrow (64-column) chunked kernels: k_fwd_tb, k_adj_tb, k_born_tb and
k_fwd_born_tb repeat one tile / row prologue and share one stencil (tb_lap, tb_t1t2: csrc/fwi.hip, DESIGN.md
"Narrow chunked kernels: shared parts"), and their header comments promise each other's bits.  This file asserts
those promises on the geometries where a prologue, a record store or an epilogue can go wrong:

  fwd_wrap        a region taller than the domain: the source row is hit twice in one region
  fwd_multi_rcv   several receivers in one padded column (receiver list, residual fold)
  fwd_small_st3   sample_temporal = 3: the recorded-step test of the store and of the residual

each with its own record (160 / 200 steps: a one- / two-step tail at depth 3), B = 2, chunked launches
(set_persistent(0)), 64-column regions (wide_chunked=False), one launch chain, graphs on and off, for every blocking
depth 1..4 and both coefficient sources.  The K = 5 checkpointed forms cut the record into 5-step segments, so
every depth above 1 also ends its segments in a short tail launch (2 + 2 + 1, 3 + 2, 4 + 1).

Everything is torch.equal.  The one exception is gk, the sponge partial sums, whose fp64 summation order the C
layer is free to choose per entry point: 1e-12 relative per model, the bar tests/test_gpu_checkpoint.py uses."""
import numpy as np
import pytest
import torch

from conftest import ctx_of, load_golden, vnorm
from test_gpu_fwi import make_fwi

pytestmark = pytest.mark.gpu

GEOMETRIES = {"fwd_wrap": {}, "fwd_multi_rcv": {}, "fwd_small_st3": dict(sample_temporal=3, sample_spatial=0.5)}
K = 5
GK_RTOL = 1e-12


class Case:
    """One geometry: the operator, a B = 2 model, a direction, a residual, and the plan's wavelet as the
    (B, ns, nt) view with zero model and shot strides that the _src entry points take as `(wav, 0, 0)`."""

    def __init__(self, name, cuda):
        z = load_golden(name)
        self.fwi = make_fwi(ctx_of(z), **GEOMETRIES[name])
        v = vnorm(z["v"])
        if v.shape[0] == 1:                     # second model: the first one mirrored left to right
            v = np.concatenate([v, v[..., ::-1]], 0)
        self.B = 2
        self.v = torch.from_numpy(np.ascontiguousarray(v[:2])).to(cuda)
        g = torch.Generator().manual_seed(20)
        self.dv = (torch.rand(self.v.shape, generator=g) - 0.5).to(cuda)
        self.plan = self.fwi._plan(self.v.shape[2], self.v.shape[3], self.v.device)
        p = self.plan
        self.r = torch.randn((self.B, p.ns, p.sizes(self.B).nrec, p.ng), generator=g).to(cuda)
        wav = torch.from_numpy(p._wav.astype(np.float32)).to(cuda)
        self.w = wav.expand(self.B, p.ns, p.nt)
        assert self.w.stride() == (0, 0, 1)


@pytest.fixture(scope="module")
def cases(cuda):
    return {name: Case(name, cuda) for name in GEOMETRIES}


def gk_close(got, want, B):
    got, want = (t.view(B, -1).sum(1).cpu().numpy() for t in (got, want))
    return np.allclose(got, want, rtol=GK_RTOL, atol=0.0)


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("name", GEOMETRIES)
def test_narrow_kernels_keep_each_others_bits(cuda, cases, name, graphs):
    c = cases[name]
    plan, B, vm, ops = c.plan, c.B, 0, torch.ops.red_diffeq
    plan.set_persistent(0)
    plan.set_graphs(graphs)
    coeffs, vstat = plan.coeffs(c.v, vm)
    seg = torch.empty(int(plan.ckpt_sizes(B, K).seg) // 4, dtype=torch.float32, device=cuda)
    assert plan.ckpt_sizes(B, K).nseg > 1
    for depth in (1, 2, 3, 4):
        plan.set_tuning(depth, depth, 1)
        for gen in (True, False):
            plan.set_variant(fwd_gen_coeffs=gen, wide_chunked=False)
            info = plan.launch_info(B)
            assert info["fwd_class"] == 0, info
            at = (name, graphs, depth, gen)
            seis, hist = plan.forward(coeffs, B, True)
            assert float(seis.abs().max()) > 0
            ds = plan.born(coeffs, vstat, hist, c.dv, B, vm)
            assert float(ds.abs().max()) > 0

            # born_fused seis == forward seis, born_fused dseis == born dseis
            seis_f, ds_f, none = plan.born_fused(coeffs, vstat, c.dv, B, vm)
            assert torch.equal(seis_f, seis) and torch.equal(ds_f, ds) and none.numel() == 0, at

            # forward_src with the plan's wavelet == the plain forward
            seis_s, hist_s = ops.fwi_forward_src(coeffs, c.w, plan.op_id, B, True)
            assert torch.equal(seis_s, seis), at

            # adjoint_src == the plain adjoint (gk: summation order)
            gA, gk, gb = plan.adjoint(coeffs, hist, c.r, B)
            assert float(gA.abs().max()) > 0 and float(gb.abs().max()) > 0
            gA_s, gk_s, gb_s, _ = ops.fwi_adjoint_src(coeffs, c.w, hist_s, c.r, plan.op_id, B, False)
            assert torch.equal(gA_s, gA) and torch.equal(gb_s, gb), at
            assert gk_close(gk_s, gk, B), at
            del hist, hist_s

            # the K = 5 checkpointed forms == store-all: plain, with the call's wavelets, and the fused pass's store
            seis_c, ckpt = plan.forward_ckpt(coeffs, B, K)
            assert torch.equal(seis_c, seis), at
            gA_c, _, gb_c = plan.adjoint_ckpt(coeffs, ckpt, c.r, B, K)
            assert torch.equal(gA_c, gA) and torch.equal(gb_c, gb), at
            seis_c, ckpt = ops.fwi_forward_ckpt_src(coeffs, c.w, plan.op_id, B, K)
            assert torch.equal(seis_c, seis), at
            gA_c, _, gb_c, _ = ops.fwi_adjoint_ckpt_src(coeffs, c.w, ckpt, seg, c.r, plan.op_id, B, K, False)
            assert torch.equal(gA_c, gA) and torch.equal(gb_c, gb), at
            seis_c, ds_c, ckpt = plan.born_fused(coeffs, vstat, c.dv, B, vm, K)
            assert torch.equal(seis_c, seis) and torch.equal(ds_c, ds), at
            gA_c, _, gb_c = plan.adjoint_ckpt(coeffs, ckpt, c.r, B, K)
            assert torch.equal(gA_c, gA) and torch.equal(gb_c, gb), at
    c.fwi.check()
