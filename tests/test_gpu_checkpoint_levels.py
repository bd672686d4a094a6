"""The checkpointed gradient's stored levels are the history (rdq_fwi_forward_ckpt / rdq_fwi_adjoint_ckpt).

tests/test_gpu_checkpoint.py pins the checkpointed calls through their outputs (seis, gA, gk, gbeta).  Here
the levels themselves are compared, bit for bit, with the store-all history of the PERSISTENT forward on
the same plan (the forward is bit-exact in every kernel family, so the chunked first pass and recompute
must reproduce the persistent kernels' slots): every checkpoint pair c is the history's slots
{b_c, b_c + 1}, and after the backward the segment buffer holds the segment run last (the first in time,
from zeros) and, above it, what is left of the segment run before it (from a checkpoint pair).  This is the
layout any other producer or consumer of the store ("Not built") has to meet.

Grid and helpers: tests/test_gpu_wave_roles.py (70 x 70, nbc = 20 -> 110 x 110 padded, periodic wrap both
ways, two shots with sources in different tiles, B = 2, f = 60 Hz from nt = 37).  Every comparison is
torch.equal: no tolerance to choose."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_wave_roles import _setup

pytestmark = pytest.mark.gpu

B, K = 2, 7


def _cells(t, plan, levels):
    sz = plan.sizes(B)
    return t.view(levels, B * plan.ns, sz.Hp, sz.ld)[..., :sz.Wp]


# nt = 57: a one-step first segment (57 = 8 x 7 + 1); 56: whole segments only; 54: five steps, more than the
# forward's depth of 4 and less than two launches of it
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "narrow"])
@pytest.mark.parametrize("nt", [57, 56, 54])
def test_stored_levels_are_the_history(cuda, nt, wide):
    from red_diffeq import _hip
    fwi, plan, v, dseis = _setup(cuda, nt, B)
    info = plan.launch_info(B)
    assert info["fwd_persistent"], info                       # the reference history: persistent forward
    coeffs, _ = plan.coeffs(v, 0)
    seis_sa, hist_t = plan.forward(coeffs, B, keep_history=True)
    plan.status()
    assert plan.debug_words()[0] == 0
    hist = _cells(hist_t, plan, nt + 2)
    plan.set_variant(wide_chunked=wide)                       # the family the (default) checkpointed calls run
    cs, sz = plan.ckpt_sizes(B, K), plan.sizes(B)
    nseg = -(-nt // K)
    level = sz.history // (nt + 2)
    assert (cs.nseg, cs.seg_levels, cs.ckpt, cs.seg) == (nseg, K + 2, 2 * (nseg - 1) * level, (K + 2) * level)

    seis, ckpt = plan.forward_ckpt(coeffs, B, K)
    plan.status()
    assert plan.debug_words()[0] == 0
    assert torch.equal(seis, seis_sa)
    # the operator's own ctx (it holds sx / gx already scaled to metres: the oracle derives them again)
    ctx = {k: val for k, val in fwi.ctx.items() if k not in ("sx", "gx")}
    oracle = O.OracleFWI(ctx, B).forward(v.cpu().numpy())[0]
    assert torch.equal(seis.cpu(), torch.from_numpy(np.ascontiguousarray(oracle, np.float32)))
    pairs = _cells(ckpt, plan, 2 * (nseg - 1))
    for c in range(1, nseg):                                  # checkpoint c = slots {b_c, b_c + 1}, pair c - 1
        b = nt - c * K
        assert torch.equal(pairs[2 * (c - 1)], hist[b]) and torch.equal(pairs[2 * (c - 1) + 1], hist[b + 1]), c
        assert float(hist[b + 1].abs().max()) > 0 or b == 0   # not vacuous (the source fires from step 0)

    f32 = lambda n: torch.empty(int(n) // 4, device=cuda)
    seg, ring, gA, gb = f32(cs.seg), f32(sz.ring), f32(sz.gA), f32(sz.gbeta)
    gk = torch.empty(int(sz.gk_part) // 8, dtype=torch.float64, device=cuda)
    seg.fill_(float("nan"))                                   # every level read below was written by the call
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = _hip.ptr
    _hip.check(plan.lib.rdq_fwi_adjoint_ckpt(plan.handle, B, K, P(coeffs), P(ckpt), P(seg), P(dseis), P(ring),
                                             P(gA), P(gk), P(gb), st), "rdq_fwi_adjoint_ckpt")
    plan.status()
    assert plan.debug_words()[0] == 0
    levels = _cells(seg, plan, K + 2)
    m = nt - (nseg - 1) * K                                   # steps of the first segment in time: [0, m)
    assert float(levels[0].abs().max()) == 0 and float(levels[1].abs().max()) == 0   # the boundary at step 0
    for j in range(2, m + 2):                                 # recomputed from zeros: level j = slot j
        assert torch.equal(levels[j], hist[j]), j
    for j in range(m + 2, K + 2):                             # left by segment [m, m + K): level j = slot m + j
        assert torch.equal(levels[j], hist[m + j]), j
    assert float(hist[m + 1].abs().max()) > 0 and float(hist[m + K + 1].abs().max()) > 0
    # the raw call's accumulators are those of the operator-level call (its own segment buffer)
    gA2, gk2, gb2 = plan.adjoint_ckpt(coeffs, ckpt, dseis, B, K)
    plan.status()
    assert torch.equal(gA, gA2) and torch.equal(gk, gk2) and torch.equal(gb, gb2)
    assert float(gA.abs().max()) > 0
