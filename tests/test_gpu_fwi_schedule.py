"""The FWI host launch paths (red-diffeq_amd/csrc/fwi.hip): every chunked call enqueues one schedule
(chunked_schedule) and the launch counts the plan reports are read from it; every persistent launch and
its occupancy query take the kernel from one table, the residency remembered per kernel.

* The counts of launch_info / ckpt_info against the schedule restated here: segments of K steps counted
  from the end of the record, each cut into launches of the kernels' depth.
* A round trip through every rows-per-wave pair leaves the persistent launches as they were."""
import numpy as np
import pytest
import torch

from conftest import vnorm
from test_gpu_checkpoint import B, NS, NT, make_fwi

pytestmark = pytest.mark.gpu

NX, NBC = 71, 10


@pytest.fixture(scope="module")
def operator(cuda):
    from red_diffeq.utils.synthetic import make_model
    ctx = dict(n_grid=NX, nt=NT, dx=10.0, dt=0.001, nbc=NBC, f=15.0, sz=10, gz=10, ng=NX, ns=NS)
    fwi = make_fwi(ctx)
    v = torch.from_numpy(vnorm(make_model("curvefault", 40, NX, seed=31, batch=B))).to(cuda)
    return fwi, v, fwi._plan(40, NX, v.device)


def launches(nt, K, T):
    """Sum over the segments [max(nt - (c + 1) K, 0), nt - c K) of ceil(len / T)."""
    K = min(K, nt)
    bounds = [max(nt - c * K, 0) for c in range(-(-nt // K) + 1)]
    return sum(-(-(hi - lo) // T) for hi, lo in zip(bounds, bounds[1:]))


@pytest.mark.parametrize("chains", [1, 2])
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "narrow"])
def test_reported_launch_counts_are_the_schedule(operator, wide, chains):
    """nt = 162 is a multiple of neither depth (4: forward and narrow adjoint, 5: wide adjoint); K = 7
    leaves a one-step segment, 40 a two-step one, 500 is one segment.  Counts are per launch chain."""
    _, _, plan = operator
    Tf, Ta = 4, (5 if wide else 4)
    assert NT % Tf and NT % Ta
    try:
        plan.set_persistent(False)
        plan.set_variant(wide_chunked=wide)
        plan.set_tuning(4, 4, chains)
        plan.set_wide_adj_steps(5)
        info = plan.launch_info(B)
        assert (info["fwd_class"], info["adj_class"], info["fwd_T"], info["adj_T"]) == (0, 0, Tf, Ta)
        assert info["fwd_launches"] == launches(NT, NT, Tf) == -(-NT // Tf)
        assert info["adj_launches"] == launches(NT, NT, Ta) == -(-NT // Ta)
        assert plan.wide_info(B)["chains"] == chains
        for K in (7, 40, 500):
            ck = plan.ckpt_info(B, K)
            nf, na = launches(NT, K, Tf), launches(NT, K, Ta)
            assert ck == {"fwd_class": 0, "nseg": -(-NT // min(K, NT)), "fwd_launches": nf, "bwd_launches": nf + na}, K
        # one segment: the store-all launches
        assert ck["fwd_launches"] == info["fwd_launches"]
        assert ck["bwd_launches"] == info["fwd_launches"] + info["adj_launches"]
    finally:
        plan.set_persistent(True)
        plan.set_variant()
        plan.set_tuning(4, 4, 0)
        plan.set_wide_adj_steps(0)


def test_rows_per_wave_round_trip_keeps_the_persistent_launch(operator):
    """Every legal (forward, adjoint) rows-per-wave pair is selected and its occupancy queried, then the
    default restored: the 96-row persistent launches (class, depth, launches; the workgroups that
    arrived per XCD, debug_words) are those of before, so no kernel's residency was remembered under
    another's key."""
    fwi, v, plan = operator

    def run():
        info = plan.launch_info(B)
        assert info["fwd_class"] == 12 and info["adj_class"] == 12, info
        words = []
        vg = v.clone().requires_grad_(True)
        seis = fwi(vg)
        words.append(plan.debug_words())                 # (synchronises) the forward launch's arrivals
        seis.backward(torch.ones_like(seis))
        words.append(plan.debug_words())                 # the adjoint's
        plan.status()
        assert words[0][0] == 0 and words[1][0] == 0 and sum(words[0][2]) > 0 and sum(words[1][2]) > 0
        return info, words, seis.detach().cpu().numpy(), vg.grad.cpu().numpy()

    try:
        plan.set_persistent(12)
        plan.set_rows_per_wave(6, 6)
        before = run()
        seen = {}
        for fr in (6, 8, 12, 24):
            for ar in (6, 8, 12):
                plan.set_rows_per_wave(fr, ar)
                seen[(fr, ar)] = plan.launch_info(B)     # queries the pair's kernels
        assert all(i["fwd_class"] == 12 and i["adj_class"] == 12 for i in seen.values()), seen
        plan.set_rows_per_wave(6, 6)
        after = run()
        assert after[0] == before[0] == seen[(6, 6)]
        assert after[1] == before[1]
        assert np.array_equal(after[2].view(np.int32), before[2].view(np.int32))
        assert np.array_equal(after[3].view(np.int32), before[3].view(np.int32))
    finally:
        plan.set_rows_per_wave(6, 6)
        plan.set_persistent(True)
