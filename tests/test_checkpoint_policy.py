"""History policy of the checkpointed FWI gradient (FWIForward(checkpoint=..., history_budget_gb=...)):
choose_checkpoint picks store-all while its nt + 2 levels fit the budget, else the largest K whose
checkpoint store + segment buffer fit, and the level count it uses equals a brute-force enumeration of the
segment layout documented in include/red_diffeq_fwi.h.  No device needed."""
import math

import pytest

from red_diffeq.solvers.pde import checkpoint_levels, choose_checkpoint

NTS = [1, 2, 162, 1000]


def layout(nt, K):
    """The layout as the header states it: segments counted from the end of the record, boundaries
    b_c = max(nt - c K, 0); a checkpoint = the slot pair (b_c, b_c + 1) of every interior boundary."""
    nseg = math.ceil(nt / K)
    bounds = [max(nt - c * K, 0) for c in range(nseg + 1)]
    segments = [(bounds[c + 1], bounds[c]) for c in range(nseg)]        # steps [lo, hi), last segment first
    ckpt_slots = [s for b in bounds if 0 < b < nt for s in (b, b + 1)]
    return nseg, bounds, segments, ckpt_slots


@pytest.mark.parametrize("nt", NTS)
def test_level_count_matches_the_segment_layout(nt):
    for K in list(range(1, nt + 3)) + [10 * nt + 7]:
        nseg, bounds, segments, ckpt_slots = layout(nt, K)
        assert bounds[0] == nt and bounds[-1] == 0 and all(a > b for a, b in zip(bounds, bounds[1:]))
        # the segments tile [0, nt), none longer than K, and only the first one in time may be shorter
        assert sorted(n for lo, hi in segments for n in range(lo, hi)) == list(range(nt))
        assert all(hi - lo == min(K, nt) for lo, hi in segments[:-1]) and 0 < segments[-1][1] - segments[-1][0] <= K
        # a segment's buffer holds slots lo .. hi + 1: what its recompute reads (lo, lo + 1) and writes
        # (n + 2 for its steps n), which covers what its adjoint reads (slot k for k = lo + 1 .. hi)
        seg_levels = max(hi + 1 - lo + 1 for lo, hi in segments)
        assert seg_levels == min(K, nt) + 2
        assert len(ckpt_slots) == 2 * (nseg - 1)
        assert checkpoint_levels(nt, K) == len(ckpt_slots) + seg_levels


def budgets(nt):
    vals = {checkpoint_levels(nt, K) for K in range(1, nt + 1)} | {nt + 2, 1, 2, 3}
    out = set()
    for v in vals:
        out |= {v - 1, v, v + 1}
    return sorted(b for b in out if b >= 0)


@pytest.mark.parametrize("level_bytes", [1, 4 * 91 * 64 * 6])
@pytest.mark.parametrize("nt", NTS)
def test_choose_checkpoint(nt, level_bytes):
    smallest = min(checkpoint_levels(nt, K) for K in range(1, nt + 1))
    for levels in budgets(nt):
        for extra in ((0,) if level_bytes == 1 else (0, level_bytes - 1)):   # a budget between two level counts
            budget = levels * level_bytes + extra
            store_all_fits = (nt + 2) * level_bytes <= budget
            if levels < smallest:
                assert not store_all_fits
                with pytest.raises(ValueError) as e:
                    choose_checkpoint(nt, level_bytes, budget)
                assert str(smallest * level_bytes) in str(e.value)     # states the bytes needed
                continue
            K = choose_checkpoint(nt, level_bytes, budget)
            assert (K is None) == store_all_fits                        # store-all exactly when it fits
            if K is None:
                continue
            assert 1 <= K <= nt
            assert checkpoint_levels(nt, K) * level_bytes <= budget     # the returned K fits
            assert K + 1 >= nt or checkpoint_levels(nt, K + 1) * level_bytes > budget
            # the largest: no larger K below nt fits either
            assert all(checkpoint_levels(nt, k) * level_bytes > budget for k in range(K + 1, nt + 1))


def test_smallest_footprint_is_near_sqrt_2nt():
    # 2 (ceil(nt / K) - 1) + K + 2 lies in [2 nt / K + K, 2 nt / K + K + 2], whose minimum over K is
    # 2 sqrt(2 nt) at K = sqrt(2 nt) (the ceilings make neighbouring K tie)
    for nt in (162, 1000):
        least = min(checkpoint_levels(nt, K) for K in range(1, nt + 1))
        assert 2 * math.sqrt(2 * nt) <= least <= 2 * math.sqrt(2 * nt) + 3
        assert checkpoint_levels(nt, round(math.sqrt(2 * nt))) <= least + 1
    assert checkpoint_levels(1000, 45) == 91                            # 2 (23 - 1) + 45 + 2


def test_choose_checkpoint_rejects_nonsense():
    with pytest.raises(ValueError):
        choose_checkpoint(0, 4, 100)
    with pytest.raises(ValueError):
        choose_checkpoint(10, 0, 100)


def test_operator_options_validate_without_a_device():
    from red_diffeq.solvers.pde import FWIForward
    ctx = dict(n_grid=24, nt=200, dx=10.0, dt=0.001, nbc=10, f=15.0, sz=10, gz=10, ng=24, ns=3)
    assert FWIForward(dict(ctx), "cpu").checkpoint is None
    assert FWIForward(dict(ctx, checkpoint=16), "cpu").checkpoint == 16               # from ctx (a YAML's pde:)
    assert FWIForward(dict(ctx, checkpoint=16), "cpu", checkpoint=8).checkpoint == 8   # the keyword wins
    f = FWIForward(dict(ctx, history_budget_gb=2.0), "cpu", history_budget_gb=0.5)
    assert f.history_budget_gb == 0.5 and f.checkpoint is None
    for bad in (0, -1, "sometimes"):
        with pytest.raises(ValueError):
            FWIForward(dict(ctx), "cpu", checkpoint=bad)
    with pytest.raises(ValueError):
        FWIForward(dict(ctx), "cpu", checkpoint="auto")                   # needs a budget
