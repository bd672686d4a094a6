"""CPU checks of tests/linear_cases.py, the inputs, reference and bar of tests/test_gpu_linear_edges.py: every case
builds and meets the adjacent-difference condition, an fp32 evaluation of the same operation in another summation
order (torch's CPU kernels) passes every bar at every element, and the per-element comparison catches each of seven
kernel mistakes restated on the fp64 reference."""
import math

import pytest
import torch

import linear_cases as C

_CACHE = {}


def case_of(cid):
    if cid not in _CACHE:
        _CACHE[cid] = C.build(cid)
    return _CACHE[cid]


def exceeding(got, case):
    """Per linear, the boolean mask of elements outside the bar (a non-finite element is outside)."""
    return [~((y.double() - ref).abs() <= bar) for y, ref, bar in zip(got, case.ref64, case.bar)]


def test_case_table():
    """The sizes the edge branches need are all there, and each case's route is the documented rule."""
    S = C.CASES
    assert len(C.CASE_IDS) == 6 + 8 + 16 + 4 * (8 + 12 + 3 + 2)
    lin = [s for s in S.values() if s.kind == "lin"]
    assert {(s.B, s.cin, s.rows[0]) for s in lin} == {(1, 1, 1), (3, 63, 5), (2, 64, 4), (2, 65, 7), (2, 200, 9), (1, 513, 3)}
    assert {(s.act_in, s.act_out) for s in lin} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert sum(not s.has_bias[0] for s in lin) == 1
    assert {(s.dim, s.theta) for s in S.values() if s.kind == "emb"} == {(d, t) for d in C.EMB_DIMS for t in C.EMB_THETAS}
    tm = [s for s in S.values() if s.kind == "tm"]
    assert {(s.B, s.dim, s.hid, s.rows[0]) for s in tm} == {(B, *sh) for B in (1, 16, 17, 25) for sh in C.TM_SHAPES}
    for s in tm:
        assert s.route == (C.BATCHED if s.B > 2 * C.TMB else C.PER_SAMPLE)
    lsm = [s for s in S.values() if s.kind == "lsm"]
    for s in lsm:
        want = C.PER_SAMPLE
        if s.B > C.LSB // 2 and s.cin == 256:
            want = C.WDOT
        elif s.B > C.LSB // 2 and s.cin <= 256:
            want = C.BATCHED
        assert s.route == want, (s.B, s.cin)
        assert len(s.rows) <= 32
    for route, sizes in ((C.PER_SAMPLE, {(i, B) for i in (1, 63, 100, 255) for B in (2, 16)} | {(257, 20), (600, 20)}),
                         (C.BATCHED, {(i, B) for i in (1, 63, 100, 255) for B in (17, 33, 35)}),
                         (C.WDOT, {(256, 17), (256, 65), (256, 130)})):
        assert {(s.cin, s.B) for s in lsm if s.route == route} == sizes
        assert {tuple(s.rows) for s in lsm if s.route == route} == {tuple(r) for r, _ in C.LSM_SETS.values()}
    assert [sum(r) for r, _ in C.LSM_SETS.values()] == [1, 17, 65, 63] and len(C.LSM_SETS["n32"][0]) == 32
    assert all(not all(hb) for name, (_, hb) in C.LSM_SETS.items() if name != "r1")      # null biases among them
    assert len(set(C.TM_T)) == 25 and max(C.TM_T) < 64
    sines = [math.sin(t) for t in C.TM_T[1:]]
    assert all(abs(v) > 0.65 for v in sines) and all(a * b < 0 for a, b in zip(sines, sines[1:]))
    w = C.wide_steps(torch.tensor(C.TM_T))
    assert len(set(w.tolist())) == 25 and int(w.max()) == 999 and int(w.min()) == 0
    a, b = C.build(C.CASE_IDS[1]), C.build(C.CASE_IDS[1])
    assert a.x.equal(b.x) and a.salt == b.salt                                           # a pure function of the id


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_case_builds_and_fp32_passes(cid):
    case = case_of(cid)
    s = case.spec
    for ref, bar, rows in zip(case.ref64, case.bar, s.rows if s.kind != "emb" else [s.dim]):
        assert ref.dtype == bar.dtype == torch.float64 and ref.shape == bar.shape == (s.B, rows)
        assert bool((bar > 0).all()) and bool(torch.isfinite(bar).all()) and bool(torch.isfinite(ref).all())
    # the same operation in fp32 on the CPU, torch's summation order: inside every bar, no element excluded
    got, _ = C.evaluate(case, torch.float32)
    assert all(y.dtype == torch.float32 for y in got)
    ratio, j, i = C.worst_ratio(got, case)
    assert ratio <= 1.0, (cid, ratio, j, i)
    assert sum(int(m.sum()) for m in exceeding(got, case)) == 0
    if s.kind == "emb":
        assert bool((case.ref64[0][0, :s.dim // 2] == 0).all()) and bool((case.ref64[0][0, s.dim // 2:] == 1).all())
    else:
        assert C.adjacent_gap(case) >= C.SEP, (cid, C.adjacent_gap(case))
        if s.kind != "tm" and s.cin >= 8:                        # SiLU's tails are among the inputs of every sample
            for v in C.SPECIALS:
                assert bool((case.x == v).any(dim=1).all()), (cid, v)


def test_silu_tail_in_the_reference():
    """silu(-95) in fp64 is -5e-40 (fp32: -95 / inf = -0); the bar's 2^-126 per input covers the difference."""
    x = torch.tensor([-95.0, 95.0, -30.0, 30.0], dtype=torch.float64)
    a = C.silu(x)
    assert -1e-38 < float(a[0]) < 0 and float(a[1]) == 95.0 and abs(float(a[2]) + 30 * math.exp(-30)) < 1e-20
    assert float(torch.nn.functional.silu(x.float())[0]) == 0.0
    assert abs(float(a[0])) < C.TINY


# ------------------------------------------------------------------------------------------------ mutations
def _ref(case, mut=None):
    return [y.clone() for y in C.evaluate(case, torch.float64, mut)[0]]


def m_last_row_unwritten(case):
    got = _ref(case)
    got[-1][:, -1] = float("nan")
    return got


def m_neighbour_bias(case):
    """Row 0 of every linear after the first takes the bias of the previous linear's last row (null: none)."""
    got = _ref(case)
    for j in range(1, len(got)):
        own = case.b[j][0].double() if case.b[j] is not None else 0.0
        prev = case.b[j - 1][-1].double() if case.b[j - 1] is not None else 0.0
        got[j][:, 0] += prev - own
    return got


def m_sample_dup(block):
    def mutate(case):
        got = _ref(case)
        for y in got:
            y[block] = y[block - 1]
        return got
    return mutate


def m_restated(mut):
    return lambda case: _ref(case, mut)


MUTATIONS = [
    ("last_row_unwritten", m_last_row_unwritten,
     ["lsm-B17-in63-r5-1-11", "lsm-B2-in255-r64-1", "lsm-B65-in256-n32", "lsm-B20-in600-r1", "tm-B25-dim260-hid255-out70",
      "lin-B2-in65-out7-ai0-ao1"]),
    ("neighbour_bias", m_neighbour_bias,
     ["lsm-B33-in100-r5-1-11", "lsm-B16-in1-r64-1", "lsm-B130-in256-n32", "lsm-B20-in257-r5-1-11"]),
    ("drop256", m_restated("drop256"),
     ["lsm-B20-in257-r1", "lsm-B20-in600-n32", "lin-B1-in513-out3-ai1-ao1", "tm-B1-dim6-hid257-out5",
      "tm-B17-dim64-hid300-out33"]),
    ("tail_twice", m_restated("tail_twice"),
     ["lsm-B17-in63-r1", "lsm-B2-in255-r5-1-11", "lin-B2-in65-out7-ai0-ao1", "lin-B2-in200-out9-ai1-ao0",
      "tm-B25-dim260-hid255-out70", "tm-B16-dim6-hid257-out5"]),
    ("sample_dup_32", m_sample_dup(C.LSB), ["lsm-B33-in63-r5-1-11", "lsm-B35-in1-n32", "lsm-B33-in255-r64-1"]),
    ("sample_dup_64", m_sample_dup(C.WD_B), ["lsm-B65-in256-r64-1", "lsm-B130-in256-r1"]),
    ("sample_dup_16", m_sample_dup(2 * C.TMB), ["tm-B17-dim6-hid257-out5", "tm-B25-dim4-hid1-out1"]),
    ("no_silu", m_restated("no_silu"), ["lsm-B2-in1-r1", "lin-B3-in63-out5-ai1-ao1", "lsm-B17-in256-r1"]),
    ("swap_halves", m_restated("swap_halves"),
     [c for c in C.CASE_IDS if c.startswith("emb-")] + ["tm-B1-dim4-hid1-out1", "tm-B17-dim260-hid255-out70"]),
]
MUTATION_ROWS = [(name, fn, cid) for name, fn, cids in MUTATIONS for cid in cids]


@pytest.mark.parametrize("name,fn,cid", MUTATION_ROWS, ids=[f"{n}-{c}" for n, _, c in MUTATION_ROWS])
def test_comparison_catches(name, fn, cid):
    """The mistake applied to the fp64 reference's output of the named case: at least one element leaves its bar
    (the unmutated reference has none outside), and worst_ratio reports it."""
    case = case_of(cid)
    assert sum(int(m.sum()) for m in exceeding(_ref(case), case)) == 0
    got = [y.float() for y in fn(case)]
    out = exceeding(got, case)
    assert sum(int(m.sum()) for m in out) >= 1, (name, cid)
    assert C.worst_ratio(got, case)[0] > 1.0
    if name.startswith("sample_dup"):                        # the condition: EVERY element of the sample shows it
        block = int(name.rsplit("_", 1)[1])
        assert all(bool(m[block].all()) for m in out)


def test_fused_case_tables():
    ids = C.fused_lsm_ids()
    assert len(ids) == 18 and len(set(ids)) == 18
    f = C.build_fused_lsm(ids[0])
    assert f.rows[0] == 2 * f.cout and [tuple(w.shape) for w in f.w] == [(r, f.cin) for r in f.rows]
    assert any(b is None for b in f.b)
    ids = C.fused_head_ids()
    assert len(ids) == 12 and len(set(ids)) == 12
    h = C.build_fused_head(ids[-1])
    assert (h.B, h.dim, h.hid, h.out, h.cout, h.k) == (16, 64, 300, 33, 64, 7) and int(h.t.max()) == 999
