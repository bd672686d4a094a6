"""Source role of the persistent FWI kernels (rdq_fwi_set_source_role).

With the role on, at 4 steps per epoch and 6 rows per wave of the 96-row regions, the wave whose rows own
the source row, that row being the receiver row too, runs every epoch but the last in a loop of its own:
the plain loop's body plus the row's own work, with the row's pair a compile-time constant (one body per
pair), and the waves with neither row a guard-free loop.  The role is the forward's: every form of it tried
in the adjoint spilled more registers than that kernel does now, so the adjoint accepts mode 0 only and
reports 0; its outputs are compared all the same.  The hand-off, the mailbox exchange and every cell's
operations and their order are the same text, so everything a call produces must equal the role off bit for
bit in the same build: seismograms (no-grad and history calls), every history slot, gA, gk_part, gbeta and
dL/dv.  The role off itself is what the rest of the suite pins.

Grid and helpers of test_gpu_wave_roles.py: 70 x 70 with nbc = 20 -> 110 x 110 padded, two shots, nt = 43,
the 96-row class forced.  Every case asserts through launch_info which mode runs before it runs.  A record
of one step has gA == 0 identically (P_0 = 0: the gradient's d term of step k = 1 is zero), so gA is
asserted non-zero from nt = 2 on."""
import pytest
import torch

from test_gpu_wave_roles import NAMES, _own, _run, _setup

pytestmark = pytest.mark.gpu


def _both_modes(plan, v, B, dseis, runs, run=_run):
    """Role 0 and role 1 in the same build: `runs` = the forward's mode launch_info must report with the
    role set; all seven outputs equal bit for bit.  Returns the role-on outputs."""
    out = {}
    for mode in (0, 1):
        plan.set_source_role(mode, 0)
        info = plan.launch_info(B)
        assert (info["fwd_src_role"], info["adj_src_role"]) == ((runs, 0) if mode else (0, 0)), info
        out[mode] = run(plan, v, B, dseis)
    for name, a, b in zip(NAMES, out[0], out[1]):
        assert torch.equal(a, b), name
    assert torch.equal(out[1][0], out[1][1])                  # the no-grad call records the same seismograms
    return out[1]


def _not_vacuous(got, nt=43):
    assert float(got[2][2:].abs().max()) > 0                  # history
    if nt >= 2:
        assert float(got[3].abs().max()) > 0                  # gA


@pytest.mark.parametrize("row", [22, 23, 24, 25, 26, 27])
def test_source_role_bitwise_every_pair_and_half(cuda, row):
    """Rows 0 .. 5 of wave 5 of tile row 0: pairs 0, 1, 2 (mirrored: {0, 5}, {1, 4}, {2, 3}), both halves."""
    assert _own(row, 12, 6) == (0, 5, row - 22, True)
    fwi, plan, v, dseis = _setup(cuda, 43, 1, row, row)
    plan.set_persistent(12)
    info = plan.launch_info(1)
    assert info["fwd_class"] == 12 and info["adj_class"] == 12 and info["fwd_T"] == 4 and info["adj_T"] == 4
    _not_vacuous(_both_modes(plan, v, 1, dseis, 1))


@pytest.mark.parametrize("case", ["rows_22_23", "rows_22_40", "halo_copy_84", "sample_temporal_3", "rows_per_wave_8",
                                  "class_16", "class_8", "depth_3", "exact_adjoint"])
def test_source_role_fallbacks(cuda, case):
    """Launches without a source/receiver wave report mode 0 and give the same bits whatever is set."""
    rows = {"rows_22_23": (22, 23), "rows_22_40": (22, 40), "halo_copy_84": (84, 84)}.get(case, (22, 22))
    fwi, plan, v, dseis = _setup(cuda, 43, 1, *rows, st=3 if case == "sample_temporal_3" else 1)
    runs, cls = 0, 12
    if case == "halo_copy_84":                                # own row of tile row 1, halo copy in tile row 0
        assert _own(84, 12, 6)[0] == 1
    elif case == "rows_per_wave_8":
        plan.set_rows_per_wave(8, 8)
    elif case in ("class_16", "class_8"):
        cls = int(case.split("_")[1])
    plan.set_persistent(cls)
    if case == "depth_3":
        plan.set_tuning(3, 3, 1)
    elif case == "exact_adjoint":
        plan.set_variant(adj_exact=True)
        runs = 1                                              # the forward still qualifies
    info = plan.launch_info(1)
    assert info["fwd_class"] == cls, info
    _not_vacuous(_both_modes(plan, v, 1, dseis, runs))


@pytest.mark.parametrize("nt", [1, 2, 3, 4, 5, 8, 9, 12])
def test_source_role_bitwise_short_records(cuda, nt):
    """No steady epoch (nt <= 4), one, two, and every tail length."""
    fwi, plan, v, dseis = _setup(cuda, nt, 1, 24, 24)
    plan.set_persistent(12)
    _not_vacuous(_both_modes(plan, v, 1, dseis, 1), nt)


def test_source_role_bitwise_two_models(cuda):
    fwi, plan, v, dseis = _setup(cuda, 43, 2, 22, 22)
    plan.set_persistent(12)
    _not_vacuous(_both_modes(plan, v, 2, dseis, 1))


def test_source_role_checkpointed_gradient(cuda):
    """The checkpointed gradient (K = 16) on the same plan: role on equals role off."""
    K = 16

    def run(plan, v, B, dseis):
        coeffs, vstat = plan.coeffs(v, 0)
        seis, ckpt = plan.forward_ckpt(coeffs, B, K)
        gA, gk, gb = plan.adjoint_ckpt(coeffs, ckpt, dseis, B, K)
        g = plan.finalize(coeffs, vstat, gA, gk, gb, B, 0)
        plan.status()
        sz = plan.sizes(B)                                    # the stored levels' cells (the row padding is not written)
        cells = ckpt.view(-1, B * plan.ns, sz.Hp, sz.ld)[..., :sz.Wp].clone()
        return seis, seis, cells, gA, gk, gb, g

    fwi, plan, v, dseis = _setup(cuda, 43, 1, 24, 24)
    plan.set_persistent(12)
    got = _both_modes(plan, v, 1, dseis, 1, run=run)
    assert float(got[2].abs().max()) > 0 and float(got[3].abs().max()) > 0
    plan.set_source_role(1, 0)
    ref = _run(plan, v, 1, dseis)                             # the store-all persistent gradient, role on
    assert torch.equal(got[1], ref[1])


def test_source_role_setter_contract(cuda):
    """The forward's modes are 0 / 1, the adjoint's 0; a rejected call changes nothing; the wave-role words of
    launch_info stay as they were; flipping the mode with cached graphs in the plan (chunked calls: one
    captured, one replayed) drops them, and calls after it give the same bits."""
    B = 1
    fwi, plan, v, dseis = _setup(cuda, 43, B, 24, 24)
    plan.set_persistent(12)
    info = plan.launch_info(B)
    assert (info["fwd_src_role"], info["adj_src_role"]) == (1, 0)              # the defaults
    assert info["fwd_roles"] == 0 and info["adj_roles"] == 1
    ref = _run(plan, v, B, dseis)
    for bad in ((2, 0), (0, 1), (1, 1), (0, 2), (-1, 0), (0, -1), (2, 2)):
        with pytest.raises(Exception):
            plan.set_source_role(*bad)
        info = plan.launch_info(B)
        assert (info["fwd_src_role"], info["adj_src_role"]) == (1, 0), (bad, info)
    assert info["fwd_roles"] == 0 and info["adj_roles"] == 1
    plan.set_wave_roles(0, 0)                                 # the two settings are independent
    info = plan.launch_info(B)
    assert (info["fwd_src_role"], info["adj_src_role"]) == (1, 0) and info["adj_roles"] == 0
    got = _run(plan, v, B, dseis)
    for name, a, b in zip(NAMES, ref, got):
        assert torch.equal(a, b), name
    plan.set_wave_roles(0, 1)
    plan.set_persistent(False)
    info = plan.launch_info(B)
    assert not info["fwd_persistent"] and (info["fwd_src_role"], info["adj_src_role"]) == (0, 0)
    first = _run(plan, v, B, dseis)                           # chunked: captures the plan's graphs
    replay = _run(plan, v, B, dseis)                          # replays them
    plan.set_source_role(0, 0)                                # drops them
    again = _run(plan, v, B, dseis)                           # captured anew
    for name, a, b, c in zip(NAMES, first, replay, again):
        assert torch.equal(a, b) and torch.equal(a, c), name
    assert torch.equal(first[1], ref[1]) and torch.equal(first[2], ref[2])  # chunked forward = persistent
    plan.set_persistent(12)
    info = plan.launch_info(B)
    assert (info["fwd_src_role"], info["adj_src_role"]) == (0, 0)              # the setting outlives the detour
    off = _run(plan, v, B, dseis)
    for name, a, b in zip(NAMES, ref, off):
        assert torch.equal(a, b), name
