"""Source/receiver role of the persistent adjoint (rdq_fwi_set_adjoint_role).

With the role on, at 4 steps per epoch and 6 rows per wave of the 96-row regions, in the recurrence adjoint with
wave roles on, the wave whose rows own the source row, that row being the receiver row too, runs every epoch but
the last in a loop of its own: the plain loop's body plus the row's own work (the receiver residual's add, the
source term's undo and the gbeta term of the gradient, the next epoch's sample and residual loads), with the row's
pair a template parameter of the kernel the host picks.  The hand-off, the mailbox exchange and every cell's
operations and their order are the same text, so everything a call produces must equal the role off bit for bit in
the same build: seismograms (no-grad and history calls), every history slot, gA, gk_part, gbeta and dL/dv.  The
role off itself is what the rest of the suite pins.

Grid and helpers of test_gpu_wave_roles.py: 70 x 70 with nbc = 20 -> 110 x 110 padded (3 x 2 tiles of the 96-row
class), two shots, nt = 43, the 96-row class forced.  Every case asserts where its rows fall (`_own`) and which
mode and pair the info call reports before it runs, and after each run the entered-role counter: the waves that
took the role's loop count themselves once per launch, one per workgroup whose interior rows own the source row
(tiles_x x shots x models), 0 where the role does not run.  A record of one step has gA == 0 identically, so gA is
asserted non-zero from nt = 2 on."""
import pytest
import torch

from test_gpu_wave_roles import NAMES, _own, _run, _setup

TILES_X = 3                                                   # ceil(110 / (64 - 16))
NS = 2


def _pair(r):
    """Mirrored row pair of row-in-wave r at 6 rows per wave: {0, 5}, {1, 4}, {2, 3}."""
    return r if r < 3 else 5 - r


def _both_modes(plan, v, B, dseis, pair, run=_run, counted=True):
    """Role 0 and role 1 in the same build.  `pair` = the pair the info call must report with the role set (-1:
    the role does not run, mode 0 reported); all seven outputs equal bit for bit; the entered-role counter after
    each run (`counted`: the run ends with a persistent adjoint call).  Returns the role-on outputs."""
    out = {}
    assert plan.launch_info(B)["adj_role"] == (1 if pair >= 0 else 0)           # the default is on
    for mode in (0, 1):
        plan.set_adjoint_role(mode)
        info = plan.launch_info(B)
        want = (1, pair) if mode and pair >= 0 else (0, -1)
        assert (info["adj_role"], info["adj_role_pair"]) == want, info
        assert info["adj_src_role"] == 0, info
        out[mode] = run(plan, v, B, dseis)
        if counted:
            assert plan.adjoint_role_waves() == (TILES_X * NS * B if want[0] else 0), (mode, plan.adjoint_role_waves())
    for name, a, b in zip(NAMES, out[0], out[1]):
        assert torch.equal(a, b), name
    assert torch.equal(out[1][0], out[1][1])                  # the no-grad call records the same seismograms
    return out[1]


def _not_vacuous(got, nt=43):
    assert float(got[2][2:].abs().max()) > 0                  # history
    if nt >= 2:
        assert float(got[3].abs().max()) > 0                  # gA
    if nt >= 37:                                              # (the 37-sample wavelet: samples at every late step)
        assert float(got[5].abs().max()) > 0                  # gbeta: the role's own term


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("row", [22, 23, 24, 25, 26, 27])
def test_adjoint_role_bitwise_every_pair_and_half(cuda, row, overlap):
    """Rows 0 .. 5 of wave 5 of tile row 0: pairs 0, 1, 2, both halves; both hand-off overlap modes (a kernel
    each)."""
    assert _own(row, 12, 6) == (0, 5, row - 22, True)
    fwi, plan, v, dseis = _setup(cuda, 43, 1, row, row)
    plan.set_persistent(12)
    plan.set_handoff_overlap(0, overlap)
    info = plan.launch_info(1)
    assert info["fwd_class"] == 12 and info["adj_class"] == 12 and info["fwd_T"] == 4 and info["adj_T"] == 4
    assert info["adj_overlap"] == overlap and info["adj_roles"] == 1
    _not_vacuous(_both_modes(plan, v, 1, dseis, _pair(row - 22)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rows_22_23", "rows_22_40", "halo_copy_84", "sample_temporal_3", "rows_per_wave_8",
                                  "class_16", "class_8", "depth_3", "exact_adjoint", "wave_roles_off"])
def test_adjoint_role_fallbacks(cuda, case):
    """Launches without a source/receiver wave of the role's kind report mode 0, count no wave and give the same
    bits whatever is set."""
    rows = {"rows_22_23": (22, 23), "rows_22_40": (22, 40), "halo_copy_84": (84, 84)}.get(case, (22, 22))
    fwi, plan, v, dseis = _setup(cuda, 43, 1, *rows, st=3 if case == "sample_temporal_3" else 1)
    cls, rw = 12, 6
    if case == "halo_copy_84":                                # own row of tile row 1, halo copy in tile row 0
        assert _own(84, 12, 6)[0] == 1
    elif case == "rows_per_wave_8":
        rw = 8
        plan.set_rows_per_wave(8, 8)
    elif case in ("class_16", "class_8"):
        cls = int(case.split("_")[1])
    plan.set_persistent(cls)
    if case == "depth_3":
        plan.set_tuning(3, 3, 1)
    elif case == "exact_adjoint":
        plan.set_variant(adj_exact=True)
    elif case == "wave_roles_off":
        plan.set_wave_roles(0, 0)
    s, r = _own(rows[0], cls, rw), _own(rows[1], cls, rw)     # each row is one region's own row
    if case == "rows_22_23":
        assert s[:2] == r[:2] and s[2] != r[2]                # one wave, two rows
    elif case == "rows_22_40":
        assert s[0] == r[0] and s[1] != r[1]                  # two waves
    else:
        assert s == r
    info = plan.launch_info(1)
    assert info["fwd_class"] == cls and info["adj_class"] == cls, info
    _not_vacuous(_both_modes(plan, v, 1, dseis, -1))


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 2, 3, 4, 5, 8, 9, 12])
def test_adjoint_role_bitwise_short_records(cuda, nt):
    """No steady epoch (nt <= 4: the wave enters the role's loop and leaves it at once), one, two, and every tail
    length."""
    assert _own(24, 12, 6) == (0, 5, 2, True)
    fwi, plan, v, dseis = _setup(cuda, nt, 1, 24, 24)
    plan.set_persistent(12)
    _not_vacuous(_both_modes(plan, v, 1, dseis, 2), nt)


@pytest.mark.gpu
def test_adjoint_role_bitwise_two_models(cuda):
    assert _own(22, 12, 6) == (0, 5, 0, True)
    fwi, plan, v, dseis = _setup(cuda, 43, 2, 22, 22)
    plan.set_persistent(12)
    assert plan.launch_info(2)["adj_launches"] == 1           # one launch: the counter holds both models' waves
    _not_vacuous(_both_modes(plan, v, 2, dseis, 0))


@pytest.mark.gpu
def test_adjoint_role_checkpointed_gradient(cuda):
    """The checkpointed gradient (K = 16) on the same plan equals the store-all gradient, whatever the role's
    setting.  Its launches are the chunked kernels (no wave enters the role's loop), so it is held against two
    store-all runs of the plan:
      the chunked one, same kernels and same finalize, with tests/test_gpu_checkpoint.py's bars: seismograms, gA
        and gbeta bit for bit, the gk sums to 1e-12 (fp64 partial sums in another order), dL/dv to 1e-6 rel-L2;
      the persistent one with the role on, the gradient this file is about.  Its adjoint is the recurrence, the
        chunked one runs the oracle's operation order, so the bar between them is the one smoke() holds the
        recurrence adjoint to against the oracle: 5e-6 rel-L2 of dL/dv; the seismograms bit for bit."""
    K = 16

    def run(plan, v, B, dseis):
        coeffs, vstat = plan.coeffs(v, 0)
        seis, ckpt = plan.forward_ckpt(coeffs, B, K)
        gA, gk, gb = plan.adjoint_ckpt(coeffs, ckpt, dseis, B, K)
        g = plan.finalize(coeffs, vstat, gA, gk, gb, B, 0)
        plan.status()
        sz = plan.sizes(B)                                    # the stored levels' cells (the row padding is not written)
        cells = ckpt.view(-1, B * plan.ns, sz.Hp, sz.ld)[..., :sz.Wp].clone()
        assert plan.adjoint_role_waves() == 0                 # (before any persistent adjoint call of this plan)
        return seis, seis, cells, gA, gk, gb, g

    assert _own(24, 12, 6) == (0, 5, 2, True)
    fwi, plan, v, dseis = _setup(cuda, 43, 1, 24, 24)
    plan.set_persistent(12)
    plan.set_tuning(4, 4, 1)                                  # one chain: the chunked launches' graphs are captured with it
    got = _both_modes(plan, v, 1, dseis, 2, run=run, counted=False)
    assert float(got[2].abs().max()) > 0 and float(got[3].abs().max()) > 0

    def rel_l2(a, b):
        a, b = a.double(), b.double()
        return float((a - b).norm() / b.norm())

    plan.set_adjoint_role(1)
    ref = _run(plan, v, 1, dseis)                             # the store-all persistent gradient, role on
    assert plan.adjoint_role_waves() == TILES_X * NS
    assert torch.equal(got[1], ref[1])
    rel = rel_l2(got[6], ref[6])
    print(f"checkpointed vs store-all persistent dL/dv: rel-L2 {rel:.3e} (bar 5e-6)")
    assert float(ref[6].abs().max()) > 0 and rel < 5e-6, rel
    plan.set_persistent(False)                                # the store-all chunked run of the same plan
    assert not plan.launch_info(1)["adj_persistent"] and plan.launch_info(1)["adj_role"] == 0
    sa = _run(plan, v, 1, dseis)
    sz = plan.sizes(1)

    def cells(gA):
        return gA.view(1, plan.ns, sz.Hp, sz.ld)[..., :sz.Wp]

    assert torch.equal(got[1], sa[1]), "seis"
    assert torch.equal(cells(got[3]), cells(sa[3])), "gA"
    assert torch.equal(got[5], sa[5]), "gbeta"
    gk_ck, gk_sa = got[4].view(1, -1).sum(1), sa[4].view(1, -1).sum(1)
    krel = float(((gk_ck - gk_sa).abs() / gk_sa.abs()).max())
    grel = rel_l2(got[6], sa[6])
    print(f"checkpointed vs store-all chunked: gk rel {krel:.3e} (bar 1e-12), dL/dv rel-L2 {grel:.3e} (bar 1e-6)")
    assert krel <= 1e-12 and grel < 1e-6, (krel, grel)


@pytest.mark.gpu
def test_adjoint_role_setter_contract(cuda):
    """Modes 0 / 1; a rejected call changes nothing; the wave-role and source-role settings stay as they were and
    theirs leave this one alone; flipping the mode with cached graphs in the plan (chunked calls with one launch
    chain: one captured, one replayed) drops them, and calls after it give the same bits."""
    B = 1
    assert _own(24, 12, 6) == (0, 5, 2, True)
    fwi, plan, v, dseis = _setup(cuda, 43, B, 24, 24)
    plan.set_persistent(12)
    plan.set_tuning(4, 4, 1)                                  # one chain: the graphs below are captured with it

    def modes():
        info = plan.launch_info(B)
        return info["adj_role"], info["adj_role_pair"], info["fwd_src_role"], info["adj_src_role"], info["adj_roles"]

    assert modes() == (1, 2, 1, 0, 1)                         # the defaults
    ref = _run(plan, v, B, dseis)
    assert plan.adjoint_role_waves() == TILES_X * NS
    for bad in (2, -1, 3, 12):
        with pytest.raises(Exception):
            plan.set_adjoint_role(bad)
        assert modes() == (1, 2, 1, 0, 1), bad
    for bad in ((0, 1), (1, 1)):                              # the source role's adjoint mode stays 0 only
        with pytest.raises(Exception):
            plan.set_source_role(*bad)
    with pytest.raises(Exception):
        plan.set_wave_roles(0, 2)
    assert modes() == (1, 2, 1, 0, 1)
    plan.set_adjoint_role(0)
    assert modes() == (0, -1, 1, 0, 1)                        # the other two settings untouched
    plan.set_source_role(0, 0)
    plan.set_adjoint_role(1)
    assert modes() == (1, 2, 0, 0, 1)                         # the forward's role off: the adjoint's still runs
    plan.set_source_role(1, 0)
    plan.set_wave_roles(0, 0)
    assert modes() == (0, -1, 1, 0, 0)                        # it needs the wave roles
    plan.set_wave_roles(0, 1)
    assert modes() == (1, 2, 1, 0, 1)
    plan.set_persistent(False)
    info = plan.launch_info(B)
    assert not info["adj_persistent"] and modes()[:2] == (0, -1)
    first = _run(plan, v, B, dseis)                           # chunked: captures the plan's graphs
    replay = _run(plan, v, B, dseis)                          # replays them
    plan.set_adjoint_role(0)                                  # drops them
    again = _run(plan, v, B, dseis)                           # captured anew
    for name, a, b, c in zip(NAMES, first, replay, again):
        assert torch.equal(a, b) and torch.equal(a, c), name
    assert torch.equal(first[1], ref[1]) and torch.equal(first[2], ref[2])  # chunked forward = persistent
    plan.set_persistent(12)
    assert modes() == (0, -1, 1, 0, 1)                        # the setting outlives the detour
    off = _run(plan, v, B, dseis)
    assert plan.adjoint_role_waves() == 0
    for name, a, b in zip(NAMES, ref, off):
        assert torch.equal(a, b), name


def test_host_pair_of_every_row_matches_the_region_geometry():
    """Host only: the pair the host computes for a padded row equals that of the row's own slot in the kernels'
    region geometry (`_own`: tile row, wave, row in wave), for every row of a 110- and a 310-row padded grid."""
    import test_gpu_wave_roles as geo
    from red_diffeq import _hip
    lib = _hip.load_library()
    assert lib.rdq_fwi_role_row_pair(-1) == -10001
    saved = geo.HP
    try:
        for hp in (110, 310):
            geo.HP = hp
            for row in range(hp):
                ty, w, r, own = geo._own(row, 12, 6)
                assert own and lib.rdq_fwi_role_row_pair(row) == _pair(r), (hp, row, ty, w, r)
    finally:
        geo.HP = saved
