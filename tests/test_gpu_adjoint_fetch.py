"""Fetch mode of the persistent adjoint's source/receiver role (rdq_fwi_set_adjoint_fetch).

The role's wave (tests/test_gpu_adjoint_role.py) needs, per step, one receiver residual and one wavelet sample.
Fetch 0 loads an epoch's four of each after the previous epoch's hand-off sweep; fetch 1 loads the residuals a
step ahead: step k issues step k - 1's ahead of its own history prefetch, the epoch's last step the next epoch's
first (the samples stay an epoch ahead), and the epoch after the role's loop (the generic last one) gets its values
as it does after the plain loop.
Only when a value is loaded differs, not which one, so everything a call produces must equal fetch 0 bit for bit
in the same build: seismograms (no-grad and history calls), every history slot, gA, gk_part, gbeta and dL/dv.
Fetch 0 is the parent's kernel text, which the rest of the suite pins.

Grid and helpers of test_gpu_wave_roles.py: 70 x 70 with nbc = 20 -> 110 x 110 padded (3 x 2 tiles of the 96-row
class, forced), two shots, nt = 43: the smallest geometry on which the role runs.  What a wrong index or a value
kept an epoch too long would read has to differ from the right one, so the setup here brings a wavelet of its own
(random: the Ricker's tail is zeros) and asserts that the wavelet and every residual trace differ from sample to
sample at every lag up to an epoch.  Each case asserts the fetch mode the info call reports and, after each run,
the entered-role counter (one wave per workgroup whose interior rows own the source row; the same in both modes).
gbeta is the role's own term, built from both fetched values; gA is non-zero from nt = 2 on (one step: gA == 0).

The cases fail for a wrong fetch: with the step-ahead index off by one every case with a steady epoch (nt >= 5)
fails, with the next epoch's first residual not fetched at the epoch boundary every case with two (nt >= 9)
(profiles/r26/fetch_mutants.txt)."""
import numpy as np
import pytest
import torch

from conftest import vnorm
from test_gpu_wave_roles import HP, NAMES, NBC, NX, NZ, T, _own, _run

pytestmark = pytest.mark.gpu

TILES_X = 3                                                   # ceil(110 / (64 - 16))
NS = 2
DEFAULT_FETCH = 1                                             # RDQ_ADJ_FETCH (csrc/fwi.hip)


def _setup(cuda, nt, B, srow, rrow):
    """test_gpu_wave_roles._setup with a wavelet whose samples all differ (no Ricker: any nt is legal)."""
    from red_diffeq.solvers.pde import FWIForward
    from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize
    from red_diffeq.utils.synthetic import make_model
    rng = np.random.default_rng(29)
    wav = rng.standard_normal(nt)
    ctx = dict(n_grid=NX, nt=nt, dx=10.0, dt=0.001, nbc=NBC, f=60.0, sz=10 * (srow - NBC), gz=10 * (rrow - NBC),
               ng=NX, ns=NS)
    fwi = FWIForward(dict(ctx), "cuda", sample_temporal=1, normalize=True, v_denorm_func=v_denormalize,
                     s_norm_func=s_normalize_none, wavelet=wav)
    v = torch.from_numpy(vnorm(make_model("curvefault", NZ, NX, seed=17, batch=B))).to(cuda)
    plan = fwi._plan(NZ, NX, v.device)
    sz = plan.sizes(B)
    assert (sz.Hp, sz.Wp, sz.nrec) == (HP, HP, nt)
    ds = rng.standard_normal((B, plan.ns, sz.nrec, plan.ng)).astype(np.float32)
    w32 = wav.astype(np.float32)
    for lag in range(1, min(T, nt - 1) + 1):                  # what a wrong fetch would read is another value
        assert (w32[lag:] != w32[:-lag]).all() and (ds[:, :, lag:] != ds[:, :, :-lag]).all(), lag
    assert (w32 != 0).all() and (ds != 0).all()
    return fwi, plan, v, torch.from_numpy(ds).to(cuda)


def _both_fetches(plan, v, B, dseis, role=True, run=_run, counted=True):
    """Fetch 0 and fetch 1 in the same build.  `role`: the role runs (else fetch 0 is reported whatever is set and
    no wave counts itself); all seven outputs equal bit for bit.  Returns the fetch-1 outputs."""
    out = {}
    for mode in (0, 1):
        plan.set_adjoint_fetch(mode)
        info = plan.launch_info(B)
        assert info["adj_role"] == int(role) and info["adj_fetch"] == (mode if role else 0), info
        out[mode] = run(plan, v, B, dseis)
        if counted:
            assert plan.adjoint_role_waves() == (TILES_X * NS * B if role else 0), (mode, plan.adjoint_role_waves())
    for name, a, b in zip(NAMES, out[0], out[1]):
        assert torch.equal(a, b), name
    assert torch.equal(out[1][0], out[1][1])                  # the no-grad call records the same seismograms
    return out[1]


def _not_vacuous(got, nt=43):
    assert float(got[1].abs().max()) > 0 and float(got[2][2:].abs().max()) > 0   # seismograms, history
    gb = got[5].abs()                                         # gbeta: the role's own term (every shot's, given an epoch)
    assert float(gb.min() if nt > T else gb.max()) > 0
    if nt >= 2:
        assert float(got[3].abs().max()) > 0                  # gA


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("row", [22, 23, 24, 25, 26, 27])
def test_adjoint_fetch_bitwise_every_pair_and_half(cuda, row, overlap):
    """Rows 0 .. 5 of wave 5 of tile row 0: pairs 0, 1 (boundary pairs: the residual goes in ahead of the wave's
    hand-off to its neighbours) and 2, both halves; both hand-off overlap modes (a kernel each)."""
    assert _own(row, 12, 6) == (0, 5, row - 22, True)
    fwi, plan, v, dseis = _setup(cuda, 43, 1, row, row)
    plan.set_persistent(12)
    plan.set_handoff_overlap(0, overlap)
    info = plan.launch_info(1)
    assert info["adj_class"] == 12 and info["adj_T"] == T and info["adj_overlap"] == overlap, info
    assert info["adj_role_pair"] == min(row - 22, 27 - row), info
    _not_vacuous(_both_fetches(plan, v, 1, dseis))


@pytest.mark.parametrize("nt", [1, 2, 3, 4, 5, 8, 9, 12])
def test_adjoint_fetch_bitwise_short_records(cuda, nt):
    """The record ends inside the first epoch (the role's loop is entered and left at once: its last-epoch values
    are fetched again), at an epoch boundary, one step past it, and after two steady epochs."""
    assert _own(23, 12, 6) == (0, 5, 1, True)
    fwi, plan, v, dseis = _setup(cuda, nt, 1, 23, 23)
    plan.set_persistent(12)
    _not_vacuous(_both_fetches(plan, v, 1, dseis), nt)


def test_adjoint_fetch_bitwise_two_models(cuda):
    assert _own(22, 12, 6) == (0, 5, 0, True)
    fwi, plan, v, dseis = _setup(cuda, 43, 2, 22, 22)
    plan.set_persistent(12)
    assert plan.launch_info(2)["adj_launches"] == 1           # one launch: the counter holds both models' waves
    _not_vacuous(_both_fetches(plan, v, 2, dseis))


def test_adjoint_fetch_without_the_role(cuda):
    """Source and receiver rows in two waves: no role, fetch 0 reported whatever is set, the same bits."""
    s, r = _own(22, 12, 6), _own(40, 12, 6)
    assert s[0] == r[0] and s[1] != r[1]
    fwi, plan, v, dseis = _setup(cuda, 43, 1, 22, 40)
    plan.set_persistent(12)
    assert plan.launch_info(1)["adj_class"] == 12
    got = _both_fetches(plan, v, 1, dseis, role=False)
    _not_vacuous(got)
    plan.set_adjoint_role(0)                                  # and with the role switched off
    assert plan.launch_info(1)["adj_fetch"] == 0
    for name, a, b in zip(NAMES, got, _run(plan, v, 1, dseis)):
        assert torch.equal(a, b), name


def test_adjoint_fetch_checkpointed_gradient(cuda):
    """The checkpointed gradient (K = 16) on the same plan: its launches are the chunked kernels, so both settings
    give the same bits, and its dL/dv stays within smoke()'s bar for the recurrence adjoint (5e-6 rel-L2) of the
    store-all persistent gradient with the step-ahead fetch, the seismograms bit for bit."""
    K = 16

    def run(plan, v, B, dseis):
        coeffs, vstat = plan.coeffs(v, 0)
        seis, ckpt = plan.forward_ckpt(coeffs, B, K)
        gA, gk, gb = plan.adjoint_ckpt(coeffs, ckpt, dseis, B, K)
        g = plan.finalize(coeffs, vstat, gA, gk, gb, B, 0)
        plan.status()
        sz = plan.sizes(B)
        cells = ckpt.view(-1, B * plan.ns, sz.Hp, sz.ld)[..., :sz.Wp].clone()
        return seis, seis, cells, gA, gk, gb, g

    assert _own(24, 12, 6) == (0, 5, 2, True)
    fwi, plan, v, dseis = _setup(cuda, 43, 1, 24, 24)
    plan.set_persistent(12)
    plan.set_tuning(4, 4, 1)                                  # one chain: the chunked launches' graphs are captured with it
    got = _both_fetches(plan, v, 1, dseis, run=run, counted=False)
    assert float(got[3].abs().max()) > 0 and float(got[5].abs().min()) > 0
    assert plan.launch_info(1)["adj_fetch"] == 1
    ref = _run(plan, v, 1, dseis)                             # the store-all persistent gradient, fetch 1
    assert plan.adjoint_role_waves() == TILES_X * NS
    assert torch.equal(got[1], ref[1])
    rel = float((got[6].double() - ref[6].double()).norm() / ref[6].double().norm())
    print(f"checkpointed vs store-all persistent (fetch 1) dL/dv: rel-L2 {rel:.3e} (bar 5e-6)")
    assert float(ref[6].abs().max()) > 0 and rel < 5e-6, rel


def test_adjoint_fetch_setter_contract(cuda):
    """Modes 0 / 1, default 1; a rejected call changes nothing; the role's own setting stays as it was and decides
    whether the fetch mode is reported; flipping the mode with cached graphs in the plan (chunked calls with one
    launch chain: one captured, one replayed) drops them, and calls after it give the same bits."""
    B = 1
    assert _own(24, 12, 6) == (0, 5, 2, True)
    fwi, plan, v, dseis = _setup(cuda, 43, B, 24, 24)
    plan.set_persistent(12)
    plan.set_tuning(4, 4, 1)

    def modes():
        info = plan.launch_info(B)
        return info["adj_fetch"], info["adj_role"], info["adj_role_pair"], info["adj_roles"]

    assert modes() == (DEFAULT_FETCH, 1, 2, 1)                # the defaults
    plan.set_adjoint_fetch(1)
    ref = _run(plan, v, B, dseis)
    assert plan.adjoint_role_waves() == TILES_X * NS
    for bad in (2, -1, 3, 12):
        with pytest.raises(Exception):
            plan.set_adjoint_fetch(bad)
        assert modes() == (1, 1, 2, 1), bad
    plan.set_adjoint_role(0)
    assert modes() == (0, 0, -1, 1)                           # no role, no fetch mode of its own
    plan.set_adjoint_role(1)
    assert modes() == (1, 1, 2, 1)                            # the setting outlives the detour
    plan.set_wave_roles(0, 0)
    assert modes() == (0, 0, -1, 0)
    plan.set_wave_roles(0, 1)
    plan.set_adjoint_fetch(0)
    assert modes() == (0, 1, 2, 1)                            # the role's setting untouched
    plan.set_adjoint_fetch(1)
    plan.set_persistent(False)
    assert not plan.launch_info(B)["adj_persistent"] and modes()[:3] == (0, 0, -1)
    first = _run(plan, v, B, dseis)                           # chunked: captures the plan's graphs
    replay = _run(plan, v, B, dseis)                          # replays them
    plan.set_adjoint_fetch(0)                                 # drops them
    again = _run(plan, v, B, dseis)                           # captured anew
    for name, a, b, c in zip(NAMES, first, replay, again):
        assert torch.equal(a, b) and torch.equal(a, c), name
    assert torch.equal(first[1], ref[1]) and torch.equal(first[2], ref[2])  # chunked forward = persistent
    plan.set_persistent(12)
    assert modes() == (0, 1, 2, 1)
    off = _run(plan, v, B, dseis)
    assert plan.adjoint_role_waves() == TILES_X * NS          # the role runs in both fetch modes
    for name, a, b in zip(NAMES, ref, off):
        assert torch.equal(a, b), name

