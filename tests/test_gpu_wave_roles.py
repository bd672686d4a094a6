"""Wave roles of the persistent FWI kernels (rdq_fwi_set_wave_roles).

With roles on, a wave of the (recurrence) adjoint whose rows hold neither the source row nor the receiver
row runs every epoch but the last in a loop with the per-step source / receiver / end-of-record tests
compiled out; the hand-off, the mailbox exchange and every cell's arithmetic are the same text, so
everything a call produces must equal roles off bit for bit in the same build: seismograms (no-grad and
history calls), every history slot, gA, gk_part, gbeta and dL/dv.  Roles off itself is what the rest of
the suite pins.  The forward kept no role split (it measured slower): its mode is 0, and its outputs are
compared all the same.

Grid (that of test_gpu_handoff_overlap.py): 70 x 70 with nbc = 20 -> 110 x 110 padded: 3 x 2 tiles of
the 96-row class (3 x 3 of the 64-row classes), periodic wrap in both directions, two shots with their
sources in different tiles.  The cases put the source row and the receiver row where a role split can
go wrong; `_slots` restates the kernels' region geometry (PT_REGION_GEOM) and each case asserts where
its rows fall before it runs.  Short records need a wavelet that fits: f = 60 Hz (37 samples) from
nt = 37, 600 Hz (3 samples) from nt = 3, 1500 Hz (one sample: a spike) below."""
import numpy as np
import pytest
import torch

from conftest import ctx_of, load_golden, vnorm

pytestmark = pytest.mark.gpu

NZ = NX = 70
NBC, HP, T = 20, 110, 4


def _shape(cls, rw):
    """(region rows, rows per wave) of region class `cls` at `rw` rows per wave (fwd_pt_T / adj_pt_T)."""
    return (96, rw) if cls == 12 else (64, 4 if cls == 16 else 8)


def _slots(row, cls, rw):
    """Every (tile row ty, wave, row in wave, own) at which padded row `row` sits in a region."""
    RH, R = _shape(cls, rw)
    H = 2 * T
    IH = RH - 2 * H
    out = []
    for ty in range(-(-HP // IH)):
        for rr in range(RH):
            uz = ty * IH - H + rr
            if uz % HP == row:                              # wrap_row
                out.append((ty, rr // R, rr % R, H <= rr < RH - H and uz < HP))
    return out


def _own(row, cls, rw):
    own = [s for s in _slots(row, cls, rw) if s[3]]
    assert len(own) == 1, own                              # every padded row is one region's own row
    return own[0]


def _all_halo(ty, w, cls, rw):
    RH, R = _shape(cls, rw)
    H = 2 * T
    return not any(H <= rr < RH - H and ty * (RH - 2 * H) - H + rr < HP for rr in range(w * R, w * R + R))


def _boundary(r, R):
    return r in (0, 1, R - 2, R - 1)


def _setup(cuda, nt, B, srow=22, rrow=23, st=1):
    from red_diffeq.solvers.pde import FWIForward
    from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize
    from red_diffeq.utils.synthetic import make_model
    f = 60.0 if nt >= 37 else 600.0 if nt >= 3 else 1500.0
    ctx = dict(n_grid=NX, nt=nt, dx=10.0, dt=0.001, nbc=NBC, f=f, sz=10 * (srow - NBC), gz=10 * (rrow - NBC),
               ng=NX, ns=2)
    fwi = FWIForward(dict(ctx), "cuda", sample_temporal=st, normalize=True, v_denorm_func=v_denormalize,
                     s_norm_func=s_normalize_none)
    v = torch.from_numpy(vnorm(make_model("curvefault", NZ, NX, seed=17, batch=B))).to(cuda)
    plan = fwi._plan(NZ, NX, v.device)
    sz = plan.sizes(B)
    assert (sz.Hp, sz.Wp) == (HP, HP)
    rng = np.random.default_rng(23)
    dseis = torch.from_numpy(rng.standard_normal((B, plan.ns, sz.nrec, plan.ng)).astype(np.float32)).to(cuda)
    return fwi, plan, v, dseis


NAMES = ("seis (no-grad)", "seis", "history", "gA", "gk_part", "gbeta", "dL/dv")


def _run(plan, v, B, dseis):
    """No-grad forward, then forward with history + adjoint + finalize, on the device; plan.status()
    raises unless the status word is clean."""
    sz = plan.sizes(B)
    coeffs, vstat = plan.coeffs(v, 0)
    seis_ng, _ = plan.forward(coeffs, B, keep_history=False)
    seis_ng = seis_ng.clone()
    plan.status()
    seis, hist = plan.forward(coeffs, B, keep_history=True)
    plan.status()
    gA, gk, gb = plan.adjoint(coeffs, hist, dseis, B)
    g = plan.finalize(coeffs, vstat, gA, gk, gb, B, 0)
    plan.status()
    assert plan.debug_words()[0] == 0
    cells = hist.view(plan.nt + 2, B * plan.ns, sz.Hp, sz.ld)[..., :sz.Wp].clone()
    return seis_ng, seis, cells, gA, gk, gb, g


def _both_modes(plan, v, B, dseis, cls, adj_runs_roles=True):
    out = {}
    assert plan.launch_info(B)["adj_roles"] == (1 if adj_runs_roles else 0)    # the default
    for mode in (0, 1):
        plan.set_wave_roles(0, mode)
        info = plan.launch_info(B)
        assert info["fwd_class"] == cls and (info["adj_class"] == cls or not adj_runs_roles), info
        assert info["fwd_T"] == T and info["adj_T"] == T, info
        assert info["fwd_roles"] == 0 and info["adj_roles"] == (mode if adj_runs_roles else 0), info
        out[mode] = _run(plan, v, B, dseis)
    for name, a, b in zip(NAMES, out[0], out[1]):
        assert torch.equal(a, b), name
    assert torch.equal(out[1][0], out[1][1])                  # the no-grad call records the same seismograms
    return out[1]


# (source row, receiver row) on the 96-row class at 6 rows per wave, and what the case is about
ROWS = {
    "same_wave": (22, 23),
    "two_waves": (22, 40),
    "two_tiles": (30, 88),
    "src_boundary_rcv_interior": (22, 24),
    "src_interior_rcv_boundary": (24, 22),
    "src_halo_copy": (84, 85),
    "rcv_halo_copy": (40, 84),
}


def _check_case(case, srow, rrow):
    s, r = _own(srow, 12, 6), _own(rrow, 12, 6)
    if case == "same_wave":
        assert s[:2] == r[:2]
    elif case == "two_waves":
        assert s[0] == r[0] and s[1] != r[1]
    elif case == "two_tiles":
        assert s[0] != r[0]
    elif case == "src_boundary_rcv_interior":
        assert s[:2] == r[:2] and _boundary(s[2], 6) and not _boundary(r[2], 6)
    elif case == "src_interior_rcv_boundary":
        assert s[:2] == r[:2] and not _boundary(s[2], 6) and _boundary(r[2], 6)
    else:   # own row of one tile, halo copy in the neighbouring tile's all-halo wave
        row, own = (srow, s) if case == "src_halo_copy" else (rrow, r)
        copies = [c for c in _slots(row, 12, 6) if not c[3] and c[0] != own[0] and _all_halo(c[0], c[1], 12, 6)]
        assert copies, _slots(row, 12, 6)


@pytest.mark.parametrize("case", list(ROWS))
def test_roles_bitwise_where_the_rows_fall(cuda, case):
    srow, rrow = ROWS[case]
    _check_case(case, srow, rrow)
    fwi, plan, v, dseis = _setup(cuda, 43, 1, srow, rrow)
    plan.set_persistent(12)
    got = _both_modes(plan, v, 1, dseis, 12)
    assert float(got[2][2:].abs().max()) > 0 and float(got[3].abs().max()) > 0   # not vacuous
    assert float(got[1].abs().max()) > 0


@pytest.mark.parametrize("nt", [1, 2, 3, 4, 5, 9, 10, 11, 12])
def test_roles_bitwise_short_records(cuda, nt):
    """No steady epoch at all (nt <= 4), one or two of them, every tail length, the adjoint's k >= 2
    history guard in the last epoch."""
    fwi, plan, v, dseis = _setup(cuda, nt, 1, 22, 24)
    plan.set_persistent(12)
    got = _both_modes(plan, v, 1, dseis, 12)
    assert float(got[2][2:].abs().max()) > 0                 # the spike went in


@pytest.mark.parametrize("rw,cls,rows,B", [
    (8, 12, (22, 23), 1),           # 8 rows per wave: rows {6, 7} of a wave
    (8, 12, (30, 88), 1),
    (6, 16, (22, 23), 1),           # the 16-wave class of 64-row regions, forced
    (6, 16, (30, 88), 1),
    (6, 8, (22, 23), 1),            # 64-row regions of 8 waves x 8 rows
    (6, 8, (30, 88), 1),
    (6, 12, (22, 40), 2),           # B = 2: the launch's slice group spans both models
])
def test_roles_bitwise_region_classes(cuda, rw, cls, rows, B):
    fwi, plan, v, dseis = _setup(cuda, 43, B, *rows)
    plan.set_rows_per_wave(rw, rw)
    plan.set_persistent(cls)
    _own(rows[0], cls, rw), _own(rows[1], cls, rw)            # each row is one region's own row
    got = _both_modes(plan, v, B, dseis, cls)
    assert float(got[3].abs().max()) > 0


def test_roles_bitwise_sample_temporal(cuda):
    fwi, plan, v, dseis = _setup(cuda, 43, 1, 22, 40, st=3)
    plan.set_persistent(12)
    assert plan.sizes(1).nrec == 15                           # ceil(43 / 3)
    _both_modes(plan, v, 1, dseis, 12)


def test_roles_shared_receiver_column(cuda):
    """fwd_multi_rcv (ng > n_grid: several receivers on one padded column; the adjoint reads residuals
    folded per column): both settings give the same bits and the fixture's seismograms.  Its nbc = 8 runs
    the exact-order adjoint, which has no roles (mode 0 reported whatever is set)."""
    from test_gpu_fwi import bits_equal, make_fwi
    z = load_golden("fwd_multi_rcv")
    ctx = ctx_of(z)
    fwi = make_fwi(ctx)
    v = torch.from_numpy(vnorm(z["v"])).to(cuda)
    B = v.shape[0]
    plan = fwi._plan(v.shape[2], v.shape[3], v.device)
    plan.set_persistent(True)
    cls = plan.launch_info(B)["fwd_class"]
    assert cls
    dseis = torch.from_numpy(np.random.default_rng(5).standard_normal(z["seis"].shape).astype(np.float32)).to(cuda)
    got = _both_modes(plan, v, B, dseis, cls, adj_runs_roles=False)
    assert bits_equal(got[1].cpu().numpy(), z["seis"])


def test_roles_setter_contract(cuda):
    """launch_info reports the mode that runs (0 off the default depth, for the exact-order adjoint and
    for chunked launches); out-of-range modes are rejected; setting a mode with cached graphs in the plan
    (chunked calls: one captured, one replayed) drops them, and calls after it give the same bits."""
    B = 1
    fwi, plan, v, dseis = _setup(cuda, 43, B)
    plan.set_persistent(12)
    ref = _run(plan, v, B, dseis)
    for bad in ((1, 0), (1, 1), (0, 2), (-1, 0), (0, -1)):   # the forward has mode 0 only
        with pytest.raises(Exception):
            plan.set_wave_roles(*bad)
    info = plan.launch_info(B)
    assert info["fwd_roles"] == 0 and info["adj_roles"] == 1  # a rejected call changes nothing
    plan.set_tuning(3, 3, 1)
    info = plan.launch_info(B)
    assert info["fwd_persistent"] and info["fwd_roles"] == 0 and info["adj_roles"] == 0
    got = _run(plan, v, B, dseis)
    assert torch.equal(ref[1], got[1]) and torch.equal(ref[2], got[2])      # forward: every depth bit-exact
    plan.set_tuning(4, 4, 1)
    plan.set_variant(adj_exact=True)
    info = plan.launch_info(B)
    assert info["fwd_roles"] == 0 and info["adj_roles"] == 0
    plan.set_variant(adj_exact=False)
    assert plan.launch_info(B)["adj_roles"] == 1
    plan.set_persistent(False)
    info = plan.launch_info(B)
    assert not info["fwd_persistent"] and info["fwd_roles"] == 0 and info["adj_roles"] == 0
    first = _run(plan, v, B, dseis)                           # chunked: captures the plan's graphs
    replay = _run(plan, v, B, dseis)                          # replays them
    plan.set_wave_roles(0, 0)                                 # drops them
    again = _run(plan, v, B, dseis)                           # captured anew
    for name, a, b, c in zip(NAMES, first, replay, again):
        assert torch.equal(a, b) and torch.equal(a, c), name
    assert torch.equal(first[1], ref[1]) and torch.equal(first[2], ref[2])  # chunked forward = persistent
    plan.set_persistent(12)
    info = plan.launch_info(B)
    assert info["fwd_roles"] == 0 and info["adj_roles"] == 0  # the setting outlives the detour
    off = _run(plan, v, B, dseis)
    for name, a, b in zip(NAMES, ref, off):
        assert torch.equal(a, b), name
