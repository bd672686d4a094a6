"""Hand-off overlap of the persistent FWI kernels (rdq_fwi_set_handoff_overlap).

Mode 1 only reorders independent operations around the per-epoch hand-off (adjoint: the sweep's first
pass issued into registers of its own and the dead cells zeroed while it is in flight; the forward
kept no overlapped form, its mode is 0), so everything a call produces must equal mode 0's bit for
bit: seismograms, every history slot, gA, gk_part, gbeta and dL/dv.  Mode 0 itself is held to what
the project already pins for the persistent kernels against the chunked ones: forward and history
bit-exact, the recurrence adjoint within its fp32 bars (test_gpu_fwi.py: gA rel-L2 < 2e-6, gbeta and
gk rtol 2e-5).

Grid: 70 x 70 with nbc = 20 -> 110 x 110 padded: 3 x 2 tiles of the 96-row class (3 x 3 of the 64-row
class) with the periodic wrap in both directions, halo rows in the first and last waves; nbc >= 20 so
the recurrence adjoint (k_adj_pr) runs.  Two shots with their sources in different tiles (padded
columns 20 and 89).  Source row 22 and receiver row 23 are region rows 30 and 31: rows {0, 1} of a
6-row wave and {6, 7} of an 8-row wave, a boundary pair in both (and in the 4-row class every pair is
one).  nt = 43: ten full epochs of T = 4 and a short last one; nt = 3: shorter than one epoch.  The
Ricker wavelet must fit the record (2.2 / (f dt) samples), so these short records use f = 60 Hz (37
samples) and, for nt = 3, f = 600 Hz (3 samples: a spike); dt and the velocities are the usual ones."""
import numpy as np
import pytest
import torch

from conftest import vnorm

pytestmark = pytest.mark.gpu

NZ = NX = 70


def _setup(cuda, nt, B):
    from red_diffeq.solvers.pde import FWIForward
    from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize
    from red_diffeq.utils.synthetic import make_model
    ctx = dict(n_grid=NX, nt=nt, dx=10.0, dt=0.001, nbc=20, f=60.0 if nt >= 37 else 600.0, sz=20, gz=30, ng=NX,
               ns=2)
    fwi = FWIForward(dict(ctx), "cuda", normalize=True, v_denorm_func=v_denormalize, s_norm_func=s_normalize_none)
    v = torch.from_numpy(vnorm(make_model("curvefault", NZ, NX, seed=17, batch=B))).to(cuda)
    plan = fwi._plan(NZ, NX, v.device)
    sz = plan.sizes(B)
    assert (sz.Hp, sz.Wp) == (110, 110)
    rng = np.random.default_rng(23)
    dseis = torch.from_numpy(rng.standard_normal((B, plan.ns, sz.nrec, plan.ng)).astype(np.float32)).to(cuda)
    return fwi, plan, v, dseis


def _run(plan, v, B, dseis):
    """One forward + adjoint + finalize: (seis, history cells [nt + 2, B ns, Hp, Wp], gA, gk_part, gbeta,
    dL/dv), on the device.  plan.status() raises unless the status word is clean."""
    sz = plan.sizes(B)
    coeffs, vstat = plan.coeffs(v, 0)
    seis, hist = plan.forward(coeffs, B, keep_history=True)
    plan.status()
    gA, gk, gb = plan.adjoint(coeffs, hist, dseis, B)
    g = plan.finalize(coeffs, vstat, gA, gk, gb, B, 0)
    plan.status()
    assert plan.debug_words()[0] == 0
    # the buffer's cells: the pad columns [Wp, ld) of a row are never written by any kernel
    cells = hist.view(plan.nt + 2, B * plan.ns, sz.Hp, sz.ld)[..., :sz.Wp].clone()
    return seis, cells, gA, gk, gb, g


NAMES = ("seis", "history", "gA", "gk_part", "gbeta", "dL/dv")


@pytest.mark.parametrize("rw,cls,delay,B,nt", [
    (6, 12, (0, 0), 1, 43),
    (8, 12, (15, 10), 1, 43),
    (6, 16, (15, 0), 1, 43),        # the 16-wave class of 64-row regions, forced
    (6, 12, (15, 0), 2, 43),        # B = 2: the launch's slice group spans both models
    (6, 12, (0, 0), 1, 3),          # shorter than one epoch
    (8, 16, (15, 10), 1, 3),
])
def test_mode1_bitwise_equals_mode0(cuda, rw, cls, delay, B, nt):
    fwi, plan, v, dseis = _setup(cuda, nt, B)
    plan.set_rows_per_wave(rw, rw)
    plan.set_persistent(cls)
    plan.set_sweep_delay(*delay)
    out = {}
    assert plan.launch_info(B)["adj_overlap"] == 1            # the default
    for mode in (0, 1):
        plan.set_handoff_overlap(0, mode)
        info = plan.launch_info(B)
        assert info["fwd_class"] == cls and info["adj_class"] == cls
        assert info["fwd_T"] == 4 and info["adj_T"] == 4
        assert info["fwd_overlap"] == 0 and info["adj_overlap"] == mode      # the recurrence adjoint runs
        assert info["fwd_launches"] == 1 and info["adj_launches"] == 1       # one slice group (B = 2: both models)
        out[mode] = _run(plan, v, B, dseis)
    for name, a, b in zip(NAMES, out[0], out[1]):
        assert torch.equal(a, b), name
    assert float(out[1][1][2:].abs().max()) > 0 and float(out[1][2].abs().max()) > 0   # not vacuous


def test_modes_off_the_default_depth_run_mode0(cuda):
    """Mode 1 is built at 4 steps per epoch; other depths and the exact-order adjoint report and run
    mode 0, with the same results."""
    fwi, plan, v, dseis = _setup(cuda, 43, 1)
    plan.set_persistent(12)
    plan.set_handoff_overlap(0, 1)
    ref = _run(plan, v, 1, dseis)
    plan.set_tuning(3, 3, 1)
    info = plan.launch_info(1)
    assert info["fwd_persistent"] and info["fwd_overlap"] == 0 and info["adj_overlap"] == 0
    got = _run(plan, v, 1, dseis)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])      # forward: every depth bit-exact
    plan.set_tuning(4, 4, 1)
    plan.set_variant(adj_exact=True)
    info = plan.launch_info(1)
    assert info["fwd_overlap"] == 0 and info["adj_overlap"] == 0
    for bad in ((1, 0), (0, 2), (0, -1)):                      # the forward has mode 0 only
        with pytest.raises(Exception):
            plan.set_handoff_overlap(*bad)


def test_mode0_equals_chunked(cuda):
    """The retained mode-0 path against the chunked kernels, as the project pins the persistent kernels
    (test_persistent_slice_groups_span_models, test_persistent_shot_groups_openfwi_ns20): forward and
    history bit-exact; the exact-order persistent adjoint bit-exact; the recurrence adjoint (the kernel
    with the two modes) within its fp32 bars."""
    B = 1
    fwi, plan, v, dseis = _setup(cuda, 43, B)
    plan.set_handoff_overlap(0, 0)
    plan.set_variant(adj_exact=True)
    plan.set_persistent(False)
    assert not plan.launch_info(B)["fwd_persistent"]
    chunked = _run(plan, v, B, dseis)
    plan.set_persistent(12)
    assert plan.launch_info(B)["fwd_class"] == 12 and plan.launch_info(B)["fwd_overlap"] == 0
    exact = _run(plan, v, B, dseis)
    assert torch.equal(chunked[0], exact[0]) and torch.equal(chunked[1], exact[1])
    assert torch.equal(chunked[2], exact[2]) and torch.equal(chunked[4], exact[4])
    np.testing.assert_allclose(exact[3].view(B, -1).sum(1).cpu().numpy(),
                               chunked[3].view(B, -1).sum(1).cpu().numpy(), rtol=1e-12)
    plan.set_variant(adj_exact=False)
    assert plan.launch_info(B)["adj_overlap"] == 0
    rec = _run(plan, v, B, dseis)
    sz = plan.sizes(B)
    ref = chunked[2].view(B, plan.ns, sz.Hp, sz.ld).sum(1).double()
    got = rec[2].view(B, plan.ns, sz.Hp, sz.ld).sum(1).double()
    assert float((got - ref).norm() / ref.norm()) < 2e-6
    cb = chunked[4].view(B, -1).cpu().numpy()
    np.testing.assert_allclose(rec[4].view(B, -1).cpu().numpy(), cb, rtol=2e-5, atol=2e-6 * np.abs(cb).max())
    np.testing.assert_allclose(rec[3].view(B, -1).sum(1).cpu().numpy(),
                               chunked[3].view(B, -1).sum(1).cpu().numpy(), rtol=2e-5)


@pytest.mark.parametrize("mode", [0, 1])
def test_profile_subbuckets_sum_to_totals(cuda, mode):
    """Profiled build: per wave, the hand-off wait is its four parts (publish end -> first pass issued,
    first pass, later passes, post-sweep tail) and the publish figure is store issue + deferred gradient,
    each within one counter tick (10 ns); the profiled kernels compute what the plain ones do."""
    B = 1
    fwi, plan, v, dseis = _setup(cuda, 43, B)
    plan.set_persistent(12)
    plan.set_handoff_overlap(0, mode)
    plain = _run(plan, v, B, dseis)
    plan.set_profile(1)
    try:
        prof = _run(plan, v, B, dseis)
        summary = plan.read_profile()
        waves = [plan.profile_waves_split(adj, ticks=True).astype(np.int64) for adj in (0, 1)]
        old = [plan.profile_waves(adj) for adj in (0, 1)]
    finally:
        plan.set_profile(0)
    for name, a, b in zip(NAMES, plain, prof):
        assert torch.equal(a, b), name
    for adj, (wv, name) in enumerate(zip(waves, ("fwd", "adj"))):
        live = wv[wv[:, 1] > 0]
        assert len(live) == 6 * 16 * 2                     # 6 tiles x 16 waves x 2 shots
        wait, parts = live[:, 0], live[:, 3:7].sum(1)
        print(name, "mode", mode, "wait ticks", wait.sum(), "parts", live[:, 3:7].sum(0), "gradient", live[:, 7].sum())
        assert np.abs(wait - parts).max() <= 1
        assert (live[:, 2] >= live[:, 7]).all()            # publish = store issue + gradient
        assert (live[:, 7] > 0).any() == bool(adj)         # only the adjoint defers a gradient
        s = summary[name]
        assert s["waves"] == len(live)
        tot = s["wait_a_issue_us"] + s["wait_b_first_us"] + s["wait_c_later_us"] + s["wait_d_tail_us"]
        assert abs(tot - s["wait_us"]) <= 0.01 + 1e-9
        assert abs(s["publish_issue_us"] + s["gradient_us"] - s["publish_us"]) <= 0.01 + 1e-9
        # the three-word records keep their meaning
        np.testing.assert_array_equal(np.rint(old[adj][:len(wv)][wv[:, 1] > 0] * 100.0).astype(np.int64), live[:, :3])
