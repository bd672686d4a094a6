"""The illumination pass on the GPU (rdq_fwi_illum / _illum_ckpt / _illum_finalize, FWIForward.illumination,
InversionEngine(precondition="illumination")): the kernel per padded cell on a synthetic history against fp64 under
a bar counted from the kernel text, the finalize per model cell, bit identity across the forward families and the
checkpointed walk, the end-to-end result against an fp64 restatement of the physics, exact power-of-two scaling,
shot shards, and the engine against a hand-written loop.  References: tests/illum_refs.py."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import illum_refs as R
from conftest import ROOT, record_margin, vnorm

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NT_SYN, B = 37, 2
SMOKE = dict(n_grid=24, nt=200, dx=10.0, dt=0.001, nbc=10, f=15.0, sz=10, gz=10, ng=24, ns=3)
# (nz, nx, nbc): Hp = Wp = 60, one exact tile column and row (k_illum_tb's interior is 60 x 60); Wp = 61, a second tile
# column with one live column, the wrap taps across the tile seam and the pitch; Hp = 61 = the interior rows + 1, the
# same for the rows; 7 x 7, the smallest grid at nbc = 2, where the +-2 wrap spans most of the grid
GRIDS = [(20, 20, 20), (20, 21, 20), (21, 20, 20), (3, 3, 2)]


def bits_equal(a, b):
    a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def raw_plan(nz, nx, nbc, nt, ns, dev, wavelet=None):
    """A plan through the C ABI with a zero wavelet (the synthetic-history tests run no forward)."""
    from red_diffeq.solvers.pde import FwiPlan
    ctx = dict(nbc=nbc, nt=nt, dx=10.0, dt=0.001)
    isx = nbc + np.round(np.linspace(0, nx - 1, ns)).astype(np.int32)
    igx = nbc + np.arange(nx, dtype=np.int32)
    return FwiPlan(nz, nx, ctx, 1, isx, nbc + 1, igx, nbc + 1, np.zeros(nt) if wavelet is None else wavelet, dev)


def synthetic_history(plan, nwf, seed, dev):
    """Seeded normal values on [.., 0..Wp), NaN on the pitch columns; also the live part as fp64 on the host."""
    sz = plan.sizes(B)
    g = torch.Generator().manual_seed(seed)
    live = torch.randn(NT_SYN + 2, B, nwf, sz.Hp, sz.Wp, generator=g)
    hist = torch.full((NT_SYN + 2, B, nwf, sz.Hp, sz.ld), float("nan"))
    hist[..., :sz.Wp] = live
    return hist.to(dev), live.double().numpy()


def illum_raw(plan, nwf, hist, hA):
    from red_diffeq import _hip
    rc = plan.lib.rdq_fwi_illum(plan.handle, B, nwf, _hip.ptr(hist), _hip.ptr(hA), _hip.stream_of(hist))
    assert rc == 0, rc


@pytest.fixture(scope="module")
def synthetic(cuda):
    """(grid, nwf) -> the plan, the GPU's hA on a NaN-filled buffer and the fp64 reference with its bar; made once."""
    made = {}

    def get(grid, nwf):
        if (grid, nwf) not in made:
            nz, nx, nbc = grid
            plan = raw_plan(nz, nx, nbc, NT_SYN, 3, cuda)
            sz = plan.sizes(B)
            assert (sz.Hp, sz.Wp) == (nz + 2 * nbc, nx + 2 * nbc) and sz.ld > sz.Wp
            hist, live = synthetic_history(plan, nwf, 100 * nz + nx + nwf, cuda)
            hA = torch.full((B, nwf, sz.Hp, sz.ld), float("nan"), device=cuda)
            illum_raw(plan, nwf, hist, hA)
            torch.cuda.synchronize()
            ref, bar = R.hA_and_bar(live, NT_SYN)
            made[(grid, nwf)] = dict(plan=plan, sz=sz, hist=hist, hA=hA, ref=ref, bar=bar)
        return made[(grid, nwf)]
    return get


@pytest.mark.parametrize("nwf", [3, 5])
@pytest.mark.parametrize("grid", GRIDS)
def test_kernel_per_cell_on_a_synthetic_history(synthetic, grid, nwf):
    """Every padded cell of every wavefield against fp64 under the bar of illum_refs.hA_and_bar (counted from
    k_illum_tb's text); the history's NaN pitch columns never reach a result, and hA's pitch columns are untouched."""
    c = synthetic(grid, nwf)
    sz = c["sz"]
    got = c["hA"].cpu().numpy()
    live, pitch = got[..., :sz.Wp], got[..., sz.Wp:]
    assert np.isfinite(live).all()
    assert np.isnan(pitch).all() and pitch.size > 0
    err = np.abs(live.astype(np.float64) - c["ref"])
    ratio = float((err / c["bar"]).max())
    print(f"illum kernel grid {grid} nwf {nwf}: worst |err| / bar = {ratio:.4f}, worst rel err = "
          f"{float((err / c['ref']).max()):.3e}")
    record_margin("illum_kernel_err_over_bar", f"{grid},{nwf}", ratio, 1.0)
    assert (err <= c["bar"]).all(), ratio


def test_second_call_on_the_same_buffers_returns_the_same_bits(synthetic):
    c = synthetic(GRIDS[1], 3)
    first = c["hA"].clone()
    illum_raw(c["plan"], 3, c["hist"], c["hA"])          # hA now holds the first result, not NaN
    live = slice(0, c["sz"].Wp)
    assert bits_equal(first[..., live], c["hA"][..., live])
    assert torch.isnan(c["hA"][..., c["sz"].Wp:]).all()


@pytest.mark.parametrize("vel_mode", [0, 1])
@pytest.mark.parametrize("grid,nwf", [(GRIDS[1], 5), (GRIDS[1], 1), (GRIDS[3], 5), (GRIDS[2], 1)])
def test_finalize_per_model_cell(synthetic, cuda, grid, nwf, vel_mode):
    """From the GPU's own hA: the sum over the planes and the replicate fold at corners, edges and the interior, both
    vel_modes.  The kernel's sums and its (dA/dv)^2 are fp64 (exact at this test's level: a few 1e-16 per add) and it
    casts once: 0.5 u |ref|; the bar allows 4 u |ref|."""
    from red_diffeq import _hip
    c = synthetic(grid, nwf)
    plan, sz = c["plan"], c["sz"]
    nz, nx, nbc = grid
    g = torch.Generator().manual_seed(7)
    v = torch.rand(B, 1, nz, nx, generator=g) * 2 - 1
    if vel_mode == 1:
        v = (v + 1) / 2 * 3000 + 1500
    coeffs, _ = plan.coeffs(v.to(cuda), vel_mode)
    H = plan.illum_finalize(coeffs, c["hA"].view(-1), B, vel_mode, nwf)
    assert H.shape == (B, 1, nz, nx) and H.dtype == torch.float32
    vheld = coeffs[:6 * B * sz.Hp * sz.ld].view(6, B, sz.Hp, sz.ld)[5][:, nbc:nbc + nz, nbc:nbc + nx].cpu().numpy()
    ref = R.H_of(c["hA"][..., :sz.Wp].cpu().numpy(), vheld, 0.001, 10.0, nbc, 1500.0 if vel_mode == 0 else 1.0)
    err = np.abs(H[:, 0].cpu().numpy().astype(np.float64) - ref)
    ratio = float((err / (4 * U * np.abs(ref))).max())
    record_margin("illum_finalize_err_over_bar", f"{grid},{nwf},{vel_mode}", ratio, 1.0)
    assert (ref > 0).all() and ratio <= 1.0, ratio
    # a bad vel_mode is refused
    colsum = torch.empty(int(sz.colsum) // 8, dtype=torch.float64, device=cuda)
    assert plan.lib.rdq_fwi_illum_finalize(plan.handle, B, nwf, _hip.ptr(coeffs), _hip.ptr(c["hA"]), 2, _hip.ptr(colsum),
                                           _hip.ptr(H), _hip.stream_of(H)) == -10001


# ------------------------------------------------------------------------------------------ real physics
def make_fwi(**kw):
    from red_diffeq.solvers.pde import FWIForward
    from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize
    return FWIForward(dict(SMOKE), "cuda", normalize=True, v_denorm_func=v_denormalize, s_norm_func=s_normalize_none, **kw)


@pytest.fixture(scope="module")
def smoke(cuda):
    """The smoke geometry: model, operator, plan, K3 fields, and hA from the persistent forward's history (shared)."""
    from red_diffeq.utils.synthetic import make_model
    vn = vnorm(make_model("curvefault", 24, 24, seed=1, batch=B))
    fwi = make_fwi()
    v = torch.from_numpy(vn).to(cuda)
    plan = fwi._plan(24, 24, v.device)
    coeffs, _ = plan.coeffs(v, 0)
    plan.set_persistent(True)
    assert plan.launch_info(B)["fwd_persistent"]
    hist = plan.forward(coeffs, B, True)[1]
    hA = plan.illum(hist, B)
    plan.status()
    sz, nbc = plan.sizes(B), SMOKE["nbc"]
    # the model cells' velocity as the operator holds it (field 5 of K3), m/s
    vheld = coeffs[:6 * B * sz.Hp * sz.ld].view(6, B, sz.Hp, sz.ld)[5][:, nbc:nbc + 24, nbc:nbc + 24].contiguous()
    return dict(vn=vn, v=v, fwi=fwi, plan=plan, coeffs=coeffs, hA=hA, vheld=vheld)


def live(plan, hA, nwf=None):
    sz = plan.sizes(B)
    return hA.view(B, -1, sz.Hp, sz.ld)[..., :sz.Wp]


def test_bit_identity_across_forward_families(smoke):
    """hA from the history of the persistent, the wide chunked and the narrow chunked forward: the same bits."""
    plan, coeffs = smoke["plan"], smoke["coeffs"]
    try:
        plan.set_persistent(False)
        for wide in (True, False):
            plan.set_variant(wide_chunked=wide)
            assert not plan.launch_info(B)["fwd_persistent"]
            hA = plan.illum(plan.forward(coeffs, B, True)[1], B)
            assert bits_equal(live(plan, hA), live(plan, smoke["hA"])), wide
    finally:
        plan.set_variant()
        plan.set_persistent(True)
    assert float(live(plan, smoke["hA"]).min()) >= 0 and float(live(plan, smoke["hA"]).max()) > 0


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("chains", [1, 3])
@pytest.mark.parametrize("depth", [1, 3, 4])
def test_bit_identity_of_the_checkpointed_walk(smoke, depth, chains, graphs):
    """rdq_fwi_illum_ckpt over the checkpoint store, for segment lengths that divide nt, do not, equal it and exceed
    it, equals the store-all pass bit for bit at every forward depth, chain count and graph setting (k descending
    inside a segment, segments from the last to the first: the adds into a cell come in the store-all order)."""
    plan, coeffs = smoke["plan"], smoke["coeffs"]
    want = live(plan, smoke["hA"])
    try:
        plan.set_persistent(False)
        plan.set_graphs(graphs)
        plan.set_tuning(depth, depth, chains)
        for K in (7, 64, 200, 1000):
            ckpt = plan.forward_ckpt(coeffs, B, K)[1]
            for _ in range(2 if K == 64 else 1):          # (the second call replays the cached graph)
                hA = plan.illum_ckpt(coeffs, ckpt, B, K)
                assert bits_equal(live(plan, hA), want), K
        plan.status()
    finally:
        plan.set_tuning(4, 4, 0)
        plan.set_graphs(True)
        plan.set_persistent(True)


def test_missing_store_with_several_segments_is_refused(smoke, cuda):
    from red_diffeq import _hip
    plan, coeffs = smoke["plan"], smoke["coeffs"]
    sz = plan.sizes(B)
    seg = torch.empty(int(plan.ckpt_sizes(B, 64).seg) // 4, device=cuda)
    ring = torch.empty(int(sz.ring) // 4, device=cuda)
    hA = torch.empty(int(sz.gA) // 4, device=cuda)
    rc = plan.lib.rdq_fwi_illum_ckpt(plan.handle, B, 64, _hip.ptr(coeffs), None, None, None, _hip.ptr(seg),
                                     _hip.ptr(ring), _hip.ptr(hA), _hip.stream_of(hA))
    assert rc == -10001


def test_bit_identity_with_a_wavelet_and_with_an_encoding(smoke, cuda):
    """One wavelet= case and one encoding= case (ne = 2): the checkpointed walk against the store-all history of the
    same call, through the public method (checkpoint=64) and through the plan."""
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(3, SMOKE["nt"], generator=g) * torch.hann_window(SMOKE["nt"])).to(cuda)
    E = torch.tensor([[1.0, -1.0, 1.0], [0.5, 0.0, -2.0]], device=cuda)
    v = smoke["v"]
    full, ck = make_fwi(), make_fwi(checkpoint=64)
    for kw, nwf in ((dict(wavelet=w), 3), (dict(encoding=E), 2), (dict(wavelet=w, encoding=E), 2)):
        a = full.illumination(v, per_wavefield=True, **kw)
        b = ck.illumination(v, per_wavefield=True, **kw)
        assert a.shape == (B, nwf, 24, 24) and bits_equal(a, b), kw
        assert bits_equal(full.illumination(v, **kw), ck.illumination(v, **kw)), kw
        assert float(a.min()) >= 0 and float(a.max()) > 0
    # a row of E with a single 1 is that shot's own wavefield
    one = full.illumination(v, encoding=torch.tensor([[0.0, 1.0, 0.0]], device=cuda), wavelet=w, per_wavefield=True)
    assert bits_equal(one[:, 0], full.illumination(v, wavelet=w, per_wavefield=True)[:, 1])
    full.check()
    ck.check()


def test_end_to_end_against_the_fp64_restatement(smoke):
    """fwi.illumination(vn) against H from the fp64 restatement of the physics, per model: e_gpu <= 4 e_ref, e_ref the
    same distance for the fp64 formula on the oracle's fp32 history (the reference's own fp32 error; 4 is the margin
    this project gives a correct fp32 operator over it)."""
    from oracle import oracle as O
    vn = smoke["vn"]
    v32 = smoke["vheld"].cpu().numpy()
    assert np.abs(v32 - R.denorm32(vn)[:, 0]).max() <= 4500 * 2 * U     # (the fused denormalisation, to an ulp)
    nt, nbc = SMOKE["nt"], SMOKE["nbc"]
    hist64 = R.forward64(v32.astype(np.float64), SMOKE)[1]
    truth = R.H_of(R.hA_and_bar(hist64, nt)[0], v32, SMOKE["dt"], SMOKE["dx"], nbc, 1500.0)
    hist32 = O.OracleFWI(dict(SMOKE), B).forward(vn, keep_history=True)[1]["hist"]
    H32 = R.H_of(R.hA_and_bar(hist32.astype(np.float64), nt)[0], v32, SMOKE["dt"], SMOKE["dx"], nbc, 1500.0)
    e_ref = R.rel_l2(H32, truth)
    H = smoke["fwi"].illumination(smoke["v"])
    assert H.shape == (B, 1, 24, 24) and H.dtype == torch.float32 and not H.requires_grad
    e_gpu = R.rel_l2(H[:, 0].cpu().numpy(), truth)
    print("illumination end to end: e_gpu", e_gpu, "e_ref", e_ref)
    for b in range(B):
        record_margin("illum_end_to_end_e_gpu_over_4_e_ref", f"model{b}", e_gpu[b], 4 * e_ref[b])
    assert (e_gpu <= 4 * e_ref).all(), (e_gpu, e_ref)
    # per (m/s)^2 with normalize=False: the same H without the two factors of 1500
    from red_diffeq.solvers.pde import FWIForward
    phys = FWIForward(dict(SMOKE), "cuda", normalize=False)
    Hp = phys.illumination(smoke["vheld"].unsqueeze(1))          # the very velocities the normalised call ran on
    np.testing.assert_allclose(Hp.cpu().numpy().astype(np.float64) * 1500.0 ** 2, H.cpu().numpy(), rtol=4 * U)


def test_exact_power_of_two_scaling(smoke, cuda):
    """A constructor wavelet multiplied by 2^3 gives 64 x the hA bits exactly (the forward is linear and every
    operation of the pass commutes with a power of two)."""
    from red_diffeq.solvers.pde import ricker
    w = ricker(SMOKE["f"], SMOKE["dt"], SMOKE["nt"])
    out = []
    for scale in (1.0, 8.0):
        fwi = make_fwi(wavelet=w * scale)
        plan = fwi._plan(24, 24, smoke["v"].device)
        coeffs, _ = plan.coeffs(smoke["v"], 0)
        out.append(live(plan, plan.illum(plan.forward(coeffs, B, True)[1], B)))
        plan.status()
    assert bits_equal(out[0], live(smoke["plan"], smoke["hA"]))        # the Ricker as a constructor wavelet
    assert bits_equal(out[0] * 64.0, out[1])


def test_shot_shards(smoke):
    """Two shots= operators' per-wavefield planes are the full survey's planes bit for bit, and their H sum to the full
    H within 2 u |H| (each H is one cast of an fp64 sum: 0.5 u each, the fp32 add of the two another 0.5 u)."""
    v = smoke["v"]
    full = smoke["fwi"].illumination(v, per_wavefield=True)
    Hfull = smoke["fwi"].illumination(v)
    parts, Hs = [], []
    for sl in ((0, 2), (2, 3)):
        op = make_fwi(shots=sl)
        p = op.illumination(v, per_wavefield=True)
        assert p.shape == (B, sl[1] - sl[0], 24, 24)
        parts.append(p)
        Hs.append(op.illumination(v))
        op.check()
    assert bits_equal(torch.cat(parts, dim=1), full)
    err = (Hs[0] + Hs[1] - Hfull).abs().double()
    assert bool((err <= 2 * U * Hfull.abs().double()).all())


def test_opcheck_of_the_three_ops(smoke, cuda):
    plan, coeffs = smoke["plan"], smoke["coeffs"]
    plan.set_persistent(False)
    try:
        hist = plan.forward(coeffs, B, True)[1]
        K = 64
        ckpt = plan.forward_ckpt(coeffs, B, K)[1]
        seg = torch.empty(int(plan.ckpt_sizes(B, K).seg) // 4, device=cuda)
        tests = ("test_schema", "test_faketensor")
        torch.library.opcheck(torch.ops.red_diffeq.illum_fwi.default, (hist, plan.op_id, B, 0), test_utils=tests)
        torch.library.opcheck(torch.ops.red_diffeq.illum_fwi_ckpt.default, (coeffs, ckpt, seg, plan.op_id, B, K),
                              test_utils=tests)
        torch.library.opcheck(torch.ops.red_diffeq.illum_fwi_finalize.default,
                              (coeffs, smoke["hA"], plan.op_id, B, 0, 0), test_utils=tests)
    finally:
        plan.set_persistent(True)


# ------------------------------------------------------------------------------------------ engine
TS, LR, LAM = 3, 0.03, 0.01


def engine_inputs(smoke, cuda):
    from red_diffeq.utils.data_trans import prepare_initial_model, v_normalize
    from red_diffeq.utils.synthetic import make_model
    vt = torch.from_numpy(make_model("curvefault", 24, 24, seed=1, batch=B))
    with torch.no_grad():
        y = smoke["fwi"](v_normalize(vt).to(cuda))
    mu0 = torch.cat([torch.nn.functional.pad(prepare_initial_model(vt[i:i + 1], "smoothed", sigma=5.0), (1, 1, 1, 1))
                     for i in range(B)], dim=0)
    return mu0, vt, y


def run_engine(cuda, fwi, mu0, vt, y, **kw):
    from red_diffeq.core.inversion import InversionEngine
    from red_diffeq.utils.ssim import SSIM

    class dm:
        device = cuda
    eng = InversionEngine(dm, SSIM(window_size=11), "tv", show_progress=False, **kw)
    eng.model_trace = []
    eng.optimize(mu0, vt, y, fwi, ts=TS, lr=LR, reg_lambda=LAM, regularization="tv")
    return eng.model_trace


class _Plain:
    """The operator without an illumination method (what precondition=None must not need)."""

    def __init__(self, fwi):
        self.fwi = fwi

    def to(self, device):
        return self

    def __call__(self, v):
        return self.fwi(v)

    def __getattr__(self, name):
        if name in ("status_word", "check", "fallback_to_chunked", "restore_persistent", "shots", "shots_explicit"):
            return getattr(self.fwi, name)
        raise AttributeError(name)


def test_engine_without_preconditioning_is_unchanged(smoke, cuda):
    """precondition=None: the model trace of the default call, bit for bit, and no use of the operator's illumination
    (an operator without the method gives the same trace)."""
    mu0, vt, y = engine_inputs(smoke, cuda)
    a = run_engine(cuda, smoke["fwi"], mu0, vt, y)
    b = run_engine(cuda, smoke["fwi"], mu0, vt, y, precondition=None, precondition_every=5)
    c = run_engine(cuda, _Plain(smoke["fwi"]), mu0, vt, y, precondition=None)
    assert len(a) == TS
    for x, y_, z in zip(a, b, c):
        assert bits_equal(x, y_) and bits_equal(x, z)


@pytest.mark.parametrize("every", [0, 2])
def test_engine_equals_a_hand_written_loop(smoke, cuda, every):
    """precondition="illumination" against the loop written out: explicit illumination, illumination_weights and a
    gradient hook on the operator's input; the regulariser's gradient is not scaled."""
    from red_diffeq.core.fused import CosineLR, FusedAdamClamp
    from red_diffeq.core.losses import LossCalculator
    from red_diffeq.regularization.base import RegularizationMethod
    from red_diffeq.utils.precondition import illumination_weights
    fwi = smoke["fwi"]
    mu0, vt, y = engine_inputs(smoke, cuda)
    eps, power = 3e-2, 0.5
    got = run_engine(cuda, fwi, mu0, vt, y, precondition="illumination", precondition_eps=eps,
                     precondition_power=power, precondition_every=every)

    class dm:
        device = cuda
    mu = mu0.float().clone().to(cuda).requires_grad_(True)
    opt, sch = FusedAdamClamp(mu, lr=LR, clamp=(-1.0, 1.0)), CosineLR(LR, T_max=TS, eta_min=0.0)
    lc = LossCalculator(RegularizationMethod("tv", dm, use_time_weight=False, sigma_x0=0.0001, fixed_timestep=None), "l1", None)
    W, want = None, []
    for it in range(TS):
        v_in = mu[:, :, 1:-1, 1:-1]
        if W is None or (every > 0 and it % every == 0):
            W = illumination_weights(fwi.illumination(v_in.detach()), eps, power)
        v_in.register_hook(lambda g, W=W: g * W)
        obs = lc.observation_loss(fwi(v_in), y, mask=None)
        reg, _ = lc.regularization_loss(mu, generator=None)
        opt.zero_grad()
        lc.total_loss(obs, reg, LAM).sum().backward()
        opt.step(guard=fwi.status_word())
        opt.lr = sch.step()
        want.append(mu.detach()[:, :, 1:-1, 1:-1].clone())
    fwi.check()
    plain = run_engine(cuda, fwi, mu0, vt, y)
    for x, y_ in zip(got, want):
        assert bits_equal(x, y_)
    assert not bits_equal(got[-1], plain[-1])            # and it is not the unpreconditioned run
    assert abs(float(W.double().mean()) - 1.0) < 1e-5


class _Faulting:
    """The operator with the plan's status word set by hand (a host-side fill of the caller-owned word, no device
    fault) right after the forward of call number `at`: what a failed persistent launch leaves behind."""

    def __init__(self, fwi, plan, at):
        self.fwi, self.plan, self.at, self.n, self.n_illum = fwi, plan, at, 0, 0

    def to(self, device):
        return self

    def __call__(self, v):
        out = self.fwi(v)
        if self.n == self.at:
            self.plan.status_t[:1].fill_(1)
        self.n += 1
        return out

    def illumination(self, v, **kw):
        self.n_illum += 1
        return self.fwi.illumination(v, **kw)

    def __getattr__(self, name):
        if name in ("status_word", "check", "fallback_to_chunked", "restore_persistent"):
            return getattr(self.fwi, name)
        raise AttributeError(name)


def test_engine_rewind_replays_with_the_snapshot_weights(smoke, cuda, monkeypatch):
    """A forced status-word fault at iteration 1 (the word written by hand: no launch fails on the device): the Adam
    guard skips iterations 1 and 2, the engine rewinds to 1 and replays.  The snapshot of an iteration carries the
    weights in force at its start, the replay of iteration 1 uses them, the refresh due at iteration 2 is computed
    again, and the run ends on the clean run's models bit for bit.  Both runs use the chunked kernels throughout, so
    the fallback changes no kernel.  (The oversubscribed-launch hook of tests/test_gpu_loop_parity.py is not used: it
    makes a launch wait out its timeout.)"""
    from red_diffeq.core import inversion as inv
    mu0, vt, y = engine_inputs(smoke, cuda)
    kw = dict(precondition="illumination", precondition_every=2)
    fwi = make_fwi()
    plan = fwi._plan(24, 24, smoke["v"].device)
    plan.set_persistent(False)
    clean = run_engine(cuda, fwi, mu0, vt, y, **kw)
    seen = []
    orig_rewind = inv.InversionEngine._rewind

    def rewind(k, snaps, *a, **k2):
        seen.append((k, [None if s is None else s[5] for s in snaps]))
        return orig_rewind(k, snaps, *a, **k2)
    monkeypatch.setattr(inv.InversionEngine, "_rewind", staticmethod(rewind))
    op = _Faulting(fwi, plan, at=1)
    with pytest.warns(RuntimeWarning, match="persistent FWI launch failed at iteration 1"):
        replay = run_engine(cuda, op, mu0, vt, y, **kw)
    fwi.check()                                           # the word was cleared by the recovery
    assert len(seen) == 1 and seen[0][0] == 1
    snaps = seen[0][1]
    assert snaps[0] is None                               # nothing in force before iteration 0's refresh
    assert snaps[1] is not None and snaps[2] is snaps[1]  # iteration 0's weights at the start of 1 and of 2
    assert op.n_illum == 3 and op.n == 5                  # refreshes at 0 and 2, and 2 again on the replay
    assert len(replay) == TS
    for x, y_ in zip(replay, clean):
        assert bits_equal(x, y_)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_engine_two_ranks(smoke, cuda, tmp_path):
    """Two ranks (gloo, both on the one GPU) each model their shots; H is summed over the ranks before the weights,
    and the data gradient is scaled after the ranks' sum.  Equal to the single-rank run to the bar of
    tests/test_gpu_sharding.py (model RMSE < 5e-5: the shots' gradients summed in another association)."""
    out = tmp_path / "rank0.npz"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(ROOT, "tests", "illum_engine_worker.py"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    s = np.load(out)
    assert bool(s["same"]) and bool(s["sharded"])
    mu0, vt, y = engine_inputs(smoke, cuda)
    single = run_engine(cuda, smoke["fwi"], mu0, vt, y, precondition="illumination", precondition_every=2)
    a, b = s["mu"].astype(np.float64), single[-1].cpu().numpy().astype(np.float64)
    rmse = float(np.sqrt(((a - b) ** 2).mean(axis=(1, 2, 3))).max())
    record_margin("illum_sharded_vs_single_rank_model_rmse", "smoke", rmse, 5e-5)
    assert rmse < 5e-5, rmse
