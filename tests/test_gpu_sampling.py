"""Prior sampling on the HIP path: the fused reverse step (rdq_sample_step, csrc/unet.hip) per element against
fp64 torch, and GaussianDiffusion.sample / p_sample_loop / ddim_sample / interpolate against the reference's own
runs (tests/golden/sampling_dim8*.npz, made by tests/golden/make_sampling.py; draws replayed through noise=).

Step bar, derived from the kernel and not from its output: every product, sum, quotient of
sample_step_elem rounds to fp32 once (contraction is off there), so with U = 2^-24
    |got - ref| <= R * U * M
R = the number of fp32 roundings on the path, M = the sum of the magnitudes of the terms that reach the output,
each carried through the factors applied after it (both written out in step_reference).  The fp64 reference
uses the same fp32 inputs, tables and step scalars, so it carries no error of its own at this scale.
    x0      pred_noise / pred_v: 2 products + 1 difference = 3;  pred_x0: 0.  The clamp is exact and 1-Lipschitz.
    last    x_next = x0: R = R0.
    anc     c1 x0, c2 x, their sum = 3;  with noise: expf (<= 1 ulp = 2 U), sd z, the sum = 4 more.
    DDIM    sr x (counted again: it enters eps directly and through x0) 1, u - x0 and / srm1 2, x0 a, c eps, their
            sum 3;  with noise: sigma z and the sum, 2 more.

Loop bar: a chain of U-Net forwards has no bound known ahead of time, so the yardstick is the reference's own fp32
error: the HIP result's max-abs distance from the reference's fp64 run is at most 4 x E_ref at every recorded step
(E_ref = the reference's fp32 run against that fp64 run).  Measured value and bar of every case and step go to
margins.jsonl (record_margin)."""

import numpy as np
import pytest
import torch

from conftest import load_golden, record_margin

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPE = (2, 1, 72, 72)
OBJ = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}
ANC, DDIM, LAST = 0, 1, 2
# (mode, (sqrt(alpha_next), c, sigma), with noise): the step scalars are arbitrary fp32 values
F32 = lambda v: float(np.float32(v))  # noqa: E731
STEPS = {"anc": (ANC, (0.0, 0.0, 0.0), True), "ddim_eta0": (DDIM, (F32(0.8), F32(0.6), 0.0), True),
         "ddim_eta1": (DDIM, (F32(0.8), F32(0.5), F32(0.33)), True), "ddim_last": (LAST, (0.0, 0.0, 0.0), False)}


@pytest.fixture(scope="module")
def diff1000(cuda):
    """A 1000-step schedule on the device (the tables do not depend on the objective or the network)."""
    from red_diffeq.models.diffusion import GaussianDiffusion

    class Net(torch.nn.Module):
        channels, out_dim, self_condition = 1, 1, False
    return GaussianDiffusion(Net(), image_size=72, timesteps=1000, objective="pred_noise").to(cuda)


def tables_of(diff):
    from red_diffeq.models import unet_ops
    return unet_ops.sample_tables(diff)


def step_inputs(tabs64, objective, t, n, seed):
    """x, out, noise (fp32, CPU) with x0 below -1, inside and above 1 in >= 10 % of the elements each: out is
    solved from a target x0 uniform in [-2, 2]."""
    sr, srm1, sa, s1ma = (tabs64[i][t][:, None] for i in range(4))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(len(t), n, generator=g, dtype=torch.float64)
    target = torch.rand(len(t), n, generator=g, dtype=torch.float64) * 4 - 2
    if objective == "pred_noise":
        out = (sr * x - target) / srm1
    elif objective == "pred_x0":
        out = target
    else:
        out = (sa * x - target) / s1ma
    z = torch.randn(len(t), n, generator=g, dtype=torch.float64)
    return x.float(), out.float(), z.float()


def step_reference(tabs64, objective, mode, coef, t, x, out, z):
    """fp64 restatement of reference diffusion.py:411-446 / 469-494 on the fp32 inputs -> (x_next, x0 clamped,
    x0 unclamped, R, M, M0); R0 * U * M0 bounds the error of x0 alone."""
    x, out = x.double(), out.double()
    sr, srm1, sa, s1ma, c1, c2, lv = (tab[t][:, None] for tab in tabs64)
    if objective == "pred_noise":
        a, b = sr * x, srm1 * out
        raw, R, M0 = a - b, 3, a.abs() + b.abs()
    elif objective == "pred_x0":
        raw, R, M0 = out, 0, out.abs()
    else:
        a, b = sa * x, s1ma * out
        raw, R, M0 = a - b, 3, a.abs() + b.abs()
    x0 = raw.clamp(-1.0, 1.0)
    if mode == LAST:
        return x0, x0, raw, R, M0, M0
    if mode == ANC:
        mean = c1 * x0 + c2 * x
        R, M = R + 3, c1.abs() * M0 + (c2 * x).abs()
        if z is None:
            return mean, x0, raw, R, M, M0
        nz = (0.5 * lv).exp() * z.double()
        return mean + nz, x0, raw, R + 4, M + nz.abs(), M0
    an, c, sigma = coef
    u = sr * x
    eps = (u - x0) / srm1
    y = x0 * an + c * eps
    R, M = R + 1 + 2 + 3, abs(an) * M0 + abs(c) * (u.abs() + M0) / srm1
    if z is None:
        return y, x0, raw, R, M, M0
    nz = sigma * z.double()
    return y + nz, x0, raw, R + 2, M + nz.abs(), M0


def run_step(cuda, diff, objective, mode, coef, t, x, out, z, t_next, alias=False, want_x0=True):
    dev = lambda v: None if v is None else v.to(cuda).contiguous()  # noqa: E731
    xd, od, zd, td = dev(x), dev(out), dev(z), dev(t)
    xn = xd if alias else torch.full_like(xd, float("nan"))
    x0 = torch.full_like(xd, float("nan")) if want_x0 else None
    t_out = torch.full_like(td, -7)
    torch.ops.red_diffeq.sample_step(xd, td, od, zd, tables_of(diff), OBJ[objective], mode, *coef, t_next, xn, x0,
                                     t_out)
    return xn.cpu(), None if x0 is None else x0.cpu(), t_out.cpu()


@pytest.mark.parametrize("n", [72 * 72, 63])
@pytest.mark.parametrize("t", [(0, 999), (37, 640)])
@pytest.mark.parametrize("step", list(STEPS))
@pytest.mark.parametrize("objective", list(OBJ))
def test_step_kernel_per_element(cuda, diff1000, objective, step, t, n):
    """3 objectives x {ancestral, DDIM eta 0, DDIM eta 1, DDIM last step}; per-sample t at both ends of the tables
    and inside; n = 72 * 72 (16-byte path, several workgroups per sample) and n = 63 (scalar path, less than one
    workgroup).  Also: x_next aliasing x_t gives the same bits, t_out = t_next, x_start_out = the clamped x0."""
    mode, coef, noisy = STEPS[step]
    tabs64 = [v.double().cpu() for v in tables_of(diff1000)]
    tt = torch.tensor(t)
    x, out, z = step_inputs(tabs64, objective, tt, n, seed=n + t[0])
    z = z if noisy else None
    ref, x0ref, raw, R, M, M0 = step_reference(tabs64, objective, mode, coef, tt, x, out, z)
    frac = [float((raw < -1).double().mean()), float((raw.abs() <= 1).double().mean()),
            float((raw > 1).double().mean())]
    assert min(frac) >= 0.10, frac
    t_next = 5 if mode != LAST else -1
    got, x0, t_out = run_step(cuda, diff1000, objective, mode, coef, tt, x, out, z, t_next)
    case = f"{objective},{step},t={t},n={n}"
    assert torch.isfinite(got).all() and torch.isfinite(x0).all(), case
    bar = R * U * M if R else torch.zeros_like(M)
    err = (got.double() - ref).abs()
    ratio = float((err / bar.clamp(min=1e-300)).max()) if R else float(err.max())
    record_margin("sample_step_err_over_bar", case, ratio, 1.0)
    print(f"{case}: R = {R}, max err {float(err.max()):.3e}, max err / bar {ratio:.3f}")
    assert (err <= bar).all(), (case, ratio)
    R0 = 0 if objective == "pred_x0" else 3
    assert ((x0.double() - x0ref).abs() <= R0 * U * M0).all(), case          # pred_x0: exactly clamp(out)
    assert float(x0.min()) == -1.0 and float(x0.max()) == 1.0            # both clamp sides were taken
    if mode == LAST:
        assert torch.equal(got, x0) and torch.equal(t_out, torch.full_like(tt, -7))   # t_out untouched
    else:
        assert torch.equal(t_out, torch.full_like(tt, 5)), case
    got2, _, _ = run_step(cuda, diff1000, objective, mode, coef, tt, x, out, z, t_next, alias=True, want_x0=False)
    assert torch.equal(got2.view(torch.int32), got.view(torch.int32)), case


@pytest.mark.parametrize("objective", list(OBJ))
def test_step_kernel_ancestral_t0_without_noise(cuda, diff1000, objective):
    """p_sample at t = 0 (reference 444: noise = 0.0): a null noise pointer gives the posterior mean."""
    tabs64 = [v.double().cpu() for v in tables_of(diff1000)]
    tt = torch.tensor([0, 0])
    x, out, _ = step_inputs(tabs64, objective, tt, 72 * 72, seed=3)
    ref, _, _, R, M, _ = step_reference(tabs64, objective, ANC, (0.0, 0.0, 0.0), tt, x, out, None)
    got, _, _ = run_step(cuda, diff1000, objective, ANC, (0.0, 0.0, 0.0), tt, x, out, None, -1)
    err = (got.double() - ref).abs()
    record_margin("sample_step_err_over_bar", f"{objective},anc,t=0,no noise", float((err / (R * U * M)).max()), 1.0)
    assert (err <= R * U * M).all()


def test_step_op_rejects_bad_arguments(cuda, diff1000):
    tabs = tables_of(diff1000)
    x = torch.zeros(2, 1, 8, 8, device=cuda)
    t = torch.zeros(2, dtype=torch.int64, device=cuda)
    op = torch.ops.red_diffeq.sample_step
    ok = dict(x_t=x, t=t, out=x.clone(), noise=x.clone(), tables=tabs, objective=0, step=DDIM, a_next=0.5, c=0.5,
              sigma=0.1, t_next=3, x_next=x.clone(), x_start_out=None, t_out=None)
    op(**ok)
    bad = [dict(out=x[:1]), dict(noise=x[:, :, :4]), dict(x_next=x.transpose(2, 3)), dict(x_start_out=x.double()),
           dict(t=t.int()), dict(t_out=t), dict(t_out=torch.zeros(3, dtype=torch.int64, device=cuda)),
           dict(tables=tabs[:6]), dict(tables=tabs[:6] + [tabs[6][:10]]), dict(objective=3), dict(step=-1),
           dict(t_next=1000), dict(noise=None)]
    for b in bad:
        with pytest.raises(ValueError):
            op(**{**ok, **b})
    with pytest.raises(RuntimeError):
        op(**{**ok, "x_t": x.cpu()})                 # no CPU fallback


def test_step_op_opcheck(cuda, diff1000):
    from torch.library import opcheck
    tabs = tables_of(diff1000)
    g = torch.Generator().manual_seed(1)
    r = lambda: torch.randn(2, 1, 8, 8, generator=g).to(cuda)  # noqa: E731
    t = torch.tensor([3, 700], device=cuda)
    for mode, noise, x0, t_out in ((ANC, r(), None, None), (ANC, None, r(), torch.zeros_like(t)),
                                   (DDIM, r(), r(), torch.zeros_like(t)), (LAST, None, None, None)):
        opcheck(torch.ops.red_diffeq.sample_step,
                (r(), t, r(), noise, tabs, 0, mode, 0.5, 0.5, 0.0 if noise is None else 0.1, 2, r(), x0, t_out))


# ------------------------------------------------------------------------------------------- loops
def _unet8(cuda, **kw):
    from red_diffeq.models.diffusion import Unet
    z = load_golden("unet_dim8")
    net = Unet(dim=8, dim_mults=(1, 2, 4, 8), channels=1, **kw)
    if not kw:
        net.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")})
    return net.to(cuda).eval()


CASES = {"ddim0": dict(timesteps=1000, sampling_timesteps=6, objective="pred_noise"),
         "ddim1": dict(timesteps=1000, sampling_timesteps=6, objective="pred_noise", ddim_sampling_eta=1.0),
         "anc": dict(timesteps=8, objective="pred_noise"),
         "interp": dict(timesteps=8, objective="pred_noise"),
         "ddim_v": dict(timesteps=1000, sampling_timesteps=3, objective="pred_v")}


def _diffusion(cuda, tag, net=None):
    from red_diffeq.models.diffusion import GaussianDiffusion
    return GaussianDiffusion(net if net is not None else _unet8(cuda), image_size=72, **CASES[tag]).to(cuda).eval()


@pytest.fixture(scope="module")
def fixtures():
    a, b = load_golden("sampling_dim8"), load_golden("sampling_dim8_more")
    return {**{k: a[k] for k in a.files}, **{k: b[k] for k in b.files}}


def _draws(z, tag):
    """The reference run's draws, regenerated from the CPU generator in call order and checked by their sums."""
    g = torch.Generator().manual_seed(int(z[tag + "_seed"]))
    out = []
    for i, s in enumerate(z[tag + "_draw_sums"]):
        d = torch.randn(SHAPE, generator=g)
        if i == 0 and tag != "interp":
            d = d * float(z[tag + "_scale"])
        assert float(d.double().sum()) == s, (tag, i)
        out.append(d)
    return out


def _run_case(cuda, z, tag, d=None):
    d = d if d is not None else _diffusion(cuda, tag)
    draws = _draws(z, tag)
    if tag == "interp":
        x1, x2 = (torch.from_numpy(z[k]).to(cuda) for k in ("interp_x1", "interp_x2"))
        return d.interpolate(x1, x2, t=5, lam=0.3, noise=draws)[:, None], draws
    return d.sample(batch_size=2, return_all_timesteps=True, noise=draws), draws


@pytest.mark.parametrize("tag", list(CASES))
def test_sampling_loops_vs_reference(cuda, fixtures, tag):
    """Every recorded step of the reference's sample() / interpolate(): distance from its fp64 run <= 4 x E_ref."""
    z = fixtures
    got, draws = _run_case(cuda, z, tag)
    ref = torch.from_numpy(z[tag + "_f64_hi"]).double() + torch.from_numpy(z[tag + "_f64_lo"]).double() * U
    if tag != "interp":
        ref = torch.cat((((draws[0].double() + 1) * 0.5)[:, None], ref), dim=1)     # step 0: unnormalize(draw 0)
        S = CASES[tag].get("sampling_timesteps", CASES[tag]["timesteps"])
        assert got.shape == (2, S + 1, 1, 72, 72)
    eref = z[tag + "_eref"]
    assert got.shape == ref.shape and got.dtype == torch.float32 and len(eref) == got.shape[1]
    err = (got.double().cpu() - ref).abs().amax(dim=(0, 2, 3, 4)).numpy()
    for k, (e, b) in enumerate(zip(err, 4 * eref)):
        record_margin("sampling_vs_fp64_over_4Eref", f"{tag},step={k}", e, b)
        print(f"{tag} step {k}: |hip - fp64| = {e:.3e}, E_ref = {eref[k]:.3e}, ratio to bar {e / b:.3f}")
    assert torch.isfinite(got).all()
    assert (err <= 4 * eref).all(), (tag, (err / eref).tolist())


def test_graph_and_eager_paths_agree_bitwise(cuda, fixtures, monkeypatch):
    d = _diffusion(cuda, "ddim1")
    a, _ = _run_case(cuda, fixtures, "ddim1", d)
    assert d.model.__dict__.get("_graphs")                       # the loop replayed a captured forward
    monkeypatch.setenv("RDQ_NO_UNET_GRAPH", "1")
    d2 = _diffusion(cuda, "ddim1")
    b, _ = _run_case(cuda, fixtures, "ddim1", d2)
    assert not d2.model.__dict__.get("_graphs")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_sample_with_generator(cuda):
    """Reproducible with generator=, the reference's shapes, in [0, 1] after unnormalize; S + 1 entries on dim 1."""
    d = _diffusion(cuda, "ddim0")
    gen = torch.Generator(device=cuda)
    a = d.sample(batch_size=2, generator=gen.manual_seed(7))
    b = d.sample(batch_size=2, generator=gen.manual_seed(7))
    c = d.sample(batch_size=2, generator=gen.manual_seed(8))
    assert a.shape == (2, 1, 72, 72) and a.dtype == torch.float32
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    steps = d.sample(batch_size=2, return_all_timesteps=True, generator=gen.manual_seed(7))
    assert steps.shape == (2, 7, 1, 72, 72) and torch.equal(steps[:, -1], a)
    anc = _diffusion(cuda, "anc")
    s8 = anc.sample(batch_size=2, return_all_timesteps=True, generator=gen.manual_seed(7))
    assert s8.shape == (2, 9, 1, 72, 72)
    assert float(s8[:, -1].min()) >= 0.0 and float(s8[:, -1].max()) <= 1.0
    img, x0 = anc.p_sample(s8[:, 0] * 2 - 1, 7, generator=gen.manual_seed(9))
    assert img.shape == x0.shape == (2, 1, 72, 72) and float(x0.abs().max()) <= 1.0


def test_bf16_precision_is_used_by_the_loop(cuda):
    d = _diffusion(cuda, "ddim_v")
    gen = torch.Generator(device=cuda)
    a = d.sample(batch_size=2, generator=gen.manual_seed(3))
    d.model.set_precision("bf16")
    b = d.sample(batch_size=2, generator=gen.manual_seed(3))
    assert torch.isfinite(b).all() and float(b.min()) >= 0.0 and float(b.max()) <= 1.0
    assert not torch.equal(a, b)                                          # the bf16 forward was the one replayed


def test_self_condition_ddim_equals_plain_torch_loop(cuda):
    """The eager fallback and the x_start_out plumbing: a self-conditioned dim-8 net (random weights), 3 DDIM steps
    with eta = 1, against the reference's loop (469-494) restated here with torch ops on self.model calls.
    Both sides evaluate the same fp32 expression tree on the same forwards, so they can differ only where
    torch's elementwise kernels round a quotient or contract differently, a few ulp per step carried through two
    more forwards; 1e-4 on values of order 1 admits that.  A self_cond that is dropped, stale or unclamped
    changes the next forward's input by order 1 and the sample by 1e-2 or more."""
    from red_diffeq.models.diffusion import GaussianDiffusion
    torch.manual_seed(21)
    net = _unet8(cuda, self_condition=True)
    d = GaussianDiffusion(net, image_size=72, timesteps=1000, sampling_timesteps=3, objective="pred_noise",
                          ddim_sampling_eta=1.0).to(cuda).eval()
    assert d.self_condition and net.graph_io(SHAPE, cuda) is None
    g = torch.Generator().manual_seed(22)
    draws = [torch.randn(SHAPE, generator=g).to(cuda) for _ in range(3)]
    got = d.ddim_sample(SHAPE, return_all_timesteps=True, noise=draws)
    with torch.no_grad():
        img, x_start, imgs, it = draws[0], None, [draws[0]], iter(draws[1:])
        times = list(reversed(torch.linspace(-1, 999, steps=4).int().tolist()))
        pairs = list(zip(times[:-1], times[1:]))
        for time, time_next in pairs:
            tc = torch.full((2,), time, device=cuda, dtype=torch.long)
            pred_noise, x_start = d.model_predictions(img, tc, x_start, clip_x_start=True, rederive_pred_noise=True)
            if time_next < 0:
                img = x_start
            else:
                alpha, alpha_next = d.alphas_cumprod[time], d.alphas_cumprod[time_next]
                sigma = 1.0 * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
                c = (1 - alpha_next - sigma ** 2).sqrt()
                img = x_start * alpha_next.sqrt() + c * pred_noise + sigma * next(it)
            imgs.append(img)
        want = d.unnormalize(torch.stack(imgs, dim=1))
    err = float((got - want).abs().max())
    record_margin("self_condition_ddim_vs_torch_loop", "dim8,3 steps", err, 1e-4)
    print(f"self-conditioned DDIM vs torch loop: max abs diff {err:.3e}")
    assert got.shape == want.shape == (2, 4, 1, 72, 72) and err <= 1e-4, err
    with torch.no_grad():
        zero_sc = d.model(draws[0], torch.full((2,), 999, device=cuda), None)
        some_sc = d.model(draws[0], torch.full((2,), 999, device=cuda), draws[1].clamp(-1, 1))
    assert float((zero_sc - some_sc).abs().max()) > 1e-2          # the network does look at its self_cond


def test_ddim_loop_never_waits_for_the_device(cuda):
    """After a warm-up call (graph capture, schedule and timestep tables), a 6-step ddim_sample makes no
    synchronising call: torch's sync debug mode raises on .item(), .cpu(), .tolist() and blocking copies."""
    d = _diffusion(cuda, "ddim1")
    gen = torch.Generator(device=cuda)
    d.ddim_sample(SHAPE, generator=gen.manual_seed(1))
    torch.cuda.synchronize()
    probe = torch.ones(1, device=cuda)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                  # the switch is honoured by this build
        out = d.ddim_sample(SHAPE, return_all_timesteps=True, generator=gen.manual_seed(2))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert out.shape == (2, 7, 1, 72, 72) and torch.isfinite(out).all()
