#!/usr/bin/env python
"""Generate tests/golden/sampling_dim8.npz and sampling_dim8_more.npz: the REFERENCE's prior samplers
(models/diffusion.py:439-514) on the CPU, with the dim-8 U-Net of make_golden.py (unet_dim8.npz's weights).

Run:  python tests/golden/make_sampling.py

Cases (B = 2, 1 x 72 x 72, objective pred_noise unless said):
  ddim0   timesteps=1000, sampling_timesteps=6, eta 0        sample(return_all_timesteps=True)
  ddim1   the same with ddim_sampling_eta=1.0
  anc     timesteps=8 (sampling_timesteps defaults to 8)      sample() -> p_sample_loop
  interp  interpolate(x1, x2, t=5, lam=0.3) on the 8-step diffusion
  ddim_v  as ddim0 but objective="pred_v", 3 steps
and, for the host test, the reference's DDIM schedule at S = 6 and S = 250 of T = 1000, eta 0 and 1 (read from
ddim_sample's own locals while it runs on a stub network).

Per case:
  <tag>_seed, <tag>_scale, <tag>_draw_sums   every torch.randn / randn_like draw of the run comes, in call order,
        from torch.Generator().manual_seed(seed) on the CPU (the first, the initial image, times `scale`);
        the float64 sum of each is stored so that a test regenerating them can check it has the same numbers.
        The draws themselves are not stored: with the results they would exceed the size limit of a fixture.
  <tag>_f64_hi (float32), <tag>_f64_lo (float16, in units of 2^-24)
        the run repeated with module and draws cast to float64, every recorded step but the initial image
        (which is draw 0): value = hi + lo * 2^-24.  Two fixture files because of the same limit.
  <tag>_eref   max |fp32 run - fp64 run| per recorded step (the reference's own fp32 error, the tests' yardstick)
  <tag>_pairs, <tag>_coef   ddim cases: (time, time_next) and (sqrt(alpha_next), c, sigma) of the fp32 run
  <tag>_clamped   per step, the fraction of elements whose x0 the clamp to [-1, 1] changed; asserted here to reach
        1 % on both sides (clamped and not) at some step
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (loads the reference through _refimport, defines _unet_dim8)

ref = G.ref
SHAPE = (2, 1, 72, 72)
LO_UNIT = 2.0 ** -24
_randn = torch.randn          # the real one: patched_draws replaces torch.randn while the reference runs


class patched_draws:
    """torch.randn / torch.randn_like replaced by `source(shape)`; ddim_sample's locals recorded at each draw."""

    def __init__(self, source, dtype):
        self.source, self.dtype, self.ddim = source, dtype, []

    def _spy(self):
        f = sys._getframe(2)
        if f.f_code.co_name == "ddim_sample":
            lo = f.f_locals
            self.ddim.append((lo["time"], lo["time_next"], float(lo["alpha_next"].sqrt()), float(lo["c"]),
                              float(lo["sigma"])))
            self.pairs = list(lo["time_pairs"])

    def __enter__(self):
        self.orig = torch.randn, torch.randn_like

        def randn(*size, **kw):
            size = size[0] if len(size) == 1 and not isinstance(size[0], int) else size
            return self.source(tuple(size)).to(self.dtype)

        def randn_like(t, **kw):
            self._spy()
            return self.source(tuple(t.shape)).to(self.dtype)
        torch.randn, torch.randn_like = randn, randn_like
        return self

    def __exit__(self, *exc):
        torch.randn, torch.randn_like = self.orig


def clamp_probe(diff, log):
    """Forward hook on the U-Net: the fraction of x0 entries outside [-1, 1] before the clamp."""
    def hook(mod, args, out):
        x, t = args[0], args[1]
        x0 = diff.predict_start_from_v(x, t, out) if diff.objective == "pred_v" else \
            diff.predict_start_from_noise(x, t, out)
        log.append(float((x0.abs() > 1).double().mean()))
    return diff.model.register_forward_hook(hook)


def run_case(tag, diff, call, seed, scale, out, more, first_is_image=True):
    """call(diff) -> tensor with the recorded steps on dim 1 (or a single image)."""
    gen = torch.Generator().manual_seed(seed)
    draws = []

    def fresh(shape):
        z = _randn(shape, generator=gen)
        if first_is_image and not draws:
            z = z * scale
        draws.append(z)
        return z
    clamped = []
    h = clamp_probe(diff, clamped)
    with patched_draws(fresh, torch.float32) as p32, torch.no_grad():
        r32 = call(diff)
    h.remove()
    d64 = copy.deepcopy(diff).double()
    it = iter(draws)
    torch.set_default_dtype(torch.float64)      # the time embedding's arange / exp too (diffusion.py:100-107)
    try:
        with patched_draws(lambda shape: next(it), torch.float64) as p64, torch.no_grad():
            r64 = call(d64)
    finally:
        torch.set_default_dtype(torch.float32)
    assert [r[:2] for r in p64.ddim] == [r[:2] for r in p32.ddim]        # the same timesteps in both runs
    assert next(it, None) is None and r64.dtype == torch.float64 and r32.dtype == torch.float32
    steps32 = r32 if r32.dim() == 5 else r32[:, None]
    steps64 = r64 if r64.dim() == 5 else r64[:, None]
    eref = (steps32.double() - steps64).abs().amax(dim=(0, 2, 3, 4)).numpy()
    keep = steps64[:, 1:] if r64.dim() == 5 else steps64           # step 0 of a sampler is draw 0
    hi = keep.float()
    lo = ((keep - hi.double()) / LO_UNIT).to(torch.float16)
    assert float((hi.double() + lo.double() * LO_UNIT - keep).abs().max()) < 1e-9
    cl = np.array(clamped)
    assert cl.max() >= 0.01 and (1 - cl).max() >= 0.01, (tag, cl)
    out.update({f"{tag}_seed": np.array(seed), f"{tag}_scale": np.array(scale, dtype=np.float32),
                f"{tag}_draw_sums": np.array([float(z.double().sum()) for z in draws]),
                f"{tag}_eref": eref, f"{tag}_clamped": cl})
    more.update({f"{tag}_f64_hi": hi.numpy(), f"{tag}_f64_lo": lo.numpy()})
    if p32.ddim:
        out[f"{tag}_pairs"] = np.array(p32.pairs, dtype=np.int64)
        out[f"{tag}_coef"] = np.array([r[2:] for r in p32.ddim], dtype=np.float32)
    print(f"{tag}: {len(draws)} draws, E_ref per step {eref}, clamped fraction per step {np.round(cl, 3)}")


class _Zero(torch.nn.Module):
    """Stub network for reading the reference's schedule: the step scalars do not depend on the model."""
    channels, out_dim, self_condition = 1, 1, False

    def forward(self, x, t, x_self_cond=None):
        return torch.zeros_like(x)


def schedule_only(S, eta, out):
    diff = ref.diffusion.GaussianDiffusion(_Zero(), image_size=8, timesteps=1000, sampling_timesteps=S,
                                           objective="pred_noise", ddim_sampling_eta=eta)
    with patched_draws(lambda shape: torch.zeros(shape), torch.float32) as p, torch.no_grad():
        diff.sample(batch_size=1)
    tag = f"sched_S{S}_eta{int(eta)}"
    out[f"{tag}_pairs"] = np.array(p.pairs, dtype=np.int64)
    out[f"{tag}_coef"] = np.array([r[2:] for r in p.ddim], dtype=np.float32)
    assert [r[:2] for r in p.ddim] == p.pairs[:-1] and p.pairs[-1][1] == -1


def main():
    torch.set_num_threads(8)
    net = G._unet_dim8()
    sd = np.load(os.path.join(HERE, "unet_dim8.npz"))
    for k, v in net.state_dict().items():
        assert np.array_equal(v.numpy(), sd["sd." + k]), k        # the GPU test loads unet_dim8.npz's weights
    GD = ref.diffusion.GaussianDiffusion
    out, more_a, more_b = {}, {}, {}

    def all_steps(d):
        return d.sample(batch_size=2, return_all_timesteps=True)
    d = GD(net, image_size=72, timesteps=1000, sampling_timesteps=6, objective="pred_noise").eval()
    run_case("ddim0", d, all_steps, 101, 1.0, out, more_a)
    d = GD(net, image_size=72, timesteps=1000, sampling_timesteps=6, objective="pred_noise",
           ddim_sampling_eta=1.0).eval()
    run_case("ddim1", d, all_steps, 102, 1.0, out, more_b)
    d8 = GD(net, image_size=72, timesteps=8, objective="pred_noise").eval()
    assert not d8.is_ddim_sampling
    run_case("anc", d8, all_steps, 103, 1.0, out, more_b)
    g = torch.Generator().manual_seed(104)
    x1, x2 = (torch.rand(SHAPE, generator=g) * 2 - 1 for _ in range(2))
    out["interp_x1"], out["interp_x2"] = x1.numpy(), x2.numpy()
    run_case("interp", d8, lambda dd: dd.interpolate(x1.to(dd.betas.dtype), x2.to(dd.betas.dtype), t=5, lam=0.3),
             105, 1.0, out, more_a, first_is_image=False)
    d = GD(net, image_size=72, timesteps=1000, sampling_timesteps=3, objective="pred_v").eval()
    run_case("ddim_v", d, all_steps, 106, 1.0, out, more_a)
    for S in (6, 250):
        for eta in (0.0, 1.0):
            schedule_only(S, eta, out)
    for name, arrays in (("sampling_dim8", {**out, **more_a}), ("sampling_dim8_more", more_b)):
        G.save(name, **arrays)
        assert os.path.getsize(os.path.join(HERE, name + ".npz")) <= 1 << 20, name


if __name__ == "__main__":
    main()
