"""Prior sampling on one MI355X: what a reverse step costs on top of the U-Net forward it follows.

dim-64 U-Net (random init), 72 x 72, B = 1 and 16; DDIM with S = 50 of T = 1000 and ancestral with T = 50.
Per (B, sampler), event-timed after a warm-up call (graph capture, schedule and timestep tables):
  ms_per_step          GaussianDiffusion.ddim_sample / p_sample_loop: replay + fused step (rdq_sample_step) + randn
  ms_per_replay        the bare Unet.replay_static of the same shape, back to back
  step_overhead_ms     the difference
  ms_per_step_torch    the same loop on the same replays with the step done by torch elementwise ops: the
                       reference's expressions (diffusion.py:411-446, 469-494) restated below
and one line for sample(batch_size=16) of the model the default config builds (250 DDIM steps).
python tools/bench_sampling.py [--reps 3] [--out profiles/r12/sampling.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "red-diffeq_amd"))
from red_diffeq.config.default_config import get_config  # noqa: E402
from red_diffeq.models.diffusion import GaussianDiffusion, Unet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(8888)
net = Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=1).to(dev).eval()


def timed(fn):
    """Median of --reps event timings of fn(), in ms."""
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


@torch.no_grad()
def torch_loop(d, shape, ddim):
    """The reference's loop with torch elementwise ops, on the captured forward's static buffers."""
    xs, ts = d.model.graph_io(shape, dev)
    xs.copy_(torch.randn(shape, device=dev))
    pairs = d._ddim_schedule()[0] if ddim else [(t, t - 1) for t in reversed(range(d.num_timesteps))]
    for time, time_next in pairs:
        ts.fill_(time)
        out = d.model.replay_static(xs, ts)
        x_start = d.predict_start_from_noise(xs, ts, out).clamp_(-1.0, 1.0)
        if not ddim:
            mean, _, logvar = d.q_posterior(x_start=x_start, x_t=xs, t=ts)
            noise = torch.randn_like(xs) if time > 0 else 0.0
            img = mean + (0.5 * logvar).exp() * noise
        elif time_next < 0:
            img = x_start
        else:
            pred_noise = d.predict_noise_from_start(xs, ts, x_start)
            alpha, alpha_next = d.alphas_cumprod[time], d.alphas_cumprod[time_next]
            sigma = d.ddim_sampling_eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            c = (1 - alpha_next - sigma ** 2).sqrt()
            img = x_start * alpha_next.sqrt() + c * pred_noise + sigma * torch.randn_like(xs)
        xs.copy_(img)
    return d.unnormalize(xs.clone())


lines = []
for B in (1, 16):
    shape = (B, 1, 72, 72)
    for name, kw in (("ddim S=50 of T=1000", dict(timesteps=1000, sampling_timesteps=50)),
                     ("ancestral T=50", dict(timesteps=50))):
        d = GaussianDiffusion(net, image_size=72, objective="pred_noise", **kw).to(dev).eval()
        steps, ddim = d.sampling_timesteps, d.is_ddim_sampling
        with torch.no_grad():
            io = d.model.graph_io(shape, dev)

        def replays():
            for _ in range(steps):
                d.model.replay_static(*io)
        d.sample(batch_size=B)
        torch_loop(d, shape, ddim)
        fused = timed(lambda: d.sample(batch_size=B)) / steps
        bare = timed(replays) / steps
        plain = timed(lambda: torch_loop(d, shape, ddim)) / steps
        lines.append({"workload": f"prior sampling, dim-64 U-Net (random init), 72x72, B={B}, {name}", "B": B,
                      "steps": steps, "precision": net.precision, "ms_per_step": round(fused, 4),
                      "ms_per_replay": round(bare, 4), "step_overhead_ms": round(fused - bare, 4),
                      "ms_per_step_torch": round(plain, 4), "torch_step_overhead_ms": round(plain - bare, 4)})
        print(json.dumps(lines[-1]), flush=True)

cfg = get_config()
d = GaussianDiffusion(net, image_size=cfg.diffusion.image_size, timesteps=cfg.diffusion.timesteps,
                      sampling_timesteps=cfg.diffusion.sampling_timesteps,
                      objective=cfg.diffusion.objective).to(dev).eval()
d.sample(batch_size=16)
out = []
ms = timed(lambda: out.append(d.sample(batch_size=16)))
s = out[-1]
lines.append({"workload": "sample(batch_size=16), default config (DDIM 250 of 1000), random-init dim-64 U-Net",
              "shape": list(s.shape), "min": float(s.min()), "max": float(s.max()), "ms_total": round(ms, 2),
              "ms_per_step": round(ms / d.sampling_timesteps, 4)})
print(json.dumps(lines[-1]), flush=True)
assert tuple(s.shape) == (16, 1, 72, 72) and 0.0 <= lines[-1]["min"] and lines[-1]["max"] <= 1.0
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)
