"""Cost of a forward + backward with caller-supplied source wavelets, forward(v, wavelet=w), at configs[1]
(70 x 70 OpenFWI model, nbc 120, 8 shots, nt = 1000, B = 1).

Legs, alternated inside one process, device events around forward + backward of <seis, r>, --warmup untimed then
--reps timed repeats, one JSON line per leg (ms as median and min - max), printed and appended to --out:
  default          fwi(v) on the plan's defaults (the persistent kernels here)
  default_narrow   fwi(v) pinned to the narrow chunked kernels (set_persistent(0), wide_chunked=False): the kernels
                   a per-call wavelet runs on, so the yardstick of the next leg
  wavelet          fwi(v, wavelet=w), w (ns, nt) with requires_grad: dL/dv and dL/dw
  wavelet_ckpt40   the same on FWIForward(checkpoint=40)
The first two legs use no wavelet interface, so --no-wavelet runs the script on an earlier checkout.

python tools/bench_wavelet.py [--reps 7] [--no-wavelet] [--label parent] [--out profiles/r19/wavelet.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "red-diffeq_amd"))
from red_diffeq.solvers.pde import FWIForward, ricker  # noqa: E402
from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize, v_normalize  # noqa: E402
from red_diffeq.utils.synthetic import make_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-wavelet", action="store_true")
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "wavelet.jsonl"))
a = ap.parse_args()
dev = torch.device("cuda:0")
nz = nx = 70
ctx = dict(n_grid=nx, nt=1000, dx=10.0, dt=0.001, nbc=120, f=15.0, sz=10, gz=10, ng=nx, ns=8)
v = v_normalize(torch.from_numpy(make_model("curvefault", nz, nx, batch=1))).to(dev)
gen = torch.Generator(device=dev).manual_seed(19)


def operator(**kw):
    return FWIForward(dict(ctx), dev, v_denorm_func=v_denormalize, s_norm_func=s_normalize_none, **kw)


default, narrow = operator(), operator()
plan = narrow._plan(nz, nx, dev)
plan.set_persistent(0)
plan.set_variant(wide_chunked=False)
with torch.no_grad():
    r = torch.randn(default(v).shape, generator=gen, device=dev)
# per-shot wavelets: the Ricker wavelet of ctx with a per-shot amplitude
w0 = torch.from_numpy(ricker(ctx["f"], ctx["dt"], ctx["nt"])).float().to(dev)
w0 = w0[None, :] * torch.linspace(0.5, 1.5, ctx["ns"], device=dev)[:, None]


def step(fwi, wavelet):
    def run():
        vv = v.clone().requires_grad_(True)
        if wavelet:
            w = w0.clone().requires_grad_(True)
            seis = fwi(vv, wavelet=w)
        else:
            seis = fwi(vv)
        (seis * r).sum().backward()
    return run


legs = {"default": step(default, False), "default_narrow": step(narrow, False)}
ops = {"default": default, "default_narrow": narrow}
if not a.no_wavelet:
    ops["wavelet"], ops["wavelet_ckpt40"] = operator(), operator(checkpoint=40)
    legs["wavelet"], legs["wavelet_ckpt40"] = step(ops["wavelet"], True), step(ops["wavelet_ckpt40"], True)
times = {name: [] for name in legs}
for i in range(a.warmup + a.reps):              # the legs alternate: drift hits all of them alike
    for name, run in legs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            times[name].append(e0.elapsed_time(e1))
for fwi in ops.values():
    fwi.check()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
for name, t in times.items():
    p = ops[name]._plan(nz, nx, dev)
    rec = {"leg": name, "grid": [nz, nx], "nbc": ctx["nbc"], "ns": ctx["ns"], "nt": ctx["nt"], "B": 1,
           "ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
           "reps": len(t)}
    if name == "default" or name == "default_narrow":
        rec["launch"] = p.launch_info(1)
    else:                                       # no persistent or wide kernel runs in these legs
        rec["launch"] = "narrow chunked kernels with the call's wavelets, depth 4, one chain" + \
            (f"; {p.ckpt_sizes(1, 40).nseg} segments of 40 steps" if name == "wavelet_ckpt40" else "")
    if a.label:
        rec["label"] = a.label
    print(json.dumps(rec), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
