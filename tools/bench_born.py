"""Cost of the linearised (Born) forward, FWIForward.born, and of the Gauss-Newton product at configs[1]
(70 x 70 OpenFWI model, nbc 120, 8 shots, nt = 1000, B = 1).

Legs, alternated inside one process, device events, --warmup untimed then --reps timed repeats, one JSON line
per leg (ms as median and min - max), printed and appended to --out:
  born_pass          the Born prologue + time loop over a stored history (FwiPlan.born)
  born_pass_fields   the same reading alpha / kappa / v from the K3 fields instead of regenerating them
                     (set_variant(fwd_gen_coeffs=False))
  fwd_hist_narrow    the narrow chunked forward that keeps the history (set_persistent(0), wide_chunked=False)
  adj_narrow         the narrow chunked adjoint over the same history: the Born pass's yardstick, it reads the same
                     history stream and does the same two stencils per step
  gauss_newton       FWIForward.gauss_newton on the plan's defaults: forward with history + Born + adjoint + finalize
  born               FWIForward.born on the plan's defaults: K3 + forward with history + Born prologue and pass
  born_fused         FWIForward.born(history=False): K3 + prologue + the fused forward + tangent pass, no history
  gauss_newton_fused FWIForward(checkpoint=40).gauss_newton(history=False): the fused pass writing the checkpoint
                     store, the checkpointed adjoint (recompute + adjoint per segment), finalize
The last four legs also report peak_bytes: the rise of torch.cuda.max_memory_allocated over one call (measured in
a pass of its own after the timed repeats).
--no-born runs only the legs that need no Born interface and --no-fused leaves out the history=False legs, so the
script can be pointed at an earlier checkout.

python tools/bench_born.py [--reps 7] [--no-born] [--out profiles/r14/born.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "red-diffeq_amd"))
from red_diffeq.solvers.pde import FWIForward  # noqa: E402
from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize, v_normalize  # noqa: E402
from red_diffeq.utils.synthetic import make_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-born", action="store_true")
ap.add_argument("--no-fused", action="store_true")
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "born.jsonl"))
a = ap.parse_args()
dev = torch.device("cuda:0")
nz = nx = 70
ctx = dict(n_grid=nx, nt=1000, dx=10.0, dt=0.001, nbc=120, f=15.0, sz=10, gz=10, ng=nx, ns=8)
v = v_normalize(torch.from_numpy(make_model("curvefault", nz, nx, batch=1))).to(dev)
gen = torch.Generator(device=dev).manual_seed(14)
dv = 0.05 * torch.randn(v.shape, generator=gen, device=dev)


def operator():
    return FWIForward(dict(ctx), dev, v_denorm_func=v_denormalize, s_norm_func=s_normalize_none)


narrow = operator()
plan = narrow._plan(nz, nx, dev)
plan.set_persistent(0)
plan.set_variant(wide_chunked=False)
default = operator()
fields = operator()
fplan = fields._plan(nz, nx, dev)
fplan.set_persistent(0)
fplan.set_variant(fwd_gen_coeffs=False, wide_chunked=False)
with torch.no_grad():
    coeffs, vstat = plan.coeffs(v, 0)
    seis, hist = plan.forward(coeffs, 1, True)
w = torch.randn(seis.shape, generator=gen, device=dev)

legs = {"fwd_hist_narrow": lambda: plan.forward(coeffs, 1, True),
        "adj_narrow": lambda: plan.adjoint(coeffs, hist, w, 1)}
if not a.no_born:
    legs["born_pass"] = lambda: plan.born(coeffs, vstat, hist, dv, 1, 0)
    legs["born_pass_fields"] = lambda: fplan.born(coeffs, vstat, hist, dv, 1, 0)
    legs["gauss_newton"] = lambda: default.gauss_newton(v, dv)
    legs["born"] = lambda: default.born(v, dv)
    if not a.no_fused:
        ckpt40 = FWIForward(dict(ctx), dev, v_denorm_func=v_denormalize, s_norm_func=s_normalize_none, checkpoint=40)
        legs["born_fused"] = lambda: default.born(v, dv, history=False)
        legs["gauss_newton_fused"] = lambda: ckpt40.gauss_newton(v, dv, history=False)
NARROW = ("fwd_hist_narrow", "adj_narrow", "born_pass", "born_pass_fields")
times = {name: [] for name in legs}
with torch.no_grad():
    for i in range(a.warmup + a.reps):          # the legs alternate: drift hits all of them alike
        for name, run in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
peak = {}
for name in ("born", "born_fused", "gauss_newton", "gauss_newton_fused"):
    if name in legs:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        legs[name]()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
narrow.check()
default.check()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
for name, t in times.items():
    rec = {"leg": name, "grid": [nz, nx], "nbc": ctx["nbc"], "ns": ctx["ns"], "nt": ctx["nt"], "B": 1,
           "ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
           "reps": len(t), "launch": (narrow if name in NARROW else default)._plan(nz, nx, dev).launch_info(1)}
    if name == "born_fused":                  # no persistent or wide kernel runs in this leg
        depth = rec["launch"]["fwd_T"]
        rec["launch"] = f"narrow chunked fused pass, {-(-ctx['nt'] // depth)} launches of {depth} steps"
    if name == "gauss_newton_fused":
        rec["launch"] = dict(ckpt40._plan(nz, nx, dev).ckpt_info(1, 40), fused="narrow chunked fused pass, K = 40")
    if name in peak:
        rec["peak_bytes"] = peak[name]
        rec["history_bytes"] = int(default._plan(nz, nx, dev).sizes(1).history)
    if a.label:
        rec["label"] = a.label
    print(json.dumps(rec), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
