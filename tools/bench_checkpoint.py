"""Cost of the checkpointed FWI gradient (FWIForward(checkpoint=K)) against the store-all history.

Default: configs[1] (70 x 70 OpenFWI model, 8 shots, nt = 1000, B = 1).  Four cases, alternated inside one
process: store-all on the default (persistent) kernels, store-all on the chunked kernels, checkpointed
with --K steps per segment (first pass, recompute and adjoint all chunked), and a chunked no-grad forward
(the recompute's expected cost: checkpointed ~ store-all chunked + one no-grad forward).  Each case:
forward + backward of one differentiable call, device events, --warmup untimed then --reps timed
repeats; ms as median and min - max, and the peak allocated bytes of one step above what was held before.
One JSON line per case, appended to --out.

--capability: one step of a job whose store-all history cannot be held: the configs[4] grid (500 x 3000)
with --ns shots and a history budget (--budget-gb); K from FWIForward's policy.

python tools/bench_checkpoint.py [--K 40] [--reps 5] [--out profiles/r7/checkpoint.jsonl]
python tools/bench_checkpoint.py --capability --ns 32 --budget-gb 64"""
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
ap.add_argument("--nz", type=int, default=70)
ap.add_argument("--nx", type=int, default=70)
ap.add_argument("--ns", type=int, default=8)
ap.add_argument("--nt", type=int, default=1000)
ap.add_argument("--K", type=int, default=40)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--capability", action="store_true")
ap.add_argument("--budget-gb", type=float, default=64.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "checkpoint.jsonl"))
a = ap.parse_args()
if a.capability and (a.nz, a.nx) == (70, 70):
    a.nz, a.nx = 500, 3000
dev = torch.device("cuda:0")
ctx = dict(n_grid=a.nx, nt=a.nt, dx=10.0, dt=0.001, nbc=120, f=15.0, sz=10, gz=10, ng=a.nx, ns=a.ns)
v0 = v_normalize(torch.from_numpy(make_model("curvefault", a.nz, a.nx, batch=1))).to(dev)


def operator(chunked, **kw):
    fwi = FWIForward(dict(ctx), dev, v_denorm_func=v_denormalize, s_norm_func=s_normalize_none, **kw)
    if chunked:
        fwi._plan(a.nz, a.nx, dev).set_persistent(False)
    return fwi


def step(fwi, w, grad=True):
    """One call (+ backward): (ms, peak bytes above the baseline)."""
    v = v0.clone().requires_grad_(grad)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if grad:
        fwi(v).backward(w)
    else:
        with torch.no_grad():
            fwi(v)
    e1.record()
    torch.cuda.synchronize()
    fwi.check()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base


def emit(rec):
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


plan0 = operator(False)._plan(a.nz, a.nx, dev)
sz = plan0.sizes(1)
w = torch.randn(1, a.ns, sz.nrec, plan0.ng, device=dev)
shape = {"grid": [a.nz, a.nx], "ns": a.ns, "nt": a.nt, "store_all_history_bytes": int(sz.history)}

if a.capability:
    fwi = operator(False, history_budget_gb=a.budget_gb)
    plan = fwi._plan(a.nz, a.nx, dev)
    K = fwi.checkpoint_interval(plan, 1)
    cs = plan.ckpt_sizes(1, K)
    ms, peak = step(fwi, w)
    emit({"case": "capability", **shape, "history_budget_gb": a.budget_gb, "K": K, "nseg": int(cs.nseg),
          "ckpt_bytes": int(cs.ckpt), "seg_bytes": int(cs.seg), "ms_first_step": round(ms, 2), "peak_bytes": int(peak),
          "status": "clean", "launch": plan.launch_info(1), "ckpt_info": plan.ckpt_info(1, K)})
    sys.exit(0)

cases = [("store_all_default", operator(False), True), ("store_all_chunked", operator(True), True),
         (f"checkpoint_K{a.K}_chunked_first_pass", operator(True, checkpoint=a.K), True),
         ("no_grad_forward_chunked", operator(True), False)]
times = {name: [] for name, _, _ in cases}
peaks = {}
for i in range(a.warmup + a.reps):          # the cases alternate: drift hits all of them alike
    for name, fwi, grad in cases:
        ms, peak = step(fwi, w, grad)
        if i >= a.warmup:
            times[name].append(ms)
            peaks[name] = max(peaks.get(name, 0), peak)
for name, fwi, grad in cases:
    plan = fwi._plan(a.nz, a.nx, dev)
    t = times[name]
    rec = {"case": name, **shape, "ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3),
           "ms_max": round(max(t), 3), "reps": len(t), "peak_bytes": int(peaks[name]), "launch": plan.launch_info(1)}
    if fwi.checkpoint:
        cs = plan.ckpt_sizes(1, a.K)
        rec.update(K=a.K, nseg=int(cs.nseg), ckpt_bytes=int(cs.ckpt), seg_bytes=int(cs.seg),
                   ckpt_info=plan.ckpt_info(1, a.K))
    emit(rec)
med = {n: statistics.median(t) for n, t in times.items()}
emit({"case": "expectation", **shape, "K": a.K,
      "checkpoint_ms": round(med[cases[2][0]], 3),
      "store_all_chunked_plus_no_grad_forward_ms": round(med["store_all_chunked"] + med["no_grad_forward_chunked"], 3)})
