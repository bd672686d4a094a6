"""Cost of a forward + backward of encoded supershots, forward(v, encoding=E), against the per-shot gradient.

--config 1 (default): configs[1], 70 x 70 OpenFWI model, nbc 120, 8 shots, nt = 1000, B = 1.  Legs:
  wavelet        fwi(v, wavelet=w), w (ns, nt) with requires_grad: the per-shot call on the same narrow chunked
                 kernels, the baseline (tools/bench_wavelet.py's leg; it uses no encoding interface, so
                 --baseline-only runs the script on the parent checkout)
  enc_ne{1,2,8}  fwi(v, encoding=E), E (ne, ns) random signs with requires_grad: dL/dv and dL/dE
--config 4: the configs[4] grid (500 x 3000 model, 740 x 3240 padded, nt = 1000) with 16 shots, B = 1.  Legs:
  plain_budget64 fwi(v) on FWIForward(history_budget_gb=64): the per-shot gradient as a user runs it at this size
                 (its store-all history is 155 GB), dL/dv only
  enc_ne{1,4}    fwi(v, encoding=E) store-all, dL/dv only (E without requires_grad: no gwav)

The legs alternate inside one process: device events around forward + backward of <seis, r>, --warmup untimed then
--reps timed repeats.  After the timing, each leg runs once more alone between reset_peak_memory_stats and
max_memory_allocated: its peak HBM as torch sees it (the tensors of the operators and the inputs included).  One JSON
line per leg (ms as median and min - max, peak GB), printed and appended to --out.

python tools/bench_encoding.py [--config 1|4] [--reps 7] [--baseline-only] [--label parent] [--out FILE]"""
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
ap.add_argument("--config", type=int, default=1, choices=(1, 4))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--baseline-only", action="store_true")
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "encoding.jsonl"))
a = ap.parse_args()
dev = torch.device("cuda:0")
if a.config == 1:
    nz, nx, ns, nes = 70, 70, 8, (1, 2, 8)
else:
    nz, nx, ns, nes = 500, 3000, 16, (1, 4)
ctx = dict(n_grid=nx, nt=1000, dx=10.0, dt=0.001, nbc=120, f=15.0, sz=10, gz=10, ng=nx, ns=ns)
v = v_normalize(torch.from_numpy(make_model("curvefault", nz, nx, batch=1))).to(dev)
gen = torch.Generator(device=dev).manual_seed(21)
nrec = ctx["nt"]


def operator(**kw):
    return FWIForward(dict(ctx), dev, v_denorm_func=v_denormalize, s_norm_func=s_normalize_none, **kw)


def residual(nwf):
    return torch.randn(1, nwf, nrec, ctx["ng"], generator=gen, device=dev)


def step(fwi, r, wavelet=None, encoding=None, grad_inputs=True):
    def run():
        vv = v.clone().requires_grad_(True)
        kw = {}
        if wavelet is not None:
            kw["wavelet"] = wavelet.clone().requires_grad_(grad_inputs)
        if encoding is not None:
            kw["encoding"] = encoding.clone().requires_grad_(grad_inputs)
        seis = fwi(vv, **kw)
        (seis * r).sum().backward()
    return run


legs, ops, notes = {}, {}, {}
if a.config == 1:
    w0 = torch.from_numpy(ricker(ctx["f"], ctx["dt"], ctx["nt"])).float().to(dev)
    w0 = w0[None, :] * torch.linspace(0.5, 1.5, ns, device=dev)[:, None]
    ops["wavelet"] = operator()
    legs["wavelet"] = step(ops["wavelet"], residual(ns), wavelet=w0)
    notes["wavelet"] = "narrow chunked kernels with the call's wavelets, depth 4, one chain; dL/dv and dL/dw"
else:
    ops["plain_budget64"] = operator(history_budget_gb=64)
    legs["plain_budget64"] = step(ops["plain_budget64"], residual(ns))
if not a.baseline_only:
    from red_diffeq.utils.encoding import random_encoding  # noqa: E402
    for ne in nes:
        name = f"enc_ne{ne}"
        E = random_encoding(ne, ns, "sign", generator=gen, device=dev)
        ops[name] = operator()
        legs[name] = step(ops[name], residual(ne), encoding=E, grad_inputs=a.config == 1)
        notes[name] = f"narrow chunked ENC kernels, depth 4, one chain, store-all; {ne} supershots of {ns} sources; " + \
            ("dL/dv and dL/dE" if a.config == 1 else "dL/dv")
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
peak = {}
for name, run in legs.items():                  # peak memory of one more repeat of each leg alone
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    run()
    torch.cuda.synchronize()
    peak[name] = torch.cuda.max_memory_allocated(dev) / 1e9
for fwi in ops.values():
    fwi.check()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
for name, t in times.items():
    p = ops[name]._plan(nz, nx, dev)
    rec = {"leg": name, "config": a.config, "grid": [nz, nx], "nbc": ctx["nbc"], "ns": ns, "nt": ctx["nt"], "B": 1,
           "ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
           "reps": len(t), "peak_GB": round(peak[name], 3)}
    if name == "plain_budget64":
        K = ops[name].checkpoint_interval(p, 1)
        rec["launch"] = dict(p.launch_info(1), checkpoint_K=K, store_all_history_GB=round(p.sizes(1).history / 1e9, 1))
    else:
        rec["launch"] = notes[name]
    if a.label:
        rec["label"] = a.label
    print(json.dumps(rec), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
