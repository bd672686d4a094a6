"""The illumination pass on the MI355X: what it costs alone, end to end, and inside the engine.

    python tools/bench_illumination.py [--config 1|4] [--rounds 5] [--calls 10] [--parts abc]
                                       [--out profiles/r27/illumination.jsonl]

configs[1] (70 x 70 OpenFWI model, 8 shots, nt = 1000, B = 1; the default):
  (a) rdq_fwi_illum alone over a stored history, through the raw ABI on caller-owned buffers: after the first call
      every call replays the plan's captured graph, so `calls` back-to-back calls between two device events time the
      device (one graph launch per ~ms of kernel).  History bytes read (nt levels) per second against the measured
      copy rate of the chip (6.29 TB/s: a copy moves two bytes per byte counted there, this pass reads only).  The
      narrow chunked adjoint over the same history runs in the same process and the same rounds, for scale.
  (b) FWIForward.illumination(v) end to end (K3, forward with history, pass, finalize), store-all and checkpoint=40.
  (c) an InversionEngine TV iteration with precondition_every in {1, 10} against precondition=None, alternated in one
      process: ms per iteration from whole optimize() calls of --iters iterations, medians and min - max over rounds.
--config 4 (500 x 3000 model, 16 shots: one rank's share of configs[4]): the store-all history does not fit the
  budget, so illumination() runs the checkpointed first pass and rdq_fwi_illum_ckpt; (b) only, next to a no-grad
  forward for scale.
One JSON line per measurement, appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "red-diffeq_amd"))
from red_diffeq import _hip  # noqa: E402
from red_diffeq.solvers.pde import FWIForward  # noqa: E402
from red_diffeq.utils.data_trans import prepare_initial_model, s_normalize_none, v_denormalize, v_normalize  # noqa: E402
from red_diffeq.utils.synthetic import make_model  # noqa: E402

COPY_TBS = 6.29

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=1, choices=(1, 4))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--budget-gb", type=float, default=32.0)
ap.add_argument("--parts", default="abc", help="which of (a), (b), (c) to run at configs[1]")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27", "illumination.jsonl"))
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_illumination.py measures on the MI355X: no ROCm device visible")
dev = torch.device("cuda:0")
nz, nx, ns = (70, 70, 8) if a.config == 1 else (500, 3000, 16)
ctx = dict(n_grid=nx, nt=1000, dx=10.0, dt=0.001, nbc=120, f=15.0, sz=10, gz=10, ng=nx, ns=ns)
vt = torch.from_numpy(make_model("curvefault", nz, nx, batch=1))
v0 = v_normalize(vt).to(dev)


def operator(**kw):
    return FWIForward(dict(ctx), dev, v_denorm_func=v_denormalize, s_norm_func=s_normalize_none, **kw)


def emit(rec):
    rec = {"config": a.config, "grid": [nz, nx], "ns": ns, "nt": ctx["nt"], **rec}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def device_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def spread(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
            "rounds": len(ts)}


def alternate(cases, rounds, calls):
    for fn in cases.values():                     # warm-up: code objects, graph capture, the allocator's blocks
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            ms[k].append(device_ms(fn, calls))
    return ms


if a.config == 4:
    fwi = operator(history_budget_gb=a.budget_gb)
    plan = fwi._plan(nz, nx, dev)
    K = fwi.checkpoint_interval(plan, 1)

    def fwd():
        with torch.no_grad():
            fwi(v0)
    ms = alternate({"illumination_ckpt": lambda: fwi.illumination(v0), "no_grad_forward": fwd}, a.rounds, 1)
    fwi.check()
    for k, t in ms.items():
        emit({"case": k, "history_budget_gb": a.budget_gb, "K": K, "store_all_history_bytes": int(plan.sizes(1).history),
              **spread(t)})
    sys.exit(0)

# ---- (a) the pass alone, and the narrow chunked adjoint over the same history
fwi = operator()
plan = fwi._plan(nz, nx, dev)
sz = plan.sizes(1)
coeffs, _ = plan.coeffs(v0, 0)
hist = plan.forward(coeffs, 1, True)[1]
hA = torch.empty(int(sz.gA) // 4, device=dev)
dseis = torch.randn(1, ns, sz.nrec, plan.ng, device=dev)
st = _hip.stream_of(hist)


def illum():
    _hip.check(plan.lib.rdq_fwi_illum(plan.handle, 1, 0, _hip.ptr(hist), _hip.ptr(hA), st), "rdq_fwi_illum")


narrow = operator()
nplan = narrow._plan(nz, nx, dev)
nplan.set_persistent(False)
nplan.set_variant(wide_chunked=False)
assert not nplan.launch_info(1)["adj_persistent"]
ms = alternate({"illum": illum, "adjoint_narrow_chunked": lambda: nplan.adjoint(coeffs, hist, dseis, 1)}, a.rounds,
               a.calls)
plan.status()
nplan.status()
read = ctx["nt"] * ns * sz.Hp * sz.ld * 4          # nt levels of every wavefield, pitch included (the rows are contiguous)
for k, t in ms.items():
    med = statistics.median(t)
    rec = {"case": "a_" + k, "history_bytes_read": int(read), **spread(t), "calls_per_round": a.calls,
           "TB_per_s": round(read / med / 1e9, 3), "fraction_of_copy_rate": round(read / med / 1e9 / COPY_TBS, 3)}
    if k == "illum":
        rec["ratio_to_adjoint"] = round(med / statistics.median(ms["adjoint_narrow_chunked"]), 3)
        rec["workgroups"] = int((sz.Hp + 59) // 60 * ((sz.Wp + 59) // 60) * ns)
    emit(rec)
del hist, hA
if "b" not in a.parts and "c" not in a.parts:
    sys.exit(0)

# ---- (b) end to end
ck = operator(checkpoint=40)
ms = alternate({"illumination_store_all": lambda: fwi.illumination(v0),
                "illumination_checkpoint40": lambda: ck.illumination(v0)}, a.rounds, 1)
fwi.check()
ck.check()
for k, t in ms.items():
    emit({"case": "b_" + k, **spread(t), "launch": plan.launch_info(1)})

# ---- (c) the engine's TV iteration
from red_diffeq.core.inversion import InversionEngine  # noqa: E402
from red_diffeq.utils.ssim import SSIM  # noqa: E402

with torch.no_grad():
    y = fwi(v0)
mu0 = torch.nn.functional.pad(prepare_initial_model(vt, "smoothed", sigma=10.0), (1, 1, 1, 1))


class dm:
    device = dev


def engine_ms(**kw):
    eng = InversionEngine(dm, SSIM(window_size=11), "tv", show_progress=False, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.optimize(mu0, vt, y, fwi, ts=a.iters, lr=0.03, reg_lambda=0.01, regularization="tv")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / a.iters


cases = {"none": dict(precondition=None), "every_10": dict(precondition="illumination", precondition_every=10),
         "every_1": dict(precondition="illumination", precondition_every=1)}
for kw in cases.values():
    engine_ms(**kw)                               # warm-up
times = {k: [] for k in cases}
for _ in range(a.rounds):
    for k, kw in cases.items():
        times[k].append(engine_ms(**kw))
fwi.check()
base = statistics.median(times["none"])
for k, t in times.items():
    emit({"case": "c_engine_tv_" + k, "iters_per_call": a.iters, **spread(t),
          "ratio_to_none": round(statistics.median(t) / base, 3)})
