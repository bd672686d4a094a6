"""Data misfits on the MI355X: device-event time of forward + backward of K5 (L1) and of K13's L2, Huber and NCC
(csrc/misfit.hip) through torch.ops.red_diffeq, and the achieved bytes/s from the bytes the definitions move.

    python tools/bench_misfit.py [--rounds 5] [--calls 20] [--graph] [--out FILE]

Sizes: configs[1]'s record (1, 8, 1000, 70), the B = 25 yaml's (25, 5, 1000, 70) and configs[4]'s per-rank record
(1, 16, 1000, 3000), as tools/l1_large.py.  No mask (the engine passes none unless traces are missing).  In every
round K5 is timed first, then each kind, so that K5's own round-to-round spread stands next to every ratio; one
JSON line per (size, kind): the median, min and max over the rounds of the ms per forward + backward, the bytes
moved, GB/s at the median, and the ratio of the medians to K5's.  At the two small sizes the stream-timed figure is
the host's enqueue time of the five launches, not the kernels'; --graph adds the time of the same calls captured
in one graph and replayed (ms_in_graph), which is the device's alone.

Bytes (fp32 operands of n elements per call, no mask): forward reads pred and y (8 n), backward reads them and
writes dpred (12 n); the partial slabs are written once and read once (16 bytes per chunk pair for L1 / L2 /
Huber; for NCC 24 bytes per (trace, time chunk) twice, the (inv, r, J) coefficients written once, and 16 of
their 24 bytes per trace read by the backward, from L2)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "red-diffeq_amd"))
from red_diffeq import _hip, ops  # noqa: E402

SIZES = ((1, 8, 1000, 70), (25, 5, 1000, 70), (1, 16, 1000, 3000))
HUBER_DELTA = 0.5


def bytes_moved(kind, shape):
    B, ns, nt, ng = shape
    n = B * ns * nt * ng
    L = _hip.lib()
    if kind == "ncc":
        ws = L.rdq_misfit_workspace_bytes(3, B, ns, nt, ng)
        return 20 * n + 2 * ws + (24 + 16) * B * ns * ng
    ws = L.rdq_l1_partial_bytes(B, n // B) if kind == "l1" else L.rdq_misfit_workspace_bytes(1, B, ns, nt, ng)
    return 20 * n + 2 * ws


def call(kind, pred, y, gout):
    if kind == "l1":
        loss, nobs = torch.ops.red_diffeq.l1_misfit(pred, y, None)
        return torch.ops.red_diffeq.l1_misfit_backward(pred, y, None, nobs, gout)
    code, delta = ops.MISFIT_KINDS[kind], HUBER_DELTA if kind == "huber" else 0.0
    loss, norm, coef = torch.ops.red_diffeq.misfit(pred, y, None, code, delta)
    return torch.ops.red_diffeq.misfit_backward(pred, y, None, norm, coef, gout, code, delta)


def timed(kind, pred, y, gout, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call(kind, pred, y, gout)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def timed_graph(kind, pred, y, gout, calls, replays=5):
    """ms per forward + backward with `calls` of them captured in one graph: the device's time without the
    host's enqueue time between the launches (the smallest of `replays` replays)."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            call(kind, pred, y, gout)
    graph.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / calls)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--graph", action="store_true", help="also time the calls captured in one graph (device time alone)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_misfit.py measures on the MI355X: no ROCm device visible")
    kinds = ("l1", "l2", "huber", "ncc")

    def inputs(shape):
        g = torch.Generator(device="cuda").manual_seed(0)
        pred = torch.randn(shape, device="cuda", generator=g)
        return pred, 0.8 * pred + 0.5 * torch.randn(shape, device="cuda", generator=g), torch.ones(shape[0], device="cuda")

    lines = []

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.writelines(json.dumps(x) + "\n" for x in lines)

    for shape in SIZES:
        pred, y, gout = inputs(shape)
        for kind in kinds:                       # warm-up: code objects, the allocator's blocks
            for _ in range(3):
                call(kind, pred, y, gout)
        torch.cuda.synchronize()
        ms = {k: [] for k in kinds}
        for _ in range(a.rounds):
            for kind in kinds:                   # K5 first in every round, each kind right after it
                ms[kind].append(timed(kind, pred, y, gout, a.calls))
        base = statistics.median(ms["l1"])
        for kind in kinds:
            med = statistics.median(ms[kind])
            nbytes = bytes_moved(kind, shape)
            lines.append({"shape": list(shape), "kind": kind, "ms_fwd_bwd_median": round(med, 5),
                          "ms_min": round(min(ms[kind]), 5), "ms_max": round(max(ms[kind]), 5),
                          "rounds": a.rounds, "calls_per_round": a.calls, "bytes": int(nbytes),
                          "GB_per_s": round(nbytes / med / 1e6, 1), "ratio_to_l1": round(med / base, 3)})
            print(json.dumps(lines[-1]), flush=True)
    save()
    if a.graph:                                  # after every stream-timed figure: a second pass over the sizes
        for shape in SIZES:
            pred, y, gout = inputs(shape)
            graph_ms = {kind: timed_graph(kind, pred, y, gout, a.calls) for kind in kinds}
            for line in lines:
                if line["shape"] == list(shape):
                    t = graph_ms[line["kind"]]
                    line.update(ms_in_graph=round(t, 5), GB_per_s_in_graph=round(line["bytes"] / t / 1e6, 1),
                                graph_ratio_to_l1=round(t / graph_ms["l1"], 3))
                    print(json.dumps(line), flush=True)
        save()


if __name__ == "__main__":
    main()
