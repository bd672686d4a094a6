"""The per-trace yardstick of the Born tests (tests/test_born_host.py, tests/test_gpu_born_terms.py), in numpy
and from the fixtures alone, and the `terms` fixture's directions (tests/golden/born_terms.npz).

A record is (B, ns, nrec, ng); trace (b, s, g) is record[b, s, :, g].  For every trace
    n64   = ||jdv64||                      the reference's fp64 J dv on that trace
    N_b   = max of n64 over model b
    e_ref = ||jdv32 - jdv64|| / n64        the reference's own fp32 jvp error on that trace
and a record `ds` meets the criterion with factor k when, on every trace,
    ||ds - jdv64||  <=  k max(e_ref, E_ref[b]) max(n64, FLOOR N_b).
The yardstick never depends on the record under test."""
import numpy as np

from conftest import load_golden

FLOOR = 1e-12
DIRECTIONS = ("argmin", "source", "corner", "edge", "interior")
DENSE = ("wrap", "tiles", "geom")


def trace_norm(a):
    """(B, ns, nrec, ng) -> (B, ns, ng), in fp64."""
    return np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum(axis=2))


def trace_yardstick(jdv64, jdv32, eref):
    """(n64, e_ref, bar at factor 1), each (B, ns, ng)."""
    n64 = trace_norm(jdv64)
    err32 = trace_norm(jdv32.astype(np.float64) - jdv64)
    big = n64.reshape(n64.shape[0], -1).max(axis=1)[:, None, None]
    # max(e_ref, E_ref) max(n64, FLOOR N_b) with n64 taken out of both factors, so that no rounding of e_ref =
    # err32 / n64 comes between the reference's fp32 record and its own bar
    bar = np.maximum(err32, np.asarray(eref)[:, None, None] * n64) * np.maximum(1.0, FLOOR * big / n64)
    return n64, err32 / n64, bar


def trace_ratio(ds, jdv64, jdv32, eref):
    """||ds - jdv64|| over the factor-1 bar, per trace."""
    return trace_norm(np.asarray(ds, dtype=np.float64) - jdv64) / trace_yardstick(jdv64, jdv32, eref)[2]


def records(case):
    """(jdv64, jdv32, E_ref) of a dense case of born.npz or of "terms/<direction>" of born_terms.npz."""
    if case.startswith("terms/"):
        z, pre = load_golden("born_terms"), "terms_" + case[len("terms/"):]
    else:
        z, pre = load_golden("born"), case
    return z[f"{pre}_jdv64"], z[f"{pre}_jdv32"], z[f"{pre}_eref"]


ALL = DENSE + tuple(f"terms/{d}" for d in DIRECTIONS)
