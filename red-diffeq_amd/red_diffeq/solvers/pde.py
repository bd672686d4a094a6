"""FWIForward — drop-in for the reference forward operator (red_diffeq/solvers/pde.py:6-93).

Same constructor, same ``ctx`` handling (including the in-place ``sx``/``gx`` mutation,
pde.py:16-24), same ``forward(v) -> seis`` contract: (B,1,H,W) fp32, possibly a non-contiguous
view, to (B, ns, ceil(nt/sample_temporal), ng') fp32, differentiable w.r.t. ``v``.

The compute is the MI355X HIP path (include/red_diffeq_fwi.h): coefficient fields (K3), the whole
time loop (stencil + periodic wrap + source injection + receiver sampling + history store) in one
persistent launch when the survey fits resident on the chip, else temporal-blocked launches of T
steps replayed from a cached hipGraph (K1), and a hand-written discrete adjoint (K2 + K4) as the
autograd backward of the custom operator torch.ops.red_diffeq.fwi (red_diffeq/ops.py) — where the
reference records a ~5 MB-per-shot-step autograd tape, this keeps one fp32 wavefield per step
(store-all history).
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _hip
from .. import ops as _ops   # registers torch.ops.red_diffeq.*
from ..utils.data_trans import s_normalize_none, v_denormalize


def ricker(f, dt, nt):
    """Ricker wavelet, pde.py:26-36 (fp64; raises ValueError when nt is shorter than it)."""
    nw = 2.2 / f / dt
    nw = 2 * np.floor(nw / 2) + 1
    nc = np.floor(nw / 2)
    k = np.arange(nw)
    alpha = (nc - k) * f * dt * np.pi
    beta = alpha ** 2
    w0 = (1 - beta * 2) * np.exp(-beta)
    w = np.zeros(nt)
    w[:len(w0)] = w0
    return w


def adj_sr(sx, sz, gx, gz, dx, nbc):
    """Physical positions -> padded-grid indices, pde.py:54-59 (np.around: half to even)."""
    isx = np.around(sx / dx) + nbc
    isz = np.around(sz / dx) + nbc
    igx = np.around(gx / dx) + nbc
    igz = np.around(gz / dx) + nbc
    return isx.astype("int"), int(isz), igx.astype("int"), int(igz)


class FwiPlan:
    """Owns one C-ABI plan (uploaded geometry + cached hipGraphs) for one device."""

    def __init__(self, nz, nx, ctx, sample_temporal, isx, isz, igx, igz, wavelet, device):
        self.lib = _hip.lib()
        self.device = device
        self._isx = np.ascontiguousarray(isx, np.int32)
        self._igx = np.ascontiguousarray(igx, np.int32)
        self._wav = np.ascontiguousarray(wavelet, np.float64)
        g = _hip.FwiGeom(nz=nz, nx=nx, nbc=int(ctx["nbc"]), nt=int(ctx["nt"]), ns=len(self._isx),
                         ng=len(self._igx), sample_temporal=int(sample_temporal),
                         dx=float(ctx["dx"]), dt=float(ctx["dt"]), isz=int(isz), igz=int(igz),
                         isx=self._isx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                         igx=self._igx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                         wavelet=self._wav.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        self.ns, self.ng, self.nt, self.nz, self.nx = len(self._isx), len(self._igx), int(ctx["nt"]), nz, nx
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _hip.check(self.lib.rdq_fwi_plan_create(ctypes.byref(g), ctypes.byref(h)), "rdq_fwi_plan_create")
        self.handle = h
        self._sizes = {}
        self.persist_mode = 1                      # rdq_fwi_set_persistent mode (the C default: auto)
        self._saved_mode = None                    # mode before fallback_to_chunked (None: not fallen back)
        # status words in torch memory (caller-owned, rdq_fwi_set_status_buffer): word 0 != 0 once a
        # persistent launch gave up; read stream-ordered (Adam guard, async host copies)
        self.status_t = torch.zeros(64, dtype=torch.int32, device=device)
        _hip.check(self.lib.rdq_fwi_set_status_buffer(self.handle, _hip.ptr(self.status_t)),
                   "rdq_fwi_set_status_buffer")
        self.op_id = _ops.register_plan(self)      # integer handle for torch.ops.red_diffeq.fwi*

    def sizes(self, B):
        if B not in self._sizes:
            s = _hip.FwiSizes()
            _hip.check(self.lib.rdq_fwi_sizes(self.handle, B, ctypes.byref(s)), "rdq_fwi_sizes")
            self._sizes[B] = s
        return self._sizes[B]

    def sizes_enc(self, B, ne):
        """rdq_fwi_sizes_t of an encoded call with ne supershots per model (rdq_fwi_sizes_enc): the buffers of
        sizes(B) with ns replaced by ne, and gbeta (B, ne, ns)."""
        key = ("enc", int(B), int(ne))
        if key not in self._sizes:
            s = _hip.FwiSizes()
            _hip.check(self.lib.rdq_fwi_sizes_enc(self.handle, int(B), int(ne), ctypes.byref(s)), "rdq_fwi_sizes_enc")
            self._sizes[key] = s
        return self._sizes[key]

    def ckpt_sizes_enc(self, B, ne, K):
        """ckpt_sizes for an encoded call with ne supershots per model."""
        key = ("ckpt_enc", int(B), int(ne), int(K))
        if key not in self._sizes:
            s = _hip.FwiCkptSizes()
            _hip.check(self.lib.rdq_fwi_ckpt_sizes_enc(self.handle, int(B), int(ne), int(K), ctypes.byref(s)),
                       "rdq_fwi_ckpt_sizes_enc")
            self._sizes[key] = s
        return self._sizes[key]

    def set_graphs(self, enable):
        _hip.check(self.lib.rdq_fwi_set_graphs(self.handle, int(bool(enable))), "rdq_fwi_set_graphs")

    def set_variant(self, fwd_gen_coeffs=True, adj_exact=False, xcd_local=True, wide_chunked=True,
                    chunked_adj_fma=False):
        """fwd_gen_coeffs: chunked forward regenerates coefficients; adj_exact: persistent adjoint in
        the oracle's exact fp32 op order (bit-identical gA) instead of FMA contraction; xcd_local:
        persistent kernels keep whole slices on one XCD with L2-resident neighbour hand-offs;
        wide_chunked: chunked kernels on 128-column regions (two columns per lane) instead of 64;
        chunked_adj_fma: the wide chunked adjoint contracts its stencils into FMAs (opt-in; the default
        chunked adjoint keeps the oracle's exact order)."""
        flags = ((1 if fwd_gen_coeffs else 0) | (2 if adj_exact else 0) | (0 if xcd_local else 4)
                 | (0 if wide_chunked else 8) | (16 if chunked_adj_fma else 0))
        _hip.check(self.lib.rdq_fwi_set_variant(self.handle, flags), "rdq_fwi_set_variant")

    def set_wide_adj_steps(self, steps):
        """Time steps per launch of the wide chunked adjoint (1..6; 0 = the default, 5: fastest at
        configs[4] for both forms); set_tuning's adj_steps
        sets the persistent / narrow chunked adjoints' depth.  Results are identical for every depth."""
        _hip.check(self.lib.rdq_fwi_set_wide_adj_steps(self.handle, int(steps)), "rdq_fwi_set_wide_adj_steps")

    def set_wide_adj_shots(self, shots):
        """Shots per workgroup of the wide chunked adjoint (1..64; 0 = auto, the default: up to 16, from a
        cost model of launch rounds x (shots + a workgroup's fixed cost); the region's alpha / kappa are
        generated once for all of them).  Results are identical for every setting."""
        _hip.check(self.lib.rdq_fwi_set_wide_adj_shots(self.handle, int(shots)), "rdq_fwi_set_wide_adj_shots")

    def set_wide_fwd_steps(self, steps):
        """Time steps per launch of the wide chunked forward (1..6; 0 = set_tuning's fwd_steps).
        Results are identical for every depth."""
        _hip.check(self.lib.rdq_fwi_set_wide_fwd_steps(self.handle, int(steps)), "rdq_fwi_set_wide_fwd_steps")

    def set_wide_fwd_shots(self, shots):
        """Shots per workgroup of the wide chunked forward (as set_wide_adj_shots; 0 = auto)."""
        _hip.check(self.lib.rdq_fwi_set_wide_fwd_shots(self.handle, int(shots)), "rdq_fwi_set_wide_fwd_shots")

    def set_rows_per_wave(self, fwd_rows, adj_rows):
        """Rows per wave of the 64 x 96-region persistent kernels (forward 6 / 8 / 12 / 24, adjoint
        6 / 8 / 12; 6 is the default for both); results are the same for every choice."""
        _hip.check(self.lib.rdq_fwi_set_rows_per_wave(self.handle, int(fwd_rows), int(adj_rows)),
                   "rdq_fwi_set_rows_per_wave")

    def set_persistent(self, enable):
        """True / 1: persistent launches when they fit (small surveys in 64 x 64 regions of 16 waves x
        4 rows, else 64 x 96 regions, else 64 x 64 of 8 waves x 8 rows); 16 / 12 / 8: persistent with
        that region class only; False / 0: chunked launches.  Results are identical in every mode.
        -1 (fault-path tests): persistent launches oversubscribed past residency, which fail.
        A direct call during an engine fallback (FWIForward.fallback_to_chunked) replaces the mode the
        restore would bring back."""
        mode = int(enable) if not isinstance(enable, bool) else int(enable)
        self._set_mode(mode)
        if self._saved_mode is not None:
            self._saved_mode = mode

    def _set_mode(self, mode):
        _hip.check(self.lib.rdq_fwi_set_persistent(self.handle, mode), "rdq_fwi_set_persistent")
        self.persist_mode = mode

    def status(self, stream=None):
        """Synchronise and raise if a persistent launch's neighbour hand-off timed out."""
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        _hip.check(self.lib.rdq_fwi_status(self.handle, ctypes.c_void_p(stream)), "rdq_fwi_status")

    def debug_words(self):
        """[status, per-XCD workgroup counts of the last persistent launch] (synchronises)."""
        out = (ctypes.c_uint32 * 32)()
        _hip.check(self.lib.rdq_fwi_debug_words(self.handle, out), "rdq_fwi_debug_words")
        return int(out[0]), [int(v) for v in out[1:7]], [int(v) for v in out[16:24]]

    def launch_info(self, B):
        """{'fwd_persistent', 'adj_persistent', 'fwd_class' / 'adj_class' (persistent region class: 16 /
        12 / 8, 0 = chunked), 'fwd_T', 'adj_T', 'fwd_launches', 'adj_launches', 'fwd_overlap' /
        'adj_overlap' (the hand-off overlap mode that runs, set_handoff_overlap), 'fwd_roles' /
        'adj_roles' (the wave-role mode that runs, set_wave_roles), 'fwd_src_role' / 'adj_src_role' (the
        source-role mode that runs, set_source_role), 'adj_role' / 'adj_role_pair' (the adjoint-role mode that
        runs, set_adjoint_role, and the row pair it runs with, -1 = none), 'adj_fetch' (the fetch mode of that role's
        residuals and samples that runs, set_adjoint_fetch: 0 wherever the role does not run)} of a
        call with batch B (launches: time-loop kernel launches per call)."""
        out = (ctypes.c_int32 * 10)()
        _hip.check(self.lib.rdq_fwi_launch_info(self.handle, int(B), out), "rdq_fwi_launch_info")
        src = (ctypes.c_int32 * 2)()
        _hip.check(self.lib.rdq_fwi_source_role_info(self.handle, int(B), src), "rdq_fwi_source_role_info")
        arole = (ctypes.c_int32 * 2)()
        _hip.check(self.lib.rdq_fwi_adjoint_role_info(self.handle, int(B), arole), "rdq_fwi_adjoint_role_info")
        fetch = ctypes.c_int32()
        _hip.check(self.lib.rdq_fwi_adjoint_fetch_info(self.handle, int(B), ctypes.byref(fetch)),
                   "rdq_fwi_adjoint_fetch_info")
        return {"fwd_persistent": bool(out[0]), "adj_persistent": bool(out[1]),
                "fwd_class": int(out[0]), "adj_class": int(out[1]), "fwd_T": int(out[2]),
                "adj_T": int(out[3]), "fwd_launches": int(out[4]), "adj_launches": int(out[5]),
                "fwd_overlap": int(out[6]), "adj_overlap": int(out[7]),
                "fwd_roles": int(out[8]), "adj_roles": int(out[9]),
                "fwd_src_role": int(src[0]), "adj_src_role": int(src[1]),
                "adj_role": int(arole[0]), "adj_role_pair": int(arole[1]), "adj_fetch": int(fetch.value)}

    def set_sweep_delay(self, fwd_ticks, adj_ticks):
        """Persistent kernels: 10 ns ticks between an epoch's publish and its first hand-off pass."""
        _hip.check(self.lib.rdq_fwi_set_sweep_delay(self.handle, int(fwd_ticks), int(adj_ticks)),
                   "rdq_fwi_set_sweep_delay")

    def set_handoff_overlap(self, fwd_mode, adj_mode):
        """Persistent kernels: 0 = the hand-off sweep, then the post-sweep work; adjoint 1 (default) = the
        dead cells zeroed while the sweep's first pass is in flight.  The forward has mode 0 only.  Results
        are bit-identical in both modes."""
        _hip.check(self.lib.rdq_fwi_set_handoff_overlap(self.handle, int(fwd_mode), int(adj_mode)),
                   "rdq_fwi_set_handoff_overlap")

    def set_wave_roles(self, fwd_mode, adj_mode):
        """Persistent kernels: adjoint 1 (default) = waves without the source or the receiver row run every
        epoch but the last in a loop without the per-step source / receiver / end-of-record tests; 0 = every
        wave runs the generic loop.  The forward has mode 0 only.  Results are bit-identical in both modes."""
        _hip.check(self.lib.rdq_fwi_set_wave_roles(self.handle, int(fwd_mode), int(adj_mode)),
                   "rdq_fwi_set_wave_roles")

    def set_source_role(self, fwd_mode, adj_mode):
        """Persistent forward at 4 steps per epoch and 6 rows per wave, source and receivers in one row: 1
        (default) = the wave that owns that row runs every epoch but the last in a loop of its own (a
        guard-free step plus the row's own work) and the waves with neither row a guard-free loop, 0 = the
        generic loop.  The adjoint has mode 0 only.  launch_info reports the mode that runs.  Results are
        bit-identical in both modes."""
        _hip.check(self.lib.rdq_fwi_set_source_role(self.handle, int(fwd_mode), int(adj_mode)),
                   "rdq_fwi_set_source_role")

    def set_adjoint_role(self, mode):
        """Persistent (recurrence) adjoint, where the forward's source role would run and with wave roles on: 1
        (default) = the wave that owns the source/receiver row runs every epoch but the last in a loop of its
        own (the guard-free step plus the row's own work, the row's pair a compile-time constant of the kernel
        the host picks), 0 = the generic loop.  launch_info reports the mode that runs.  Results are
        bit-identical in both modes."""
        _hip.check(self.lib.rdq_fwi_set_adjoint_role(self.handle, int(mode)), "rdq_fwi_set_adjoint_role")

    def set_adjoint_fetch(self, mode):
        """The adjoint's source/receiver role (set_adjoint_role): 0 = the role's wave loads an epoch's
        receiver residuals and wavelet samples after the previous epoch's hand-off sweep, 1 (default) = the residuals a
        step ahead, each step the next step's ahead of its own history prefetch (the samples as in mode 0).  launch_info reports the mode that runs (0
        without the role).  Results are bit-identical in both modes."""
        _hip.check(self.lib.rdq_fwi_set_adjoint_fetch(self.handle, int(mode)), "rdq_fwi_set_adjoint_fetch")

    def adjoint_role_waves(self):
        """Waves that entered the adjoint's source/receiver loop in the last persistent adjoint call
        (synchronises): one per workgroup whose interior rows own the source row; 0 where the role did not run."""
        out = (ctypes.c_uint32 * 32)()
        _hip.check(self.lib.rdq_fwi_debug_words(self.handle, out), "rdq_fwi_debug_words")
        return int(out[24])

    def wide_info(self, B):
        """{'chains', 'fwd_spw', 'adj_spw', 'chain0_shots'}: the wide chunked kernels' concurrent launch
        chains and shots per workgroup of chain 0's full-depth forward / adjoint launches for batch B
        (the automatic choice unless set_wide_*_shots fixed one)."""
        out = (ctypes.c_int32 * 4)()
        _hip.check(self.lib.rdq_fwi_wide_info(self.handle, int(B), out), "rdq_fwi_wide_info")
        return {"chains": int(out[0]), "fwd_spw": int(out[1]), "adj_spw": int(out[2]), "chain0_shots": int(out[3])}

    def set_profile(self, enable):
        _hip.check(self.lib.rdq_fwi_set_profile(self.handle, int(bool(enable))), "rdq_fwi_set_profile")

    def read_profile(self):
        """Per-wave average phase times (us) of the persistent kernels since the last read."""
        out = (ctypes.c_uint64 * 12)()
        _hip.check(self.lib.rdq_fwi_read_profile(self.handle, out), "rdq_fwi_read_profile")
        res = {}
        for name, o in (("fwd", 0), ("adj", 6)):
            n = max(int(out[o + 3]), 1)
            res[name] = {"wait_us": out[o] / n / 100.0, "steps_us": out[o + 1] / n / 100.0,
                         "publish_us": out[o + 2] / n / 100.0, "waves": int(out[o + 3]),
                         "first_pass_us": out[o + 4] / n / 100.0, "passes": out[o + 5] / n}
        sp = (ctypes.c_uint64 * 10)()
        _hip.check(self.lib.rdq_fwi_profile_split(self.handle, sp), "rdq_fwi_profile_split")
        for name, o in (("fwd", 0), ("adj", 5)):
            n = max(res[name]["waves"], 1)
            # wait_us = a + b + c + d; publish_us = publish_issue_us + gradient_us
            res[name].update({"wait_a_issue_us": sp[o] / n / 100.0, "wait_b_first_us": sp[o + 1] / n / 100.0,
                              "wait_c_later_us": sp[o + 2] / n / 100.0, "wait_d_tail_us": sp[o + 3] / n / 100.0,
                              "gradient_us": sp[o + 4] / n / 100.0,
                              "publish_issue_us": res[name]["publish_us"] - sp[o + 4] / n / 100.0})
        return res

    def profile_waves(self, adj):
        """(blocks*16, 3) per-wave {hand-off, steps, publish} us of the last read_profile()."""
        n = 4096 * 16 * 3
        out = (ctypes.c_uint64 * n)()
        _hip.check(self.lib.rdq_fwi_profile_waves(self.handle, int(bool(adj)), out, n), "rdq_fwi_profile_waves")
        return np.frombuffer(out, dtype=np.uint64).reshape(-1, 3).astype(np.float64) / 100.0

    def profile_waves_split(self, adj, ticks=False):
        """(blocks*16, 8) per-wave {hand-off, steps, publish, a, b, c, d, gradient} us (ticks: the raw 10 ns
        counts) of the last read_profile(): hand-off = a + b + c + d (rdq_fwi_profile_split)."""
        n = 4096 * 16 * 8
        out = (ctypes.c_uint64 * n)()
        _hip.check(self.lib.rdq_fwi_profile_waves_split(self.handle, int(bool(adj)), out, n),
                   "rdq_fwi_profile_waves_split")
        raw = np.frombuffer(out, dtype=np.uint64).reshape(-1, 8)
        return raw.copy() if ticks else raw.astype(np.float64) / 100.0

    def set_tuning(self, fwd_steps, adj_steps, chains=0):
        """Blocking depths (1..4) and concurrent launch chains of the chunked kernels (0 = auto)."""
        _hip.check(self.lib.rdq_fwi_set_tuning(self.handle, int(fwd_steps), int(adj_steps), int(chains)),
                   "rdq_fwi_set_tuning")

    def __del__(self):
        try:
            _ops.unregister_plan(getattr(self, "op_id", -1))
        except Exception:          # interpreter shutdown: module globals already torn down
            pass
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                self.lib.rdq_fwi_plan_destroy(h)
            except Exception:
                pass
            self.handle = None

    # ---- the C ABI entry points as torch.ops.red_diffeq operators (red_diffeq/ops.py) ----
    def coeffs(self, v, vel_mode):
        return torch.ops.red_diffeq.fwi_coeffs(v, self.op_id, vel_mode)

    def forward(self, coeffs, B, keep_history):
        seis, hist = torch.ops.red_diffeq.fwi_forward(coeffs, self.op_id, B, bool(keep_history))
        return seis, (hist if keep_history else None)

    def adjoint(self, coeffs, hist, dseis, B):
        return torch.ops.red_diffeq.fwi_adjoint(coeffs, hist, dseis, self.op_id, B)

    def finalize(self, coeffs, vstat, gA, gk, gb, B, vel_mode):
        return torch.ops.red_diffeq.fwi_grad_finalize(coeffs, vstat, gA, gk, gb, self.op_id, B, vel_mode)

    def born(self, coeffs, vstat, hist, dv, B, vel_mode):
        """J dv (the seismograms' shape) over the store-all history `hist` of forward(coeffs, B, True): the
        narrow chunked Born kernels at set_tuning's forward depth and chains, whatever the persistent / wide
        settings are; bit-identical for every depth, chain count and graph setting."""
        return torch.ops.red_diffeq.fwi_born(coeffs, vstat, hist, dv, self.op_id, int(B), int(vel_mode))

    def born_fused(self, coeffs, vstat, dv, B, vel_mode, K=None):
        """(seis, J dv, ckpt) from one time loop that computes the forward and its tangent together and keeps no
        history (rdq_fwi_born_fused): seis is bit-identical to forward's, J dv to born's.  K = None: no
        checkpoints (ckpt is empty); K >= 1: ckpt is forward_ckpt(coeffs, B, K)'s store, bit for bit, for
        adjoint_ckpt.  Narrow chunked kernels at set_tuning's forward depth and chains, as born."""
        if K is not None and int(K) < 1:
            raise ValueError(f"born_fused: K must be None or >= 1, got {K}")
        return torch.ops.red_diffeq.fwi_born_fused(coeffs, vstat, dv, self.op_id, int(B), int(vel_mode),
                                                   0 if K is None else int(K))

    # ---- checkpointed gradient (rdq_fwi_*_ckpt): history bounded by recomputation ----
    def ckpt_sizes(self, B, K):
        """rdq_fwi_ckpt_sizes_t of a checkpointed gradient with K steps per segment: .nseg, .seg_levels,
        .ckpt / .seg bytes."""
        key = ("ckpt", int(B), int(K))
        if key not in self._sizes:
            s = _hip.FwiCkptSizes()
            _hip.check(self.lib.rdq_fwi_ckpt_sizes(self.handle, int(B), int(K), ctypes.byref(s)), "rdq_fwi_ckpt_sizes")
            self._sizes[key] = s
        return self._sizes[key]

    def ckpt_info(self, B, K):
        """{'fwd_class' (first-pass persistent class, 0 = chunked), 'nseg', 'fwd_launches', 'bwd_launches'}
        (time-loop launches per launch chain; the backward's are every segment's recompute + adjoint)."""
        out = (ctypes.c_int32 * 4)()
        _hip.check(self.lib.rdq_fwi_ckpt_info(self.handle, int(B), int(K), out), "rdq_fwi_ckpt_info")
        return {"fwd_class": int(out[0]), "nseg": int(out[1]), "fwd_launches": int(out[2]),
                "bwd_launches": int(out[3])}

    def forward_ckpt(self, coeffs, B, K):
        """First pass: (seis, ckpt)."""
        return torch.ops.red_diffeq.fwi_forward_ckpt(coeffs, self.op_id, int(B), int(K))

    def adjoint_ckpt(self, coeffs, ckpt, dseis, B, K):
        """Backward over the recomputed segments: (gA, gk, gbeta); the segment buffer lives for the call."""
        seg = torch.empty(int(self.ckpt_sizes(B, K).seg) // 4, dtype=torch.float32, device=coeffs.device)
        return torch.ops.red_diffeq.fwi_adjoint_ckpt(coeffs, ckpt, seg, dseis, self.op_id, int(B), int(K))

    # ---- source illumination / pseudo-Hessian diagonal (rdq_fwi_illum*) ----
    def illum(self, hist, B, nwf=0):
        """hA (flat [B][nwf][Hp][ld]) = sum_k q_k^2 over a store-all history of nwf wavefields per model (0: the
        plan's shots), whichever forward family wrote it."""
        return torch.ops.red_diffeq.illum_fwi(hist, self.op_id, int(B), int(nwf))

    def illum_ckpt(self, coeffs, ckpt, B, K, w=None, weff=None):
        """The same bits from a checkpoint store (forward_ckpt, or the _src / enc_ forms with their wavelets `w` /
        effective wavelets `weff`): each segment recomputed, then accumulated; the segment buffer lives for the call."""
        ne = None if weff is None else weff.shape[1]
        cs = self.ckpt_sizes(B, K) if ne is None else self.ckpt_sizes_enc(B, ne, K)
        seg = torch.empty(int(cs.seg) // 4, dtype=torch.float32, device=coeffs.device)
        if weff is not None:
            return torch.ops.red_diffeq.illum_fwi_ckpt_enc(coeffs, weff, ckpt, seg, self.op_id, int(B), int(K))
        if w is not None:
            return torch.ops.red_diffeq.illum_fwi_ckpt_src(coeffs, w, ckpt, seg, self.op_id, int(B), int(K))
        return torch.ops.red_diffeq.illum_fwi_ckpt(coeffs, ckpt, seg, self.op_id, int(B), int(K))

    def illum_finalize(self, coeffs, hA, B, vel_mode, nwf=0):
        """H (B, 1, nz, nx) from hA: the nwf planes summed, the replicate fold, (dA/dv)^2."""
        return torch.ops.red_diffeq.illum_fwi_finalize(coeffs, hA, self.op_id, int(B), int(nwf), int(vel_mode))


def checkpoint_levels(nt, K):
    """Wavefield levels a checkpointed gradient with K steps per segment holds (include/red_diffeq_fwi.h):
    two per interior segment boundary, plus the segment buffer of min(K, nt) + 2."""
    K = min(int(K), int(nt))
    nseg = -(-int(nt) // K)
    return 2 * (nseg - 1) + K + 2


def choose_checkpoint(nt, level_bytes, budget_bytes):
    """History policy under a byte budget: None = store-all (its nt + 2 levels fit), else the LARGEST K
    whose checkpoint store + segment buffer fit (fewest segments = fewest short tail launches; the
    recompute costs one forward whatever K is).  ValueError when even the smallest footprint (K near
    sqrt(2 nt)) does not fit."""
    nt, level_bytes = int(nt), int(level_bytes)
    if nt < 1 or level_bytes < 1:
        raise ValueError("choose_checkpoint: nt and level_bytes must be positive")
    if (nt + 2) * level_bytes <= budget_bytes:
        return None
    for K in range(nt, 0, -1):
        if checkpoint_levels(nt, K) * level_bytes <= budget_bytes:
            return K
    need = min(checkpoint_levels(nt, K) for K in range(1, nt + 1)) * level_bytes
    raise ValueError(f"history budget of {int(budget_bytes)} bytes is too small: the smallest checkpointed "
                     f"history needs {need} bytes (store-all: {(nt + 2) * level_bytes})")


class FWIForward(nn.Module):
    """Drop-in for red_diffeq.solvers.pde.FWIForward (pde.py:6-93)."""

    def __init__(self, ctx, device, sample_temporal=1, sample_spatial=1.0, normalize=True,
                 v_denorm_func=None, s_norm_func=None, shots=None, checkpoint=None, history_budget_gb=None,
                 wavelet=None):
        """wavelet: None = the Ricker wavelet of ``ctx`` (f, dt, nt), as the reference; otherwise an array-like
        or tensor of shape (nt,), the source signature of every shot: copied to host fp64 and handed to the plan in
        place of the Ricker (which casts it to fp32 the same way), so every kernel family, checkpointing, born /
        gauss_newton, shots= and the engine run on it unchanged.  ricker() is then not called, so a record shorter
        than the Ricker is legal.  Per-shot / per-model and differentiable wavelets: forward(v, wavelet=...).

        checkpoint / history_budget_gb (also read from ``ctx`` when the keyword is None, so a YAML's
        ``pde:`` section can set them): None / None = the store-all history, today's path; checkpoint = K
        (int >= 1) = a checkpointed gradient with K steps per segment (two wavefield levels kept every K
        steps, each segment recomputed in the backward: 2 nt / K + K levels instead of nt + 2, one extra
        forward); checkpoint = "auto", or a budget alone = store-all while its history fits
        history_budget_gb (GiB), else the largest K that fits (choose_checkpoint)."""
        super().__init__()
        self.device = device
        self.normalize = normalize
        if normalize:
            self.v_denorm_func = v_denorm_func
            self.s_norm_func = s_norm_func
        self.sample_temporal = sample_temporal
        if "sx" not in ctx.keys():
            ctx["sx"] = np.linspace(0, ctx["n_grid"] - 1, num=ctx["ns"]) * ctx["dx"]
        else:
            ctx["sx"] = np.array(ctx["sx"]) * ctx["dx"]
        if "gx" not in ctx.keys():
            ctx["gx"] = np.linspace(0, ctx["n_grid"] - 1, num=int(sample_spatial * ctx["ng"])) * ctx["dx"]
        else:
            ctx["gx"] = np.array(ctx["gx"]) * ctx["dx"]
        self.ctx = ctx
        self.checkpoint = checkpoint if checkpoint is not None else ctx.get("checkpoint")
        self.history_budget_gb = history_budget_gb if history_budget_gb is not None else ctx.get("history_budget_gb")
        if isinstance(self.checkpoint, str):
            if self.checkpoint != "auto":
                raise ValueError(f"checkpoint must be None, an int >= 1 or 'auto', got {self.checkpoint!r}")
            if self.history_budget_gb is None:
                raise ValueError("checkpoint='auto' needs history_budget_gb")
        elif self.checkpoint is not None:
            self.checkpoint = int(self.checkpoint)
            if self.checkpoint < 1:
                raise ValueError(f"checkpoint must be >= 1, got {self.checkpoint}")
        # shot-parallel sharding: this operator models only shots[start:stop]
        self.shots = (0, len(ctx["sx"])) if shots is None else (int(shots[0]), int(shots[1]))
        self.shots_explicit = shots is not None
        self.wavelet = None
        if wavelet is not None:
            wav = wavelet.detach().cpu().numpy() if isinstance(wavelet, torch.Tensor) else np.asarray(wavelet)
            if wav.ndim != 1 or wav.shape[0] != int(ctx["nt"]):
                raise ValueError(f"wavelet must have shape (nt,) = ({int(ctx['nt'])},), got {tuple(wav.shape)}")
            self.wavelet = np.array(wav, dtype=np.float64)      # the plan's own host copy
        self._plans = {}
        self._last = None
        self._fallen_back = False      # between fallback_to_chunked() and restore_persistent()

    # --- reference helpers kept with their signatures -------------------------------------
    def ricker(self, f, dt, nt):
        return ricker(f, dt, nt)

    def adj_sr(self, sx, sz, gx, gz, dx, nbc):
        return adj_sr(sx, sz, gx, gz, dx, nbc)

    def get_Abc(self, vp, nbc, dx):
        """Sponge damping field of a padded velocity (pde.py:38-52), for inspection only.

        The hot path never calls this: the same profile is fused into the HIP coefficient kernel
        (rdq_fwi_coeffs).  Columns overwrite rows, so the corners take the column profile."""
        dimrange = 1.0 * torch.unsqueeze(torch.arange(nbc, device=vp.device), dim=-1)
        velmin, _ = torch.min(vp.view(vp.shape[0], -1), dim=-1)
        a = (nbc - 1) * dx
        kappa = (3.0 * velmin * np.log(10000000.0) / (2.0 * a)).unsqueeze(0).expand(nbc, -1)
        prof = (kappa * (dimrange * dx / a) ** 2).permute(1, 0).unsqueeze(1)   # (B,1,nbc)
        damp = torch.zeros_like(vp)
        H, W = vp.shape[-2:]
        damp[:, :, :nbc, :] = torch.flip(prof, dims=[-1]).unsqueeze(-1).expand(-1, -1, -1, W)
        damp[:, :, H - nbc:, :] = prof.unsqueeze(-1).expand(-1, -1, -1, W)
        damp[:, :, :, :nbc] = torch.flip(prof, dims=[-1]).unsqueeze(-2).expand(-1, -1, H, -1)
        damp[:, :, :, W - nbc:] = prof.unsqueeze(-2).expand(-1, -1, H, -1)
        return damp

    # --- HIP path --------------------------------------------------------------------------
    def _plan(self, nz, nx, device, per_call=False):
        """The plan of a grid shape on a device.  per_call: the caller brings its own wavelets, so a ctx whose
        record is shorter than its Ricker wavelet, with no constructor wavelet, still gets a plan (its plan-level
        wavelet is zeros and is marked absent: every call that would read it raises the Ricker's error)."""
        key = (nz, nx, device.index)
        if key in self._plans and getattr(self._plans[key], "no_wavelet", False) and not per_call:
            ricker(self.ctx["f"], self.ctx["dt"], self.ctx["nt"])      # raises: nt is shorter than the wavelet
        if key not in self._plans:
            c = self.ctx
            isx, isz, igx, igz = adj_sr(np.asarray(c["sx"]), c["sz"], np.asarray(c["gx"]), c["gz"],
                                        c["dx"], c["nbc"])
            isx = isx[self.shots[0]:self.shots[1]]
            if len(isx) == 0:
                raise ValueError("empty shot range")
            wav = self.wavelet
            if wav is None:
                try:
                    wav = ricker(c["f"], c["dt"], c["nt"])
                except ValueError:
                    if not per_call:
                        raise
            self._plans[key] = FwiPlan(nz, nx, c, self.sample_temporal, isx, isz, igx, igz,
                                       wav if wav is not None else np.zeros(int(c["nt"])), device)
            self._plans[key].no_wavelet = wav is None
            if os.environ.get("RDQ_NO_XCD_LOCAL"):       # A/B switches (tools/, experiments)
                self._plans[key].set_variant(xcd_local=False)
            if os.environ.get("RDQ_NO_GRAPHS"):
                self._plans[key].set_graphs(False)
            if os.environ.get("RDQ_ROWS_PER_WAVE"):          # "fwd,adj" (tools/ab_rw.sh, red_loop A/B)
                self._plans[key].set_rows_per_wave(*[int(x) for x in os.environ["RDQ_ROWS_PER_WAVE"].split(",")])
            if self._fallen_back:     # created during a fallback: chunked until restore_persistent()
                plan = self._plans[key]
                plan._saved_mode = plan.persist_mode
                plan._set_mode(0)
        return self._plans[key]

    def _fused_denorm(self):
        return self.normalize and self.v_denorm_func is v_denormalize

    def _call_wavelet(self, v, w):
        """Checks a per-call wavelet against v and the survey (before any device work) and returns it as this
        operator's shots' (B, ns_local, nt) fp32 view: a shared axis is an expand(), not a copy, so autograd sums
        its gradient, and with shots= the slice is taken in torch, so the other shots' rows get zeros."""
        if not isinstance(w, torch.Tensor) or not w.is_floating_point():
            raise ValueError("wavelet must be a float tensor of shape (nt,), (ns, nt) or (B, ns, nt)")
        if v.dim() != 4 or v.shape[1] != 1:
            raise ValueError(f"expected v of shape (B,1,H,W), got {tuple(v.shape)}")
        B, ns, nt = v.shape[0], len(self.ctx["sx"]), int(self.ctx["nt"])
        if w.dim() not in (1, 2, 3) or w.shape[-1] != nt or tuple(w.shape[:-1]) not in ((), (ns,), (B, ns)):
            raise ValueError(f"wavelet must have shape ({nt},), ({ns}, {nt}) or ({B}, {ns}, {nt}) "
                             f"(nt; shots, nt; models, shots, nt), got {tuple(w.shape)}")
        if w.device != v.device:
            raise ValueError(f"wavelet is on {w.device}, v on {v.device}")
        if w.dtype != torch.float32:
            w = w.float()
        if w.dim() > 1:
            w = w[..., self.shots[0]:self.shots[1], :]
        return w.expand(B, self.shots[1] - self.shots[0], nt)

    def _call_encoding(self, v, E):
        """Checks an encoding against v and the survey (before any device work) and returns it as (B, ne, ns) fp32:
        a shared model axis is an expand(), so autograd sums its gradient."""
        if self.shots_explicit:
            raise ValueError("encoding= fires every source of the survey into each supershot: it is not available on "
                             "an instance constructed with shots=")
        if not isinstance(E, torch.Tensor) or not E.is_floating_point():
            raise ValueError("encoding must be a float tensor of shape (ne, ns) or (B, ne, ns)")
        if v.dim() != 4 or v.shape[1] != 1:
            raise ValueError(f"expected v of shape (B,1,H,W), got {tuple(v.shape)}")
        B, ns = v.shape[0], len(self.ctx["sx"])
        if E.dim() not in (2, 3) or E.shape[-1] != ns or (E.dim() == 3 and E.shape[0] != B):
            raise ValueError(f"encoding must have shape (ne, {ns}) or ({B}, ne, {ns}) (supershots, sources; models, "
                             f"supershots, sources), got {tuple(E.shape)}")
        if E.shape[-2] < 1:
            raise ValueError("encoding needs at least one supershot (ne >= 1)")
        if E.device != v.device:
            raise ValueError(f"encoding is on {E.device}, v on {v.device}")
        if E.dtype != torch.float32:
            E = E.float()
        return E.expand(B, E.shape[-2], ns)

    def _encoded(self, v, wavelet, E):
        """forward(v, wavelet, encoding=E): see forward."""
        E = self._call_encoding(v, E)                      # ValueErrors before any device work
        if wavelet is not None:
            w = self._call_wavelet(v, wavelet)
        _hip.require_device(v)
        if v.dtype != torch.float32:
            v = v.float()
        if self._fused_denorm():
            vel_mode = 0
        else:
            if self.normalize:
                v = self.v_denorm_func(v)
            vel_mode = 1
        plan = self._plan(v.shape[2], v.shape[3], v.device, per_call=wavelet is not None)
        self._last = plan
        B, ne = E.shape[0], E.shape[1]
        if wavelet is None:      # the constructor's (or the Ricker) signature, as the plan holds it: fp32 of the fp64
            w = torch.from_numpy(plan._wav).to(device=v.device, dtype=torch.float32).expand(B, plan.ns, plan.nt)
        weff = E.unsqueeze(-1) * w.unsqueeze(1)            # (B, ne, ns, nt): autograd gives E.grad and w.grad from gwav
        keep = bool((v.requires_grad or weff.requires_grad) and torch.is_grad_enabled())
        K = None
        if keep:
            if isinstance(self.checkpoint, int):
                K = self.checkpoint
            elif self.history_budget_gb is not None:
                K = choose_checkpoint(plan.nt, plan.sizes_enc(B, ne).history // (plan.nt + 2),
                                      int(float(self.history_budget_gb) * 2 ** 30))
        if K is not None:
            s = torch.ops.red_diffeq.enc_fwi_ckpt(v, weff, plan.op_id, vel_mode, K)[0]
        else:
            s = torch.ops.red_diffeq.enc_fwi(v, weff, plan.op_id, vel_mode, keep)[0]
        return self.s_norm_func(s) if self.normalize else s

    def forward(self, v, wavelet=None, encoding=None):
        """seis = forward(v).  wavelet: None = the constructor's wavelet (the Ricker by default) on the plan's
        kernels, today's path.  Otherwise a float tensor on v's device of shape (nt,), (ns, nt) or (B, ns, nt)
        (ns = the survey's full shot count, also with shots=): sample n of model b, shot s is injected as
        P_{n+1}[b, s, src] += beta[b, src] * w[b, s, n], and the result is differentiable in v and in the wavelet
        (a shared wavelet receives the fp32 sum of the per-shot gradients).  Such a call always runs the narrow
        chunked kernels (set_tuning's depths and chains), store-all or checkpointed as the instance says.  By
        linearity J_w dw is forward(v, wavelet=dw) under no_grad.  born / gauss_newton take no wavelet: they use
        the constructor's.

        encoding: None, or a float tensor E on v's device of shape (ne, ns) or (B, ne, ns): source encoding.  The
        call models ne simultaneous-source "supershots" per model instead of ns shots: wavefield (b, e) is fired by
        every source s at once with the effective wavelet E[b, e, s] * w[b, s, :] (w = wavelet=, or the
        constructor's / Ricker signature; the product is formed with torch ops), the sources injected in ascending
        s, each one including those whose code is zero.  Returns (B, ne, nrec, ng), through s_norm_func like the
        plain call, differentiable in v, E and the wavelet (broadcast axes receive the fp32 sums).  It runs the
        narrow chunked kernels, store-all or checkpointed as the instance says; time and history scale with ne, not
        ns.  A row of E with a single 1 reproduces forward(v, wavelet=w)[:, s] bit for bit.  Codes and the matching
        combination of observed data: red_diffeq.utils.encoding (random_encoding, encode).  ValueError for a wrong
        shape, dtype or device, ne < 1, or an instance constructed with shots=.

        Not covered: per-call wavelets or encodings on the persistent or wide kernels; born / gauss_newton with an
        encoding (they take none); shots= sharding of a supershot; engine / YAML wiring of per-shot wavelets or of
        encodings (redraw schedules, encoded observed data inside InversionEngine: the two helpers are what a caller
        needs to do it by hand)."""
        if encoding is not None:
            return self._encoded(v, wavelet, encoding)
        if wavelet is not None:
            wavelet = self._call_wavelet(v, wavelet)      # ValueError before any device work
        _hip.require_device(v)
        if v.dim() != 4 or v.shape[1] != 1:
            raise ValueError(f"expected v of shape (B,1,H,W), got {tuple(v.shape)}")
        if v.dtype != torch.float32:
            v = v.float()
        if self._fused_denorm():
            vel_mode = 0                      # denormalisation fused into K3 / K4
        else:
            if self.normalize:
                v = self.v_denorm_func(v)     # arbitrary user callable: autograd through torch
            vel_mode = 1
        plan = self._plan(v.shape[2], v.shape[3], v.device, per_call=wavelet is not None)
        self._last = plan
        keep = bool((v.requires_grad or (wavelet is not None and wavelet.requires_grad)) and torch.is_grad_enabled())
        K = self.checkpoint_interval(plan, v.shape[0]) if keep else None
        if wavelet is not None:   # the call's own wavelets: narrow chunked kernels, gradients in v and w
            if K is not None:
                s = torch.ops.red_diffeq.fwi_ckpt_src(v, wavelet, plan.op_id, vel_mode, K)[0]
            else:
                s = torch.ops.red_diffeq.fwi_src(v, wavelet, plan.op_id, vel_mode, keep)[0]
        elif K is not None:   # history bounded by recomputation; backward: recompute + K2 per segment, K4
            s = torch.ops.red_diffeq.fwi_ckpt(v, plan.op_id, vel_mode, K)[0]
        else:
            s = torch.ops.red_diffeq.fwi(v, plan.op_id, vel_mode, keep)[0]   # backward: K2 + K4 (ops.py)
        return self.s_norm_func(s) if self.normalize else s

    # --- linearisation: J dv and the Gauss-Newton product ---------------------------------------
    def _linearise(self, v, dv, what, need_checkpoint=False):
        """Checks (before any device work), then the model, the direction and vel_mode as K3 takes them, and
        the pull-back of a model gradient through a custom denormalisation (None when it is fused)."""
        if v.dim() != 4 or v.shape[1] != 1:
            raise ValueError(f"{what}: expected v of shape (B,1,H,W), got {tuple(v.shape)}")
        if tuple(dv.shape) != tuple(v.shape):
            raise ValueError(f"{what}: dv has shape {tuple(dv.shape)}, v {tuple(v.shape)}")
        if need_checkpoint and self.checkpoint is None and self.history_budget_gb is None:
            raise ValueError(f"{what}(history=False) runs its adjoint over checkpoints: construct FWIForward with "
                             f"checkpoint=K or history_budget_gb (neither is set)")
        _hip.require_device(v, dv)
        v, dv = v.detach().float(), dv.detach().float()
        if self._fused_denorm():
            return v, dv, 0, None
        if not self.normalize:
            return v, dv, 1, None
        vn = v                                   # an arbitrary callable: its tangent and transpose through torch
        v, dv = torch.func.jvp(self.v_denorm_func, (vn,), (dv,))
        return v, dv, 1, lambda g: torch.func.vjp(self.v_denorm_func, vn)[1](g)[0]

    def _born(self, v, dv, vel_mode):
        """K3, the forward with its store-all history, the Born prologue and time loop."""
        plan = self._plan(v.shape[2], v.shape[3], v.device)
        self._last = plan
        B = v.shape[0]
        need = int(plan.sizes(B).history)
        if self.history_budget_gb is not None and need > int(float(self.history_budget_gb) * 2 ** 30):
            raise ValueError(f"born / gauss_newton keep a store-all history of {need} bytes, more than "
                             f"history_budget_gb = {self.history_budget_gb}; pass history=False for the fused "
                             f"pass, which keeps no history")
        coeffs, vstat = plan.coeffs(v, vel_mode)
        seis, hist = plan.forward(coeffs, B, True)
        return plan, coeffs, vstat, hist, seis, plan.born(coeffs, vstat, hist, dv, B, vel_mode)

    def _born_fused(self, v, dv, vel_mode, checkpoints):
        """K3, the Born prologue and the fused forward + tangent time loop: no history, no budget check.
        `checkpoints`: also the checkpoint store of this instance's interval, for the checkpointed adjoint."""
        plan = self._plan(v.shape[2], v.shape[3], v.device)
        self._last = plan
        B = v.shape[0]
        K = None
        if checkpoints:
            K = self.checkpoint_interval(plan, B)
            if K is None:                        # the whole history fits the budget: one segment, no store
                K = plan.nt
        coeffs, vstat = plan.coeffs(v, vel_mode)
        seis, ds, ckpt = plan.born_fused(coeffs, vstat, dv, B, vel_mode, K)
        return plan, coeffs, vstat, ckpt, K, seis, ds

    def _custom_s_norm(self):
        return self.normalize and self.s_norm_func is not s_normalize_none

    @staticmethod
    def _no_encoding(what, encoding):
        if encoding is not None:
            raise ValueError(f"{what} takes no encoding=: it linearises the per-shot survey (encoded supershots are "
                             f"forward(v, encoding=E) only)")

    def born(self, v, dv, return_seis=False, history=True, encoding=None):
        """Linearised (Born) modelling: J dv, J = d forward(v) / d v, with the shape of forward(v); with
        return_seis, (forward(v), J dv).  Runs under no_grad; the result does not require grad.  history=True
        (the default): the forward keeps its store-all history and the Born pass streams it back (ValueError with
        the byte count when history_budget_gb is set and it does not fit).  history=False: one fused time loop
        computes the forward and its tangent together and keeps no history at all (no budget applies); both
        outputs are bit-identical to history=True's.  A custom v_denorm_func, and an s_norm_func other than
        s_normalize_none, are chained with torch.func.jvp.  With shots=, this rank's shots only, as forward.  The source is
        the constructor's wavelet (born and gauss_newton take no wavelet= of their own, and no encoding=: passing one
        raises ValueError)."""
        self._no_encoding("born", encoding)
        v, dv, vel_mode, _ = self._linearise(v, dv, "born")
        with torch.no_grad():
            if history:
                seis, ds = self._born(v, dv, vel_mode)[4:]
            else:
                seis, ds = self._born_fused(v, dv, vel_mode, False)[5:]
        if self._custom_s_norm():
            seis, ds = torch.func.jvp(self.s_norm_func, (seis,), (ds,))
        seis, ds = seis.detach(), ds.detach()
        return (seis, ds) if return_seis else ds

    def gauss_newton(self, v, dv, weight=None, history=True, encoding=None):
        """The Gauss-Newton product J^T (weight * J dv), with the shape of v.  history=True (the default): one
        forward with history, one Born pass, then the adjoint and the finalize on the same history (no second
        forward).  Bit-equal to s = forward(v); s.backward(weight * born(v, dv)); v.grad.  history=False: the
        fused forward + Born pass, which also writes the checkpoint store of checkpoint_interval(), then the
        checkpointed adjoint and the finalize: the memory of a checkpointed gradient, bit-equal to the same
        three lines on this instance.  It needs checkpoint= or history_budget_gb (ValueError otherwise)."""
        self._no_encoding("gauss_newton", encoding)
        v, dv, vel_mode, pull = self._linearise(v, dv, "gauss_newton", need_checkpoint=not history)
        with torch.no_grad():
            if history:
                plan, coeffs, vstat, hist, seis, ds = self._born(v, dv, vel_mode)
            else:
                plan, coeffs, vstat, hist, K, seis, ds = self._born_fused(v, dv, vel_mode, True)
        if self._custom_s_norm():
            ds = torch.func.jvp(self.s_norm_func, (seis,), (ds,))[1]
        r = ds if weight is None else weight * ds
        if self._custom_s_norm():
            r = torch.func.vjp(self.s_norm_func, seis)[1](r)[0]
        with torch.no_grad():
            if history:
                gA, gk, gb = plan.adjoint(coeffs, hist, r.detach().contiguous(), v.shape[0])
            else:
                gA, gk, gb = plan.adjoint_ckpt(coeffs, hist, r.detach().contiguous(), v.shape[0], K)
            del hist
            g = plan.finalize(coeffs, vstat, gA, gk, gb, v.shape[0], vel_mode)
        return (g if pull is None else pull(g)).detach()

    def illumination(self, v, wavelet=None, encoding=None, per_wavefield=False):
        """Source illumination / pseudo-Hessian diagonal of the survey at the model v (Shin et al.):
        H = (dA/dv)^2 sum over wavefields, padded cells of the model cell and time steps of q_k^2, with q_k = 2 c1
        P_{k-1} + Lap(P_{k-1}) the virtual-source factor the adjoint multiplies its field by (include/
        red_diffeq_fwi.h).  (B, 1, nz, nx) fp32, per normalised model unit squared with the fused denormalisation
        and per (m/s)^2 with normalize=False; per_wavefield=True: (B, nwf, nz, nx), one plane per shot (or per
        supershot of `encoding`), each finalised on its own.  Runs under no_grad: K3, a forward that keeps its
        history (what forward(v, wavelet, encoding) would run), the streaming pass, the finalize; under checkpoint= /
        history_budget_gb the checkpointed first pass and the pass over its recomputed segments, with the same
        bits.  With shots=, this rank's shots only (sum the ranks' H).  The sponge and source-amplitude terms of the
        Hessian diagonal and the receiver side are left out.  ValueError, before any device work, for a custom
        v_denorm_func (an arbitrary callable has no diagonal chain rule: construct with normalize=False and pass
        physical velocities) and for wrong shapes."""
        if self.normalize and not self._fused_denorm():
            raise ValueError("illumination: a custom v_denorm_func has no diagonal chain rule; construct FWIForward "
                             "with normalize=False and pass physical velocities")
        if not isinstance(v, torch.Tensor) or v.dim() != 4 or v.shape[1] != 1:
            raise ValueError(f"illumination: expected v of shape (B,1,H,W), got {tuple(getattr(v, 'shape', ()))}")
        E = self._call_encoding(v, encoding) if encoding is not None else None
        w = self._call_wavelet(v, wavelet) if wavelet is not None else None
        _hip.require_device(v)
        with torch.no_grad():
            v = v.detach().float()
            vel_mode = 0 if self._fused_denorm() else 1
            plan = self._plan(v.shape[2], v.shape[3], v.device, per_call=wavelet is not None)
            self._last = plan
            B, nwf, weff = v.shape[0], plan.ns, None
            if w is not None:
                w = w.detach()
            if E is not None:
                if w is None:
                    w = torch.from_numpy(plan._wav).to(device=v.device, dtype=torch.float32).expand(B, plan.ns, plan.nt)
                weff, nwf = E.detach().unsqueeze(-1) * w.unsqueeze(1), E.shape[1]
            K = None
            if isinstance(self.checkpoint, int):
                K = self.checkpoint
            elif self.history_budget_gb is not None:
                sz = plan.sizes(B) if weff is None else plan.sizes_enc(B, nwf)
                K = choose_checkpoint(plan.nt, sz.history // (plan.nt + 2), int(float(self.history_budget_gb) * 2 ** 30))
            ops = torch.ops.red_diffeq
            coeffs, _ = plan.coeffs(v, vel_mode)
            if K is None:
                if weff is not None:
                    hist = ops.enc_fwi_forward(coeffs, weff, plan.op_id, B, True)[1]
                elif w is not None:
                    hist = ops.fwi_forward_src(coeffs, w, plan.op_id, B, True)[1]
                else:
                    hist = plan.forward(coeffs, B, True)[1]
                hA = plan.illum(hist, B, nwf)
                del hist
            else:
                if weff is not None:
                    ckpt = ops.enc_fwi_forward_ckpt(coeffs, weff, plan.op_id, B, K)[1]
                elif w is not None:
                    ckpt = ops.fwi_forward_ckpt_src(coeffs, w, plan.op_id, B, K)[1]
                else:
                    ckpt = plan.forward_ckpt(coeffs, B, K)[1]
                hA = plan.illum_ckpt(coeffs, ckpt, B, K, w=w if weff is None else None, weff=weff)
                del ckpt
            if not per_wavefield:
                return plan.illum_finalize(coeffs, hA, B, vel_mode, nwf)
            planes = hA.view(B, nwf, -1)
            return torch.cat([plan.illum_finalize(coeffs, planes[:, j].contiguous().view(-1), B, vel_mode, 1)
                              for j in range(nwf)], dim=1)

    def checkpoint_interval(self, plan, B):
        """Steps per segment of the checkpointed gradient a differentiable call with batch B runs, or None
        for the store-all history (see __init__)."""
        if isinstance(self.checkpoint, int):
            return self.checkpoint
        if self.history_budget_gb is None:
            return None
        sz = plan.sizes(B)
        return choose_checkpoint(plan.nt, sz.history // (plan.nt + 2), int(float(self.history_budget_gb) * 2 ** 30))

    def check(self):
        """Raise if a persistent kernel's neighbour hand-off timed out since the last check
        (synchronises the current stream)."""
        for plan in self._plans.values():
            plan.status()

    def status_word(self):
        """Device int32 view (1,) of the status word of the plan the last call used (None before the
        first call): non-zero once a persistent launch gave up.  Stream-ordered, no sync."""
        return None if self._last is None else self._last.status_t[:1]

    def fallback_to_chunked(self):
        """After a persistent-launch failure: every plan runs the chunked (non-resident) kernels until
        restore_persistent(), and the status words are cleared (stream-ordered).  Each plan's mode
        is saved once (a second fallback before the restore keeps the first saved mode); plans created
        while fallen back (a new grid shape) start chunked too (_plan)."""
        self._fallen_back = True
        for plan in self._plans.values():
            if plan._saved_mode is None:
                plan._saved_mode = plan.persist_mode
            plan._set_mode(0)
            plan.status_t.zero_()

    def restore_persistent(self):
        """Back to the persistent kernels (where they fit) after fallback_to_chunked(): the engine
        re-promotes after a number of clean iterations (core/inversion.py _FaultMonitor).  Each plan
        gets back the mode it had before the fallback: a plan pinned to the chunked kernels (0) or to
        one region class (8 / 12 / 16) keeps it; the fault-path test mode (-1) comes back as auto (1).
        A plan whose mode was set directly (set_persistent) during the fallback keeps that mode."""
        self._fallen_back = False
        for plan in self._plans.values():
            mode = plan._saved_mode
            if mode is None:
                continue                           # never fell back: nothing to restore
            plan._saved_mode = None
            plan._set_mode(1 if mode == -1 else mode)

    def coefficients(self, v):
        """Debug/inspection: the K3 fields (alpha, temp1, temp2, kappa, beta, v) on the padded grid."""
        _hip.require_device(v)
        plan = self._plan(v.shape[2], v.shape[3], v.device)
        v = v.float()
        if self.normalize and not self._fused_denorm():
            v = self.v_denorm_func(v)
        coeffs, vstat = plan.coeffs(v, 0 if self._fused_denorm() else 1)
        sz = plan.sizes(v.shape[0])
        f = coeffs[:6 * v.shape[0] * sz.Hp * sz.ld].view(6, v.shape[0], sz.Hp, sz.ld)[..., :sz.Wp]
        return dict(zip(("alpha", "temp1", "temp2", "kappa", "beta", "v"), f.unbind(0)))
