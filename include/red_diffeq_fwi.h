/*
 * red_diffeq_fwi.h — C ABI of the MI355X-native FWI hot path (libred_diffeq_hip.so).
 *
 * Replaces, as a drop-in boundary, the compute behind the reference's Python plugin
 * ``FWIForward`` (SimingShan/red-diffeq red_diffeq/solvers/pde.py:6-93) and the autograd
 * adjoint PyTorch derives from it (triggered at red_diffeq/core/inversion.py:86).  The Python
 * mirror of the reference interface (red-diffeq_amd/red_diffeq/solvers/pde.py) binds these
 * symbols with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - Plain pointers and sizes; device pointers unless stated "host".  No torch types.
 *   - Every call is stream-ordered on the given hipStream_t (NULL = legacy default stream) and
 *     returns 0 or a negative error code (-hipError_t, or RDQ_E_* below).
 *   - One call in flight per plan, enforced by the plan: its host state (graph cache, chain streams)
 *     is mutex-guarded, so any host thread may call it, and a forward / adjoint call on a different
 *     stream than the plan's previous one first waits (an event, no host sync) for the work that
 *     stream had queued, so calls on one plan never overlap on the device.  The previous call's
 *     stream must still exist at that point.  Different plans are independent.
 *   - The caller owns every buffer; sizes come from rdq_fwi_sizes().  The plan owns only the
 *     uploaded geometry (a few KB) and its cached hipGraphs.
 *   - Results are deterministic: every reduction has a fixed order.  The one float atomic, the wide
 *     chunked adjoint's fp64 add of a workgroup's sponge partial into its gk_part slot, has exactly
 *     one writer per slot and launch and no slot shared between concurrent launch chains (checked on
 *     the host for every launch of a time loop before it is enqueued; RDQ_E_INVALID otherwise), so
 *     each slot's adds arrive one launch after another in stream order: a fixed order.
 *   - Layout: padded grid Hp = nz + 2*nbc rows, Wp = nx + 2*nbc columns, row pitch `ld`
 *     floats (Wp rounded up to 64).  fp32 throughout, as the reference.
 */
#ifndef RED_DIFFEQ_FWI_H
#define RED_DIFFEQ_FWI_H

#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDQ_E_INVALID (-10001) /* bad argument / shape */
#define RDQ_E_NOMEM (-10002)   /* host allocation failed */
#define RDQ_E_HANDOFF (-10003) /* a persistent kernel's neighbour hand-off timed out (results invalid) */

/* Acquisition geometry, host memory.  Mirrors FWIForward's ctx after __init__ and adj_sr
 * (pde.py:16-23, 54-59): all indices already on the padded grid. */
typedef struct rdq_fwi_geom {
    int32_t nz, nx;            /* model size (rows = depth, cols = width) */
    int32_t nbc;               /* sponge width, pde.py ctx['nbc'] */
    int32_t nt;                /* time steps */
    int32_t ns, ng;            /* shots, receivers */
    int32_t sample_temporal;   /* record every k-th step (pde.py:82) */
    float dx, dt;
    int32_t isz, igz;          /* source / receiver row on the padded grid */
    const int32_t *isx;        /* host [ns] source columns (padded grid) */
    const int32_t *igx;        /* host [ng] receiver columns (padded grid) */
    const double *wavelet;     /* host [nt] source wavelet, fp64, shared by every shot: the Ricker wavelet
                                  (pde.py:26-36) or any other signature; cast to fp32 by the plan */
} rdq_fwi_geom;

typedef struct rdq_fwi_plan rdq_fwi_plan;

/* Byte sizes of the caller-owned buffers for batch B (number of velocity models). */
typedef struct rdq_fwi_sizes_t {
    int32_t Hp, Wp, ld, nrec;  /* padded grid, row pitch (floats), recorded steps */
    size_t coeffs;             /* float [6][B][Hp][ld] alpha, temp1, temp2, kappa, beta, v; then
                                  v_model [B][nz][nx] and the sponge amplitude ks [B] */
    size_t vstat;              /* float vmin[B] then int64 argmin[B] (row-major index into nz*nx) */
    size_t seis;               /* float [B][ns][nrec][ng] */
    size_t history;            /* float [nt+2][B][ns][Hp][ld]; slot j = P_{j-1} */
    size_t ring;               /* workspace, 32 B per grid cell: the chunked kernels use it as float
                                  [4][B][ns][Hp][ld] (two in/out level pairs: no-grad forward,
                                  adjoint lambdas), the persistent kernels as u64 hand-off granules
                                  [2 parity][2 level][B][ns][Hp][ld] */
    size_t gA;                 /* float [B][ns][Hp][ld] per-shot accumulator d(loss)/d(alpha) */
    size_t gk_part;            /* double [B][ns][n_adj_blocks] sponge-coefficient partial sums */
    size_t gbeta;              /* float [B][ns] source-amplitude gradient */
    size_t colsum;             /* double [B][Hp][nx] replicate-fold workspace */
} rdq_fwi_sizes_t;

/* Create / destroy a plan (uploads geometry; replaces FWIForward.__init__, pde.py:8-24). */
int rdq_fwi_plan_create(const rdq_fwi_geom *geom, rdq_fwi_plan **plan);
int rdq_fwi_plan_destroy(rdq_fwi_plan *plan);
int rdq_fwi_sizes(const rdq_fwi_plan *plan, int32_t B, rdq_fwi_sizes_t *out);
/* 1 = capture each time loop into a cached hipGraph (default), 0 = direct launches. */
int rdq_fwi_set_graphs(rdq_fwi_plan *plan, int32_t enable);
/* Time steps advanced per launch by the forward / adjoint kernels (temporal blocking depth,
 * 1..4; the wide chunked adjoint has its own depth, rdq_fwi_set_wide_adj_steps) and the number of
 * concurrent shot-group launch chains of the chunked kernels (1..16, or 0 = auto, the default: 2 for
 * the wide kernels, 1 for the 64-column ones).  Results are identical for every setting; only speed
 * changes. */
int rdq_fwi_set_tuning(rdq_fwi_plan *plan, int32_t fwd_steps, int32_t adj_steps, int32_t chains);
/* Kernel variant flags (a new plan starts at RDQ_VARIANT_FWD_GEN):
 *   RDQ_VARIANT_FWD_GEN    the chunked forward regenerates alpha/temp1/temp2 from the model in
 *                          registers instead of loading the three K3 fields (identical results;
 *                          14% faster on the configs[4] grid);
 *   RDQ_VARIANT_ADJ_EXACT  the adjoint keeps the oracle's exact fp32 operation order (gA
 *                          bit-identical to oracle/fwi_oracle.c) instead of, in the persistent
 *                          kernels, rebuilding the gradient's stencil term from the forward's time
 *                          recurrence with FMA contraction (dL/dv within ~1e-5 rel-L2) and, in the
 *                          wide chunked kernels, contracting the stencils into FMAs (dL/dv within
 *                          ~2e-5).  Plans whose sponge is thinner than 20 cells (nbc < 20) always run
 *                          the exact order: there the recurrence's cancellation is not fp32-accurate
 *                          (5e-3 at nbc = 4) and standing modes amplify any contraction;
 *   RDQ_VARIANT_NO_XCD_LOCAL the persistent kernels publish every neighbour hand-off write-through
 *                          (sc1) instead of keeping whole slices on one XCD (read from HW_REG_XCC_ID)
 *                          with L2-resident hand-offs (identical results; slower);
 *   RDQ_VARIANT_NARROW_CHUNKED the chunked (non-resident) kernels run 64-column regions, one column
 *                          per lane, instead of 128-column regions of two columns per lane
 *                          (identical results; more halo traffic);
 *   RDQ_VARIANT_CHUNKED_ADJ_FMA the wide chunked adjoint contracts its stencils into FMAs (about 4 %
 *                          faster at configs[4]; dL/dv within ~2e-5 of the oracle, the sponge sum gk,
 *                          a difference of nearly equal adjoint levels, within ~1.3e-4).  Without it
 *                          (default) the chunked adjoint keeps the oracle's exact order: gA / gbeta
 *                          bit-identical, gk to fp64 summation order.  Ignored when
 *                          RDQ_VARIANT_ADJ_EXACT is set or nbc < 20. */
#define RDQ_VARIANT_FWD_GEN 1
#define RDQ_VARIANT_ADJ_EXACT 2
#define RDQ_VARIANT_NO_XCD_LOCAL 4
#define RDQ_VARIANT_NARROW_CHUNKED 8
#define RDQ_VARIANT_CHUNKED_ADJ_FMA 16
int rdq_fwi_set_variant(rdq_fwi_plan *plan, int32_t flags);
/* Time steps per launch of the WIDE chunked adjoint (k_adj_tw, 1..6, or 0 = the default, 5: the
 * fastest depth measured at configs[4] for both the exact-order and the contracted kernels,
 * profiles/r5/configs4_wide_adj_depth.jsonl).  rdq_fwi_set_tuning's adj_steps sets the persistent and the
 * narrow chunked adjoints' depth only.  A time loop whose nt is not a multiple of the depth ends with
 * one shorter launch of its own depth.  Results are identical for every depth. */
int rdq_fwi_set_wide_adj_steps(rdq_fwi_plan *plan, int32_t steps);
/* Shots per workgroup of the WIDE chunked adjoint (1..64, or 0 = auto, the default: the cheapest of
 * 16 / 8 / 4 / 2 / 1 under rounds of one workgroup per CU x (shots + a workgroup's fixed cost)): a workgroup runs that many
 * shots of one region in turn and generates the region's alpha / kappa once for all of them.
 * Results are identical for every setting. */
int rdq_fwi_set_wide_adj_shots(rdq_fwi_plan *plan, int32_t shots);
/* The same for the WIDE chunked forward (k_fwd_tw; 0 = auto, the default). */
int rdq_fwi_set_wide_fwd_shots(rdq_fwi_plan *plan, int32_t shots);
/* Time steps per launch of the WIDE chunked forward (k_fwd_tw, 1..6, or 0 = rdq_fwi_set_tuning's
 * fwd_steps, the default).  Results are identical for every depth. */
int rdq_fwi_set_wide_fwd_steps(rdq_fwi_plan *plan, int32_t steps);
/* Rows per wave of the 64 x 96-region persistent kernels: forward 6, 8, 12 or 24 (16, 12, 8 or 4
 * waves per workgroup), adjoint (FMA build) 6, 8 or 12.  Same region geometry and results.  The time
 * step is latency-bound, so more resident waves win (configs[1], tools/ab_rw.sh, tools/ab_adj_nb6.sh):
 * forward 6 rows 1.31 ms (barrier-free exchange), 8 rows 1.40, 12 rows 1.63, 24 rows 2.42; adjoint
 * 6 rows 1.65 ms, 8 rows 1.67, 12 rows 2.08.  Default 6 / 6. */
int rdq_fwi_set_rows_per_wave(rdq_fwi_plan *plan, int32_t fwd_rows, int32_t adj_rows);
/* Delay, in 10 ns ticks (0..100000), between a persistent launch's per-epoch publish of its border and
 * its first hand-off sweep pass, for the forward and the adjoint (defaults 15 / 0 = 0.15 / 0 us: a
 * forward pass issued at once mostly finds the neighbours' granules not there yet and queues ahead of
 * the one that would; configs[1] forward 1.210 -> 1.196 ms against 0.25 us; the barrier-free adjoint
 * is fastest without a delay).  Results are identical for every delay; only speed changes. */
int rdq_fwi_set_sweep_delay(rdq_fwi_plan *plan, int32_t fwd_ticks, int32_t adj_ticks);
/* What a persistent launch overlaps with the round trip of its per-epoch hand-off sweep, for the forward
 * and the (recurrence) adjoint; 0 = nothing (sweep, then the post-sweep work):
 *   adjoint 1 (default): the sweep's first pass is issued into registers of its own and the dead cells
 *              (outside the next epoch's dependence cone) are zeroed while it is in flight, instead of
 *              after the sweep on the path to the next step (configs[1]: 1.490 -> 1.458 ms);
 *   forward:   0 only (RDQ_E_INVALID otherwise): no overlapped form of the forward measured faster.
 * Mode 1 is built at 4 steps per epoch (the default depth); other depths and the exact-order adjoint run
 * mode 0 (rdq_fwi_launch_info reports the mode that runs).  Only the order of independent register and
 * memory operations differs: results are bit-identical in both modes. */
int rdq_fwi_set_handoff_overlap(rdq_fwi_plan *plan, int32_t fwd_mode, int32_t adj_mode);
/* Wave roles of the persistent forward and (recurrence) adjoint; 0 = every wave runs the generic time loop:
 *   adjoint 1 (default): a wave whose rows hold neither the source row nor the receiver row runs every
 *              epoch but the last in a loop of its own, with the per-step source / receiver /
 *              end-of-record / history-guard tests compiled out (they are wave-uniform and constant for
 *              the launch); the other waves, and the last epoch, run the generic loop (configs[1]:
 *              1.446 -> 1.419 ms);
 *   forward:   0 only (RDQ_E_INVALID otherwise): the same split of the forward measured no faster.
 * Mode 1 is built at 4 steps per epoch (the default depth); other depths and the exact-order adjoint run
 * mode 0 (rdq_fwi_launch_info reports the mode that runs).  The hand-off, the mailbox exchange and every
 * cell's arithmetic are the same in both modes: results are bit-identical.  Changing the mode drops the
 * plan's cached graphs. */
int rdq_fwi_set_wave_roles(rdq_fwi_plan *plan, int32_t fwd_mode, int32_t adj_mode);
/* Source role of the persistent forward; 0 = every wave runs the generic time loop (RDQ_E_INVALID for any
 * other mode than those below, nothing changed):
 *   forward 1 (default): the wave whose rows own the source row is the one every step waits for.  Where that
 *              row is the receiver row too (isz == igz) and every step is recorded (sample_temporal 1), that
 *              wave runs every epoch but the last in a loop of its own: a guard-free step plus its real work
 *              with the row's pair a compile-time constant (one packed add of the source term, the receiver
 *              value, the wavelet loads and the record), and the waves with neither row run the guard-free
 *              loop (no source / receiver / history / end-of-record test, no wavelet loads); configs[1]:
 *              1.034 -> 0.958 ms;
 *   adjoint:   0 only here (RDQ_E_INVALID otherwise): the adjoint's role has a setter of its own,
 *              rdq_fwi_set_adjoint_role.
 * Built at 4 steps per epoch and 6 rows per wave of the 96-row regions; not run where the source row has a
 * live halo copy in a neighbouring region, by a call that keeps no history, or at other depths, rows per wave
 * or region classes: those run the generic loop (rdq_fwi_source_role_info reports the mode that runs).  Per
 * cell the operations and their order are the same: results are bit-identical in both modes.  Changing the
 * mode drops the plan's cached graphs. */
int rdq_fwi_set_source_role(rdq_fwi_plan *plan, int32_t fwd_mode, int32_t adj_mode);
/* out = {the source-role mode the forward of a call with batch B runs, the same for the adjoint (0)}; 0 for
 * chunked launches. */
int rdq_fwi_source_role_info(rdq_fwi_plan *plan, int32_t B, int32_t out[2]);
/* Source/receiver role of the persistent (recurrence) adjoint; mode 0 / 1, default 1 (RDQ_E_INVALID for any
 * other mode, nothing changed):
 *   1: the wave whose rows own the source row, where that row is the receiver row too, runs every epoch but the
 *      last in a loop of its own: the guard-free step plus the row's own work (the receiver residual's add, the
 *      source term's undo and the gbeta term of the gradient, the next epoch's sample and residual loads) with
 *      the row's pair a compile-time constant.  The pair is the same for every tile, shot and model, so the
 *      host picks the kernel built for it;
 *   0: that wave runs the generic loop.
 * Runs where the forward's source role would (4 steps per epoch, 6 rows per wave of the 96-row regions,
 * isz == igz, sample_temporal 1, no live halo copy of the row) and only with the adjoint's wave roles on
 * (rdq_fwi_set_wave_roles) in the recurrence adjoint; the phase-profiled build has no role.  Per cell the
 * operations and their order are the same: results are bit-identical in both modes.  Changing the mode drops
 * the plan's cached graphs. */
int rdq_fwi_set_adjoint_role(rdq_fwi_plan *plan, int32_t mode);
/* out = {the adjoint-role mode the adjoint of a call with batch B runs (0 for chunked launches), the mirrored
 * row pair 0..2 of the source/receiver row in the wave that owns it, or -1 where the role does not run}.  A
 * launch that ran the role leaves in status word 24 (rdq_fwi_debug_words) the number of waves that entered the
 * role's loop: one per workgroup whose interior rows own the source row; the word is zeroed by every
 * persistent adjoint call. */
int rdq_fwi_adjoint_role_info(rdq_fwi_plan *plan, int32_t B, int32_t out[2]);
/* How the adjoint's source/receiver role fetches its receiver residuals and wavelet samples; mode 0 / 1, default
 * 1 (RDQ_E_INVALID for any other mode, nothing changed):
 *   0: an epoch ahead: the T residuals and T samples of the next epoch, issued after the hand-off sweep;
 *   1: the residuals a step ahead: step k issues step k - 1's residual ahead of its own history prefetch, the
 *      epoch's last step that of the next epoch's first step; a step's head, where the residual goes into the
 *      rows the neighbouring waves wait for, then finds a value issued a whole step earlier.  The samples,
 *      read at a step's end, stay an epoch ahead.
 * Only the role's loop differs (launches without the role run the same kernels whatever is set); the values
 * loaded are the same: results are bit-identical in both modes.  Changing the mode drops the plan's cached
 * graphs. */
int rdq_fwi_set_adjoint_fetch(rdq_fwi_plan *plan, int32_t mode);
/* *out = the fetch mode the adjoint of a call with batch B runs: 0 wherever the role does not run. */
int rdq_fwi_adjoint_fetch_info(rdq_fwi_plan *plan, int32_t B, int32_t *out);
/* The mirrored row pair (0..2) the role uses for padded row `padded_row` (>= 0; host only, no plan). */
int rdq_fwi_role_row_pair(int32_t padded_row);
/* 1 (default) = run each time loop as ONE persistent launch (regions resident in registers for
 * all nt steps, epoch-wise neighbour hand-offs) whenever the whole grid fits resident on the
 * device: small surveys (at most 200 workgroups, e.g. 3 OpenFWI shots) in 64 x 64 regions of 16
 * waves x 4 rows, otherwise 64 x 96 regions if they fit, else 64 x 64 regions of 8 waves x 8 rows;
 * 16 / 12 / 8 = only that region class; 0 = always the chunked launches.  Identical results in every mode.  -1 (fault-path tests only):
 * persistent launches oversubscribed to twice the resident capacity, so they report "not resident"
 * through the status word instead of computing. */
int rdq_fwi_set_persistent(rdq_fwi_plan *plan, int32_t mode);
/* Synchronises `stream` and reports (then clears) a persistent-kernel hand-off timeout:
 * 0, or RDQ_E_HANDOFF when some launch since the last call gave up waiting for a neighbour. */
int rdq_fwi_status(rdq_fwi_plan *plan, hipStream_t stream);
/* Diagnostics (synchronises the device): the plan's 32 status words: [0] hand-off status
 * (1 = neighbour timeout, 2 = launch not resident), [16..23] workgroups per XCD of the last
 * persistent launch. */
int rdq_fwi_debug_words(rdq_fwi_plan *plan, uint32_t out[32]);
/* Caller-owned status words (device memory, >= 64 uint32, zeroed by the caller; NULL = the plan's
 * own): word 0 is non-zero once a persistent launch gave up (1 = neighbour hand-off timeout,
 * 2 = launch not resident) and stays so until the caller clears it.  Lets the caller read it
 * stream-ordered without a host sync (e.g. as the Adam guard of rdq_adam_step, or copied
 * asynchronously to pinned host memory).  Replaces the plan's internal words for later launches. */
int rdq_fwi_set_status_buffer(rdq_fwi_plan *plan, uint32_t *words);
/* Which kernels a forward / adjoint call for batch B runs: out = {forward persistent region
 * class (16 = 64 x 64 regions of 16 waves x 4 rows, 12 = 64 x 96 regions, 8 = 64 x 64 of 8 waves x 8
 * rows; 0 = chunked), the same for the adjoint, forward steps per epoch/launch,
 * adjoint steps per epoch/launch, forward time-loop launches per call, adjoint time-loop launches
 * per call (persistent: one per resident shot group; chunked: ceil(nt / T)), the hand-off overlap mode
 * the forward runs, the same for the adjoint (rdq_fwi_set_handoff_overlap; 0 for chunked launches), the
 * wave-role mode the forward runs, the same for the adjoint (rdq_fwi_set_wave_roles; 0 for chunked
 * launches)}.  `out` holds 10 words (8 before rdq_fwi_set_wave_roles existed). */
int rdq_fwi_launch_info(rdq_fwi_plan *plan, int32_t B, int32_t out[10]);
/* The wide chunked kernels' launch shape for batch B: out = {concurrent launch chains, shots per
 * workgroup of the forward's and of the adjoint's full-depth launches of chain 0 (the automatic choice
 * unless rdq_fwi_set_wide_*_shots fixed one), shots in chain 0}. */
int rdq_fwi_wide_info(rdq_fwi_plan *plan, int32_t B, int32_t out[4]);
/* Diagnostics: 1 = the persistent kernels accumulate per-wave phase times (s_memrealtime, 10 ns
 * ticks); read_profile synchronises the device, returns and clears them:
 * out[0..5] forward {hand-off wait, time steps, publish, waves, first sweep pass, sweep passes},
 * out[6..11] the same for the adjoint. */
int rdq_fwi_set_profile(rdq_fwi_plan *plan, int32_t enable);
int rdq_fwi_read_profile(rdq_fwi_plan *plan, uint64_t out[12]);
/* Per-wave records of the last read_profile: out[(block * 16 + wave) * 3 + {0,1,2}] = {hand-off,
 * steps, publish} ticks of the forward (adj = 0) or adjoint (adj = 1) kernel. */
int rdq_fwi_profile_waves(rdq_fwi_plan *plan, int32_t adj, uint64_t *out, size_t count);
/* The finer split of the last read_profile: out[0..4] forward, out[5..9] adjoint, each {a, b, c, d,
 * gradient} ticks summed over waves.  The hand-off wait = a + b + c + d exactly: a = publish end to the
 * first sweep pass's issue (delay, scalar loads), b = the first pass's round trip, c = later passes,
 * d = after the sweep (dead-cell zeroing, deferred history stores, the next step's boundary rows, receiver
 * records / next-epoch loads; also the launch prologue and the last epoch).  gradient = the adjoint's
 * deferred gradient, which the publish figure of read_profile includes; publish - gradient = the granule
 * stores' issue. */
int rdq_fwi_profile_split(rdq_fwi_plan *plan, uint64_t out[10]);
/* Per-wave records in full: out[(block * 16 + wave) * 8 + i], i = {hand-off, steps, publish, a, b, c, d,
 * gradient} as above. */
int rdq_fwi_profile_waves_split(rdq_fwi_plan *plan, int32_t adj, uint64_t *out, size_t count);

/* Velocity input convention of rdq_fwi_coeffs / rdq_fwi_grad_finalize. */
#define RDQ_VEL_NORMALIZED 0  /* v_norm in [-1,1], denormalised in-kernel: (v+1)/2*3000+1500 */
#define RDQ_VEL_PHYSICAL 1    /* velocity in m/s (FWIForward(normalize=False) or a custom denorm) */

/* K3: coefficient fields from a velocity v[b][0][iz][ix] given by element strides (any view,
 * e.g. mu[:, :, 1:-1, 1:-1]).  Replaces v_denormalize + F.pad(replicate) + get_Abc + the
 * alpha/temp1/temp2/beta lines (data_trans.py:13-15, pde.py:91, 38-52, 63-71). */
int rdq_fwi_coeffs(const rdq_fwi_plan *plan, int32_t B, const float *v, const int64_t strides[4],
                   int32_t vel_mode, float *coeffs, void *vstat, hipStream_t stream);

/* K1: forward time loop (pde.py:74-86).  history == NULL: no-grad forward; otherwise every P_j
 * is kept in `history` for the adjoint.  `ring` is the workspace (required when the persistent
 * kernel runs; the chunked history path does not touch it). */
int rdq_fwi_forward(const rdq_fwi_plan *plan, int32_t B, const float *coeffs, float *seis,
                    float *history, float *ring, hipStream_t stream);

/* K2: discrete adjoint of the forward (the autograd backward of pde.py:74-86), given
 * dseis = d(loss)/d(seis).  Writes the accumulators gA, gk_part, gbeta (overwritten).  All buffers
 * are device memory (hipMalloc / torch CUDA tensors): the wide chunked kernels add into gk_part with
 * hardware fp64 atomics, which fine-grained host memory does not support. */
int rdq_fwi_adjoint(const rdq_fwi_plan *plan, int32_t B, const float *coeffs,
                    const float *history, const float *dseis, float *ring, float *gA,
                    double *gk_part, float *gbeta, hipStream_t stream);

/* Checkpointed gradient: K1 + K2 with the wavefield history bounded by recomputation, for jobs whose
 * store-all history (rdq_fwi_sizes().history, nt + 2 levels) does not fit.  The first pass keeps two
 * levels every K steps; the backward walks the segments from the last to the first, recomputes each
 * one's levels from its checkpoint into `seg` and runs the adjoint over it: 2 (nseg - 1) + K + 2 levels
 * instead of nt + 2, for one extra forward.
 *   Layout.  Segments are counted from the END of the record: nseg = ceil(nt / K), boundaries
 *   b_c = max(nt - c K, 0) for c = 0 .. nseg, segment c = the steps [b_{c+1}, b_c) (the first segment in
 *   time is the short one).  Checkpoint c, 0 < c < nseg, is the history's slots {b_c, b_c + 1} =
 *   {P_{b_c - 1}, P_{b_c}}: levels {2 (c - 1), 2 (c - 1) + 1} of `ckpt`, float [nseg - 1][2][B][ns][Hp][ld].
 *   The boundary at 0 is two zero levels and is not stored.  `seg` is float [K + 2][B][ns][Hp][ld]: while
 *   segment c is worked on, its level j is the history's slot b_{c+1} + j.  Any K >= 1 is legal (K < 1:
 *   RDQ_E_INVALID); K >= nt is one segment with no checkpoint (`ckpt` may be NULL) and counts as K = nt.
 *   Identical results.  Both calls run the chunked kernels (wide or narrow, the plan's depths, chains
 *   and variant flags) whatever rdq_fwi_set_persistent says.  The recomputed levels are the forward's own
 *   bits and the adjoint adds into gA / gbeta per launch in the fixed order k = nt .. 1, so seis, gA and
 *   gbeta are bit-identical to rdq_fwi_forward + rdq_fwi_adjoint on the chunked kernels for every K; each
 *   gk_part slot receives its launches' fp64 partials in the same k order, but a launch never spans a
 *   boundary, so gk_part is bit-identical when K is a multiple of the adjoint's depth (then the launches
 *   are those of the store-all run) and equal to fp64 summation order (~1e-15 relative) otherwise.
 *   The recompute records no seismograms: `seis` is not needed by rdq_fwi_adjoint_ckpt.  `ring` as for
 *   rdq_fwi_forward / rdq_fwi_adjoint (one buffer may serve both calls). */
typedef struct rdq_fwi_ckpt_sizes_t {
    int32_t nseg; int32_t seg_levels;   /* segments; levels in `seg` (min(K, nt) + 2) */
    size_t ckpt;                        /* checkpoint store bytes (0 for one segment) */
    size_t seg;                         /* segment history bytes (<= K+2 levels) */
} rdq_fwi_ckpt_sizes_t;
int rdq_fwi_ckpt_sizes(const rdq_fwi_plan *plan, int32_t B, int32_t K, rdq_fwi_ckpt_sizes_t *out);
/* First pass: seis as rdq_fwi_forward's, and the checkpoint store. */
int rdq_fwi_forward_ckpt(const rdq_fwi_plan *plan, int32_t B, int32_t K, const float *coeffs,
                         float *seis, float *ckpt, float *ring, hipStream_t stream);
/* Backward: the accumulators gA, gk_part, gbeta (overwritten) as rdq_fwi_adjoint's; `seg` is scratch. */
int rdq_fwi_adjoint_ckpt(const rdq_fwi_plan *plan, int32_t B, int32_t K, const float *coeffs,
                         const float *ckpt, float *seg, const float *dseis, float *ring,
                         float *gA, double *gk_part, float *gbeta, hipStream_t stream);
/* out = {first-pass persistent class (0 = chunked: always, today), nseg, first-pass time-loop launches
 * per launch chain, backward time-loop launches per chain (every segment's recompute and adjoint)}. */
int rdq_fwi_ckpt_info(rdq_fwi_plan *plan, int32_t B, int32_t K, int32_t out[4]);

/* Linearised (Born) forward: dseis = J dv, J = d(seis)/d(v) at the model `coeffs` was made from; with K2 + K4
 * (which apply J^T) the Gauss-Newton product J^T W J dv.
 *   Equations.  The forward step is P_{n+1} = T1 P_n - T2 P_{n-1} + A Lap(P_n) + beta_src w[n], T1 = 2 + 2 c1 A - K,
 *   T2 = 1 - K, Lap = c2 S1 + c3 S2 (the four nearest and the four second neighbours, periodic wrap).  Its tangent is
 *     dP_{n+1} = T1 dP_n - T2 dP_{n-1} + A Lap(dP_n) + dA (2 c1 P_n + Lap(P_n)) - dK (P_n - P_{n-1}) + dbeta_src w[n],
 *   dP_0 = dP_{-1} = 0, recorded at the receivers when n % sample_temporal == 0, where the forward records, with
 *     dA    = 2 v (dt/dx)^2 dv   on the padded grid, dv replicate-padded (the clamped model index, as K3 reads v),
 *     dbeta = 2 v dt^2 dv        at each source cell,
 *     dK    = K dv[argmin] / vmin: the sponge is linear in vmin (pde.py:41-46) and torch.min passes the tangent of
 *             the first row-major argmin only, the cell `vstat` holds,
 *   and dv = 1500 dv_norm under RDQ_VEL_NORMALIZED.  The two bracketed terms are the ones whose transposes K2
 *   accumulates into gA and gk_part.
 *   Scale.  J is linear, so the prologue brings each model's direction to a fixed magnitude with a power of two
 *   (dvs = dv 2^-k, max |dvs| in [2^-64, 2^-63)) and the time loop multiplies what it records by 2^k: the loop runs
 *   on the same bits whatever the magnitude of dv, and for max |dv| >= 2^-64 the rescale is exact.  k = floor(log2
 *   max |dv|) + 64, kept within [-63, 126] so that 2^k and 2^-k are normal floats: for max |dv| >= 2^63 the scale
 *   stays at 2^-126 and max |dvs| grows with the direction (2 at the largest float: still an exact rescale, far
 *   from overflow), and for max |dv| below the smallest normal float (denormals, or a zero direction) the scale is
 *   2^63 and max |dvs| < 2^-63.
 *   Layout.  `dwork` (rdq_fwi_born_sizes bytes) is float dam [B][nz][nx] (dA per model cell, from dvs in m/s; a
 *   padded cell reads the model cell its clamped index names), then ratio [B] (dvs[argmin] / vmin), dbeta [B][ns],
 *   oscale [B] (2^k) and uint32 dmax [B] (the bits of max |dv|);
 *   rdq_fwi_dcoeffs, the prologue, writes it from a direction
 *   dv[b][0][iz][ix] given by element strides (any view, as rdq_fwi_coeffs reads v) and the `coeffs` / `vstat` of
 *   rdq_fwi_coeffs for the same model.  `history` is the store-all history rdq_fwi_forward kept for the same
 *   `coeffs` (slot j = P_{j-1}); `dseis_out` is float [B][ns][nrec][ng] like seis; `ring` as for rdq_fwi_forward
 *   (its four levels carry dP between launches; one buffer may serve every call).
 *   rdq_fwi_born always runs the narrow chunked kernels at rdq_fwi_set_tuning's fwd_steps and chains, whatever
 *   rdq_fwi_set_persistent or RDQ_VARIANT_NARROW_CHUNKED say (RDQ_VARIANT_FWD_GEN chooses its coefficient source as
 *   for the forward), under the one-call-in-flight rule of the other time loops.  One fixed fp32 operation order (no
 *   contraction; written next to the kernel): dseis is bit-identical for every depth, chain count and graph
 *   setting, and J (2^j dv) = 2^j J dv bit for bit while max |dv| >= 2^-64 on both sides.  RDQ_E_INVALID for a
 *   null argument or B < 1. */
int rdq_fwi_born_sizes(const rdq_fwi_plan *plan, int32_t B, size_t *bytes);
int rdq_fwi_dcoeffs(const rdq_fwi_plan *plan, int32_t B, const float *dv, const int64_t strides[4],
                    int32_t vel_mode, const float *coeffs, const void *vstat, float *dwork,
                    hipStream_t stream);
int rdq_fwi_born(const rdq_fwi_plan *plan, int32_t B, const float *coeffs, const float *dwork,
                 const float *history, float *dseis_out, float *ring, hipStream_t stream);

/* Fused forward + Born pass: seis and dseis = J dv in ONE time loop that keeps no wavefield history, for jobs whose
 * store-all history does not fit (rdq_fwi_born needs all nt + 2 levels).  Forward-mode linearisation reads P_n and
 * P_{n-1} only, and the forward step of the same register region produces exactly those levels on exactly the
 * cells the tangent's taps read, so the kernel carries two levels of P and two of dP per launch, in and out.
 *   Equations.  The forward step and its tangent as written above (rdq_fwi_born); `dwork` is what rdq_fwi_dcoeffs
 *   writes, unchanged.
 *   Layout.  `seis` and `dseis_out` are float [B][ns][nrec][ng].  `ring` as for rdq_fwi_forward: its levels 0-3
 *   carry the P pair between launches and its levels 4-7 the dP pair.  K and `ckpt` choose the checkpoint store of
 *   rdq_fwi_forward_ckpt: with `ckpt` non-null and K < nt the launches are cut at the segment boundaries b_c =
 *   max(nt - c K, 0) and the launch that ends on an interior boundary writes {P_{b_c - 1}, P_{b_c}} into levels
 *   {2 (c - 1), 2 (c - 1) + 1} of `ckpt` (rdq_fwi_ckpt_sizes(K).ckpt bytes), exactly the layout and bits of
 *   rdq_fwi_forward_ckpt's store, so rdq_fwi_adjoint_ckpt consumes it unchanged (the Gauss-Newton product under a
 *   history budget: this call, then rdq_fwi_adjoint_ckpt on weight * dseis, then K4).  K >= nt or `ckpt` == NULL is
 *   one segment and nothing is stored.
 *   The call always runs the narrow chunked kernels at rdq_fwi_set_tuning's fwd_steps and chains, as rdq_fwi_born
 *   does, under the one-call-in-flight rule of the other time loops.  The P update is the chunked forward's
 *   operation order and the dP update rdq_fwi_born's (no contraction; written next to the kernel), and the
 *   Laplacian of P_n is one expression that serves both.  The forward's bits are therefore the stored history's
 *   bits: `seis` is bit-identical to rdq_fwi_forward's, `dseis_out` to rdq_fwi_born's and `ckpt` to
 *   rdq_fwi_forward_ckpt's, for every depth, chain count, graph setting and K.  RDQ_E_INVALID for a null required
 *   argument (all but `ckpt`), B < 1, or K < 1 with a non-null `ckpt`. */
int rdq_fwi_born_fused(const rdq_fwi_plan *plan, int32_t B, int32_t K, const float *coeffs,
                       const float *dwork, float *seis, float *dseis_out, float *ckpt, float *ring,
                       hipStream_t stream);

/* Caller-supplied source wavelets, per model and per shot, and their gradient: K1 / K2 and their checkpointed
 * forms with the samples read from device memory instead of the plan's wavelet (rdq_fwi_geom.wavelet).
 *   Equations.  The forward step as written above (rdq_fwi_born) with w[n] replaced by the call's own sample,
 *     P_{n+1}[b, s, isz, isx[s]] += beta[b, isz, isx[s]] * w[b, s, n],   n = 0 .. nt - 1,
 *   w[b, s, n] = wav[b * model_stride + s * shot_stride + n] (s is the plan's own shot index), in the chunked
 *   forward's fp32 order (add = beta * w; P = P + add).  The seismograms are linear in w.  With L_k the adjoint field
 *   of P_k (K2), taken after step k's receiver residual has been added (where K2 reads it for gbeta), the transpose is
 *     gwav[b, s, k - 1] = L_k[b, s, isz, isx[s]] * beta[b, isz, isx[s]]      (one fp32 multiply),
 *   and gbeta[b, s] = sum_k L_k(src) w[b, s, k - 1] as before, with the loaded sample.  A wavelet shared between
 *   shots or models (a zero stride) receives the sum of gwav over the shared axes, which is the caller's to take.
 *   One writer per element.  The narrow kernels' tile interiors partition the padded grid, so exactly one lane of one
 *   workgroup owns a shot's source cell, and a call runs every step k once (a checkpointed call: once in the
 *   segment that holds it).  Every gwav element is therefore written exactly once per call, with a plain store: no
 *   atomics, no dependence on what the buffer held (it is overwritten, not accumulated), one fixed result.
 *   These calls always run the narrow chunked kernels at rdq_fwi_set_tuning's depths and chains, whatever
 *   rdq_fwi_set_persistent or RDQ_VARIANT_NARROW_CHUNKED say (RDQ_VARIANT_FWD_GEN chooses the forward's coefficient
 *   source), stream-ordered on caller-owned buffers under the one-call-in-flight rule.  The other arguments are
 *   those of the call each one mirrors; a checkpointed backward's recompute reads the same device wavelets, so they
 *   must be unchanged between the two calls.  seis, gwav, gA and gbeta are bit-identical for every depth, chain
 *   count, graph setting and K, and with the plan's own wavelet passed as (wav, 0, 0) seis, gA and gbeta are those
 *   of the plain calls on the narrow chunked kernels.  RDQ_E_INVALID for a null `src` or `wav`, B < 1 or a
 *   negative stride. */
typedef struct rdq_fwi_source {
    const float *wav;                    /* device, fp32: sample n of model b, shot s at wav[b*model_stride + s*shot_stride + n] */
    int64_t model_stride, shot_stride;   /* in floats; 0 = shared by all models / all shots */
    float *gwav;                         /* adjoint calls only: float [B][ns][nt] = d(loss)/d(w[b, s, :]), overwritten;
                                            NULL = not wanted */
} rdq_fwi_source;
int rdq_fwi_forward_src(const rdq_fwi_plan *plan, int32_t B, const float *coeffs, const rdq_fwi_source *src,
                        float *seis, float *history, float *ring, hipStream_t stream);
int rdq_fwi_adjoint_src(const rdq_fwi_plan *plan, int32_t B, const float *coeffs, const rdq_fwi_source *src,
                        const float *history, const float *dseis, float *ring, float *gA, double *gk_part,
                        float *gbeta, hipStream_t stream);
int rdq_fwi_forward_ckpt_src(const rdq_fwi_plan *plan, int32_t B, int32_t K, const float *coeffs,
                             const rdq_fwi_source *src, float *seis, float *ckpt, float *ring, hipStream_t stream);
int rdq_fwi_adjoint_ckpt_src(const rdq_fwi_plan *plan, int32_t B, int32_t K, const float *coeffs,
                             const rdq_fwi_source *src, const float *ckpt, float *seg, const float *dseis,
                             float *ring, float *gA, double *gk_part, float *gbeta, hipStream_t stream);

/* Encoded simultaneous sources ("supershots") and their gradient: ne wavefields per model, each fired by ALL ns
 * sources of the plan at once, source s of supershot e with its own effective wavelet (a code E[b, e, s] times a
 * signature, formed by the caller).  K1 / K2, their checkpointed forms and K4 for such a call.
 *   Equations.  Wavefield (b, e) obeys the forward step as written above (rdq_fwi_born) with the source term
 *     P_{n+1}[b, e, isz, isx[s]] += beta[b, isz, isx[s]] * weff[b, e, s, n]     for every s = 0 .. ns - 1,
 *   weff[b, e, s, n] = wav[b * model_stride + e * enc_stride + s * source_stride + n], in ascending s and per source
 *   in the chunked forward's fp32 order (add = beta * weff; P = P + add).  Sources that share a padded cell add one
 *   after the other, ascending s.  Every source is injected, one whose samples are zero included: the bits do not
 *   depend on the sparsity pattern of a code.  The receivers record as in K1.  With L_k the adjoint field of (b, e)
 *   after step k's receiver residual (rdq_fwi_*_src above), the transposes are
 *     gwav [b, e, s, k - 1] = L_k[b, e, isz, isx[s]] * beta[b, isz, isx[s]]       (one fp32 multiply),
 *     gbeta[b, e, s]        = sum_k L_k[b, e, isz, isx[s]] * weff[b, e, s, k - 1]  (fp32, k = nt .. 1, as K2),
 *   and gA, gk_part are per wavefield, exactly K2's with ns replaced by ne.
 *   Layout.  Every per-shot buffer of the calls these mirror has ns replaced by ne: seis and dseis [B][ne][nrec][ng],
 *   history [nt + 2][B][ne][Hp][ld], ring, gA [B][ne][Hp][ld], gk_part [B][ne][nblk], the checkpoint store and the
 *   segment buffer.  rdq_fwi_sizes_enc / rdq_fwi_ckpt_sizes_enc give their sizes (rdq_fwi_sizes / rdq_fwi_ckpt_sizes
 *   with ns replaced by ne), except that gbeta is float [B][ne][ns].  gwav is float [B][ne][ns][nt].
 *   One writer per element.  The tile interiors partition the padded grid, so exactly one lane of one workgroup owns
 *   a source cell of wavefield (b, e); it owns every source on that cell and writes their gwav and gbeta elements,
 *   and a call runs every step k once.  gwav is stored plainly, once per element and call (overwritten, not
 *   accumulated); gbeta is zeroed by the call and accumulated by its owner lane alone, in the order of k.  No atomics.
 *   rdq_fwi_grad_finalize_enc is K4 for these accumulators: the ne planes of gA and of gk_part are summed in order
 *   where K4 sums its ns planes, and source cell s takes sum_e gbeta[b, e, s] (fp32, ascending e).
 *   The calls always run the narrow chunked kernels at rdq_fwi_set_tuning's depths and chains, whatever
 *   rdq_fwi_set_persistent or RDQ_VARIANT_NARROW_CHUNKED say, stream-ordered on caller-owned buffers under the
 *   one-call-in-flight rule, with the checkpoint layout of rdq_fwi_forward_ckpt; a checkpointed backward's recompute
 *   reads the same device samples, which must be unchanged between the two calls.  seis, gwav, gA and gbeta are
 *   bit-identical for every depth, chain count, graph setting and K.  A supershot whose samples are zero but for one
 *   source s records rdq_fwi_forward_src's seismogram of shot s with the same samples (a zero term leaves a sum's
 *   value unchanged), and with ne = ns and weff[b, e, s] = (e == s) w[b, s] the accumulators hold the values of
 *   rdq_fwi_adjoint_src's, gbeta on its diagonal.  RDQ_E_INVALID for a null `enc` or `wav`, ne < 1, B < 1 or a
 *   negative stride (and, as in the calls they mirror, a null required buffer). */
typedef struct rdq_fwi_encoding {
    int32_t ne;                          /* supershots per model */
    const float *wav;                    /* device, fp32: weff[b, e, s, n] at wav[b*model_stride + e*enc_stride + s*source_stride + n] */
    int64_t model_stride, enc_stride, source_stride;   /* in floats; 0 = shared along that axis */
    float *gwav;                         /* adjoint calls only: float [B][ne][ns][nt] = d(loss)/d(weff), overwritten;
                                            NULL = not wanted */
} rdq_fwi_encoding;
int rdq_fwi_sizes_enc(const rdq_fwi_plan *plan, int32_t B, int32_t ne, rdq_fwi_sizes_t *out);
int rdq_fwi_ckpt_sizes_enc(const rdq_fwi_plan *plan, int32_t B, int32_t ne, int32_t K, rdq_fwi_ckpt_sizes_t *out);
int rdq_fwi_forward_enc(const rdq_fwi_plan *plan, int32_t B, const float *coeffs, const rdq_fwi_encoding *enc,
                        float *seis, float *history, float *ring, hipStream_t stream);
int rdq_fwi_adjoint_enc(const rdq_fwi_plan *plan, int32_t B, const float *coeffs, const rdq_fwi_encoding *enc,
                        const float *history, const float *dseis, float *ring, float *gA, double *gk_part,
                        float *gbeta, hipStream_t stream);
int rdq_fwi_forward_ckpt_enc(const rdq_fwi_plan *plan, int32_t B, int32_t K, const float *coeffs,
                             const rdq_fwi_encoding *enc, float *seis, float *ckpt, float *ring, hipStream_t stream);
int rdq_fwi_adjoint_ckpt_enc(const rdq_fwi_plan *plan, int32_t B, int32_t K, const float *coeffs,
                             const rdq_fwi_encoding *enc, const float *ckpt, float *seg, const float *dseis,
                             float *ring, float *gA, double *gk_part, float *gbeta, hipStream_t stream);

/* K4: d(loss)/d(v) [B][nz][nx] (contiguous) from the accumulators: chain through
 * alpha/beta/sponge(vmin), replicate-pad fold, and (RDQ_VEL_NORMALIZED) the x1500 of the
 * denormalisation. */
int rdq_fwi_grad_finalize(const rdq_fwi_plan *plan, int32_t B, const float *coeffs,
                          const void *vstat, const float *gA, const double *gk_part,
                          const float *gbeta, int32_t vel_mode, double *colsum, float *g_v,
                          hipStream_t stream);
/* K4 of an encoded call (rdq_fwi_*_enc above): gA [B][ne][Hp][ld], gk_part [B][ne][nblk], gbeta [B][ne][ns].
 * RDQ_E_INVALID for ne < 1 and whatever rdq_fwi_grad_finalize refuses. */
int rdq_fwi_grad_finalize_enc(const rdq_fwi_plan *plan, int32_t B, int32_t ne, const float *coeffs,
                              const void *vstat, const float *gA, const double *gk_part,
                              const float *gbeta, int32_t vel_mode, double *colsum, float *g_v,
                              hipStream_t stream);

/* Source illumination / pseudo-Hessian diagonal (Shin et al.): the diagonal of J_A^T J_A with the Green's functions
 * dropped, per wavefield.  With C1X2 = -5, C2 = fp32(4/3), C3 = fp32(-1/12) and S1 / S2 the nearest / second-neighbour
 * sums with periodic wrap, ((up + down) + left) + right:
 *
 *   q_k[b,w,z,x] = C1X2 P_{k-1} + (C2 S1(P_{k-1}) + C3 S2(P_{k-1}))    fp32, one rounding per operation, no contraction:
 *                                                                       the factor the adjoint multiplies L_k by for gA
 *   hA[b,w,z,x]  = sum_{k = nt .. 1} q_k^2                              fp32: t = q q; acc = acc + t; k DESCENDING from 0
 *   H[b,iz,ix]   = (dA/dv)^2 sum_{(z,x) -> (iz,ix)} sum_w hA[b,w,z,x]   fp64: ascending w, then the replicate fold (the
 *                                                                       padded cells whose clamped index is (iz,ix), the
 *                                                                       set K4 folds gA over), one cast to fp32
 *   dA/dv        = 2 v (dt/dx)^2 in fp64, v the model cell's fp32 velocity in m/s; x 1500 under RDQ_VEL_NORMALIZED
 *
 * The sponge (gk) and source-amplitude (gbeta) paths of the Jacobian are left out, and so is the receiver side.
 *
 * rdq_fwi_illum: hA from a stored history [nt+2][B][nwf][Hp][ld] written by any forward family (persistent, wide,
 * narrow, _src, _enc); nwf = the history's wavefields per model, 0 = the plan's ns.  hA has the size and layout of
 * rdq_fwi_sizes(B).gA (rdq_fwi_sizes_enc(B, nwf).gA for nwf wavefields) and is overwritten: every element of
 * [B][nwf][Hp][0..Wp) is written whatever the buffer held, the pitch columns are neither read nor written, and the
 * history's pitch columns are never read.
 * rdq_fwi_illum_ckpt: the same bits from the checkpoint store of rdq_fwi_forward_ckpt / _src / _enc /
 * rdq_fwi_born_fused with K steps per segment: segments from the last to the first, each recomputed into `seg` by the
 * forward the matching rdq_fwi_adjoint_ckpt{,_src,_enc} call would run (src / enc: that call's, at most one of them),
 * then accumulated in k = hi .. lo + 1.  ckpt may be NULL when K >= nt (one segment).
 * rdq_fwi_illum_finalize: H [B][nz][nx] (contiguous) from hA; colsum is rdq_fwi_sizes(B).colsum bytes of workspace.
 * Stream-ordered on caller-owned buffers, one call per plan at a time, graph-cached like the passes above.
 * RDQ_E_INVALID: a null required pointer, B < 1, nwf < 0, K < 1, both src and enc, an unusable src / enc, a missing
 * ckpt with more than one segment, a vel_mode other than 0 / 1. */
int rdq_fwi_illum(const rdq_fwi_plan *plan, int32_t B, int32_t nwf, const float *history, float *hA,
                  hipStream_t stream);
int rdq_fwi_illum_ckpt(const rdq_fwi_plan *plan, int32_t B, int32_t K, const float *coeffs,
                       const rdq_fwi_source *src, const rdq_fwi_encoding *enc, const float *ckpt, float *seg,
                       float *ring, float *hA, hipStream_t stream);
int rdq_fwi_illum_finalize(const rdq_fwi_plan *plan, int32_t B, int32_t nwf, const float *coeffs, const float *hA,
                           int32_t vel_mode, double *colsum, float *H, hipStream_t stream);

/* K5: L1 observation loss (red_diffeq/core/losses.py:14-41), contiguous [B][n] operands.
 * forward:  loss[b] = sum(|y - pred| * mask) / nobs[b],  nobs[b] = max(sum(mask), 1)
 * backward: dpred = sign(pred - y) * mask * (gout[b] / nobs[b])       (mask NULL = all ones)
 * `partial` is a workspace of rdq_l1_partial_bytes(B, n) bytes. */
size_t rdq_l1_partial_bytes(int32_t B, int64_t n);
int rdq_l1_forward(int32_t B, int64_t n, const float *pred, const float *y, const float *mask,
                   float *loss, float *nobs, void *partial, hipStream_t stream);
int rdq_l1_backward(int32_t B, int64_t n, const float *pred, const float *y, const float *mask,
                    const float *nobs, const float *gout, float *dpred, hipStream_t stream);

/* K6: TV / Tikhonov regulariser (red_diffeq/regularization/benchmark.py:4-37) on a contiguous
 * mu[B][1][H][W].  kind: 0 = TV (mean|dx| + mean|dy|), 1 = Tikhonov (mean dx^2 + mean dy^2).
 * backward writes grad = d(sum_b gout[b] * loss[b]) / d(mu) (overwritten). */
int rdq_smooth_reg_forward(int32_t kind, int32_t B, int32_t H, int32_t W, const float *mu,
                           float *loss, hipStream_t stream);
int rdq_smooth_reg_backward(int32_t kind, int32_t B, int32_t H, int32_t W, const float *mu,
                            const float *gout, float *grad, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RED_DIFFEQ_FWI_H */
