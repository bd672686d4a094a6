/*
 * red_diffeq_misfit.h — C ABI of the data misfits beyond L1 (libred_diffeq_hip.so, csrc/misfit.hip).
 *
 * K13: masked L2, Huber and trace-normalised correlation (global-correlation) misfits of a predicted
 * against an observed record, per model.  The masked L1 misfit stays K5 (red_diffeq_fwi.h, rdq_l1_*).
 *
 * Operands: pred, y and the optional mask are contiguous fp32 [B][ns][nt][ng] (mask NULL = all ones);
 * loss, norm and gout are fp32 [B].  Caller-owned buffers, stream-ordered on `stream`, no allocation and no
 * host synchronisation inside (the calls can sit in a captured graph), no float atomics: every sum has a
 * fixed order, results are bitwise reproducible, and what is computed for one trace or element does not
 * depend on B, ns or the launch grid (a shot shard computes the bits the full survey computes for its shots).
 * 0 or a negative error code (-hipError_t, RDQ_E_INVALID = -10001).
 *
 * Definitions.  m is the mask value (1 without a mask).  d = fl32(pred - y), one fp32 rounding, as K5.
 * Everything after that is fp64 (the widened fp32 values), with ONE final rounding to fp32 per output.
 *
 * RDQ_MISFIT_L2
 *   loss[b]  = fl32( sum(m d^2) / nobs[b] ),  nobs[b] = max(fl32(sum m), 1)  (K5's normaliser); the term is
 *              fl64(m (d d)), d d exact in fp64.
 *   dpred    = fl32( ((2 m) d) g ),  g = fl64(gout[b] / nobs[b]); (2 m) d is exact in fp64.
 * RDQ_MISFIT_HUBER, delta > 0 finite (fp32)
 *   rho(d)   = fl64((d d) / (2 delta)) where |d| <= delta, else fl64(|d| - delta / 2); the branch compares
 *              the fp32 values.  rho and rho' are continuous at delta.
 *   loss[b]  = fl32( sum fl64(m rho(d)) / nobs[b] )
 *   dpred    = fl32( (m clamp(fl64(d / delta), -1, 1)) g )
 * RDQ_MISFIT_NCC, per trace tau = (b, s, g) over time
 *   pt = m p, yt = m y (exact in fp64);  a = sum_t fl64(pt pt), c = sum_t fl64(yt yt), q = sum_t fl64(pt yt)
 *   (the products are exact for 0 / 1 masks), summed in fp64 in a fixed order that depends on nt and ng only.
 *   A trace is live iff c > 0 (y and mask only: loop-invariant, and a sharded run can count globally).
 *   inv = fl64(1 / fl64(sqrt(fl64(a c)))), r = fl64(q / a) if live and a > 0, else inv = r = 0.
 *   J   = fl64(1 - fl64(q / fl64(sqrt(fl64(a c))))) if live and a > 0;  1 if live and a == 0;  0 if dead.
 *   ntr[b]  = max(fl32(#live), 1),  loss[b] = fl32( sum_tau J / ntr[b] )
 *   dpred_t = fl32( (m g) ((r pt - yt) inv) ),  g = fl64(gout[b] / ntr[b]): exactly 0 on dead traces and on
 *             traces with a == 0.
 *
 * `norm` receives nobs (L2, Huber) or ntr (NCC) from the forward and is read by the backward; a shot-sharded
 * caller passes the backward the survey's global value instead.
 */
#ifndef RED_DIFFEQ_MISFIT_H
#define RED_DIFFEQ_MISFIT_H

#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDQ_MISFIT_L2 1
#define RDQ_MISFIT_HUBER 2
#define RDQ_MISFIT_NCC 3

/* Host-only (no GPU needed); 0 for bad arguments.
 *   workspace  L2 / Huber: double [B][nchunk][2], nchunk = ceil(ns nt ng / 4096) (K5's layout);
 *              NCC: double [B][ns][ntc][3][ng] partial (a, c, q) sums, ntc = ceil(nt / 64) time chunks, then
 *              double [B][ntile][2] (sum J, #live) of 256 traces each, ntile = ceil(ns ng / 256).
 *   coef       NCC only (0 for the other kinds): double [B][ns][ng][3] = (inv, r, J) per trace. */
size_t rdq_misfit_workspace_bytes(int32_t kind, int32_t B, int32_t ns, int32_t nt, int32_t ng);
size_t rdq_misfit_coef_bytes(int32_t kind, int32_t B, int32_t ns, int32_t ng);

/* RDQ_E_INVALID: an unknown kind, a non-positive dimension, Huber with delta <= 0 or not finite, a null
 * required buffer (mask may be NULL; coef is required by NCC only; delta is ignored by L2 and NCC). */
int rdq_misfit_forward(int32_t kind, int32_t B, int32_t ns, int32_t nt, int32_t ng, float delta, const float *pred,
                       const float *y, const float *mask, float *loss, float *norm, double *coef, void *workspace,
                       hipStream_t stream);
int rdq_misfit_backward(int32_t kind, int32_t B, int32_t ns, int32_t nt, int32_t ng, float delta, const float *pred,
                        const float *y, const float *mask, const float *norm, const double *coef, const float *gout,
                        float *dpred, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RED_DIFFEQ_MISFIT_H */
