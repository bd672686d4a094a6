/*
 * red_diffeq_sampling.h — C ABI of the prior-sampling reverse step (libred_diffeq_hip.so).
 *
 * One fused elementwise launch per reverse step of the reference's samplers
 * (SimingShan/red-diffeq red_diffeq/models/diffusion.py: model_predictions 411-429,
 * p_mean_variance / p_sample 431-446, ddim_sample 469-494).  Same conventions as the rdq_red_*
 * entry points of red_diffeq_unet.h: plain fp32 pointers, caller-owned, stream-ordered, no host
 * synchronisation, 0 / negative error codes, RDQ_E_INVALID (-10001) on null or bad arguments.
 */
#ifndef RED_DIFFEQ_SAMPLING_H
#define RED_DIFFEQ_SAMPLING_H

#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* What the U-Net output `out` is (GaussianDiffusion.objective). */
#define RDQ_OBJ_PRED_NOISE 0
#define RDQ_OBJ_PRED_X0 1
#define RDQ_OBJ_PRED_V 2

/* Which reverse step. */
#define RDQ_STEP_ANCESTRAL 0  /* p_sample (431-446) */
#define RDQ_STEP_DDIM 1       /* ddim_sample with time_next >= 0 (485-490) */
#define RDQ_STEP_DDIM_LAST 2  /* ddim_sample with time_next < 0 (481-483): x_next = x0 */

/* The seven fp32 schedule buffers of GaussianDiffusion, each of `T` entries on the device.  A table that
 * the chosen objective / mode does not read may be null (see rdq_sample_step). */
typedef struct rdq_sample_tables {
    const float *sqrt_recip_ac;    /* sr   : pred_noise, DDIM */
    const float *sqrt_recipm1_ac;  /* srm1 : pred_noise, DDIM */
    const float *sqrt_ac;          /* sa   : pred_v */
    const float *sqrt_1mac;        /* s1ma : pred_v */
    const float *post_coef1;       /* c1   : ancestral */
    const float *post_coef2;       /* c2   : ancestral */
    const float *post_logvar;      /* posterior_log_variance_clipped: ancestral with noise */
} rdq_sample_tables;

/* One reverse step over B samples of n elements each; t int64 [B] on the device, one timestep per sample,
 * each in [0, T) (an index outside is clamped into the tables, never read out of bounds).
 *
 *   x0 (411-429)   pred_noise: sr[t] x - srm1[t] out;  pred_x0: out;  pred_v: sa[t] x - s1ma[t] out;
 *                  then clamped to [-1, 1].
 *   ancestral      mean = c1[t] x0 + c2[t] x;  x_next = mean + exp(0.5 logvar[t]) noise.
 *                  noise null = the t = 0 step: x_next = mean.
 *   DDIM           eps = (sr[t] x - x0) / srm1[t]  (re-derived from the clamped x0, all objectives);
 *                  x_next = x0 a_next + c eps + sigma noise, with a_next = sqrt(alpha_next), c and sigma of
 *                  lines 485-488 formed on the host.  noise may be null only when sigma == 0.
 *   DDIM last      x_next = x0.
 *
 * Every product and sum above is rounded to fp32 on its own, in the reference's order (no FMA contraction).
 *
 * x_next may alias x_t: every thread reads its elements before it writes them.  No other output may overlap an
 * input; in particular t_out must not be t, which the other workgroups of a sample are still reading
 * (RDQ_E_INVALID).  x_start_out (nullable) receives the clamped x0.  t_out (nullable, int64 [B]) receives t_next in
 * the same launch when t_next >= 0 and is left untouched otherwise, so that x_next / t_out can be the static
 * input buffers of a captured U-Net forward (Unet.graph_io) and the next replay needs no copies.
 * a_next, c, sigma are read in DDIM mode only.  16-byte accesses when n % 4 == 0 and every tensor pointer is
 * 16-byte aligned, scalar accesses otherwise. */
int rdq_sample_step(int32_t B, int64_t n, int32_t objective, int32_t mode, int32_t T,
                    const rdq_sample_tables *tables, const int64_t *t, const float *x_t, const float *out,
                    const float *noise, float a_next, float c, float sigma, int64_t t_next, float *x_next,
                    float *x_start_out, int64_t *t_out, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RED_DIFFEQ_SAMPLING_H */
