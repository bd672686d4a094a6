// misfit.hip — K13: the data misfits beyond L1 on the MI355X (C ABI and definitions: include/red_diffeq_misfit.h).
//
// L2 / Huber  K5's two-pass shape (csrc/fwi.hip): per (model, chunk) fp64 partial sums of the element terms
//             and of the mask, then one workgroup per model adding them in chunk order; an elementwise
//             backward.  One element functor per kind (MfL2, MfHuber), one copy of each kernel.
// NCC         pass 1  per-trace partial sums (a, c, q) over one time chunk of NCC_TC samples.  The [nt][ng]
//                     slab of a shot is contiguous with time at stride ng: a 256-thread workgroup takes a tile
//                     of wt = min(256, ng - c0) columns and uses R wt threads, R = 256 / wt (210 of 256 at
//                     ng = 70); thread k owns column k % wt and walks the rows phase, phase + R, ... of the
//                     chunk (phase = k / wt), so that consecutive threads read consecutive floats whatever ng
//                     is.  The R phases of a column are added through LDS in phase order.
//             pass 2  one thread per trace adds its chunks in chunk order, stores (inv, r, J) and the
//                     workgroup's (sum J, #live) of 256 traces in a fixed tree.
//             pass 3  the L2 / Huber final pass on the tile sums: loss and ntr.
//             backward one elementwise pass with the per-trace coefficients (L2-resident).
// No float atomics; the order of every sum depends on (nt, ng) or on the model's element count only, never on
// B, ns or the grid.  Built with -ffp-contract=off: the rounding counts of the header are literally true.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "red_diffeq_misfit.h"

namespace {

constexpr int RDQ_E_INVALID = -10001;
constexpr int MF_BLOCK = 256;
constexpr int MF_ITEMS = 16;    // elements per thread per chunk (chunk = MF_BLOCK * MF_ITEMS, K5's)
constexpr int NCC_BLOCK = 256;  // threads of every NCC kernel; columns per tile, traces per pass-2 workgroup
constexpr int NCC_TC = 64;      // time samples per pass-1 workgroup: fixed, so a trace's bits are the grid's no matter
constexpr int NCC_UNROLL = 4;   // rows a pass-1 thread loads before it adds them (in row order)

__device__ __forceinline__ double block_sum(double v, double *sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int w = blockDim.x / 2; w > 0; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// element functors: rho(d) the loss term, psi(d) = rho'(d) (before the mask and gout / nobs)
struct MfL2 {
    __device__ static double rho(float d, float) { const double w = (double)d; return w * w; }
    __device__ static double psi(float d, float) { return 2.0 * (double)d; }
};
struct MfHuber {
    __device__ static double rho(float d, float delta)
    {
        const double w = (double)d, dl = (double)delta;
        return fabsf(d) <= delta ? (w * w) / (2.0 * dl) : fabs(w) - 0.5 * dl;
    }
    __device__ static double psi(float d, float delta)
    {
        return fmin(fmax((double)d / (double)delta, -1.0), 1.0);
    }
};

// pass 1: per (model, chunk) partial sums of mask * rho(pred - y) and of mask (fp64, fixed order)
template <class F>
__global__ __launch_bounds__(MF_BLOCK) void k_mf_partial(int64_t n, float delta, const float *__restrict__ pred,
                                                         const float *__restrict__ y,
                                                         const float *__restrict__ mask,
                                                         double *__restrict__ part, int nchunk)
{
    __shared__ double sh[MF_BLOCK];
    const int b = blockIdx.y, c = blockIdx.x;
    const int64_t base = (int64_t)b * n;
    const int64_t c0 = (int64_t)c * MF_BLOCK * MF_ITEMS;
    double se = 0.0, sm = 0.0;
    float dv[MF_ITEMS], mv[MF_ITEMS];
#pragma unroll
    for (int k = 0; k < MF_ITEMS; ++k) {      // all loads first (clamped index, no branch per element)
        const int64_t j = min(c0 + (int64_t)k * MF_BLOCK + threadIdx.x, n - 1);
        mv[k] = mask ? mask[base + j] : 1.0f;
        dv[k] = pred[base + j] - y[base + j];
    }
#pragma unroll
    for (int k = 0; k < MF_ITEMS; ++k) {
        const int64_t j = c0 + (int64_t)k * MF_BLOCK + threadIdx.x;
        if (j < n) {
            se += (double)mv[k] * F::rho(dv[k], delta);
            sm += (double)mv[k];
        }
    }
    se = block_sum(se, sh);
    sm = block_sum(sm, sh);
    if (threadIdx.x == 0) {
        part[((size_t)b * nchunk + c) * 2] = se;
        part[((size_t)b * nchunk + c) * 2 + 1] = sm;
    }
}

// final pass of every kind: one workgroup per model; thread t adds the (sum, count) pairs t, t + 256, ... in
// order, then a fixed tree.  norm = max(fl32(count), 1), loss = fl32(sum / norm).
__global__ __launch_bounds__(MF_BLOCK) void k_mf_final(int npart, const double *__restrict__ part, float *loss,
                                                       float *norm)
{
    __shared__ double sh[MF_BLOCK];
    const int b = blockIdx.x;
    const double *pb = part + (size_t)b * npart * 2;
    double se = 0.0, sm = 0.0;
    int c = threadIdx.x;
    for (; c + 7 * MF_BLOCK < npart; c += 8 * MF_BLOCK) {   // eight independent loads in flight
        double e[8], m[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { e[u] = pb[(c + u * MF_BLOCK) * 2]; m[u] = pb[(c + u * MF_BLOCK) * 2 + 1]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { se += e[u]; sm += m[u]; }
    }
    for (; c < npart; c += MF_BLOCK) { se += pb[c * 2]; sm += pb[c * 2 + 1]; }
    se = block_sum(se, sh);
    sm = block_sum(sm, sh);
    if (threadIdx.x == 0) {
        const float no = fmaxf((float)sm, 1.0f);
        norm[b] = no;
        loss[b] = (float)(se / (double)no);
    }
}

template <class F>
__global__ __launch_bounds__(256) void k_mf_backward(int64_t n, float delta, const float *__restrict__ pred,
                                                     const float *__restrict__ y, const float *__restrict__ mask,
                                                     const float *__restrict__ norm,
                                                     const float *__restrict__ gout, float *__restrict__ dpred)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (j >= n) return;
    const int64_t i = (int64_t)b * n + j;
    const double g = (double)gout[b] / (double)norm[b];
    const float m = mask ? mask[i] : 1.0f;
    const float d = pred[i] - y[i];
    dpred[i] = (float)(((double)m * F::psi(d, delta)) * g);
}

// ------------------------------------------------------------------------------------------- NCC
__device__ __forceinline__ void ncc_add(float p, float yv, float m, double &a, double &c, double &q)
{
    const double pt = (double)m * (double)p, yt = (double)m * (double)yv;
    a += pt * pt;
    c += yt * yt;
    q += pt * yt;
}

// pass 1: grid (B ns, column tiles, time chunks); part is double [B ns][ntc][3][ng]
__global__ __launch_bounds__(NCC_BLOCK) void k_ncc_partial(int nt, int ng, int ntc, const float *__restrict__ pred,
                                                           const float *__restrict__ y,
                                                           const float *__restrict__ mask,
                                                           double *__restrict__ part)
{
    __shared__ double sh[3][NCC_BLOCK];
    const int bs = blockIdx.x, ch = blockIdx.z;
    const int c0 = blockIdx.y * NCC_BLOCK;
    const int wt = min(NCC_BLOCK, ng - c0);
    const int R = NCC_BLOCK / wt;
    const int k = threadIdx.x;
    const int phase = k / wt;
    const int col = c0 + (k - phase * wt);
    const int t1 = min(nt, (ch + 1) * NCC_TC);
    double a = 0.0, c = 0.0, q = 0.0;
    if (phase < R) {
        const size_t base = (size_t)bs * nt * ng + col;
        int t = ch * NCC_TC + phase;
        for (; t + (NCC_UNROLL - 1) * R < t1; t += NCC_UNROLL * R) {
            float pv[NCC_UNROLL], yv[NCC_UNROLL], mv[NCC_UNROLL];
#pragma unroll
            for (int u = 0; u < NCC_UNROLL; ++u) {
                const size_t i = base + (size_t)(t + u * R) * ng;
                pv[u] = pred[i];
                yv[u] = y[i];
                mv[u] = mask ? mask[i] : 1.0f;
            }
#pragma unroll
            for (int u = 0; u < NCC_UNROLL; ++u) ncc_add(pv[u], yv[u], mv[u], a, c, q);
        }
        for (; t < t1; t += R) {
            const size_t i = base + (size_t)t * ng;
            ncc_add(pred[i], y[i], mask ? mask[i] : 1.0f, a, c, q);
        }
    }
    sh[0][k] = a;
    sh[1][k] = c;
    sh[2][k] = q;
    __syncthreads();
    if (k < wt) {                              // phase 0 adds the column's other phases in phase order
        for (int ph = 1; ph < R; ++ph) {
            a += sh[0][k + ph * wt];
            c += sh[1][k + ph * wt];
            q += sh[2][k + ph * wt];
        }
        double *o = part + ((size_t)bs * ntc + ch) * 3 * ng + col;
        o[0] = a;
        o[ng] = c;
        o[2 * (size_t)ng] = q;
    }
}

// pass 2: grid (trace tiles of NCC_BLOCK, B); coef is double [B][ns ng][3] = (inv, r, J), tiles double [B][ntile][2]
__global__ __launch_bounds__(NCC_BLOCK) void k_ncc_trace(int ns, int ng, int ntc, const double *__restrict__ part,
                                                         double *__restrict__ coef, double *__restrict__ tiles)
{
    __shared__ double sh[NCC_BLOCK];
    const int b = blockIdx.y;
    const int ntrace = ns * ng;
    const int j = blockIdx.x * NCC_BLOCK + threadIdx.x;
    double J = 0.0, live = 0.0;
    if (j < ntrace) {
        const int s = j / ng, g = j - s * ng;
        const double *pp = part + ((size_t)(b * ns + s) * ntc) * 3 * ng + g;
        double a = 0.0, c = 0.0, q = 0.0;
        for (int ch = 0; ch < ntc; ++ch) {
            a += pp[0];
            c += pp[ng];
            q += pp[2 * (size_t)ng];
            pp += 3 * (size_t)ng;
        }
        double inv = 0.0, r = 0.0;
        if (c > 0.0) {
            live = 1.0;
            J = 1.0;
            if (a > 0.0) {
                const double root = sqrt(a * c);
                inv = 1.0 / root;
                r = q / a;
                J = 1.0 - q / root;
            }
        }
        double *o = coef + ((size_t)b * ntrace + j) * 3;
        o[0] = inv;
        o[1] = r;
        o[2] = J;
    }
    J = block_sum(J, sh);
    live = block_sum(live, sh);
    if (threadIdx.x == 0) {
        tiles[((size_t)b * gridDim.x + blockIdx.x) * 2] = J;
        tiles[((size_t)b * gridDim.x + blockIdx.x) * 2 + 1] = live;
    }
}

// backward: grid (ceil(nt ng / 256), ns, B)
__global__ __launch_bounds__(256) void k_ncc_backward(int ns, int nt, int ng, const float *__restrict__ pred,
                                                      const float *__restrict__ y, const float *__restrict__ mask,
                                                      const float *__restrict__ norm, const double *__restrict__ coef,
                                                      const float *__restrict__ gout, float *__restrict__ dpred)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y, b = blockIdx.z;
    if (j >= nt * ng) return;
    const int g = j % ng;
    const size_t tr = ((size_t)b * ns + s) * ng + g;
    const size_t i = ((size_t)b * ns + s) * nt * ng + j;
    const double inv = coef[tr * 3], r = coef[tr * 3 + 1];
    const double gn = (double)gout[b] / (double)norm[b];
    const double m = mask ? (double)mask[i] : 1.0;
    const double pt = m * (double)pred[i], yt = m * (double)y[i];
    dpred[i] = (float)((m * gn) * ((r * pt - yt) * inv));
}

inline bool dims_ok(int32_t kind, int32_t B, int32_t ns, int32_t nt, int32_t ng)
{
    if (kind != RDQ_MISFIT_L2 && kind != RDQ_MISFIT_HUBER && kind != RDQ_MISFIT_NCC) return false;
    if (B < 1 || ns < 1 || nt < 1 || ng < 1) return false;
    if (B > 65535 || (int64_t)B * ns > 0x7fffffff) return false;                    // grid limits
    if (kind == RDQ_MISFIT_NCC && (ns > 65535 || (int64_t)nt * ng > 0x7fffffff - 256 ||
                                   (int64_t)ns * ng > 0x7fffffff - 256)) return false;
    return true;
}

inline int64_t mf_chunks(int64_t n) { return (n + MF_BLOCK * MF_ITEMS - 1) / (MF_BLOCK * MF_ITEMS); }
inline int ncc_tc(int nt) { return (nt + NCC_TC - 1) / NCC_TC; }
inline int ncc_tiles(int ns, int ng) { return (int)(((int64_t)ns * ng + NCC_BLOCK - 1) / NCC_BLOCK); }

}  // namespace

extern "C" {

size_t rdq_misfit_workspace_bytes(int32_t kind, int32_t B, int32_t ns, int32_t nt, int32_t ng)
{
    if (!dims_ok(kind, B, ns, nt, ng)) return 0;
    if (kind == RDQ_MISFIT_NCC)
        return ((size_t)B * ns * ncc_tc(nt) * 3 * ng + (size_t)B * ncc_tiles(ns, ng) * 2) * sizeof(double);
    return (size_t)B * mf_chunks((int64_t)ns * nt * ng) * 2 * sizeof(double);
}

size_t rdq_misfit_coef_bytes(int32_t kind, int32_t B, int32_t ns, int32_t ng)
{
    if (!dims_ok(kind, B, ns, 1, ng)) return 0;
    return kind == RDQ_MISFIT_NCC ? (size_t)B * ns * ng * 3 * sizeof(double) : 0;
}

int rdq_misfit_forward(int32_t kind, int32_t B, int32_t ns, int32_t nt, int32_t ng, float delta, const float *pred,
                       const float *y, const float *mask, float *loss, float *norm, double *coef, void *workspace,
                       hipStream_t st)
{
    if (!dims_ok(kind, B, ns, nt, ng) || !pred || !y || !loss || !norm || !workspace) return RDQ_E_INVALID;
    if (kind == RDQ_MISFIT_HUBER && !(delta > 0.0f && std::isfinite(delta))) return RDQ_E_INVALID;
    double *ws = (double *)workspace;
    if (kind == RDQ_MISFIT_NCC) {
        if (!coef) return RDQ_E_INVALID;
        const int ntc = ncc_tc(nt), ntile = ncc_tiles(ns, ng);
        const int ctiles = (ng + NCC_BLOCK - 1) / NCC_BLOCK;
        if (ntc > 65535 || ctiles > 65535) return RDQ_E_INVALID;
        double *tiles = ws + (size_t)B * ns * ntc * 3 * ng;
        hipLaunchKernelGGL(k_ncc_partial, dim3(B * ns, ctiles, ntc), dim3(NCC_BLOCK), 0, st, nt, ng, ntc, pred, y, mask,
                           ws);
        hipLaunchKernelGGL(k_ncc_trace, dim3(ntile, B), dim3(NCC_BLOCK), 0, st, ns, ng, ntc, (const double *)ws, coef,
                           tiles);
        hipLaunchKernelGGL(k_mf_final, dim3(B), dim3(MF_BLOCK), 0, st, ntile, (const double *)tiles, loss, norm);
        return -(int)hipGetLastError();
    }
    const int64_t n = (int64_t)ns * nt * ng;
    const int64_t nchunk = mf_chunks(n);
    if (nchunk > 0x7fffffff) return RDQ_E_INVALID;
    if (kind == RDQ_MISFIT_L2)
        hipLaunchKernelGGL(k_mf_partial<MfL2>, dim3((unsigned)nchunk, B), dim3(MF_BLOCK), 0, st, n, delta, pred, y, mask,
                           ws, (int)nchunk);
    else
        hipLaunchKernelGGL(k_mf_partial<MfHuber>, dim3((unsigned)nchunk, B), dim3(MF_BLOCK), 0, st, n, delta, pred, y,
                           mask, ws, (int)nchunk);
    hipLaunchKernelGGL(k_mf_final, dim3(B), dim3(MF_BLOCK), 0, st, (int)nchunk, (const double *)ws, loss, norm);
    return -(int)hipGetLastError();
}

int rdq_misfit_backward(int32_t kind, int32_t B, int32_t ns, int32_t nt, int32_t ng, float delta, const float *pred,
                        const float *y, const float *mask, const float *norm, const double *coef, const float *gout,
                        float *dpred, hipStream_t st)
{
    if (!dims_ok(kind, B, ns, nt, ng) || !pred || !y || !norm || !gout || !dpred) return RDQ_E_INVALID;
    if (kind == RDQ_MISFIT_HUBER && !(delta > 0.0f && std::isfinite(delta))) return RDQ_E_INVALID;
    if (kind == RDQ_MISFIT_NCC) {
        if (!coef) return RDQ_E_INVALID;
        hipLaunchKernelGGL(k_ncc_backward, dim3((unsigned)(((int64_t)nt * ng + 255) / 256), ns, B), dim3(256), 0, st, ns,
                           nt, ng, pred, y, mask, norm, coef, gout, dpred);
        return -(int)hipGetLastError();
    }
    const int64_t n = (int64_t)ns * nt * ng;
    const dim3 grid((unsigned)((n + 255) / 256), B);
    if (kind == RDQ_MISFIT_L2)
        hipLaunchKernelGGL(k_mf_backward<MfL2>, grid, dim3(256), 0, st, n, delta, pred, y, mask, norm, gout, dpred);
    else
        hipLaunchKernelGGL(k_mf_backward<MfHuber>, grid, dim3(256), 0, st, n, delta, pred, y, mask, norm, gout, dpred);
    return -(int)hipGetLastError();
}

}  // extern "C"
