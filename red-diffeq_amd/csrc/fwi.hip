// fwi.hip — MI355X (gfx950) kernels + C ABI for red-diffeq's acoustic FWI hot path.
//
// Reference behaviour (SimingShan/red-diffeq):
//   K3 rdq_fwi_coeffs      red_diffeq/solvers/pde.py:91 (replicate pad), 38-52 (get_Abc),
//                          63-71 (alpha/temp1/temp2/beta), utils/data_trans.py:13-15 (denorm)
//   K1 rdq_fwi_forward     pde.py:74-86: the whole nt-step time loop (stencil + periodic wrap + source
//                          injection + receiver sampling + history store) in ONE persistent launch when
//                          the survey fits resident (k_fwd_pt), else launches of T steps (k_fwd_tb)
//   K2 rdq_fwi_adjoint     the autograd backward of pde.py:74-86 (discrete adjoint)
//   K4 rdq_fwi_grad_finalize  chain rule back to v_norm incl. the vmin/argmin sponge term
//   -- rdq_fwi_dcoeffs / rdq_fwi_born  torch.func.jvp of pde.py:88-93 in a direction dv: the linearised (Born)
//                          forward over K1's stored history (k_dcoeffs, k_born_tb)
//   -- rdq_fwi_born_fused  the same jvp, primal and tangent records from one time loop that keeps no history
//                          (k_fwd_born_tb), optionally writing the checkpoint store of rdq_fwi_forward_ckpt
//
// fp32 operation order follows the reference expression order exactly and the file is built
// with -ffp-contract=off, so K1 reproduces the reference seismograms bit-for-bit and K2's
// exact-order variant matches the oracle's gA accumulator bit-for-bit (tests/test_gpu_fwi.py).
//
// Data layout (HBM): padded grid Hp x Wp with row pitch ld = roundup(Wp, 64) floats (256-B
// aligned rows -> every row of a 64-wide tile is 1 or 2 full 128-B lines).
//   coeffs  [6][B][Hp][ld]       alpha, temp1, temp2, kappa, beta, v (per velocity model)
//   history [nt+2][B][ns][Hp][ld] slot j = P_{j-1}; one time step of all shots is contiguous
//   ring    [3][B][ns][Hp][ld]    rotating wavefields (no-grad forward) / adjoint lambdas
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>
#include <initializer_list>
#include <mutex>
#include <utility>

#include "red_diffeq_fwi.h"

#pragma clang fp contract(off)

namespace {

constexpr float C1X2 = -5.0f;                      // 2*c1, pde.py:66,69
constexpr float C2 = (float)(4.0 / 3.0);           // pde.py:67
constexpr float C3 = (float)(-1.0 / 12.0);         // pde.py:68

#define RDQ_CHECK(x)                                   \
    do {                                               \
        hipError_t e_ = (x);                           \
        if (e_ != hipSuccess) return -(int)e_;         \
    } while (0)
#define RDQ_TRY(x)                                     \
    do {                                               \
        const int rc_ = (x);                           \
        if (rc_ != 0) return rc_;                      \
    } while (0)


// --------------------------------------------------------------------------------------- K3
// vmin / first row-major argmin over the (unpadded) model; the padded field's first minimum
// folds back to this cell (pde.py:41, torch.min tie rule = first index).
// vmin and its first argmin per model (torch.min's tie rule, pde.py:41), in two passes: gridDim.y parts
// of each model reduce contiguous index ranges to (min, first index) partials, then one workgroup per
// model combines them (a 1.5 M-cell configs[4] model took 630 us in one workgroup).  The comparison
// (value, then index) is order-independent, so the result is the one-pass scan's bit for bit.
__device__ __forceinline__ void vstat_reduce(float &best, int64_t &bi, float *sv, int64_t *si)
{
    sv[threadIdx.x] = best;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const float ov = sv[threadIdx.x + w];
            const int64_t oi = si[threadIdx.x + w];
            if (ov < sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) {
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    best = sv[0];
    bi = si[0];
}

__global__ __launch_bounds__(256) void k_vstat_part(const float *__restrict__ vn, int64_t s0, int64_t s2,
                                                    int64_t s3, int nz, int nx, int vel_mode, int chunk,
                                                    float *pv, int64_t *pi)
{
    const int b = blockIdx.x, part = blockIdx.y;
    const int n = nz * nx, i0 = part * chunk, i1 = min(n, i0 + chunk);
    float best = INFINITY;
    int64_t bi = INT64_MAX;
    // each thread's elements in increasing order, loads issued 8 at a time
    constexpr int CH = 8;
    for (int base = i0 + threadIdx.x; base < i1; base += CH * blockDim.x) {
        float t[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int i = base + u * blockDim.x;
            const int iz = i / nx, ix = i - iz * nx;
            t[u] = i < i1 ? vn[b * s0 + iz * s2 + ix * s3] : INFINITY;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int i = base + u * blockDim.x;
            float v = t[u];
            if (vel_mode == 0) { v = v + 1.0f; v = v / 2.0f; v = v * 3000.0f; v = v + 1500.0f; }
            if (i < i1 && v < best) { best = v; bi = i; }
        }
    }
    __shared__ float sv[256];
    __shared__ int64_t si[256];
    vstat_reduce(best, bi, sv, si);
    if (threadIdx.x == 0) {
        pv[(size_t)b * gridDim.y + part] = best;
        pi[(size_t)b * gridDim.y + part] = bi;
    }
}

__global__ __launch_bounds__(256) void k_vstat_final(const float *__restrict__ pv, const int64_t *__restrict__ pi,
                                                     int parts, float lnk, float two_a, float *vmin, int64_t *amin,
                                                     float *ks)
{
    const int b = blockIdx.x;
    float best = INFINITY;
    int64_t bi = INT64_MAX;
    for (int j = threadIdx.x; j < parts; j += blockDim.x) {
        const float v = pv[(size_t)b * parts + j];
        const int64_t i = pi[(size_t)b * parts + j];
        if (v < best || (v == best && i < bi)) { best = v; bi = i; }
    }
    __shared__ float sv[256];
    __shared__ int64_t si[256];
    vstat_reduce(best, bi, sv, si);
    if (threadIdx.x == 0) {
        vmin[b] = best;
        amin[b] = bi;
        float k = 3.0f * best; k = k * lnk; k = k / two_a;   // kappa = 3*vmin*ln(1e7)/(2a), pde.py:43
        ks[b] = k;
    }
}

// Coefficient fields at one padded-grid point (pde.py:38-52, 63-71), from the model velocity
// and the per-model sponge amplitude ks = 3*vmin*ln(1e7)/(2a).  K3 stores them for inspection and
// for K4; the time-loop kernels regenerate them in registers (bit-identical: same function), so a
// launch reads a 20 KB model instead of three 400 KB padded fields per shot.
struct CoefGen {
    const float *vmod;   // [B][nz][nx] velocity (m/s)
    const float *ks;     // [B]
    int nz, nx, nbc, Hp, Wp;
    float dt, dx, a;
};

struct Coef { float v, al, t1, t2, kp; };

__device__ __forceinline__ Coef gen_coef(const CoefGen &c, int b, int z, int x)
{
    const int iz = min(max(z - c.nbc, 0), c.nz - 1);
    const int ix = min(max(x - c.nbc, 0), c.nx - 1);
    Coef o;
    o.v = c.vmod[((size_t)b * c.nz + iz) * c.nx + ix];
    const int nbc = c.nbc;
    int pi = -1;                                   // rows first, then columns overwrite (corners)
    if (z < nbc) pi = nbc - 1 - z;
    if (z >= c.Hp - nbc) pi = z - (c.Hp - nbc);
    if (x < nbc) pi = nbc - 1 - x;
    if (x >= c.Wp - nbc) pi = x - (c.Wp - nbc);
    float dmp = 0.0f;
    if (pi >= 0) { float d = (float)pi * c.dx; d = d / c.a; d = d * d; dmp = c.ks[b] * d; }
    float al = o.v * c.dt; al = al / c.dx; al = al * al;                   // pde.py:63
    o.al = al;
    o.kp = dmp * c.dt;                                                      // pde.py:65
    float t1 = C1X2 * al; t1 = t1 + 2.0f; t1 = t1 - o.kp;                   // pde.py:69
    o.t1 = t1;
    o.t2 = 1.0f - o.kp;                                                     // pde.py:70
    return o;
}

__device__ __forceinline__ float beta_of(float v, float dt) { float bt = v * dt; return bt * bt; }  // pde.py:71

struct CoefArgs {
    const float *vn;
    int64_t s0, s2, s3;
    int vel_mode, ld;
    CoefGen cg;
    float *vmod_out;
    float *coeffs;
    size_t cstride;  // B*Hp*ld
};

__global__ __launch_bounds__(256) void k_coeffs(CoefArgs p)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int z = blockIdx.y;
    const int b = blockIdx.z;
    const CoefGen &c = p.cg;
    if (x >= p.ld) return;
    const size_t i = ((size_t)b * c.Hp + z) * p.ld + x;
    if (x >= c.Wp) {
        for (int f = 0; f < 6; ++f) p.coeffs[f * p.cstride + i] = 0.0f;
        return;
    }
    const int iz = z - c.nbc, ix = x - c.nbc;
    if (iz >= 0 && iz < c.nz && ix >= 0 && ix < c.nx) {   // the model itself (unpadded)
        float v = p.vn[b * p.s0 + iz * p.s2 + ix * p.s3];
        if (p.vel_mode == 0) { v = v + 1.0f; v = v / 2.0f; v = v * 3000.0f; v = v + 1500.0f; }  // data_trans.py:15
        p.vmod_out[((size_t)b * c.nz + iz) * c.nx + ix] = v;
    }
}

__global__ __launch_bounds__(256) void k_coeff_fields(CoefArgs p)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int z = blockIdx.y;
    const int b = blockIdx.z;
    const CoefGen &c = p.cg;
    if (x >= c.Wp) return;
    const size_t i = ((size_t)b * c.Hp + z) * p.ld + x;
    const Coef o = gen_coef(c, b, z, x);
    p.coeffs[i] = o.al;
    p.coeffs[p.cstride + i] = o.t1;
    p.coeffs[2 * p.cstride + i] = o.t2;
    p.coeffs[3 * p.cstride + i] = o.kp;
    p.coeffs[4 * p.cstride + i] = beta_of(o.v, c.dt);
    p.coeffs[5 * p.cstride + i] = o.v;
}

// buffer addressing: scalar base + 32-bit lane offset; an offset past the range is dropped (no
// memory access; loads return 0)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void *base, int bytes = 0x7fffffff)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, bytes, 0x00020000);
}
constexpr int OOB = (int)0x80000000u;               // buffer offset beyond every range: store dropped
// buffer cache policy "nt" (non-temporal, streaming): the history stream is written once and read
// once, GBs apart; without the hint it churns the L2 that carries the persistent kernels' hand-offs
// (their first sweep pass: 306 -> 220 us per forward launch, 299 -> 214 us per adjoint launch)
constexpr int CP_NT = 2;
__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
// --------------------------------------------------------------------------------------- K1/K2
// Temporal blocking on a register-resident region (the MI355X design of the time loop).
//
// A workgroup of NW waves owns a region of 64 columns (one per lane) x NW*R rows (R consecutive
// rows per wave, held in VGPRs) of one (model, shot) slice, and advances it T time steps per
// launch.  Halo H = 2T on every side: after t steps the outermost 2t rows/columns are stale, the
// interior (64-2H) x (NW*R-2H) stays exact and is the only part that is stored.  Per step:
//   - vertical taps: the wave's own registers; the two rows above/below its slab come from the
//     neighbouring waves through a 2 KB LDS exchange (double-buffered: one barrier per step);
//   - horizontal taps: DPP wave shifts (v_mov_b32_dpp wave_shr:1 / wave_shl:1) — no LDS traffic;
//   - periodic wrap (torch.roll, pde.py:79) is in the region->grid map (global index mod Hp/Wp),
//     so a tile at the domain edge simply loads wrapped rows/columns.
// T steps per launch divide the launch count (the latency floor of the per-step design) by T and
// cut the wavefield re-reads to two levels per launch; the extra arithmetic is the halo.
constexpr int TB_NW = 8;                 // waves per workgroup
constexpr int TB_R = 8;                  // rows per wave
constexpr int TB_RH = TB_NW * TB_R;      // region rows
constexpr int TB_MAXT = 4;
constexpr int TW_FWD_MAXT = 6;          // deepest wide chunked forward (k_fwd_tw instantiations 1 .. 6)
constexpr int FWD_W_MAX = TW_FWD_MAXT > TB_MAXT ? TW_FWD_MAXT : TB_MAXT;   // wavelet samples per chunked forward launch

__device__ __forceinline__ float dpp_shr1(float v)   // lane i <- lane i-1 (x-1); lane 0 reads 0
{
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_shl1(float v)   // lane i <- lane i+1 (x+1); lane 63 reads 0
{
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}

struct TBGeo {
    int B, ns, Hp, Wp, ld, isz, igz, ng, nrec, st;
    int s_off, ns_grp;                   // chunked launch: shots [s_off, s_off + ns_grp) of all B models
    int sl_off, nsl;                     // persistent launch: flat slices [sl_off, sl_off + nsl), slice = b * ns + s
    int tiles_x, ntiles;                 // tile grid of this launch's blocking depth
    size_t cstride, slice, level;        // level = B*ns*slice (one time level of all slices)
    const int *isx, *rcv_start, *rcv_list;
    const int *rlane;                    // [Wp] adjoint residual index of a column (-1: no receiver)
    int dstride;                         // residual row stride: ng, or ncolr after the fold
};

struct FwdTBArgs {
    TBGeo g;
    CoefGen cg;                          // model + sponge amplitude (GEN variant)
    const float *coeffs;                 // K3 fields: alpha, temp1, temp2 at 0, 1, 2 x cstride
    const float *in_prev, *in_cur;       // P_{n-1}, P_n   (each [B][ns][Hp][ld])
    float *hist;                         // history base (slot j = P_{j-1}) or nullptr
    float *out_prev, *out_cur;           // ring path: P_{n+T-1}, P_{n+T}
    float *seis;
    int n0, nsteps;
    int spw, ns_sh;                      // wide kernels: shots per workgroup, shots of the launch's chain
    float w[FWD_W_MAX];                  // wavelet samples w[n0 .. n0+nsteps-1]
    int hbase;                           // virtual slot held by hist's first level (0: the whole history;
                                         // a checkpointed segment's buffer starts at its first boundary)
    // SRC instantiations (rdq_fwi_*_src): the call's own wavelets, sample n of model b, shot s at
    // wav[b * wms + s * wss + n] (strides in floats, 0 = shared); `w` is not read
    const float *wav;
    long long wms, wss;
    // ENC instantiations (rdq_fwi_*_enc): g.ns counts the call's ne supershots and the kernels' `s` is the supershot
    // e; the effective sample of source j is wav[b * wms + e * wes + j * wss + n].  A lane's sources are those of
    // its column, src_list[src_start[gx] .. src_start[gx + 1]), ascending j (the twin of rcv_start / rcv_list).
    // These instantiations read neither g.isx nor the samples `w`, and their three extra arguments ride there, so
    // that the argument block (and with it the compiled text of every other instantiation) stays as it was:
    // g.isx = the plan's source table {src_start [Wp + 1], src_list [ns]} (src_start[Wp] = the source count), and
    // wes = the 64 bits of w[0], w[1] (enc_stride_bits / enc_stride).
};

__device__ __forceinline__ long long enc_stride(const float *w)
{
    return (long long)(((unsigned long long)__builtin_bit_cast(unsigned, w[1]) << 32) | __builtin_bit_cast(unsigned, w[0]));
}

// exchange two boundary rows each way between the NW waves of the workgroup
struct Halo4 { float u2, u1, d1, d2; };

template <int NW>
__device__ __forceinline__ Halo4 exchange_nw(float (*xch)[NW][4][64], int buf, int w, int lane, float top0,
                                             float top1, float bot1, float bot0)
{
    xch[buf][w][0][lane] = top0;      // row 0
    xch[buf][w][1][lane] = top1;      // row 1
    xch[buf][w][2][lane] = bot1;      // row R-2
    xch[buf][w][3][lane] = bot0;      // row R-1
    __syncthreads();
    Halo4 h;
    const int wu = w > 0 ? w - 1 : 0, wd = w < NW - 1 ? w + 1 : NW - 1;
    h.u2 = xch[buf][wu][2][lane];     // row -2 (garbage for w == 0: outside the region)
    h.u1 = xch[buf][wu][3][lane];     // row -1
    h.d1 = xch[buf][wd][0][lane];     // row R
    h.d2 = xch[buf][wd][1][lane];     // row R+1
    return h;
}

// ---- Barrier-free wave-to-wave exchange of the persistent forward and adjoint.  Each step a wave
// needs two rows above and below its own from its neighbour waves; instead of a workgroup barrier per
// step, each wave waits only for the two waves it reads from, and publishes its boundary rows as soon
// as they are computed (its interior rows follow), so the neighbours' rows are normally there at the
// first read.  History of the form (configs[1], profiles/r3/barrier_free_ab.txt, profiles/r6/
// fwd_xf_ab.txt, mailbox_ab.txt): 16-byte tagged slots {row, tag, row, tag} (round 3: forward 1.364 ->
// 1.31 ms); a per-lane flag word after the rows, which drops the 8 register moves that built the
// tagged slots and the 6 compares that checked them (1.208 -> 1.111 ms with the trims of the same
// change; every instruction a wave issues sits on the step's path: profiles/r6/issue_pad_ab.txt); the
// mailbox below (same speed for the forward, adjoint 1.560 -> 1.548 ms: it needs fewer VGPRs, which
// the 128-VGPR adjoint has none of).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
constexpr unsigned XQ_NONE = 0xFFFFFFFFu;                 // flag of a never-written inbox
// Wave priorities of the barrier-free persistent kernels (s_setprio; the SIMD's arbiter issues the
// higher-priority wave first).  A wave polling its LDS inbox (xm_wait) or the hand-off
// granules (PT_SWEEP) drops to WAIT, so its spin loop does not take issue cycles from the waves still
// computing; a wave that got its neighbours' rows runs its two boundary row pairs (what the neighbours
// wait for next) at EDGE, then its interior pairs at BODY.  Configs[1] forward, interleaved x3
// (profiles/r6/wave_priority_ab.txt): 1.342 -> 1.262 ms with the LDS spin alone at WAIT, 1.225 with the
// sweep too, 1.212 with the edge / body split; 1.362 -> 1.204 ms against no priorities in a second run,
// 1.194 with the post-sweep priority at EDGE (the default) and 1.217 with BODY = 2.  (With a barrier
// per step the adjoint gained nothing, 1.638 -> 1.646 ms with the sweep at WAIT; its barrier-free form,
// ADJR_STEP_NB, uses the same exchange and priorities: 1.646 -> 1.577 ms.)
constexpr int PT_PRIO_WAIT = 0, PT_PRIO_BODY = 1, PT_PRIO_SWEPT = 3, PT_PRIO_EDGE = 3;
// ---- Mailbox exchange (xm_*): each wave owns an inbox per buffer, {rows -1, R, -2, R+1} as 16 bytes
// (halo pairs E1 = {-1, R}, E2 = {-2, R+1}: one ds_read_b128 straight into them) and a flag pair
// {from above, from below}.  A wave writes its rows R-1, R-2 into the lower wave's inbox and its rows
// 0, 1 into the upper wave's (ds_write2_b32 straight from its row-pair registers), each followed by
// its flag there (the step's tag); waves 0 / NW-1 fill their own inbox's missing half (rows outside
// the region: any value, the halo absorbs it).  A wave's LDS instructions execute in order, so a
// reader that reads its flags before its rows and finds both tags reads rows written before them;
// buffer reuse is safe without a barrier (a wave writes step n+1's rows only after it read its step-n inbox,
// whose writers wrote it after reading their step n-1 inboxes).  Per step and wave: 4 writes, 2 reads
// and 2 compares, no register moves on either side.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
typedef __attribute__((address_space(3))) u32x2 lds_u32x2;
typedef __attribute__((address_space(3))) float lds_float;
typedef __attribute__((address_space(3))) unsigned lds_uint;
template <int NW> struct XmBox { f32x4 rows[2][NW][64]; u32x4 flags[2][NW][64]; };   // [buffer][wave][lane]
template <int NW>
__device__ __forceinline__ void xm_init(XmBox<NW> &m, int w, int lane)
{
    const u32x4 z = {XQ_NONE, XQ_NONE, 0u, 0u};
    m.flags[0][w][lane] = z;
    m.flags[1][w][lane] = z;
}
// p0 = rows {0, R-1}, p1 = rows {1, R-2} (mirrored pairs 0, 1)
template <int NW>
__device__ __forceinline__ void xm_put(XmBox<NW> &m, int buf, int w, int lane, unsigned tag, f32x2 p0, f32x2 p1)
{
    constexpr int FLAGS = NW * 64 * 4 * 2;                // flags[buf] - rows[buf] in floats (same layout)
    lds_float *dn = (lds_float *)&m.rows[buf][w < NW - 1 ? w + 1 : w][lane] + (w < NW - 1 ? 0 : 1);
    lds_float *up = (lds_float *)&m.rows[buf][w > 0 ? w - 1 : w][lane] + (w > 0 ? 1 : 0);
    dn[0] = p0.y; dn[2] = p1.y;                           // the lower wave's rows -1, -2
    up[0] = p0.x; up[2] = p1.x;                           // the upper wave's rows R, R+1
    asm volatile("" ::: "memory");                        // rows before flags (program order = LDS order)
    ((lds_uint *)dn)[FLAGS] = tag;
    ((lds_uint *)up)[FLAGS] = tag;
}
template <int NW>
__device__ __forceinline__ void xm_load(XmBox<NW> &m, int buf, int w, int lane, u32x2 &f, f32x2 &E1, f32x2 &E2)
{
    asm volatile("" ::: "memory");
    f = *(const lds_u32x2 *)&m.flags[buf][w][lane];
    asm volatile("" ::: "memory");                        // flags before rows
    const f32x4 e = *(const lds_f32x4 *)&m.rows[buf][w][lane];
    E1 = f32x2{e.x, e.y};
    E2 = f32x2{e.z, e.w};
}
__device__ __forceinline__ bool xm_ready(u32x2 f, unsigned tag)
{
    return (__builtin_amdgcn_ballot_w64(f.x == tag) & __builtin_amdgcn_ballot_w64(f.y == tag)) == ~0ull;
}
template <int NW>
__device__ __forceinline__ void xm_wait(XmBox<NW> &m, int buf, int w, int lane, unsigned tag, u32x2 f, f32x2 &E1,
                                        f32x2 &E2, unsigned *status, bool &live)
{
    if (!xm_ready(f, tag)) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_setprio(PT_PRIO_WAIT);        // (see PT_PRIO_*)
        for (unsigned it = 1;; ++it) {
            xm_load<NW>(m, buf, w, lane, f, E1, E2);
            if (xm_ready(f, tag)) break;
            if (!live) break;
            if ((it & 255u) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > 100000000ull) {   // 1 s
                __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                live = false;
                break;
            }
        }
    }
    __builtin_amdgcn_s_setprio(PT_PRIO_EDGE);
}


// the same for two fields with ONE barrier (adjoint: A*L_{k+1} and the history P_{k-1})
__device__ __forceinline__ void exchange2(float (*xa)[TB_NW][4][64], float (*xb)[TB_NW][4][64], int buf, int w,
                                          int lane, const float (&fa)[4], const float (&fb)[4], Halo4 &ha,
                                          Halo4 &hb)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) { xa[buf][w][i][lane] = fa[i]; xb[buf][w][i][lane] = fb[i]; }
    __syncthreads();
    const int wu = w > 0 ? w - 1 : 0, wd = w < TB_NW - 1 ? w + 1 : TB_NW - 1;
    ha.u2 = xa[buf][wu][2][lane]; ha.u1 = xa[buf][wu][3][lane]; ha.d1 = xa[buf][wd][0][lane]; ha.d2 = xa[buf][wd][1][lane];
    hb.u2 = xb[buf][wu][2][lane]; hb.u1 = xb[buf][wu][3][lane]; hb.d1 = xb[buf][wd][0][lane]; hb.d2 = xb[buf][wd][1][lane];
}

// XCD-aware block -> (tile, shot) map.  Blocks are dealt round-robin over the 8 XCDs (block b
// and b+8 share an L2); every shot of one tile gets the same (block mod 8), so the per-model
// coefficient rows a tile reads are fetched once per XCD and re-read from that L2 by the other
// shots of the group.  A placement guess only changes speed, never results.
struct TileId { int tx, ty, tile, sl; bool valid; };

__host__ __device__ __forceinline__ TileId decode_tile(int L, int tiles_x, int ntiles, int nsg)
{
    TileId t;
    t.tile = (L / (8 * nsg)) * 8 + (L & 7);
    t.sl = (L >> 3) % nsg;
    t.valid = t.tile < ntiles;
    t.ty = t.tile / tiles_x;
    t.tx = t.tile - t.ty * tiles_x;
    return t;
}

// record index of time step n under sample_temporal st (-1: not a recorded step); st == 1, the
// reference default, needs no integer division
__device__ __forceinline__ int rec_index(int n, int st)
{
    if (st == 1) return n;
    return (n % st) == 0 ? n / st : -1;
}

// cheap wrap for |v| < a few n (general v handled by the loops)
__device__ __forceinline__ int wrapn(int v, int n)
{
    while (v < 0) v += n;
    while (v >= n) v -= n;
    return v;
}

// ---- Shared parts of the narrow chunked kernels (k_fwd_tb, k_adj_tb, k_born_tb, k_fwd_born_tb): the expressions
// whose fp32 order the kernels' bit-exactness rests on, written once.  The kernels' header comments name the part
// that implements each of their lines.  (The tile / row prologue, the receiver store and the ring epilogue stay in
// the kernels: as helpers they changed the compiled text of most instantiations, DESIGN.md "Narrow chunked kernels:
// shared parts".)
//
// C2 S1 + C3 S2 of row r of a field held as TB_R rows per lane, in the reference's association (pde.py:79):
// S1 / S2 = ((up + down) + left) + right over the nearest / second neighbours.  Vertical taps: the wave's own
// rows and the halo rows of the exchange; horizontal taps: DPP lane shifts.  Call it with every lane of the wave
// active: a DPP read of a lane that a divergent branch has masked off returns 0 (bound_ctrl), which would corrupt
// the tap at the tile's interior edge.  The two stars that are NOT this function, and why: k_adj_tb's gA star does
// its arithmetic inside the branch on the interior with the shifts outside it, and k_fwd_born_tb's P star, written
// through this function, comes out with commuted multiply operands in the GEN instantiations; both are written
// out where they stand, in this order.
__device__ __forceinline__ float tb_lap(const float *f, int r, const Halo4 &h)
{
    const float m2 = r >= 2 ? f[r - 2] : (r == 1 ? h.u1 : h.u2);
    const float m1 = r >= 1 ? f[r - 1] : h.u1;
    const float p1 = r + 1 < TB_R ? f[r + 1] : h.d1;
    const float p2 = r + 2 < TB_R ? f[r + 2] : (r + 2 == TB_R ? h.d1 : h.d2);
    const float c = f[r];
    const float l1 = dpp_shr1(c), r1 = dpp_shl1(c);
    const float l2 = dpp_shr1(l1), r2 = dpp_shl1(r1);
    float s1 = m1 + p1; s1 = s1 + l1; s1 = s1 + r1;
    float s2 = m2 + p2; s2 = s2 + l2; s2 = s2 + r2;
    float lap = C2 * s1; const float q = C3 * s2; lap = lap + q;
    return lap;
}

// temp1 / temp2 re-derived from alpha and kappa as gen_coef derives them (pde.py:69-70; bit-identical)
__device__ __forceinline__ void tb_t1t2(float A, float kp, float &t1, float &t2)
{
    t1 = C1X2 * A; t1 = t1 + 2.0f; t1 = t1 - kp;     // pde.py:69
    t2 = 1.0f - kp;                                  // pde.py:70
}

// SRC: the source samples are the call's own wavelets, read from a.wav (rdq_fwi_*_src) instead of the
// kernel-argument samples a.w of the plan's wavelet; b and s are workgroup-uniform, so the launch's T
// samples are uniform loads, hoisted ahead of the step loop.  Same operation order either way.
// SRC_ENC: an encoded supershot (rdq_fwi_*_enc).  Wavefield (b, e) takes every source of the plan, each with its own
// effective samples; a lane injects the sources of its own column on the source row(s), in ascending source index,
// each as add = beta * w; P = P + add.  The T samples of the lane's first source are per-lane loads hoisted like
// SRC_CALL's, in the waves that hold the source row; a column's further sources (rare: smulti, wave-uniform, like
// rmulti) are read in the step.  Every source is injected, a zero sample included.
constexpr int SRC_PLAN = 0, SRC_CALL = 1, SRC_ENC = 2;
template <int T, bool GEN, int SRC = SRC_PLAN>
__global__ __launch_bounds__(64 * TB_NW) void k_fwd_tb(FwdTBArgs a)
{
    constexpr int H = 2 * T, IW = 64 - 2 * H, IH = TB_RH - 2 * H;
    __shared__ float xch[2][TB_NW][4][64];
    const TBGeo &g = a.g;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
    const TileId ti = decode_tile(blockIdx.x, g.tiles_x, g.ntiles, g.B * g.ns_grp);
    if (!ti.valid) return;                                            // whole workgroup: uniform
    const int b = ti.sl / g.ns_grp, s = g.s_off + (ti.sl - b * g.ns_grp), bs = b * g.ns + s;
    const int ux = ti.tx * IW - H + lane;                             // unwrapped column
    const int gx = wrapn(ux, g.Wp);
    const bool xin = lane >= H && lane < 64 - H && ux < g.Wp;
    const int uz0 = ti.ty * IH - H + w * TB_R;                        // unwrapped row of r = 0
    const size_t so = (size_t)bs * g.slice;
    const float *AL = a.coeffs + (size_t)b * g.slice;
    const float *T1p = AL + g.cstride, *T2p = AL + 2 * g.cstride;
    const int isx = SRC == SRC_ENC ? gx : g.isx[s];      // ENC: every column's own cell; its sources below
    float A[TB_R], C1[TB_R], C2v[TB_R], P0[TB_R], P1[TB_R];
    int rofs[TB_R];                 // wave-uniform row offsets gz*ld
    unsigned rin = 0;               // wave-uniform: row is interior and inside the domain
    int rrow = -1;                  // wave-uniform: row holding the receivers
#pragma unroll
    for (int r = 0; r < TB_R; ++r) {
        const int uz = uz0 + r, gz = wrapn(uz, g.Hp);
        rofs[r] = gz * g.ld;
        const int o = rofs[r] + gx;
        if constexpr (GEN) {   // regenerate from the 20 KB model (L1-resident) instead of 3 fields
            const Coef cf = gen_coef(a.cg, b, gz, gx);
            A[r] = cf.al; C1[r] = cf.t1; C2v[r] = cf.t2;
        } else {
            A[r] = AL[o]; C1[r] = T1p[o]; C2v[r] = T2p[o];
        }
        P0[r] = a.in_prev[so + o];
        P1[r] = a.in_cur[so + o];
        const int rr = w * TB_R + r;
        if (rr >= H && rr < TB_RH - H && uz < g.Hp) rin |= 1u << r;
        if (gz == g.igz) rrow = r;          // (a region row maps to one grid row: one hit per wave)
    }
    // tiny domains (region taller than Hp) can hold the source row twice: keep every hit
    unsigned smask = 0;
#pragma unroll
    for (int r = 0; r < TB_R; ++r) if (wrapn(uz0 + r, g.Hp) == g.isz) smask |= 1u << r;
    int es0 = 0, es1 = 0, esrc0 = -1;   // ENC: this column's sources, src_list[es0 .. es1), and the first of them
    bool smulti = false;                // wave-uniform: a column with several sources
    const int *src_list = nullptr;
    if constexpr (SRC == SRC_ENC) {
        const int *src_start = g.isx;
        src_list = g.isx + g.Wp + 1;
        if (smask) { es0 = src_start[gx]; es1 = src_start[gx + 1]; }
        if (es0 < es1) esrc0 = src_list[es0];
        smulti = __any(es1 - es0 > 1);
    }
    (void)esrc0; (void)smulti; (void)src_list;
    const bool scol = SRC == SRC_ENC ? es0 < es1 : gx == isx;
    const float bsrc = (smask != 0) ? a.coeffs[4 * g.cstride + (size_t)b * g.slice + (size_t)g.isz * g.ld + isx] : 0.0f;
    const int rs = (rrow >= 0) ? g.rcv_start[gx] : 0, re = (rrow >= 0) ? g.rcv_start[gx + 1] : 0;
    // this lane's (usually only) receiver, read once: a per-step index load would put an L2 round
    // trip in front of every step's seismogram store
    const int rcv0 = rs < re ? g.rcv_list[rs] : -1;
    const bool rmulti = __any(re - rs > 1);               // wave-uniform: a column with several receivers
    float ws[T];                    // SRC: w[b, s, n0 .. n0 + nsteps - 1]
    const float *wpe = nullptr;     // ENC: w[b, e, 0, n0]
    if constexpr (SRC == SRC_CALL) {
        const float *wp = a.wav + (size_t)b * a.wms + (size_t)s * a.wss + a.n0;
#pragma unroll
        for (int t = 0; t < T; ++t) ws[t] = t < a.nsteps ? wp[t] : 0.0f;
    }
    if constexpr (SRC == SRC_ENC) {
        wpe = a.wav + (size_t)b * a.wms + (size_t)s * enc_stride(a.w) + a.n0;
        const float *wp = wpe + (size_t)(scol ? esrc0 : 0) * a.wss;
#pragma unroll
        for (int t = 0; t < T; ++t) ws[t] = (scol && t < a.nsteps) ? wp[t] : 0.0f;
    }
    (void)wpe;
    (void)ws;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (t >= a.nsteps) break;
        float *cur = (t & 1) ? P0 : P1;     // P_{n+t}
        float *prv = (t & 1) ? P1 : P0;     // P_{n+t-1}  -> overwritten with P_{n+t+1}
        const Halo4 h4 = exchange_nw<TB_NW>(xch, t & 1, w, lane, cur[0], cur[1], cur[TB_R - 2], cur[TB_R - 1]);
#pragma unroll
        for (int r = 0; r < TB_R; ++r) {
            const float c = cur[r];
            const float lap = tb_lap(cur, r, h4);                      // pde.py:79, reference evaluation order
            float a1 = C1[r] * c; const float a2 = C2v[r] * prv[r]; a1 = a1 - a2;
            const float a3 = A[r] * lap;
            prv[r] = a1 + a3;
        }
        if (smask) {                                                   // pde.py:80-81
#pragma unroll
            for (int r = 0; r < TB_R; ++r)
                if ((smask & (1u << r)) && scol) {
                    float wt;
                    if constexpr (SRC != SRC_PLAN) wt = ws[t]; else wt = a.w[t];
                    const float add = bsrc * wt; prv[r] = prv[r] + add;
                }
            if constexpr (SRC == SRC_ENC) {
                if (smulti)
                    for (int j = es0 + 1; j < es1; ++j) {
                        const float add = bsrc * wpe[(size_t)src_list[j] * a.wss + t];
#pragma unroll
                        for (int r = 0; r < TB_R; ++r) if (smask & (1u << r)) prv[r] = prv[r] + add;
                    }
            }
        }
        const int n = a.n0 + t;
        if (a.hist && xin) {
            float *HS = a.hist + (size_t)(n + 2 - a.hbase) * g.level + so + gx;
#pragma unroll
            for (int r = 0; r < TB_R; ++r)
                if (rin & (1u << r)) __builtin_nontemporal_store(prv[r], &HS[rofs[r]]);   // streaming
        }
        if (a.seis && rrow >= 0 && (rin & (1u << rrow)) && xin && (n % g.st) == 0) {   // pde.py:82-83 (no seis: a recompute)
            float val = 0.0f;
#pragma unroll
            for (int r = 0; r < TB_R; ++r) if (r == rrow) val = prv[r];
            float *SK = a.seis + ((size_t)bs * g.nrec + n / g.st) * g.ng;
            if (rcv0 >= 0) SK[rcv0] = val;
            if (rmulti)
                for (int j = rs + 1; j < re; ++j) SK[g.rcv_list[j]] = val;
        }
    }
    if (a.out_cur && xin) {   // ring path: keep the last two levels
        const bool odd = (a.nsteps & 1) != 0;   // after nsteps steps the newest level is in P0 if odd
#pragma unroll
        for (int r = 0; r < TB_R; ++r)
            if (rin & (1u << r)) {
                const size_t o = so + rofs[r] + gx;
                a.out_cur[o] = odd ? P0[r] : P1[r];
                a.out_prev[o] = odd ? P1[r] : P0[r];
            }
    }
}

constexpr int TW_ADJ_MAXT = 6;          // deepest wide chunked adjoint (k_adj_tw instantiations 1 .. 6)
constexpr int ADJ_W_MAX = TW_ADJ_MAXT > TB_MAXT ? TW_ADJ_MAXT : TB_MAXT;   // wavelet samples per chunked adjoint launch
struct AdjTBArgs {
    TBGeo g;
    CoefGen cg;                          // model + sponge amplitude (wide kernels regenerate alpha / kappa)
    const float *coeffs;                 // K3 fields: alpha, temp1, temp2, kappa at 0..3 x cstride
    const float *in_l1, *in_l2;          // L_{k0+1}, L_{k0+2}
    float *out_l1, *out_l2;              // L_{k0-nsteps+1}, L_{k0-nsteps+2}
    const float *hist;                   // slot k = P_{k-1}
    const float *dseis;
    float *gA;                           // [B][ns][Hp][ld]
    double *gk_part;                     // [B*ns][nblk]
    float *gbeta;                        // [B*ns]
    int k0, nsteps, nblk;
    int spw, ns_sh;                      // wide kernels: shots per workgroup, shots of the launch's chain
    float w[ADJ_W_MAX];                  // w[k0-1-t], t < nsteps (narrow: <= TB_MAXT, wide: <= TW_ADJ_MAXT steps)
    int hbase;                           // virtual slot held by hist's first level (FwdTBArgs::hbase)
    // SRC instantiations (rdq_fwi_*_src): the call's own wavelets as FwdTBArgs::wav (`w` is not read), and
    // gwav [B][ns][nt] = d(loss)/d(wav), one plain store per shot-step (nullptr: not wanted)
    const float *wav;
    long long wms, wss;
    float *gwav;
    int nt;
    // ENC instantiations (rdq_fwi_*_enc): g.isx and w[0], w[1] as in FwdTBArgs; gbeta is [B][ne][nsrc] and gwav
    // [B][ne][nsrc][nt], nsrc = the plan's source count
};

// Adjoint with the same register-region blocking, walking k = k0, k0-1, ...:
//   L_k = T1 L_{k+1} - T2 L_{k+2} + (c2 N1(A L_{k+1}) + c3 N2(A L_{k+1})) [+ R^T dseis[k-1]]
// and, on the interior only, the per-shot accumulators (loaded once, stored once per launch):
//   gA_s += L_k (2c1 P_{k-1} + c2 S1(P_{k-1}) + c3 S2(P_{k-1})),  gk += (K P_{k-1})(L_{k+1} - L_k),
//   gbeta[s] += L_k(src) w[k-1].
// N1 / N2 of A L_{k+1} are tb_lap and T1 / T2 are tb_t1t2; the P star is tb_lap's expression written out, its lane
// shifts outside the branch on the interior and its arithmetic inside.
// SRC: w is the call's own wavelet of (b, s), loaded from a.wav (uniform loads, hoisted), and the transpose
// of the source injection P_k(src) += beta(src) w[b, s, k-1] is
//   gwav[b, s, k-1] = L_k(src) beta(src):   one fp32 multiply, L_k taken after step k's receiver residual,
// stored by the lane that owns the source cell (gbl).  The tiles' interiors partition the grid, so exactly one
// lane of one workgroup owns that cell, and a call runs every k once: one writer per element, a plain store,
// no atomics and no dependence on what gwav held.
// SRC_ENC: wavefield (b, e) of an encoded call.  The lane that owns a source cell owns every source j on it:
//   gwav[b, e, j, k-1] = L_k(cell) beta(cell),   gbeta[b, e, j] += L_k(cell) w[b, e, j, k-1],
// the cell's first source through the registers above (gbacc, ws), its further ones (smulti, rare) with the sample
// read in the step and a read-modify-write of their gbeta element by this one lane, in the same order of k.  One
// owner lane per cell and every k run once: one writer per element of gwav and gbeta, as above.
template <int T, int SRC = SRC_PLAN>
__global__ __launch_bounds__(64 * TB_NW, 4) void k_adj_tb(AdjTBArgs a)
{
    constexpr int H = 2 * T, IW = 64 - 2 * H, IH = TB_RH - 2 * H;
    __shared__ float xch[2][TB_NW][4][64];
    __shared__ float pxc[2][TB_NW][4][64];
    __shared__ double red[64 * TB_NW];
    const TBGeo &g = a.g;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileId ti = decode_tile(blockIdx.x, g.tiles_x, g.ntiles, g.B * g.ns_grp);
    if (!ti.valid) return;                                            // whole workgroup: uniform
    const int b = ti.sl / g.ns_grp, s = g.s_off + (ti.sl - b * g.ns_grp), bs = b * g.ns + s;
    const int ux = ti.tx * IW - H + lane;
    const int gx = wrapn(ux, g.Wp);
    const bool xin = lane >= H && lane < 64 - H && ux < g.Wp;
    const int uz0 = ti.ty * IH - H + w * TB_R;
    const size_t so = (size_t)bs * g.slice;
    const float *AL = a.coeffs + (size_t)b * g.slice;
    const float *KAp = AL + 3 * g.cstride;
    const int isx = SRC == SRC_ENC ? gx : g.isx[s];      // ENC: every column's own cell; its sources below
    float A[TB_R], L0[TB_R], L1[TB_R];   // temp1/temp2 are re-derived from A and K (tb_t1t2)
    float gal[TB_R], kal[TB_R];          // gA_s accumulators and the sponge coefficient K, in registers
    int rofs[TB_R];
    unsigned rin = 0, pmask = 0, smask = 0, rmask = 0;   // wave-uniform row masks
#pragma unroll
    for (int r = 0; r < TB_R; ++r) {
        const int uz = uz0 + r, gz = wrapn(uz, g.Hp);
        rofs[r] = gz * g.ld;
        const int o = rofs[r] + gx;
        A[r] = AL[o];                // (regenerating alpha / K from the model, as the forward does,
        kal[r] = KAp[o];             //  measured 5% slower here: the loads are cheaper than the math)
        L1[r] = a.in_l1[so + o];     // L_{k+1}
        L0[r] = a.in_l2[so + o];     // L_{k+2}
        const int rr = w * TB_R + r;
        if (rr >= H && rr < TB_RH - H && uz < g.Hp) rin |= 1u << r;
        if (rr >= H - 2 && rr < TB_RH - H + 2) pmask |= 1u << r;
        if (gz == g.isz) smask |= 1u << r;
        if (gz == g.igz) rmask |= 1u << r;
        gal[r] = ((rin & (1u << r)) && xin) ? a.gA[so + o] : 0.0f;
    }
    // ENC: this column's sources are src_list[es0 .. es1); kept past this prologue are only the first one's index
    // and its slot in gbeta / gwav, (b, e, source) (the rare further sources are looked up again where they are used:
    // the depth-4 kernel has no register to spare at 4 workgroups per CU)
    int es0 = 0, es1 = 0, esrc0 = 0, gslot = 0;
    bool smulti = false;                // wave-uniform: a column with several sources
    if constexpr (SRC == SRC_ENC) {
        const int *src_start = g.isx, *src_list = g.isx + g.Wp + 1;
        if (smask & rin) { es0 = src_start[gx]; es1 = src_start[gx + 1]; }
        if (es0 < es1) { esrc0 = src_list[es0]; gslot = bs * src_start[g.Wp] + esrc0; }
        smulti = __any(es1 - es0 > 1);
    }
    (void)smulti; (void)gslot;
    const bool scol = SRC == SRC_ENC ? es0 < es1 : gx == isx;
    // residual of this lane's column: one receiver's dseis, or several receivers' folded sum
    const int rcv0 = rmask ? g.rlane[gx] : -1;
    const float *DSb = a.dseis + (size_t)bs * g.nrec * g.dstride;
    // gbeta of this shot accumulates in a register over the launch's steps (same order as a
    // per-step read-modify-write of a.gbeta[bs]), stored once at the end
    const bool gbl = (smask & rin) && scol && xin;       // the source cell is this lane's own cell
    // (ENC: this lane's element is its first source's of wavefield (b, e))
    float gbacc;
    if constexpr (SRC == SRC_ENC) gbacc = gbl ? a.gbeta[gslot] : 0.0f;
    else gbacc = gbl ? a.gbeta[bs] : 0.0f;
    float ws[T];                    // SRC: w[b, s, k0 - 1 - t]
    float bsrc = 0.0f;              // SRC: beta at the source cell, on the lane that owns it and stores gwav
    bool gw = false;
    if constexpr (SRC == SRC_CALL) {
        const float *wp = a.wav + (size_t)b * a.wms + (size_t)s * a.wss + a.k0 - 1;
#pragma unroll
        for (int t = 0; t < T; ++t) ws[t] = t < a.nsteps ? wp[-t] : 0.0f;
        gw = gbl && a.gwav;
        if (gw) bsrc = a.coeffs[4 * g.cstride + (size_t)b * g.slice + (size_t)g.isz * g.ld + isx];
    }
    if constexpr (SRC == SRC_ENC) {
        const float *wp = a.wav + (size_t)b * a.wms + (size_t)s * enc_stride(a.w) + (size_t)esrc0 * a.wss + a.k0 - 1;
#pragma unroll
        for (int t = 0; t < T; ++t) ws[t] = (gbl && t < a.nsteps) ? wp[-t] : 0.0f;
        gw = gbl && a.gwav;
        if (gw) bsrc = a.coeffs[4 * g.cstride + (size_t)b * g.slice + (size_t)g.isz * g.ld + isx];
    }
    (void)ws; (void)bsrc; (void)gw; (void)esrc0;
    double ksum = 0.0;
    // history P_{k-1} on the rows whose stencil the interior needs: HBM stream, prefetched one
    // step ahead so its latency hides under the previous step
    // Buffer loads with an out-of-range offset outside pmask (no memory access, returns 0): no
    // select on the loaded value, so the compiler need not wait for each load in turn.
    float Pn[TB_R];
    int pofs[TB_R];
#pragma unroll
    for (int r = 0; r < TB_R; ++r) pofs[r] = (pmask & (1u << r)) ? (rofs[r] + gx) * 4 : OOB;
    const int slice_bytes = (int)(g.slice * 4);
    {
        const __amdgpu_buffer_rsrc_t HR = rsrc_of(a.hist + (size_t)(a.k0 - a.hbase) * g.level + so, slice_bytes);
#pragma unroll
        for (int r = 0; r < TB_R; ++r) Pn[r] = bload(HR, pofs[r], 0);   // (not nt: vertically adjacent
    }                                                                          //  tiles re-read halo rows from L2)
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (t >= a.nsteps) break;
        const int k = a.k0 - t;
        float *cur = (t & 1) ? L0 : L1;     // L_{k+1}
        float *prv = (t & 1) ? L1 : L0;     // L_{k+2} -> overwritten with L_k
        float P[TB_R];
#pragma unroll
        for (int r = 0; r < TB_R; ++r) P[r] = Pn[r];
        if (t + 1 < a.nsteps) {
            const __amdgpu_buffer_rsrc_t HR = rsrc_of(a.hist + (size_t)(k - 1 - a.hbase) * g.level + so, slice_bytes);
#pragma unroll
            for (int r = 0; r < TB_R; ++r) Pn[r] = bload(HR, pofs[r], 0);
        }
        // this step's receiver residual, loaded before the stencil so its latency hides under it
        const bool rstep = rmask && ((k - 1) % g.st) == 0;   // wave-uniform
        const float dsv = (rstep && rcv0 >= 0) ? DSb[(size_t)((k - 1) / g.st) * g.dstride + rcv0] : -0.0f;
        float q[TB_R];
#pragma unroll
        for (int r = 0; r < TB_R; ++r) q[r] = A[r] * cur[r];
        Halo4 h4, hp;
        const float qe[4] = {q[0], q[1], q[TB_R - 2], q[TB_R - 1]};
        const float pe[4] = {P[0], P[1], P[TB_R - 2], P[TB_R - 1]};
        exchange2(xch, pxc, t & 1, w, lane, qe, pe, h4, hp);
#pragma unroll
        for (int r = 0; r < TB_R; ++r) {
            const float nb = tb_lap(q, r, h4);
            float t1, t2;
            tb_t1t2(A[r], kal[r], t1, t2);
            float l = t1 * cur[r]; const float l2 = t2 * prv[r]; l = l - l2; l = l + nb;
            prv[r] = l;
        }
        if (rstep) {                            // adjoint of the receiver sampling
#pragma unroll
            for (int r = 0; r < TB_R; ++r)
                if (rmask & (1u << r)) prv[r] = prv[r] + dsv;     // -0 on lanes without a receiver
        }
        // gradient accumulators on the interior (P halo rows came with the same exchange)
#pragma unroll
        for (int r = 0; r < TB_R; ++r) {
            // tb_lap's star of P, written out: the DPP shifts here, with every lane active, the arithmetic inside the branch
            const float pm2 = r >= 2 ? P[r - 2] : (r == 1 ? hp.u1 : hp.u2), pm1 = r >= 1 ? P[r - 1] : hp.u1;
            const float pp1 = r + 1 < TB_R ? P[r + 1] : hp.d1, pp2 = r + 2 < TB_R ? P[r + 2] : (r + 2 == TB_R ? hp.d1 : hp.d2);
            const float pc = P[r];
            const float xl1 = dpp_shr1(pc), xr1 = dpp_shl1(pc);
            const float xl2 = dpp_shr1(xl1), xr2 = dpp_shl1(xr1);
            if ((rin & (1u << r)) && xin) {
                float s1 = pm1 + pp1; s1 = s1 + xl1; s1 = s1 + xr1;
                float s2 = pm2 + pp2; s2 = s2 + xl2; s2 = s2 + xr2;
                float lap = C2 * s1; const float lq = C3 * s2; lap = lap + lq;
                float d = C1X2 * pc; d = d + lap;
                const float l = prv[r];
                const float c = l * d;
                float &ga = gal[r];
                ga = ga + c;
                float kk = kal[r] * pc; const float dl = cur[r] - l; kk = kk * dl;  // fp32 term,
                ksum += (double)kk;                                                             // fp64 sum
                if ((smask & (1u << r)) && scol) {
                    float wt;
                    if constexpr (SRC != SRC_PLAN) wt = ws[t]; else wt = a.w[t];
                    const float gb = l * wt; gbacc = gbacc + gb;
                }
            }
        }
        if constexpr (SRC == SRC_CALL) {   // one store per step, not one per row: the source row's L_k picked by the wave-uniform mask
            if (gw) {
                float ls = 0.0f;
#pragma unroll
                for (int r = 0; r < TB_R; ++r) if (smask & rin & (1u << r)) ls = prv[r];
                a.gwav[(size_t)bs * a.nt + (k - 1)] = ls * bsrc;
            }
        }
        if constexpr (SRC == SRC_ENC) {    // the same store for the cell's first source, then its further sources
            if (gw || (smulti && gbl)) {
                float ls = 0.0f;
#pragma unroll
                for (int r = 0; r < TB_R; ++r) if (smask & rin & (1u << r)) ls = prv[r];
                const float gwv = ls * bsrc;
                if (gw) a.gwav[(size_t)gslot * a.nt + (k - 1)] = gwv;
                if (smulti && gbl) {
                    const int *src_start = g.isx, *src_list = g.isx + g.Wp + 1;
                    const float *wk = a.wav + (size_t)b * a.wms + (size_t)s * enc_stride(a.w) + (k - 1);
                    const int slot0 = bs * src_start[g.Wp];
                    for (int j = src_start[gx] + 1; j < src_start[gx + 1]; ++j) {
                        const int sj = src_list[j];
                        const float gb = ls * wk[(size_t)sj * a.wss];
                        float *gbj = a.gbeta + (slot0 + sj);
                        *gbj = *gbj + gb;
                        if (gw) a.gwav[(size_t)(slot0 + sj) * a.nt + (k - 1)] = gwv;
                    }
                }
            }
        }
    }
    if (xin) {
        const bool odd = (a.nsteps & 1) != 0;   // newest level (L_{k0-nsteps+1}) is in L0 if odd
#pragma unroll
        for (int r = 0; r < TB_R; ++r)
            if (rin & (1u << r)) {
                const size_t o = so + rofs[r] + gx;
                a.out_l1[o] = odd ? L0[r] : L1[r];
                a.out_l2[o] = odd ? L1[r] : L0[r];
                a.gA[o] = gal[r];
            }
    }
    if constexpr (SRC == SRC_ENC) { if (gbl) a.gbeta[gslot] = gbacc; }
    else if (gbl) a.gbeta[bs] = gbacc;
    // deterministic workgroup reduction of the sponge-coefficient partial sum
    const int tid = threadIdx.x;
    red[tid] = ksum;
    __syncthreads();
    for (int w2 = 32 * TB_NW; w2 > 0; w2 >>= 1) {
        if (tid < w2) red[tid] += red[tid + w2];
        __syncthreads();
    }
    if (tid == 0) a.gk_part[(size_t)bs * a.nblk + ti.tile] += red[0];
}

// --------------------------------------------------------------------------------------- Illumination
// Source illumination / pseudo-Hessian diagonal (rdq_fwi_illum, include/red_diffeq_fwi.h): per wavefield and padded
// cell,
//   hA = sum_{k = first, first - 1, ...} q_k^2,   q_k = 2c1 P_{k-1} + (c2 S1(P_{k-1}) + c3 S2(P_{k-1})),
// q_k the factor k_adj_tb multiplies L_k by for gA (tb_lap's star of P, then d = C1X2 P; d = d + lap), every
// operation a separate fp32 rounding: t = q q; acc = acc + t, k descending.  The term of step k needs level k of
// the history only, so the pass is a stream over the levels with no temporal blocking: the depth-1 region of the
// narrow kernels (64 columns x 8 waves x 8 rows, halo 2, interior 60 x 60, tiles_x / tiles_y at T = 1), the
// vertical taps through the LDS exchange (one barrier per level) and the horizontal ones through DPP, as
// k_fwd_tb.  The loads of IL_DEPTH levels are in flight per wave (a register ring, indexed statically by the
// unrolled loop); a level past the launch's last gets a zero-length buffer descriptor (no memory access, zeros),
// so no load sits behind a branch.  The column of a lane is wrapped into [0, Wp): the history's pitch columns are
// never read, and hA is read and written on the tile's interior only (columns < Wp).  `init`: the call's first
// launch on these wavefields starts from zero instead of reading hA, so the result does not depend on what hA held.
constexpr int IL_DEPTH = 4;              // levels of history loads in flight per wave
__device__ __forceinline__ float bload_nt(__amdgpu_buffer_rsrc_t r, int voff, int soff);   // (with the persistent adjoint)
struct IllumTBArgs {
    TBGeo g;
    const float *hist;                   // slot k = P_{k-1}
    float *hA;                           // [B][nwf][Hp][ld]
    int first, nsteps;                   // steps first, first - 1, ... (nsteps of them)
    int hbase;                           // virtual slot held by hist's first level (FwdTBArgs::hbase)
    int init;                            // 1: start from zero, 0: continue from hA
};

__global__ __launch_bounds__(64 * TB_NW) void k_illum_tb(IllumTBArgs a)
{
    constexpr int H = 2, IW = 64 - 2 * H, IH = TB_RH - 2 * H;
    __shared__ float xch[2][TB_NW][4][64];
    const TBGeo &g = a.g;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileId ti = decode_tile(blockIdx.x, g.tiles_x, g.ntiles, g.B * g.ns_grp);
    if (!ti.valid) return;                                            // whole workgroup: uniform
    const int b = ti.sl / g.ns_grp, s = g.s_off + (ti.sl - b * g.ns_grp), bs = b * g.ns + s;
    const int ux = ti.tx * IW - H + lane;
    const int gx = wrapn(ux, g.Wp);
    const bool xin = lane >= H && lane < 64 - H && ux < g.Wp;
    const int uz0 = ti.ty * IH - H + w * TB_R;
    const size_t so = (size_t)bs * g.slice;
    float acc[TB_R];
    int pofs[TB_R];
    unsigned rin = 0;                    // wave-uniform mask of the interior rows
#pragma unroll
    for (int r = 0; r < TB_R; ++r) {
        const int uz = uz0 + r, gz = wrapn(uz, g.Hp);
        const int rr = w * TB_R + r;
        pofs[r] = (gz * g.ld + gx) * 4;
        if (rr >= H && rr < TB_RH - H && uz < g.Hp) rin |= 1u << r;
        acc[r] = (!a.init && (rin & (1u << r)) && xin) ? a.hA[so + (size_t)gz * g.ld + gx] : 0.0f;
    }
    const int slice_bytes = (int)(g.slice * 4);
    // level of step k: slot k (P_{k-1}); t >= nsteps: a zero-length descriptor
    auto level_of = [&](int t) {
        const int tc = t < a.nsteps ? t : 0;
        return rsrc_of(a.hist + (size_t)(a.first - tc - a.hbase) * g.level + so, t < a.nsteps ? slice_bytes : 0);
    };
    float Pq[IL_DEPTH][TB_R];
#pragma unroll
    for (int u = 0; u < IL_DEPTH; ++u) {
        const __amdgpu_buffer_rsrc_t HR = level_of(u);
#pragma unroll
        for (int r = 0; r < TB_R; ++r) Pq[u][r] = bload_nt(HR, pofs[r], 0);
    }
    for (int t0 = 0; t0 < a.nsteps; t0 += IL_DEPTH) {
#pragma unroll
        for (int u = 0; u < IL_DEPTH; ++u) {
            const int t = t0 + u;
            if (t >= a.nsteps) break;                                 // uniform
            float P[TB_R];
#pragma unroll
            for (int r = 0; r < TB_R; ++r) P[r] = Pq[u][r];
            {
                const __amdgpu_buffer_rsrc_t HR = level_of(t + IL_DEPTH);
#pragma unroll
                for (int r = 0; r < TB_R; ++r) Pq[u][r] = bload_nt(HR, pofs[r], 0);
            }
            const Halo4 h4 = exchange_nw<TB_NW>(xch, t & 1, w, lane, P[0], P[1], P[TB_R - 2], P[TB_R - 1]);
#pragma unroll
            for (int r = 0; r < TB_R; ++r) {
                const float lap = tb_lap(P, r, h4);                   // every lane active (DPP)
                float d = C1X2 * P[r]; d = d + lap;
                const float q2 = d * d;
                acc[r] = acc[r] + q2;                                 // (halo cells too: never stored)
            }
        }
    }
    if (xin) {
#pragma unroll
        for (int r = 0; r < TB_R; ++r)
            if (rin & (1u << r)) a.hA[so + (size_t)(pofs[r] >> 2)] = acc[r];
    }
}

// --------------------------------------------------------------------------------------- Born
// Linearised forward J dv (rdq_fwi_born).  The tangent of the time step in the direction dv,
//   dP_{n+1} = T1 dP_n - T2 dP_{n-1} + A Lap(dP_n) + dA (2c1 P_n + Lap(P_n)) - dK (P_n - P_{n-1}) + dbeta_src w[n],
// dP_0 = dP_{-1} = 0, recorded at the receivers where the forward records.  The two bracketed terms are the ones
// whose transposes k_adj_tb accumulates into gA and gk_part.
//
// Scale.  J is linear, so each model's direction is brought to a fixed magnitude by a power of two before anything
// is derived from it, dvs = dv 2^-k with max |dvs| in [2^-64, 2^-63), and the record is multiplied by 2^k where it
// is stored.  The time loop then runs on the same bits whatever the magnitude of dv (no direction is too small to
// linearise, none overflows), and for max |dv| >= 2^-64 the rescale is an up-scale, which is exact: J (2^j dv) =
// 2^j J dv bit for bit.  (Without it the equality breaks wherever the tangent field is near the underflow
// threshold: measured at the 88 x 118 test grid, 1575 of 23040 recorded values, all below 1e-13 of the record's
// peak.)  2^-64 leaves the loop 85 binades between a unit response and the smallest denormal; fp32 resolves 24.
// The fixed magnitude holds for 2^-126 <= max |dv| < 2^63.  k = floor(log2 max |dv|) + 64 is kept within [-63, 126],
// where 2^k and 2^-k are normal floats (dcoef_exp): for max |dv| >= 2^63 the scale stays at 2^-126 and max |dvs| grows
// with the direction (2 at the largest float: an exact rescale still, far from overflow); for a max |dv| below the
// smallest normal float (biased exponent 0: denormals, or a zero direction) the scale is 2^63 and max |dvs| < 2^-63.
//
// Perturbation workspace (rdq_fwi_born_sizes; written by the prologue, k_dmax + k_dcoeffs):
//   dam    [B][nz][nx]  dA per model cell, (2 (v dt / dx)) ((dvs dt) / dx) with dvs in m/s (x1500 of a normalised
//                       one): a padded cell's dA is that of the model cell its clamped index names (the replicate
//                       pad), so the divisions are done once per model cell here, not per padded cell, shot and launch
//   ratio  [B]          dvs[argmin] / vmin: the sponge is linear in vmin and torch.min passes the tangent of the
//                       first row-major argmin only, the cell K3 leaves in vstat
//   dbeta  [B][ns]      2 (v dt)(dvs dt) at each source cell
//   oscale [B]          2^k, the record's rescale
//   dmax   [B]          bits of max |dv| over the model (uint32, zeroed, then atomic max: order-free)
struct DCoefArgs {
    const float *dv;                     // the caller's direction, element strides s0 / s2 / s3 (as k_coeffs reads v)
    int64_t s0, s2, s3;
    int vel_mode, B, nz, nx, ns, nbc, isz, ld;
    float dt, dx;
    size_t slice, cstride;
    const float *coeffs;                 // K3 fields (v at 5 x cstride)
    const float *vmod;                   // K3's model copy [B][nz][nx] (m/s)
    const float *vmin;
    const int64_t *amin;
    const int *isx;
    float *dam, *ratio, *dbeta, *oscale;
    unsigned *dmax;
};

// max |dv| of each model, as the bits of a non-negative float (they order as the values do); grid (parts, B)
__global__ __launch_bounds__(256) void k_dmax(DCoefArgs p)
{
    const int b = blockIdx.y, n = p.nz * p.nx;
    unsigned m = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int iz = i / p.nx, ix = i - iz * p.nx;
        m = max(m, __float_as_uint(p.dv[b * p.s0 + iz * p.s2 + ix * p.s3]) & 0x7fffffffu);
    }
    __shared__ unsigned sm[256];
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) sm[threadIdx.x] = max(sm[threadIdx.x], sm[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(&p.dmax[b], sm[0]);
}

// biased exponent of max |dv|, kept where both powers of two below are normal floats: 0 (max |dv| denormal or zero)
// gives the scale 2^63, 189 and above (max |dv| >= 2^63) the scale 2^-126
__device__ __forceinline__ unsigned dcoef_exp(const DCoefArgs &p, int b) { return min(p.dmax[b] >> 23, 189u); }

__device__ __forceinline__ float dcoef_dv(const DCoefArgs &p, int b, int iz, int ix)
{
    float d = p.dv[b * p.s0 + iz * p.s2 + ix * p.s3];
    d = d * __uint_as_float((190u - dcoef_exp(p, b)) << 23);   // 2^-k: max |d| into [2^-64, 2^-63), exact
    if (p.vel_mode == 0) d = d * 1500.0f;          // tangent of data_trans.py:15: ((v + 1) / 2) * 3000 + 1500
    return d;
}

__global__ __launch_bounds__(256) void k_dcoeffs(DCoefArgs p)
{
    const int n = p.nz * p.nx, nm = p.B * n;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nm) {
        const int b = i / n, c = i - b * n, iz = c / p.nx, ix = c - iz * p.nx;
        float x = p.vmod[i] * p.dt; x = x / p.dx; x = 2.0f * x;         // tangent of pde.py:63, (v dt / dx)^2
        float d = dcoef_dv(p, b, iz, ix) * p.dt; d = d / p.dx;
        p.dam[i] = x * d;
    } else if (i < nm + p.B) {
        const int b = i - nm;
        const int c = (int)p.amin[b], iz = c / p.nx, ix = c - iz * p.nx;
        p.ratio[b] = dcoef_dv(p, b, iz, ix) / p.vmin[b];
        p.oscale[b] = __uint_as_float((dcoef_exp(p, b) + 64u) << 23);   // 2^k
    } else if (i < nm + p.B + p.B * p.ns) {
        const int j = i - nm - p.B, b = j / p.ns, s = j - b * p.ns;
        const int iz = min(max(p.isz - p.nbc, 0), p.nz - 1), ix = min(max(p.isx[s] - p.nbc, 0), p.nx - 1);
        const float v = p.coeffs[5 * p.cstride + (size_t)b * p.slice + (size_t)p.isz * p.ld + p.isx[s]];
        float bt = v * p.dt; bt = 2.0f * bt;                            // tangent of pde.py:71, (v dt)^2
        const float dbt = dcoef_dv(p, b, iz, ix) * p.dt;
        p.dbeta[j] = bt * dbt;
    }
}

struct BornTBArgs {
    TBGeo g;
    CoefGen cg;                          // model + sponge amplitude (GEN variant)
    const float *coeffs;                 // K3 fields: alpha, kappa at 0, 3 x cstride
    const float *in_prev, *in_cur;       // dP_{n-1}, dP_n
    float *out_prev, *out_cur;           // dP_{n+T-1}, dP_{n+T}
    const float *hist;                   // the forward's store-all history, slot j = P_{j-1}
    const float *dam, *ratio, *dbeta, *oscale;   // perturbation workspace (above)
    float *dseis;
    int n0, nsteps;
    float w[TB_MAXT];                    // wavelet samples w[n0 .. n0+nsteps-1]
};

// The narrow chunked layout of k_fwd_tb / k_adj_tb: 64 columns x 8 waves x 8 rows in registers, halo 2T.  dP is
// carried as the forward carries P (two levels in, two out, through the ring); P_n streams from the history as in
// k_adj_tb: buffer loads, prefetched one step ahead, out-of-range offsets on the rows no live cell reads (at
// step t of a launch the live cells are the region less 2 (t + 1) on every side, their P taps less 2 t), halo rows
// through the second LDS exchange.  The level before, P_{n-1}, is the previous step's registers.  dA is read once
// per launch from the dam cell gen_coef's clamped index names (the replicate pad), dK = K ratio per use.
//
// Operation order (contraction off), per cell and step; S1 / S2 = the four nearest / second neighbours summed as
// ((up + down) + left) + right:
//   lap  = C2 S1(dP_n) + C3 S2(dP_n)                                    tb_lap
//   hom  = (T1 dP_n - T2 dP_{n-1}) + A lap                              the forward's own order; T1, T2: tb_t1t2
//   d    = 2c1 P_n + (C2 S1(P_n) + C3 S2(P_n))                          k_adj_tb's gA factor (tb_lap)
//   f    = dA d - (K ratio)(P_n - P_{n-1})
//   dP_{n+1} = hom + f, then + dbeta w[n] at the source cell
// with dA from the prologue; a recorded value is stored as dP 2^k (the scale above).
template <int T, bool GEN>
__global__ __launch_bounds__(64 * TB_NW) void k_born_tb(BornTBArgs a)
{
    constexpr int H = 2 * T, IW = 64 - 2 * H, IH = TB_RH - 2 * H;
    __shared__ float xch[2][TB_NW][4][64];
    __shared__ float pxc[2][TB_NW][4][64];
    const TBGeo &g = a.g;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
    const TileId ti = decode_tile(blockIdx.x, g.tiles_x, g.ntiles, g.B * g.ns_grp);
    if (!ti.valid) return;                                            // whole workgroup: uniform
    const int b = ti.sl / g.ns_grp, s = g.s_off + (ti.sl - b * g.ns_grp), bs = b * g.ns + s;
    const int ux = ti.tx * IW - H + lane;
    const int gx = wrapn(ux, g.Wp);
    const bool xin = lane >= H && lane < 64 - H && ux < g.Wp;
    const int uz0 = ti.ty * IH - H + w * TB_R;
    const size_t so = (size_t)bs * g.slice;
    const float *AL = a.coeffs + (size_t)b * g.slice;
    const float *KAp = AL + 3 * g.cstride;
    const int isx = g.isx[s];
    const float ratio = a.ratio[b], oscale = a.oscale[b];
    float A[TB_R], K[TB_R], dA[TB_R], D0[TB_R], D1[TB_R];
    float Q[3][TB_R];               // history levels in rotation: step t reads P_{n-1} = Q[t % 3], P_n = Q[(t + 1) % 3]
    int rofs[TB_R], pofs[TB_R];
    unsigned rin = 0, smask = 0;    // wave-uniform row masks: interior and inside the domain; the source row
    int rrow = -1;                  // wave-uniform: row holding the receivers
#pragma unroll
    for (int r = 0; r < TB_R; ++r) {
        const int uz = uz0 + r, gz = wrapn(uz, g.Hp);
        rofs[r] = gz * g.ld;
        const int o = rofs[r] + gx;
        pofs[r] = o * 4;
        if constexpr (GEN) {
            const Coef cf = gen_coef(a.cg, b, gz, gx);
            A[r] = cf.al; K[r] = cf.kp;
        } else {
            A[r] = AL[o]; K[r] = KAp[o];
        }
        const int iz = min(max(gz - a.cg.nbc, 0), a.cg.nz - 1), ix = min(max(gx - a.cg.nbc, 0), a.cg.nx - 1);
        dA[r] = a.dam[((size_t)b * a.cg.nz + iz) * a.cg.nx + ix];
        D0[r] = a.in_prev[so + o];
        D1[r] = a.in_cur[so + o];
        const int rr = w * TB_R + r;
        if (rr >= H && rr < TB_RH - H && uz < g.Hp) rin |= 1u << r;
        if (gz == g.isz) smask |= 1u << r;      // a region taller than a tiny domain holds the row more than once
        if (gz == g.igz) rrow = r;
    }
    const bool scol = gx == isx;
    const float dbsrc = smask ? a.dbeta[bs] : 0.0f;
    const int rs = (rrow >= 0) ? g.rcv_start[gx] : 0, re = (rrow >= 0) ? g.rcv_start[gx + 1] : 0;
    const int rcv0 = rs < re ? g.rcv_list[rs] : -1;
    const bool rmulti = __any(re - rs > 1);               // wave-uniform: a column with several receivers
    const int slice_bytes = (int)(g.slice * 4);
    {   // slots n0, n0 + 1 = P_{n0-1}, P_{n0}: every row (step 0's taps reach the region's edge)
        const __amdgpu_buffer_rsrc_t H0 = rsrc_of(a.hist + (size_t)a.n0 * g.level + so, slice_bytes);
        const __amdgpu_buffer_rsrc_t H1 = rsrc_of(a.hist + (size_t)(a.n0 + 1) * g.level + so, slice_bytes);
#pragma unroll
        for (int r = 0; r < TB_R; ++r) { Q[0][r] = bload(H0, pofs[r], 0); Q[1][r] = bload(H1, pofs[r], 0); }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (t >= a.nsteps) break;
        const int n = a.n0 + t;
        float *cur = (t & 1) ? D0 : D1;     // dP_n
        float *prv = (t & 1) ? D1 : D0;     // dP_{n-1} -> overwritten with dP_{n+1}
        const float *Pp = Q[t % 3], *P = Q[(t + 1) % 3];
        float *Pn = Q[(t + 2) % 3];
        if (t + 1 < a.nsteps) {             // P_{n+1} on the rows step t + 1's taps read
            const __amdgpu_buffer_rsrc_t HR = rsrc_of(a.hist + (size_t)(n + 2) * g.level + so, slice_bytes);
#pragma unroll
            for (int r = 0; r < TB_R; ++r) {
                const int rr = w * TB_R + r;
                Pn[r] = bload(HR, (rr >= 2 * (t + 1) && rr < TB_RH - 2 * (t + 1)) ? pofs[r] : OOB, 0);
            }
        }
        Halo4 hd, hp;
        const float de[4] = {cur[0], cur[1], cur[TB_R - 2], cur[TB_R - 1]};
        const float pe[4] = {P[0], P[1], P[TB_R - 2], P[TB_R - 1]};
        exchange2(xch, pxc, t & 1, w, lane, de, pe, hd, hp);
#pragma unroll
        for (int r = 0; r < TB_R; ++r) {
            const float c = cur[r], kp = K[r];
            const float lap = tb_lap(cur, r, hd);
            float t1, t2;
            tb_t1t2(A[r], kp, t1, t2);
            float hom = t1 * c; const float a2 = t2 * prv[r]; hom = hom - a2;
            const float a3 = A[r] * lap; hom = hom + a3;
            const float pc = P[r];
            const float plap = tb_lap(P, r, hp);
            float d = C1X2 * pc; d = d + plap;
            float f = dA[r] * d;
            const float dk = kp * ratio, dp = pc - Pp[r];
            const float fk = dk * dp; f = f - fk;
            prv[r] = hom + f;
        }
        if (smask) {
#pragma unroll
            for (int r = 0; r < TB_R; ++r)
                if ((smask & (1u << r)) && scol) { const float add = dbsrc * a.w[t]; prv[r] = prv[r] + add; }
        }
        if (rrow >= 0 && (rin & (1u << rrow)) && xin && (n % g.st) == 0) {   // pde.py:82-83
            float val = 0.0f;
#pragma unroll
            for (int r = 0; r < TB_R; ++r) if (r == rrow) val = prv[r];
            val = val * oscale;
            float *SK = a.dseis + ((size_t)bs * g.nrec + n / g.st) * g.ng;
            if (rcv0 >= 0) SK[rcv0] = val;
            if (rmulti)
                for (int j = rs + 1; j < re; ++j) SK[g.rcv_list[j]] = val;
        }
    }
    if (xin) {
        const bool odd = (a.nsteps & 1) != 0;   // after nsteps steps the newest level is in D0 if odd
#pragma unroll
        for (int r = 0; r < TB_R; ++r)
            if (rin & (1u << r)) {
                const size_t o = so + rofs[r] + gx;
                a.out_cur[o] = odd ? D0[r] : D1[r];
                a.out_prev[o] = odd ? D1[r] : D0[r];
            }
    }
}

struct FwdBornTBArgs {
    TBGeo g;
    CoefGen cg;                          // model + sponge amplitude (GEN variant)
    const float *coeffs;                 // K3 fields: alpha, kappa, beta at 0, 3, 4 x cstride
    const float *p_in_prev, *p_in_cur;   // P_{n-1}, P_n       (ring levels 0-3, or a checkpoint pair)
    float *p_out_prev, *p_out_cur;       // P_{n+T-1}, P_{n+T} (ring levels 0-3, or a checkpoint pair)
    const float *in_prev, *in_cur;       // dP_{n-1}, dP_n     (ring levels 4-7)
    float *out_prev, *out_cur;           // dP_{n+T-1}, dP_{n+T}
    const float *dam, *ratio, *dbeta, *oscale;   // perturbation workspace (above)
    float *seis, *dseis;
    int n0, nsteps;
    float w[TB_MAXT];                    // wavelet samples w[n0 .. n0+nsteps-1]
};

// The forward and its tangent in one time loop: k_born_tb with the P levels computed instead of loaded.  The
// tangent step reads P_n and P_{n-1} only, and the forward step of the same region produces exactly those on
// exactly the cells the tangent's taps read: at step t of a launch P_{n+t} is exact on the region less 2 t on
// every side (k_fwd_tb's halo), dP_{n+t+1} is live on the region less 2 (t + 1) and its P taps reach the region
// less 2 t.  So two P levels are carried in registers beside the two dP levels, P_{n-1}[r] is overwritten with
// P_{n+1}[r] once the tangent has read it, and no history is read or written.
//
// Operation order (contraction off).  d's stencil term and the forward's lap are the same expression of P_n in
// the same association, so it is evaluated once:
//   plap = C2 S1(P_n) + C3 S2(P_n)                                      tb_lap's expression, written out
//   dP_{n+1} as in k_born_tb (lap, hom, d = 2c1 P_n + plap, f, then + dbeta w[n] at the source cell)
//   P_{n+1}  = (T1 P_n - T2 P_{n-1}) + A plap, then + beta w[n] at the source cell    (k_fwd_tb's order)
// with T1 / T2 re-derived from A and K as gen_coef derives them (tb_t1t2, as k_adj_tb and k_born_tb).  The forward's bits are
// therefore the stored history's bits: dseis is bit-identical to rdq_fwi_born's and seis to rdq_fwi_forward's.
template <int T, bool GEN>
__global__ __launch_bounds__(64 * TB_NW) void k_fwd_born_tb(FwdBornTBArgs a)
{
    constexpr int H = 2 * T, IW = 64 - 2 * H, IH = TB_RH - 2 * H;
    __shared__ float xch[2][TB_NW][4][64];
    __shared__ float pxc[2][TB_NW][4][64];
    const TBGeo &g = a.g;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
    const TileId ti = decode_tile(blockIdx.x, g.tiles_x, g.ntiles, g.B * g.ns_grp);
    if (!ti.valid) return;                                            // whole workgroup: uniform
    const int b = ti.sl / g.ns_grp, s = g.s_off + (ti.sl - b * g.ns_grp), bs = b * g.ns + s;
    const int ux = ti.tx * IW - H + lane;
    const int gx = wrapn(ux, g.Wp);
    const bool xin = lane >= H && lane < 64 - H && ux < g.Wp;
    const int uz0 = ti.ty * IH - H + w * TB_R;
    const size_t so = (size_t)bs * g.slice;
    const float *AL = a.coeffs + (size_t)b * g.slice;
    const float *KAp = AL + 3 * g.cstride;
    const int isx = g.isx[s];
    const float ratio = a.ratio[b], oscale = a.oscale[b];
    float A[TB_R], K[TB_R], dA[TB_R], D0[TB_R], D1[TB_R], P0[TB_R], P1[TB_R];
    int rofs[TB_R];
    unsigned rin = 0, smask = 0;    // wave-uniform row masks: interior and inside the domain; the source row
    int rrow = -1;                  // wave-uniform: row holding the receivers
#pragma unroll
    for (int r = 0; r < TB_R; ++r) {
        const int uz = uz0 + r, gz = wrapn(uz, g.Hp);
        rofs[r] = gz * g.ld;
        const int o = rofs[r] + gx;
        if constexpr (GEN) {
            const Coef cf = gen_coef(a.cg, b, gz, gx);
            A[r] = cf.al; K[r] = cf.kp;
        } else {
            A[r] = AL[o]; K[r] = KAp[o];
        }
        const int iz = min(max(gz - a.cg.nbc, 0), a.cg.nz - 1), ix = min(max(gx - a.cg.nbc, 0), a.cg.nx - 1);
        dA[r] = a.dam[((size_t)b * a.cg.nz + iz) * a.cg.nx + ix];
        D0[r] = a.in_prev[so + o];
        D1[r] = a.in_cur[so + o];
        P0[r] = a.p_in_prev[so + o];
        P1[r] = a.p_in_cur[so + o];
        const int rr = w * TB_R + r;
        if (rr >= H && rr < TB_RH - H && uz < g.Hp) rin |= 1u << r;
        if (gz == g.isz) smask |= 1u << r;      // a region taller than a tiny domain holds the row more than once
        if (gz == g.igz) rrow = r;
    }
    const bool scol = gx == isx;
    const float bsrc = smask ? a.coeffs[4 * g.cstride + (size_t)b * g.slice + (size_t)g.isz * g.ld + isx] : 0.0f;
    const float dbsrc = smask ? a.dbeta[bs] : 0.0f;
    const int rs = (rrow >= 0) ? g.rcv_start[gx] : 0, re = (rrow >= 0) ? g.rcv_start[gx + 1] : 0;
    const int rcv0 = rs < re ? g.rcv_list[rs] : -1;
    const bool rmulti = __any(re - rs > 1);               // wave-uniform: a column with several receivers
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (t >= a.nsteps) break;
        const int n = a.n0 + t;
        float *cur = (t & 1) ? D0 : D1;     // dP_n
        float *prv = (t & 1) ? D1 : D0;     // dP_{n-1} -> overwritten with dP_{n+1}
        float *P = (t & 1) ? P0 : P1;       // P_n
        float *Pp = (t & 1) ? P1 : P0;      // P_{n-1}  -> overwritten with P_{n+1}
        Halo4 hd, hp;
        const float de[4] = {cur[0], cur[1], cur[TB_R - 2], cur[TB_R - 1]};
        const float pe[4] = {P[0], P[1], P[TB_R - 2], P[TB_R - 1]};
        exchange2(xch, pxc, t & 1, w, lane, de, pe, hd, hp);
#pragma unroll
        for (int r = 0; r < TB_R; ++r) {
            const float c = cur[r], kp = K[r];
            const float lap = tb_lap(cur, r, hd);
            float t1, t2;
            tb_t1t2(A[r], kp, t1, t2);
            float hom = t1 * c; const float a2 = t2 * prv[r]; hom = hom - a2;
            const float a3 = A[r] * lap; hom = hom + a3;
            // tb_lap's star of P, written out (see tb_lap)
            const float pm2 = r >= 2 ? P[r - 2] : (r == 1 ? hp.u1 : hp.u2), pm1 = r >= 1 ? P[r - 1] : hp.u1;
            const float pp1 = r + 1 < TB_R ? P[r + 1] : hp.d1, pp2 = r + 2 < TB_R ? P[r + 2] : (r + 2 == TB_R ? hp.d1 : hp.d2);
            const float pc = P[r], pv = Pp[r];
            const float pl1 = dpp_shr1(pc), pr1 = dpp_shl1(pc);
            const float pl2 = dpp_shr1(pl1), pr2 = dpp_shl1(pr1);
            float q1 = pm1 + pp1; q1 = q1 + pl1; q1 = q1 + pr1;
            float q2 = pm2 + pp2; q2 = q2 + pl2; q2 = q2 + pr2;
            float plap = C2 * q1; const float pq = C3 * q2; plap = plap + pq;
            float d = C1X2 * pc; d = d + plap;
            float f = dA[r] * d;
            const float dk = kp * ratio, dp = pc - pv;
            const float fk = dk * dp; f = f - fk;
            prv[r] = hom + f;
            float b1 = t1 * pc; const float b2 = t2 * pv; b1 = b1 - b2;   // the forward, k_fwd_tb's order
            const float b3 = A[r] * plap;
            Pp[r] = b1 + b3;
        }
        if (smask) {                                                   // pde.py:80-81 and its tangent
#pragma unroll
            for (int r = 0; r < TB_R; ++r)
                if ((smask & (1u << r)) && scol) {
                    const float add = bsrc * a.w[t]; Pp[r] = Pp[r] + add;
                    const float dadd = dbsrc * a.w[t]; prv[r] = prv[r] + dadd;
                }
        }
        if (rrow >= 0 && (rin & (1u << rrow)) && xin && (n % g.st) == 0) {   // pde.py:82-83
            float val = 0.0f, dval = 0.0f;
#pragma unroll
            for (int r = 0; r < TB_R; ++r) if (r == rrow) { val = Pp[r]; dval = prv[r]; }
            dval = dval * oscale;
            const size_t ko = ((size_t)bs * g.nrec + n / g.st) * g.ng;
            float *SK = a.seis + ko, *DK = a.dseis + ko;
            if (rcv0 >= 0) { SK[rcv0] = val; DK[rcv0] = dval; }
            if (rmulti)
                for (int j = rs + 1; j < re; ++j) { const int k = g.rcv_list[j]; SK[k] = val; DK[k] = dval; }
        }
    }
    if (xin) {
        const bool odd = (a.nsteps & 1) != 0;   // after nsteps steps the newest levels are in D0 / P0 if odd
#pragma unroll
        for (int r = 0; r < TB_R; ++r)
            if (rin & (1u << r)) {
                const size_t o = so + rofs[r] + gx;
                a.out_cur[o] = odd ? D0[r] : D1[r];
                a.out_prev[o] = odd ? D1[r] : D0[r];
                a.p_out_cur[o] = odd ? P0[r] : P1[r];
                a.p_out_prev[o] = odd ? P1[r] : P0[r];
            }
    }
}

// --------------------------------------------------------------------------------------- K1/K2
// Chunked kernels on WIDE regions (configs[4]-size grids; the default chunked layout).  A region is
// 128 columns x NW*R rows: every lane holds TWO adjacent columns {2l, 2l+1} of R rows as one f32x2
// per row, so every add / mul of the stencil is one packed v_pk_*_f32 for two cells, and the
// horizontal taps of a column pair need four DPP lane shifts (x-1 of column 2l is lane l-1's .y, x-2
// its .x; x+1 of column 2l+1 is lane l+1's .x, x+2 its .y) instead of four per cell.  The region's
// halo H = 2T is then 16 of 128 columns instead of 16 of 64: a tile re-reads (128 x RH) / (112 x IH)
// of what it stores instead of (64 x 64) / (48 x 48), and its 512-B rows span 4-5 128-B lines per
// 112 owned columns instead of 3 per 48 (profiles/r3: the 64-column adjoint moved 1.34x its
// algorithmic bytes at configs[4]).  Same per-cell operations in the same order as k_fwd_tb /
// k_adj_tb (bit-exact with them and with the oracle).  PAIR (even Wp): a lane's two columns are
// adjacent in memory, one 8-byte access; odd Wp wraps a pair across the domain edge, two 4-byte ones.
constexpr int TW_W = 128;                // wide region columns (two per lane)

template <bool PAIR, int CP = 0>
__device__ __forceinline__ f32x2 ld2(__amdgpu_buffer_rsrc_t r, int v0, int v1, int soff)
{
    if constexpr (PAIR) {
        const u32x2 x = __builtin_amdgcn_raw_buffer_load_b64(r, v0, soff, CP);
        return f32x2{__uint_as_float(x.x), __uint_as_float(x.y)};
    } else {
        return f32x2{__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, v0, soff, CP)),
                     __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, v1, soff, CP))};
    }
}
template <bool PAIR, int CP = 0>
__device__ __forceinline__ void st2(f32x2 v, __amdgpu_buffer_rsrc_t r, int v0, int v1, int soff)
{
    if constexpr (PAIR) {
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(v.x), __float_as_uint(v.y)}, r, v0, soff, CP);
    } else {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.x), r, v0, soff, CP);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.y), r, v1, soff, CP);
    }
}

// the four horizontal taps of a column pair c = {x, x+1} (lane shifts; region edges read 0)
struct HTaps { f32x2 l1, r1, l2, r2; };
__device__ __forceinline__ HTaps htaps(f32x2 c)
{
    const float sx = dpp_shr1(c.x), sy = dpp_shr1(c.y), lx = dpp_shl1(c.x), ly = dpp_shl1(c.y);
    HTaps h;
    h.l1 = f32x2{sy, c.x}; h.r1 = f32x2{c.y, lx};
    h.l2 = f32x2{sx, sy};  h.r2 = f32x2{lx, ly};
    return h;
}

// boundary rows 0, 1, R-2, R-1 of every wave through LDS; rows -2, -1, R, R+1 of this wave back
struct Halo2 { f32x2 u2, u1, d1, d2; };
template <int NW, int R>
__device__ __forceinline__ void tw_put(f32x2 (*x)[NW][4][64], int buf, int w, int lane, const f32x2 *v)
{
    x[buf][w][0][lane] = v[0]; x[buf][w][1][lane] = v[1];
    x[buf][w][2][lane] = v[R - 2]; x[buf][w][3][lane] = v[R - 1];
}
template <int NW>
__device__ __forceinline__ Halo2 tw_get(f32x2 (*x)[NW][4][64], int buf, int w, int lane)
{
    const int wu = w > 0 ? w - 1 : 0, wd = w < NW - 1 ? w + 1 : NW - 1;   // (edge waves: halo rows)
    Halo2 h;
    h.u2 = x[buf][wu][2][lane]; h.u1 = x[buf][wu][3][lane];
    h.d1 = x[buf][wd][0][lane]; h.d2 = x[buf][wd][1][lane];
    return h;
}
#define TW_VERT(ARR, r, H2, m2, m1, p1, p2)                                       \
    const f32x2 m2 = (r) >= 2 ? ARR[(r) - 2] : ((r) == 1 ? H2.u1 : H2.u2);        \
    const f32x2 m1 = (r) >= 1 ? ARR[(r) - 1] : H2.u1;                            \
    const f32x2 p1 = (r) + 1 < R ? ARR[(r) + 1] : H2.d1;                         \
    const f32x2 p2 = (r) + 2 < R ? ARR[(r) + 2] : ((r) + 2 == R ? H2.d1 : H2.d2);

// Region geometry shared by the wide kernels (flat locals: uniform values stay SGPRs).
#define TW_REGION_INIT()                                                                           \
    constexpr int H = 2 * T, IW = TW_W - 2 * H, RH = NW * R, IH = RH - 2 * H;                      \
    const TBGeo &g = a.g;                                                                          \
    const int lane = threadIdx.x & 63;                                                             \
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                                \
    const TileId ti = decode_tile(blockIdx.x, g.tiles_x, g.ntiles, g.B * g.ns_grp);                \
    if (!ti.valid) return;                                          /* whole workgroup: uniform */ \
    const int b = ti.sl / g.ns_grp, s = g.s_off + (ti.sl - b * g.ns_grp), bs = b * g.ns + s;       \
    const int ux = ti.tx * IW - H + 2 * lane;                       /* unwrapped column of .x */   \
    const int gx0 = wrapn(ux, g.Wp), gx1 = wrapn(ux + 1, g.Wp);                                    \
    const bool lin = lane >= H / 2 && lane < 64 - H / 2;            /* interior lane (both cols) */\
    const bool xin0 = lin && ux < g.Wp, xin1 = lin && ux + 1 < g.Wp;                               \
    const int uz0 = ti.ty * IH - H + w * R;                                                        \
    const size_t so = (size_t)bs * g.slice;                                                        \
    const int sbytes = (int)(g.slice * 4);                                                         \
    const int v0 = gx0 * 4, v1 = gx1 * 4;                           /* lane byte offsets in a row */\
    const int vi0 = xin0 ? v0 : OOB, vi1 = xin1 ? v1 : OOB;         /* own (interior) cells only */\
    int rofs[R];                                                    /* wave-uniform gz * ld */     \
    unsigned rin = 0;                                               /* wave-uniform interior rows */\
    _Pragma("unroll") for (int r = 0; r < R; ++r) {                                                \
        const int uz = uz0 + r;                                                                    \
        rofs[r] = wrapn(uz, g.Hp) * g.ld;                                                          \
        const int rr = w * R + r;                                                                  \
        if (rr >= H && rr < RH - H && uz < g.Hp) rin |= 1u << r;                                   \
    }

template <int T, int NW, int R, bool GEN, bool PAIR>
__global__ __launch_bounds__(64 * NW) void k_fwd_tw(FwdTBArgs a)
{
    __shared__ f32x2 xch[2][NW][4][64];
    __shared__ f32x2 As[NW][R][64];      // alpha of the wave's own rows (wave-private), as k_adj_tw
    TW_REGION_INIT()
    // this workgroup's shots: a.spw of the model's shots on one region (k_adj_tw): the coefficients
    // are generated once for all of them
    const int jg = s - g.s_off, s_first = g.s_off + jg * a.spw, nsh = min(a.spw, a.ns_sh - jg * a.spw);
    (void)bs; (void)so;
    f32x2 C1[R], C2v[R];
    unsigned smask = 0;
    int rrow = -1;
    {
        const float *AL = a.coeffs + (size_t)b * g.slice;
        const __amdgpu_buffer_rsrc_t RA = rsrc_of(AL, sbytes), R1 = rsrc_of(AL + g.cstride, sbytes),
                                     R2 = rsrc_of(AL + 2 * g.cstride, sbytes);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int gz = wrapn(uz0 + r, g.Hp);
            if constexpr (GEN) {   // regenerated from the 20 KB-per-row model (L2-resident) instead of 3 fields
                const Coef c0 = gen_coef(a.cg, b, gz, gx0), c1 = gen_coef(a.cg, b, gz, gx1);
                As[w][r][lane] = f32x2{c0.al, c1.al}; C1[r] = f32x2{c0.t1, c1.t1}; C2v[r] = f32x2{c0.t2, c1.t2};
            } else {
                As[w][r][lane] = ld2<PAIR>(RA, v0, v1, rofs[r] * 4);
                C1[r] = ld2<PAIR>(R1, v0, v1, rofs[r] * 4);
                C2v[r] = ld2<PAIR>(R2, v0, v1, rofs[r] * 4);
            }
            if (gz == g.isz) smask |= 1u << r;          // (tiny domains: a wave can hold the row twice)
            if (gz == g.igz) rrow = r;
        }
    }
    // receivers of the lane's two columns (usually one each), read once
    int rs0 = 0, re0 = 0, rs1 = 0, re1 = 0;
    if (rrow >= 0) { rs0 = g.rcv_start[gx0]; re0 = g.rcv_start[gx0 + 1]; rs1 = g.rcv_start[gx1]; re1 = g.rcv_start[gx1 + 1]; }
    const int rc0 = xin0 && rs0 < re0 ? g.rcv_list[rs0] : -1, rc1 = xin1 && rs1 < re1 ? g.rcv_list[rs1] : -1;
    const bool rmulti = __any(re0 - rs0 > 1 || re1 - rs1 > 1);   // wave-uniform
    const f32x2 kC2 = {C2, C2}, kC3 = {C3, C3};
    // kernel arguments re-read from the kernarg segment per shot (k_adj_tw); a shot's two input levels
    // are loaded when the previous shot's last levels have been stored (k_adj_tw's pipelining)
    auto kargs = [&]() {
        const __attribute__((address_space(4))) FwdTBArgs *k_ =
            (const __attribute__((address_space(4))) FwdTBArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(k_));
        return k_;
    };
    f32x2 P0[R], P1[R];
    auto load_shot = [&](int ss_) {
        const auto *k_ = kargs();
        const size_t so_ = (size_t)(b * k_->g.ns + ss_) * k_->g.slice;
        const __amdgpu_buffer_rsrc_t RPv = rsrc_of(k_->in_prev + so_, sbytes), RCu = rsrc_of(k_->in_cur + so_, sbytes);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            P0[r] = ld2<PAIR>(RPv, v0, v1, rofs[r] * 4);
            P1[r] = ld2<PAIR>(RCu, v0, v1, rofs[r] * 4);
        }
    };
    load_shot(s_first);
    for (int sh = 0; sh < nsh; ++sh) {
    const auto *ka = kargs();
    const int ss = s_first + sh, bss = b * ka->g.ns + ss;
    const size_t soo = (size_t)bss * ka->g.slice;
    // an odd T ends on exchange buffer 0, which the next shot's first step rewrites: wait for every
    // wave's last halo reads (an even T ends on buffer 1, and buffer 0's last reads precede the last
    // step's barrier)
    if ((T & 1) && sh) __syncthreads();
    const int isx = ka->g.isx[ss];
    const bool sc0 = gx0 == isx, sc1 = gx1 == isx;
    const float bsrc = smask ? ka->coeffs[4 * ka->g.cstride + (size_t)b * ka->g.slice + (size_t)ka->g.isz * ka->g.ld + isx] : 0.0f;
#pragma unroll
    for (int t = 0; t < T; ++t) {       // exactly T steps (the host launches a shorter tail as its own T)
        f32x2 *cur = (t & 1) ? P0 : P1;     // P_{n+t}
        f32x2 *prv = (t & 1) ? P1 : P0;     // P_{n+t-1} -> P_{n+t+1}
        tw_put<NW, R>(xch, t & 1, w, lane, cur);
        __syncthreads();
        const Halo2 h2 = tw_get<NW>(xch, t & 1, w, lane);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            TW_VERT(cur, r, h2, zm2, zm1, zp1, zp2)
            const f32x2 c = cur[r];
            const HTaps x = htaps(c);
            // pde.py:79, reference evaluation order per cell
            f32x2 s1 = zm1 + zp1; s1 = s1 + x.l1; s1 = s1 + x.r1;
            f32x2 s2 = zm2 + zp2; s2 = s2 + x.l2; s2 = s2 + x.r2;
            f32x2 lap = kC2 * s1; const f32x2 l2 = kC3 * s2; lap = lap + l2;
            f32x2 a1 = C1[r] * c; const f32x2 a2 = C2v[r] * prv[r]; a1 = a1 - a2;
            const f32x2 a3 = As[w][r][lane] * lap;
            prv[r] = a1 + a3;
        }
        if (smask) {                                                   // pde.py:80-81
            const float add = bsrc * ka->w[t];
            const f32x2 av = {sc0 ? add : -0.0f, sc1 ? add : -0.0f};   // x + (-0) == x bit for bit
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (smask & (1u << r)) prv[r] = prv[r] + av;
        }
        const int n = ka->n0 + t;
        if (ka->hist) {
            const __amdgpu_buffer_rsrc_t HS = rsrc_of(ka->hist + (size_t)(n + 2 - ka->hbase) * ka->g.level + soo, sbytes);
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (rin & (1u << r)) st2<PAIR, CP_NT>(prv[r], HS, vi0, vi1, rofs[r] * 4);   // streaming
        }
        if (ka->seis && rrow >= 0 && (rin & (1u << rrow)) && (n % ka->g.st) == 0) {   // pde.py:82-83 (no seis: a recompute)
            f32x2 val = prv[0];
#pragma unroll
            for (int r = 1; r < R; ++r) if (r == rrow) val = prv[r];
            float *SK = ka->seis + ((size_t)bss * ka->g.nrec + n / ka->g.st) * ka->g.ng;
            if (rc0 >= 0) SK[rc0] = val.x;
            if (rc1 >= 0) SK[rc1] = val.y;
            if (rmulti) {
                if (xin0) for (int j = rs0 + 1; j < re0; ++j) SK[ka->g.rcv_list[j]] = val.x;
                if (xin1) for (int j = rs1 + 1; j < re1; ++j) SK[ka->g.rcv_list[j]] = val.y;
            }
        }
    }
    if (ka->out_cur) {   // ring path: keep the last two levels
        constexpr bool odd = (T & 1) != 0;      // after T steps the newest level is in P0 if odd
        const __amdgpu_buffer_rsrc_t OC = rsrc_of(ka->out_cur + soo, sbytes), OP = rsrc_of(ka->out_prev + soo, sbytes);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (rin & (1u << r)) {
                st2<PAIR>(odd ? P0[r] : P1[r], OC, vi0, vi1, rofs[r] * 4);
                st2<PAIR>(odd ? P1[r] : P0[r], OP, vi0, vi1, rofs[r] * 4);
            }
    }
    if (sh + 1 < nsh) load_shot(ss + 1);
    }   // shots
}

// Adjoint on wide regions (k_adj_tb's per-cell arithmetic):
//   L_k = T1 L_{k+1} - T2 L_{k+2} + (c2 N1(A L_{k+1}) + c3 N2(A L_{k+1})) [+ R^T dseis[k-1]]
//   gA_s += L_k (2c1 P_{k-1} + c2 S1(P_{k-1}) + c3 S2(P_{k-1})),  gk += (K P_{k-1})(L_{k+1} - L_k)
//   gbeta[s] += L_k(src) w[k-1]           (own cells; gA loaded and stored once per launch)
// EXACT: the oracle's fp32 operation order (bitwise gA / gbeta).  Else the same stencils with FMA
// contraction (fp32-level tolerance: rdq_fwi_set_variant without RDQ_VARIANT_ADJ_EXACT, nbc >= 20).
// Every gk term is summed in fp64 in both.  alpha and kappa are
// regenerated from the model in registers (gen_coef, bit-identical to K3's fields): the 16 shots of a
// tile then read the L2-resident 6 MB model instead of two padded fields each.  Loads are issued in
// the order the first step uses them (alpha's model values and L_{k+1} first).
template <int T, int NW, int R, bool PAIR, bool EXACT>
__global__ __launch_bounds__(64 * NW) void k_adj_tw(AdjTBArgs a)
{
    __shared__ f32x2 xq[2][NW][4][64];
    __shared__ f32x2 xp[2][NW][4][64];
    __shared__ f32x2 As[NW][R][64];      // alpha of the wave's own rows (wave-private: no barrier), in LDS
                                         // instead of 8 VGPRs live across the shot loop
    TW_REGION_INIT()
    // this workgroup's shots: group jg of the model's shots (a.spw each), all on the same region, so
    // alpha / kappa are generated once for all of them (~10 ms of the adjoint at configs[4] when every
    // shot's workgroup generated its own: profiles/r5/configs4_adj_coef_ab.jsonl)
    const int jg = s - g.s_off, s_first = g.s_off + jg * a.spw, nsh = min(a.spw, a.ns_sh - jg * a.spw);
    (void)bs; (void)so;
    f32x2 KP[R];                         // temp1 / temp2 re-derived per step (bit-identical)
    unsigned pmask = 0, smask = 0, rmask = 0;            // wave-uniform row masks
    const f32x2 kC2 = {C2, C2}, kC3 = {C3, C3}, kC1X2 = {C1X2, C1X2}, k2 = {2.0f, 2.0f}, k1 = {1.0f, 1.0f};
    // history P_{k-1}: only the columns the own cells' gradient stencil reaches (own +- 2: lanes H/2 - 1
    // .. 64 - H/2), the other halo lanes' loads are out of range (no memory access, zeros): 112 of 128
    // columns at T = 5, the history being the adjoint's largest stream
    const bool plane = lane >= H / 2 - 1 && lane < 64 - H / 2 + 1;
    const int pv0 = plane ? v0 : OOB, pv1 = plane ? v1 : OOB;
    {
        int gz[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            gz[r] = wrapn(uz0 + r, g.Hp);
            const int rr = w * R + r;
            if (rr >= H - 2 && rr < RH - H + 2) pmask |= 1u << r;
            if (gz[r] == g.isz) smask |= 1u << r;
            if (gz[r] == g.igz) rmask |= 1u << r;
        }
        Coef c0[R], c1[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { c0[r] = gen_coef(a.cg, b, gz[r], gx0); c1[r] = gen_coef(a.cg, b, gz[r], gx1); }
#pragma unroll
        for (int r = 0; r < R; ++r) { As[w][r][lane] = f32x2{c0[r].al, c1[r].al}; KP[r] = f32x2{c0[r].kp, c1[r].kp}; }
    }
    const int rcv0 = rmask ? g.rlane[gx0] : -1, rcv1 = rmask ? g.rlane[gx1] : -1;
    // a shot's launch-start loads (levels L_{k0+1}, L_{k0+2}, history P_{k0-1}, gA): shot 0's here,
    // shot s+1's right after shot s's output stores, so they are in flight during shot s's gk
    // reduction.  Kernel arguments are re-read from the kernarg segment (an opaque pointer) per
    // shot: kept live across the shot loop they exhaust the SGPRs and spill.
    f32x2 L0[R], L1[R], GA[R], Pn[R];
    auto kargs = [&]() {
        const __attribute__((address_space(4))) AdjTBArgs *k_ =
            (const __attribute__((address_space(4))) AdjTBArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(k_));
        return k_;
    };
    auto load_shot = [&](int ss_) {
        const auto *k_ = kargs();
        const size_t so_ = (size_t)(b * k_->g.ns + ss_) * k_->g.slice;
        const __amdgpu_buffer_rsrc_t RL1 = rsrc_of(k_->in_l1 + so_, sbytes), RL2 = rsrc_of(k_->in_l2 + so_, sbytes);
        const __amdgpu_buffer_rsrc_t RG = rsrc_of(k_->gA + so_, sbytes);
        const __amdgpu_buffer_rsrc_t HR = rsrc_of(k_->hist + (size_t)(k_->k0 - k_->hbase) * k_->g.level + so_, sbytes);
#pragma unroll
        for (int r = 0; r < R; ++r) L1[r] = ld2<PAIR>(RL1, v0, v1, rofs[r] * 4);   // L_{k+1}
#pragma unroll
        for (int r = 0; r < R; ++r) L0[r] = ld2<PAIR>(RL2, v0, v1, rofs[r] * 4);   // L_{k+2}
#pragma unroll
        for (int r = 0; r < R; ++r) Pn[r] = (pmask & (1u << r)) ? ld2<PAIR>(HR, pv0, pv1, rofs[r] * 4) : f32x2{0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < R; ++r) GA[r] = (rin & (1u << r)) ? ld2<PAIR>(RG, vi0, vi1, rofs[r] * 4) : f32x2{0.0f, 0.0f};
    };
    load_shot(s_first);
    for (int sh = 0; sh < nsh; ++sh) {
    const auto *ka = kargs();
    const int ss = s_first + sh, bss = b * ka->g.ns + ss;
    const size_t soo = (size_t)bss * ka->g.slice;
    // (no barrier between shots: the gk reduction's LDS words are wave 0's own exchange slot, which
    //  only wave 0 rewrites, after its thread 0 has read them; the reduction's two barriers order the
    //  last step's halo reads before the next shot's first exchange)
    const int isx = ka->g.isx[ss];
    const bool sc0 = xin0 && gx0 == isx, sc1 = xin1 && gx1 == isx;   // the source cell is an own cell
    const __amdgpu_buffer_rsrc_t DSR = rsrc_of(ka->dseis + (size_t)bss * ka->g.nrec * ka->g.dstride);
    const bool gbl = (smask & rin) && (sc0 || sc1);
    float gbacc = gbl ? ka->gbeta[bss] : 0.0f;
    double ksum = 0.0;                   // every gk term in fp64
#pragma unroll
    for (int t = 0; t < T; ++t) {       // exactly T steps (the host launches a shorter tail as its own T)
        __builtin_amdgcn_sched_barrier(0);  // no step's work moved into another (live ranges: no spills)
        const int k = ka->k0 - t;
        f32x2 *cur = (t & 1) ? L0 : L1;     // L_{k+1}
        f32x2 *prv = (t & 1) ? L1 : L0;     // L_{k+2} -> L_k
        f32x2 P[R];
#pragma unroll
        for (int r = 0; r < R; ++r) P[r] = Pn[r];
        if (t + 1 < T) {   // history P_{k-2} of the next step, on the rows the interior's stencil needs
            const __amdgpu_buffer_rsrc_t HR = rsrc_of(ka->hist + (size_t)(k - 1 - ka->hbase) * ka->g.level + soo, sbytes);
#pragma unroll
            for (int r = 0; r < R; ++r) if (pmask & (1u << r)) Pn[r] = ld2<PAIR>(HR, pv0, pv1, rofs[r] * 4);
        }
        // this step's receiver residuals, loaded before the stencil so their latency hides under it
        const int ri = rmask ? rec_index(k - 1, ka->g.st) : -1;   // wave-uniform
        f32x2 dsv = {-0.0f, -0.0f};
        if (ri >= 0) {
            const int ro = ri * ka->g.dstride;
            const float d0 = bload(DSR, rcv0 >= 0 ? (ro + rcv0) * 4 : OOB, 0);
            const float d1 = bload(DSR, rcv1 >= 0 ? (ro + rcv1) * 4 : OOB, 0);
            dsv = f32x2{rcv0 >= 0 ? d0 : -0.0f, rcv1 >= 0 ? d1 : -0.0f};
        }
        f32x2 q[R];
#pragma unroll
        for (int r = 0; r < R; ++r) q[r] = As[w][r][lane] * cur[r];
        tw_put<NW, R>(xq, t & 1, w, lane, q);
        tw_put<NW, R>(xp, t & 1, w, lane, P);
        __syncthreads();
        const Halo2 hq = tw_get<NW>(xq, t & 1, w, lane);
        const Halo2 hp = tw_get<NW>(xp, t & 1, w, lane);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            TW_VERT(q, r, hq, qm2, qm1, qp1, qp2)
            const HTaps x = htaps(q[r]);
            f32x2 n1 = qm1 + qp1; n1 = n1 + x.l1; n1 = n1 + x.r1;
            f32x2 n2 = qm2 + qp2; n2 = n2 + x.l2; n2 = n2 + x.r2;
            if constexpr (EXACT) {
                f32x2 nb = kC2 * n1; const f32x2 nb2 = kC3 * n2; nb = nb + nb2;
                f32x2 t1 = kC1X2 * As[w][r][lane]; t1 = t1 + k2; t1 = t1 - KP[r];      // pde.py:69
                const f32x2 t2 = k1 - KP[r];                                  // pde.py:70
                f32x2 l = t1 * cur[r]; const f32x2 l2 = t2 * prv[r]; l = l - l2; l = l + nb;
                prv[r] = l;
            } else {
                const f32x2 nb = fma2(kC3, n2, kC2 * n1);
                const f32x2 t1 = fma2(kC1X2, As[w][r][lane], k2) - KP[r], t2 = k1 - KP[r];
                prv[r] = fma2(t1, cur[r], fma2(-t2, prv[r], nb));
            }
        }
        if (ri >= 0) {                          // adjoint of the receiver sampling
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (rmask & (1u << r)) prv[r] = prv[r] + dsv;      // -0 on lanes without a receiver
        }
        // gradient accumulators (own cells are the ones stored; halo lanes compute and discard)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!(rin & (1u << r))) continue;   // wave-uniform
            TW_VERT(P, r, hp, pm2, pm1, pp1, pp2)
            const f32x2 pc = P[r];
            const HTaps x = htaps(pc);
            f32x2 s1 = pm1 + pp1; s1 = s1 + x.l1; s1 = s1 + x.r1;
            f32x2 s2 = pm2 + pp2; s2 = s2 + x.l2; s2 = s2 + x.r2;
            const f32x2 l = prv[r];
            const f32x2 dl = cur[r] - l;
            if constexpr (EXACT) {
                f32x2 lap = kC2 * s1; const f32x2 lq = kC3 * s2; lap = lap + lq;
                f32x2 d = kC1X2 * pc; d = d + lap;
                const f32x2 c = l * d;
                GA[r] = GA[r] + c;
                f32x2 kk = KP[r] * pc; kk = kk * dl;                      // fp32 term, fp64 sum
                ksum += xin0 ? (double)kk.x : 0.0;
                ksum += xin1 ? (double)kk.y : 0.0;
            } else {
                const f32x2 d = fma2(kC1X2, pc, fma2(kC3, s2, kC2 * s1));
                GA[r] = fma2(l, d, GA[r]);
                const f32x2 kk = (KP[r] * pc) * dl;                    // fp32 term, fp64 sum (the total
                ksum += (double)(xin0 ? kk.x : 0.0f);                   //  cancels: fp32 partials lost
                ksum += (double)(xin1 ? kk.y : 0.0f);                   //  1.3e-4 of it at OpenFWI)
            }
            if ((smask & (1u << r)) && (sc0 || sc1)) { const float gb = (sc0 ? l.x : l.y) * ka->w[t]; gbacc = gbacc + gb; }
        }
    }
    {
        constexpr bool odd = (T & 1) != 0;      // newest level (L_{k0-T+1}) is in L0 if odd
        const __amdgpu_buffer_rsrc_t O1 = rsrc_of(ka->out_l1 + soo, sbytes), O2 = rsrc_of(ka->out_l2 + soo, sbytes);
        const __amdgpu_buffer_rsrc_t RG = rsrc_of(ka->gA + soo, sbytes);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (rin & (1u << r)) {
                st2<PAIR>(odd ? L0[r] : L1[r], O1, vi0, vi1, rofs[r] * 4);
                st2<PAIR>(odd ? L1[r] : L0[r], O2, vi0, vi1, rofs[r] * 4);
                st2<PAIR>(GA[r], RG, vi0, vi1, rofs[r] * 4);
            }
    }
    if (sh + 1 < nsh) load_shot(ss + 1);
    if (gbl) ka->gbeta[bss] = gbacc;
    // deterministic workgroup reduction of the sponge-coefficient partial sum: a fixed xor tree per
    // wave, then the NW wave sums in wave order (LDS of the exchange)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ksum += __shfl_xor(ksum, o, 64);
    double *red = reinterpret_cast<double *>(&xq[0][0][0][0]);
    __syncthreads();
    if (lane == 0) red[w] = ksum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = red[0];
        for (int i = 1; i < NW; ++i) tot += red[i];
        // one add per (slot, launch), launches in stream order: the same sum as a load-add-store, but
        // without the load's round trip before the next shot's barrier
        unsafeAtomicAdd(&ka->gk_part[(size_t)bss * ka->nblk + ti.tile], tot);
    }
    }   // shots
}
#undef TW_VERT
#undef TW_REGION_INIT

// --------------------------------------------------------------------------------------- K1/K2
// Persistent variants: ONE launch runs the whole time loop.  Every workgroup keeps its region
// (coefficients + two wavefield levels) in VGPRs for all nt steps; after each epoch of T steps it
// publishes the H-wide border of its interior (the only cells any other region's halo reads) and
// reloads its own halo ring from the neighbours' publications.  The hand-off is the
// data-is-the-flag form (8-byte {tag, value} granules, write-through `sc1` stores, `sc1` loads
// re-read until every tag matches: cdna_hip_programming.md §6 G16, R2), so there is no flag, no
// fence and no kernel boundary between epochs — the per-launch prologue, store drain and launch gap
// of the chunked path (≈7.5 µs per forward launch at OpenFWI size) become one hand-off per epoch.
// Needs every workgroup of the launch resident at once: the host checks the grid against the
// occupancy query and uses the chunked kernels otherwise; every spin is bounded (a timeout sets
// the plan's status word, reported by rdq_fwi_status, and the kernel still runs to completion).
//
// The time step is VALU-issue-bound (wave64 fp32 VALU = 4 cycles), so the kernels are written
// to keep per-cell instructions at the stencil's own: row predicates are wave-uniform bits, the
// per-lane ones are three loop-invariant masks, and every history / granule access is a buffer
// instruction (scalar base + one lane offset + one uniform row offset: no 64-bit address VALU).
// Region height is a template parameter (NW waves x 8 rows): 12 waves -> 64 x 96 regions, one
// workgroup per CU at OpenFWI size (28 tiles x 8 shots = 224 <= 256 CUs).
//
// Granule buffer (inside the caller's `ring`): [2 epoch parity][B][ns][Hp][ld] x 16-B granules,
// zeroed before each launch; tag = epoch index (>= 1) so a zeroed granule never matches.
constexpr int CP_SC1 = 16;                            // buffer cache policy: sc1 (write-through / L1 bypass)
constexpr int PT_ADJ_SG = 8;                          // adjoint hand-off sweep: rows per load group
constexpr int PT_ROLES_T = 4;                         // wave roles (rdq_fwi_set_wave_roles) are built at this depth
constexpr int PT_ROLE_WORD = 24;                      // status word: waves that entered the adjoint's source/receiver loop
constexpr int PT_SROLE_RW = 6;                        // the source role (rdq_fwi_set_source_role): that depth, these rows per wave
constexpr size_t PROF_RAW = 16;                       // per-wave records after the 11 summary words (PT_PROF_FLUSH)
constexpr size_t PROF_REC = 8;                        // words per wave record
constexpr size_t PROF_WAVES = 4096 * 16;              // blocks x waves recorded
constexpr size_t PROF_WORDS = PROF_RAW + PROF_WAVES * PROF_REC;   // per kernel (fwd, then adj)
constexpr unsigned long long PT_TIMEOUT_TICKS = 20000000ull;   // 200 ms of s_memrealtime (100 MHz)

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// One cell's hand-off granule = BOTH wavefield levels, 16 bytes {v0, tag, v1, tag}: each 8-byte
// half carries its own epoch tag, so a read torn between the halves is still caught by the tag
// check (the guarantee used is only that an aligned 8-byte store is seen whole), and a sweep or a
// publish is one dwordx4 instruction per row instead of two dwordx2.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x4 gran2(unsigned tag, float v0, float v1)
{
    u32x4 x;
    x.x = __float_as_uint(v0); x.y = tag; x.z = __float_as_uint(v1); x.w = tag;
    return x;
}
__device__ __forceinline__ void gran_put(__amdgpu_buffer_rsrc_t r, int voff, int soff, unsigned tag, float v0, float v1)
{
    __builtin_amdgcn_raw_buffer_store_b128(gran2(tag, v0, v1), r, voff, soff, CP_SC1);
}
// XCD-local hand-off: a plain store stays in the producer XCD's L2, where a same-XCD consumer's
// sc1 (L1-bypassing, L2-served) load sees it without the write-through round trip to memory
// (tools/probe/l2_probe.hip)
__device__ __forceinline__ void gran_put_l2(__amdgpu_buffer_rsrc_t r, int voff, int soff, unsigned tag, float v0, float v1)
{
    __builtin_amdgcn_raw_buffer_store_b128(gran2(tag, v0, v1), r, voff, soff, 0);
}
__device__ __forceinline__ u32x4 gran_get(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, CP_SC1);
}

// A wavelet sample at a wave-uniform step, read through the scalar cache (s_load into an SGPR): out of
// the vector memory queue, where, with gfx9's in-order vmcnt, the forward's source row waited for its
// next epoch's samples behind the deferred history stores.  Forward: issued right after the publish,
// 1.362 -> 1.334 ms at configs[1] (profiles/r6/wav_scalar_ab.txt); the adjoint keeps vector loads.
__device__ __forceinline__ float wav_s(const float *w, int i)
{
    return ((const __attribute__((address_space(4))) float *)w)[i];
}

// padded-grid row of region row uz (periodic wrap, pde.py:79); |uz| < 2 Hp
__device__ __forceinline__ int wrap_row(int uz, int Hp)
{
    uz = uz < 0 ? uz + Hp : uz;
    return uz >= Hp ? uz - Hp : uz;
}

// Slice / tile assignment of a persistent launch by the XCD each workgroup actually runs on.
// Every workgroup reads its XCD id (s_getreg HW_REG_XCC_ID), takes a slot on that XCD's arrival
// counter and waits until all gridDim.x workgroups have arrived (the launch is fully resident by
// construction: the host sizes the grid to the occupancy query).  From the final per-XCD counts
// every workgroup derives the same assignment: whole (model, shot) slices go to single XCDs in XCD
// order ("local" slices: every hand-off between their tiles stays inside one L2, so granules are
// published with plain stores that stay in that L2); slices that do not fit whole on one XCD are
// dealt over the leftover workgroups ("global": write-through sc1 granules, as before).
// Correctness never depends on the placement guess: the XCD id is read, not assumed, and every
// granule carries its epoch tag, so a stale read is re-polled, never consumed.
struct PtTile { int tx, ty, tile, sl; bool valid, local; };
constexpr unsigned long long PT_ARRIVE_TICKS = 10000000ull;   // 100 ms

__device__ PtTile pt_assign(const TBGeo &g, unsigned *status, int xcd_mode)
{
    __shared__ int sh[3];
    unsigned *cnt = status + 16;                         // [8] per-XCD arrivals (zeroed per launch)
    if (threadIdx.x == 0) {
        unsigned x = 0;
        if (xcd_mode) {
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
            x &= 7u;
        }
        const unsigned slot = __hip_atomic_fetch_add(cnt + x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned n[8], tot = 0;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        bool ok = true;
        for (;;) {
            tot = 0;
            for (int i = 0; i < 8; ++i) {
                n[i] = __hip_atomic_load(cnt + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                tot += n[i];
            }
            if (tot >= gridDim.x) break;
            if (__builtin_amdgcn_s_memrealtime() - t0 > PT_ARRIVE_TICKS) { ok = false; break; }
            __builtin_amdgcn_s_sleep(2);
        }
        int sl = -1, tile = 0, local = 0;
        if (ok) {
            const int Tt = g.ntiles, S = g.nsl;
            int placed = 0, take[8];
            for (int i = 0; i < 8; ++i) {
                take[i] = xcd_mode ? min((int)n[i] / Tt, S - placed) : 0;
                placed += take[i];
            }
            int base = 0;
            for (int i = 0; i < (int)x; ++i) base += take[i];
            if ((int)slot < take[x] * Tt) {
                sl = base + (int)slot / Tt; tile = (int)slot % Tt; local = 1;
            } else {
                int r = (int)slot - take[x] * Tt;
                for (int i = 0; i < (int)x; ++i) r += (int)n[i] - take[i] * Tt;
                if (r < (S - placed) * Tt) { sl = placed + r / Tt; tile = r % Tt; }
            }
        } else {
            __hip_atomic_store(status, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // not resident
        }
        sh[0] = sl; sh[1] = tile; sh[2] = local;
    }
    __syncthreads();
    PtTile t;
    t.sl = sh[0]; t.tile = sh[1]; t.local = sh[2] != 0;
    t.valid = t.sl >= 0;
    t.ty = t.tile / g.tiles_x;
    t.tx = t.tile - t.ty * g.tiles_x;
    return t;
}

// Region geometry of the persistent kernels (flat locals so every block-/wave-uniform value stays
// provably uniform: SGPRs and scalar branches, never waterfall loops).  Row classes are
// wave-uniform bit masks; lane classes: xin (own interior column), bx (interior column within H of
// the tile's x edge, or a one-tile-wide grid), cx (column within H of the own interior: the
// T-step dependence cone).
#define PT_REGION_INIT(NW_, RW_)                                                                    \
    PT_REGION_HEAD(NW_, RW_)                                                                        \
    const int bs = __builtin_amdgcn_readfirstlane(g.sl_off + ti.sl);                                \
    const int b = __builtin_amdgcn_readfirstlane(bs / g.ns);                                        \
    const int s = __builtin_amdgcn_readfirstlane(bs - b * g.ns);                                    \
    PT_REGION_GEOM()

// Workgroup placement (pt_assign: a (slice, tile) of the launch) and the region's constants
#define PT_REGION_HEAD(NW_, RW_)                                                                    \
    constexpr int R = (RW_), RP = (RW_) / 2, RH = (NW_) * (RW_), H = 2 * T, IW = 64 - 2 * H,       \
                  IH = RH - 2 * H;                                                                  \
    const int lane = threadIdx.x & 63;                                                              \
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                                \
    const PtTile ti = pt_assign(g, a.status, a.xcd_mode);                                           \
    if (!ti.valid) return;                                                                          \
    const bool gl2 = ti.local;                     /* uniform: XCD-local slice, L2 hand-offs */

// The slice-independent part of PT_REGION_INIT (`bs` = the workgroup's flat (model, shot) slice)
#define PT_REGION_GEOM()                                                                            \
    const int tx = __builtin_amdgcn_readfirstlane(ti.tx), ty = __builtin_amdgcn_readfirstlane(ti.ty); \
    const int tile = __builtin_amdgcn_readfirstlane(ti.tile);                                       \
    const int ux = tx * IW - H + lane;                                                              \
    const int gx = wrapn(ux, g.Wp);                                                                 \
    const bool xin = lane >= H && lane < 64 - H && ux < g.Wp;                                       \
    const int vw = min(IW, g.Wp - tx * IW), vh = min(IH, g.Hp - ty * IH);                           \
    const bool bx = g.tiles_x == 1 || lane - H < H || lane - H >= vw - H;                           \
    const bool cx = lane - H < vw + H;                                                              \
    const int uz0 = ty * IH - H + w * R;                                                            \
    unsigned rin = 0, rby = 0, rcy = 0;                                                             \
    _Pragma("unroll") for (int r = 0; r < R; ++r) {                                                 \
        const int rr = w * R + r, ly = rr - H;                                                      \
        if (rr >= H && rr < RH - H && uz0 + r < g.Hp) rin |= 1u << r;                               \
        if (g.ntiles == g.tiles_x || ly < H || ly >= vh - H) rby |= 1u << r;                        \
        if (ly < vh + H) rcy |= 1u << r;                                                            \
    }                                                                                               \
    const size_t so = (size_t)bs * g.slice;                                                         \
    const int vo16 = gx * 16;                                                                       \
    const bool hx = !xin && cx, xb = xin && bx;                                                     \
    /* hand-off lane offsets (OOB: no access) */                                                    \
    const int vo_hx = hx ? vo16 : OOB, vo_cx = cx ? vo16 : OOB;                                     \
    const int vo_xin = xin ? vo16 : OOB, vo_xb = xb ? vo16 : OOB;                                   \
    const bool keep_in = xin || cx;
#define PT_ROFS(r) (wrap_row(uz0 + (r), g.Hp) * g.ld)

// Reload the halo cells of two levels V0/V1 from the granule slot GR (16-byte two-level granules),
// zero the dead cells.  `live` turns false once this wave gave up (timeout / another's timeout).
// The wave's own traffic for the next epoch (history stores / prefetch loads, wavelet, receiver
// residuals) is issued only AFTER the sweep (FWD_ISSUE / ADJ_ISSUE), not before it: a hand-off's
// latency is set by the consumer CU's own memory queue (MI355X_MICROARCH.md, handoff-1to1), and on
// gfx9 the in-order vmcnt also counts stores, so the granule loads would otherwise wait behind it.
#define PT_SWEEP(GR, TAG, V0, V1, SG)                                                               \
    {                                                                                               \
        unsigned long long t0_ = 0;                                                                 \
        const unsigned long long ts_ = prof ? __builtin_amdgcn_s_memrealtime() : 0;                 \
        unsigned long long tb_ = ts_;                                                               \
        if (prof) tsa += ts_ - tm;                                                                  \
        if constexpr (PT_PRIO) __builtin_amdgcn_s_setprio(PT_PRIO_WAIT);                            \
        PT_SWEEP_PASSES(GR, TAG, V0, V1, SG, 0)                                                     \
        if (prof) { tlast = __builtin_amdgcn_s_memrealtime(); tsc += tlast - tb_; }                 \
        if constexpr (PT_PRIO) __builtin_amdgcn_s_setprio(PT_PRIO_SWEPT);                           \
        PT_SWEEP_ZERO(V0, V1)                                                                       \
    }
// the sweep's passes from pass number P0 on, until every halo granule carries TAG (or the wave gave up)
#define PT_SWEEP_PASSES(GR, TAG, V0, V1, SG, P0)                                                    \
    {                                                                                               \
        for (unsigned pass_ = (P0); live; ++pass_) {                                                \
            /* the loads of a group of SG rows are all issued before any is checked: lanes        \
               without a halo cell in a row load from an out-of-range offset (no memory access,   \
               returns 0) instead of branching, which would make the compiler wait vmcnt(0) after \
               each load (one serial L2 round trip per row).  SG < R bounds the registers held.   \
               The row classes are laundered per pass so no per-row lane mask stays live (SGPR    \
               pressure) across the time loop.                                                    */ \
            unsigned rin_ = rin, rcy_ = rcy;                                                        \
            LAUNDER(rin_); LAUNDER(rcy_);                                                           \
            bool ok_ = true;                                                                        \
            _Pragma("unroll") for (int g_ = 0; g_ < R; g_ += (SG)) {                                \
                u32x4 x_[(SG)];                                                                     \
                int o_[(SG)];                                                                       \
                constexpr int GN_ = (SG) < R ? (SG) : R;   /* SG need not divide R: rows past R skipped */ \
                _Pragma("unroll") for (int i_ = 0; i_ < GN_; ++i_) {                                \
                    const int r = g_ + i_ < R ? g_ + i_ : R - 1;                                    \
                    const bool rowin_ = g_ + i_ < R && ((rin_ >> r) & 1u), rowcy_ = g_ + i_ < R && ((rcy_ >> r) & 1u); \
                    o_[i_] = rowin_ ? vo_hx : (rowcy_ ? vo_cx : OOB);                               \
                    x_[i_] = gran_get(GR, o_[i_], PT_ROFS(r) * 16);                                 \
                }                                                                                   \
                _Pragma("unroll") for (int i_ = 0; i_ < GN_; ++i_) {                                \
                    const int r = g_ + i_ < R ? g_ + i_ : R - 1;                                    \
                    const bool nd_ = o_[i_] != OOB;                                                 \
                    ok_ = ok_ && (!nd_ || (x_[i_].y == (TAG) && x_[i_].w == (TAG)));                \
                    PT_AT(V0, r) = nd_ ? __uint_as_float(x_[i_].x) : PT_AT(V0, r);                  \
                    PT_AT(V1, r) = nd_ ? __uint_as_float(x_[i_].z) : PT_AT(V1, r);                  \
                }                                                                                   \
            }                                                                                       \
            const bool done_ = __all(ok_);                                                          \
            if (prof && pass_ == 0) { tb_ = __builtin_amdgcn_s_memrealtime(); tfp += tb_ - ts_; tsb += tb_ - ts_; } \
            if (done_) { npass += pass_ + 1; break; }                                               \
            if (pass_ == 0) t0_ = __builtin_amdgcn_s_memrealtime();                                 \
            if ((pass_ & 15) == 15) {                                                               \
                if (__hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)   \
                    live = false;                                                                   \
                else if (__builtin_amdgcn_s_memrealtime() - t0_ > PT_TIMEOUT_TICKS) {               \
                    __hip_atomic_store(a.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   \
                    if (lane == 0) {                    /* diagnostics: rdq_fwi_debug_words */      \
                        a.status[1] = (TAG); a.status[2] = blockIdx.x; a.status[3] = bs;            \
                        a.status[4] = tile; a.status[5] = gl2; a.status[6] = w;                      \
                    }                                                                               \
                    live = false;                                                                   \
                }                                                                                   \
            }                                                                                       \
            __builtin_amdgcn_s_sleep(1);                                                            \
        }                                                                                           \
    }
#define PT_SWEEP_ZERO(V0, V1)                                                                       \
    {                                                                                               \
        /* cells outside the next epoch's dependence cone: zeroed (bounded garbage) */             \
        unsigned rin_ = rin, rcy_ = rcy;                                                            \
        LAUNDER(rin_); LAUNDER(rcy_);                                                               \
        _Pragma("unroll") for (int r = 0; r < R; ++r) {                                             \
            const bool rowin_ = (rin_ >> r) & 1u, rowcy_ = (rcy_ >> r) & 1u;                        \
            const bool keep_ = rowin_ ? keep_in : (rowcy_ && cx);                                   \
            PT_AT(V0, r) = keep_ ? PT_AT(V0, r) : 0.0f;                                             \
            PT_AT(V1, r) = keep_ ? PT_AT(V1, r) : 0.0f;                                             \
        }                                                                                           \
    }
// The same zeroing in fewer instructions (PT_SWEEP_SHADOW).  PT_SWEEP_ZERO compiles to 7 VALU per row: the
// keep mask is rebuilt from 0 / 1 lane values (three selects, an and, a compare) before the two selects
// that zero.  Here the lane's classes are one word (bit 0 keep_in, bit 1 cx) tested against the row's
// scalar class: and, compare, two selects.  Same cells, same values.  (After the sweep, in the forward, it
// changes nothing: 1.0101 -> 1.0102 ms, profiles/r9/kernel_ab_lean_zeroing.jsonl.)
#define PT_SWEEP_ZERO_LEAN(V0, V1)                                                                  \
    {                                                                                               \
        unsigned rin_ = rin, rcy_ = rcy;                                                            \
        LAUNDER(rin_); LAUNDER(rcy_);                                                               \
        const unsigned kc_ = (keep_in ? 1u : 0u) | (cx ? 2u : 0u);                                  \
        _Pragma("unroll") for (int r = 0; r < R; ++r) {                                             \
            const unsigned sel_ = ((rin_ >> r) & 1u) ? 1u : (((rcy_ >> r) & 1u) ? 2u : 0u);         \
            const bool keep_ = (kc_ & sel_) != 0u;                                                  \
            PT_AT(V0, r) = keep_ ? PT_AT(V0, r) : 0.0f;                                             \
            PT_AT(V1, r) = keep_ ? PT_AT(V1, r) : 0.0f;                                             \
        }                                                                                           \
    }

// Hand-off overlap (rdq_fwi_set_handoff_overlap), PT_SWEEP_SHADOW: PT_SWEEP with the dead-cell zeroing
// moved from after the sweep (where all of a SIMD's waves run it at once, on the path to the next step)
// into the first pass's round trip.  The dead cells (not `keep_`) and the halo cells a pass reloads
// (`nd_`) are disjoint sets fixed by the region's masks, so the cells hold the same values at the next
// step whichever comes first.  The first pass's loads of rows 0 .. EN-1 are issued by PT_SWEEP_EARLY
// into registers of their own, XE; then the zeroing; PT_SWEEP_OV issues the rows past EN, checks and
// merges that first pass, and on a stale tag goes on with PT_SWEEP's passes unchanged (same bounded spin,
// status word and `live`).  The compiler barrier keeps the loads ahead of the zeroing, and the register
// pins keep the zeroing ahead of the wait for them.  tei: profile stamp of the first pass's issue.
#define PT_SWEEP_SHADOW(GR, TAG, V0, V1, SG, EN)                                                    \
    {                                                                                               \
        u32x4 xe_[(EN)];                                                                            \
        unsigned long long tei = 0;                                                                 \
        PT_SWEEP_EARLY(GR, xe_, EN)                                                                 \
        PT_SWEEP_ZERO_LEAN(V0, V1)                                                                  \
        _Pragma("unroll") for (int i_ = 0; i_ < RP; ++i_) asm volatile("" : "+v"(V0[i_]), "+v"(V1[i_])); \
        PT_SWEEP_OV(GR, TAG, V0, V1, SG, xe_, EN)                                                   \
    }
#define PT_SWEEP_ROW_OFS(r) ((((rin_) >> (r)) & 1u) ? vo_hx : ((((rcy_) >> (r)) & 1u) ? vo_cx : OOB))
#define PT_SWEEP_EARLY(GR, XE, EN)                                                                  \
    {                                                                                               \
        if (prof) { tei = __builtin_amdgcn_s_memrealtime(); tsa += tei - tm; }                      \
        unsigned rin_ = rin, rcy_ = rcy;                                                            \
        LAUNDER(rin_); LAUNDER(rcy_);                                                               \
        _Pragma("unroll") for (int r = 0; r < (EN); ++r)                                            \
            XE[r] = gran_get(GR, PT_SWEEP_ROW_OFS(r), PT_ROFS(r) * 16);                             \
        asm volatile("" ::: "memory");                                                              \
    }
#define PT_SWEEP_MERGE(X, r, TAG, V0, V1)                                                           \
    {                                                                                               \
        const bool nd_ = PT_SWEEP_ROW_OFS(r) != OOB;                                                \
        ok_ = ok_ && (!nd_ || ((X).y == (TAG) && (X).w == (TAG)));                                  \
        PT_AT(V0, r) = nd_ ? __uint_as_float((X).x) : PT_AT(V0, r);                                 \
        PT_AT(V1, r) = nd_ ? __uint_as_float((X).z) : PT_AT(V1, r);                                 \
    }
#define PT_SWEEP_OV(GR, TAG, V0, V1, SG, XE, EN)                                                    \
    {                                                                                               \
        constexpr int LN_ = R - (EN);                   /* rows of the first pass not issued early */ \
        static_assert(LN_ >= 0 && LN_ <= (SG), "PT_SWEEP_OV: one load group after the early rows"); \
        unsigned long long t0_ = 0;                                                                 \
        const unsigned long long ts_ = tei;                                                         \
        unsigned long long tb_ = tei;                                                               \
        if constexpr (PT_PRIO) __builtin_amdgcn_s_setprio(PT_PRIO_WAIT);                            \
        bool first_ = false;                                                                        \
        if (live) {                                                                                 \
            unsigned rin_ = rin, rcy_ = rcy;                                                        \
            LAUNDER(rin_); LAUNDER(rcy_);                                                           \
            bool ok_ = true;                                                                        \
            u32x4 x_[LN_ > 0 ? LN_ : 1];                                                            \
            _Pragma("unroll") for (int i_ = 0; i_ < LN_; ++i_)                                      \
                x_[i_] = gran_get(GR, PT_SWEEP_ROW_OFS((EN) + i_), PT_ROFS((EN) + i_) * 16);        \
            _Pragma("unroll") for (int r = 0; r < (EN); ++r) PT_SWEEP_MERGE(XE[r], r, TAG, V0, V1)  \
            _Pragma("unroll") for (int i_ = 0; i_ < LN_; ++i_) PT_SWEEP_MERGE(x_[i_], (EN) + i_, TAG, V0, V1) \
            first_ = __all(ok_);                                                                    \
            if (prof) {                                                                             \
                const unsigned long long now_ = __builtin_amdgcn_s_memrealtime();                   \
                tfp += now_ - ts_; tsb += now_ - tb_; tb_ = now_;                                   \
            }                                                                                       \
            if (first_) npass += 1;                                                                 \
            else { t0_ = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_s_sleep(1); }           \
        }                                                                                           \
        if (!first_) PT_SWEEP_PASSES(GR, TAG, V0, V1, SG, 1)                                        \
        if (prof) { tlast = __builtin_amdgcn_s_memrealtime(); tsc += tlast - tb_; }                 \
        if constexpr (PT_PRIO) __builtin_amdgcn_s_setprio(PT_PRIO_SWEPT);                           \
    }

// publish the own-interior border cells of two levels (rows: interior; lanes: the interior
// columns of border rows, else the border columns)
#define PT_PUBLISH(GR, TAG, V0, V1)                                                                 \
    {                                                                                               \
        unsigned rin_ = rin, rby_ = rby;                                                            \
        LAUNDER(rin_); LAUNDER(rby_);                                                               \
        if (gl2) {                                                                                  \
            _Pragma("unroll") for (int r = 0; r < R; ++r) {                                         \
                if (!((rin_ >> r) & 1u)) continue;                                                  \
                gran_put_l2(GR, ((rby_ >> r) & 1u) ? vo_xin : vo_xb, PT_ROFS(r) * 16, (TAG),        \
                            PT_AT(V0, r), PT_AT(V1, r));                                            \
            }                                                                                       \
        } else {                                                                                    \
            _Pragma("unroll") for (int r = 0; r < R; ++r) {                                         \
                if (!((rin_ >> r) & 1u)) continue;                                                  \
                gran_put(GR, ((rby_ >> r) & 1u) ? vo_xin : vo_xb, PT_ROFS(r) * 16, (TAG),           \
                         PT_AT(V0, r), PT_AT(V1, r));                                               \
            }                                                                                       \
        }                                                                                           \
    }

// The first hand-off pass of an epoch is issued `a.sweep_delay` ticks after the wave's publish: a pass
// issued at once mostly finds the neighbours' granules not yet there (1.9 passes per epoch, each an L2
// round trip of ~0.7 us) and a failed pass's loads sit in the CU's memory queue ahead of the next
// pass's.  Measured at configs[1] (profiles/r6/sweep_delay_*): 0.25 us takes the forward 1.371 ->
// 1.321 ms and the adjoint 1.688 -> 1.647 ms; 1 us is flat, 2 us slower.  With the wave priorities and
// the barrier-free adjoint (profiles/r6/delay_retune_ab.txt): forward best at 0.15 us (1.210 -> 1.196
// ms against 0.25), adjoint at 0 (1.588 -> 1.562 ms), the defaults.  Timing only: results are
// identical for every delay.
#define PT_SWEEP_DELAY()                                                                            \
    if (a.sweep_delay > 0) {                                                                        \
        const unsigned long long d0_ = __builtin_amdgcn_s_memrealtime();                            \
        while (__builtin_amdgcn_s_memrealtime() - d0_ < (unsigned long long)a.sweep_delay)          \
            __builtin_amdgcn_s_sleep(1);                                                            \
    }

#define PT_PROF(ACC)                                                                                \
    if (prof) { const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); ACC += now_ - tm; tm = now_; }
// Phase counters of the profiled build (10 ns ticks).  tsw / tst / tpb: hand-off wait, steps, publish
// (the granule stores' issue); tgr: the adjoint's deferred gradient.  The wait splits, with no tick lost
// between them (tsw = tsa + tsb + tsc + tsd), into tsa: publish end -> first sweep pass issued (delay,
// scalar loads), tsb: the first pass's round trip, tsc: later passes, tsd: after the sweep (dead-cell
// zeroing, deferred history stores, xm_put, FWD_RECORD / ADJ_ISSUE) and whatever else the wait counter
// took (launch prologue, last epoch).  tfp: first pass issue -> checked (= tsb unless work overlaps it).
#define PT_PROF_VARS                                                                                \
    unsigned long long tsw = 0, tst = 0, tpb = 0, tgr = 0, tm = prof ? __builtin_amdgcn_s_memrealtime() : 0; \
    unsigned long long tsa = 0, tsb = 0, tsc = 0, tsd = 0, tlast = 0;                               \
    unsigned long long tfp = 0, npass = 0;                /* first-pass latency, sweep passes */
// the wait counter's stamp: its part since the sweep ended (or all of it, without a sweep) is the tail
#define PT_PROF_TAIL                                                                                \
    if (prof) {                                                                                     \
        const unsigned long long now_ = __builtin_amdgcn_s_memrealtime();                           \
        tsw += now_ - tm; tsd += now_ - (tlast ? tlast : tm);                                       \
        tm = now_; tlast = 0;                                                                       \
    }
// summary words [0..10] and the wave's record {wait, steps, publish + gradient, a, b, c, d, gradient}
#define PT_PROF_FLUSH                                                                               \
    if (prof && lane == 0) {                                                                        \
        atomicAdd(prof + 0, tsw); atomicAdd(prof + 1, tst); atomicAdd(prof + 2, tpb + tgr); atomicAdd(prof + 3, 1ull); \
        atomicAdd(prof + 4, tfp); atomicAdd(prof + 5, npass);                                       \
        atomicAdd(prof + 6, tsa); atomicAdd(prof + 7, tsb); atomicAdd(prof + 8, tsc); atomicAdd(prof + 9, tsd); \
        atomicAdd(prof + 10, tgr);                                                                  \
        if (blockIdx.x < PROF_WAVES / 16) {                                                         \
            unsigned long long *raw = prof + PROF_RAW + ((size_t)blockIdx.x * 16 + w) * PROF_REC;   \
            raw[0] = tsw; raw[1] = tst; raw[2] = tpb + tgr; raw[3] = tsa; raw[4] = tsb; raw[5] = tsc; \
            raw[6] = tsd; raw[7] = tgr;                                                             \
        }                                                                                           \
    }

// Re-materialise a wave-uniform value inside the time loop: stops the compiler from hoisting the
// per-row compares on it out of the loop as live 64-bit lane masks (which spill to VGPR lanes and
// cost v_readlane pairs in every step).
#define LAUNDER(x)                                                                                  \
    do {                                                                                            \
        x = __builtin_amdgcn_readfirstlane(x);   /* uniform by construction: never a VGPR->SGPR copy */ \
        asm volatile("" : "+s"(x));                                                                 \
    } while (0)

struct FwdPtArgs {
    TBGeo g;
    const float *coeffs;                 // alpha, temp1, temp2 at 0, 1, 2 x cstride; beta at 4
    const float *wav;                    // [nt] fp32 wavelet
    float *hist;                         // history base (slot j = P_{j-1}) or nullptr (no-grad)
    float *seis;
    unsigned long long *gran;
    unsigned *status;
    unsigned long long *prof;            // nullable: [0] hand-off, [1] steps, [2] publish (10 ns ticks), [3] waves
    int nt;
    int xcd_mode;                        // 1: XCD-local slices (pt_assign), 0: all hand-offs write-through
    int sweep_delay;                     // s_memrealtime ticks (10 ns) between an epoch's publish and its first sweep pass
    int srole;                           // source role (rdq_fwi_set_source_role): 1 the plain and the source/receiver
                                         // waves run loops of their own, 0 every wave the generic loop
};

// One forward step P_{n+1} = temp1 P_n - temp2 P_{n-1} + alpha N(P_n) (+ source), pde.py:79-81, on
// packed fp32: a wave's 8 rows are held as 4 row PAIRS {r, r+4} (float2 = one VGPR pair), so every
// add / mul of the stencil is one v_pk_*_f32 for two rows (IEEE-identical to the scalar ops, same
// operation order per row).  With this pairing the vertical neighbours of pair i are pairs i-1 /
// i+1 / i-2 / i+2 except at the slab ends, where four pairs are assembled from the halo rows.  The
// horizontal taps stay per-row DPP lane shifts (DPP has no packed form).
// (one descriptor per epoch, HFe = slot n0 + 2, and the step's slot as the scalar offset: no
// per-step 64-bit address arithmetic; the lanes' offsets stay OOB for cells the wave does not own)
#define FWD_HIST(V, N)                                                                              \
    {                                                                                               \
        const int so_ = ((N) - n0) * L4;                                                            \
        _Pragma("unroll") for (int r = 0; r < R; ++r)                                               \
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(PT_AT(V, r)), HFe, hv[r], so_, CP_NT); \
    }
// the receiver row's values of the epoch's steps n0 .. n0+T-1 (after the hand-off sweep): one buffer
// store per recorded step (lanes without a receiver at an OOB offset, the record row as the scalar
// offset), the per-column receiver lists only where a column has several
#define FWD_RECORD                                                                                  \
    if constexpr (RL_SR >= 0) {                      /* source role: every step exists and is recorded */ \
        _Pragma("unroll") for (int t = 0; t < T; ++t) {                                             \
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rv[t]), SKR, vrec, (n0 + t) * ng4, 0); \
            unsigned rm_ = rmulti;                                                                  \
            LAUNDER(rm_);                                                                           \
            if (rm_ && rec) {                                                                       \
                float *SK = a.seis + ((size_t)bs * g.nrec + n0 + t) * g.ng;                         \
                for (int j = rs + 1; j < re; ++j) SK[g.rcv_list[j]] = rv[t];                        \
            }                                                                                       \
        }                                                                                           \
    } else if constexpr (!RL_PLAIN) {                                                               \
        int rrw_ = rrow;                                                                            \
        LAUNDER(rrw_);                                                                              \
        if (rrw_ >= 0) {                                                                            \
            _Pragma("unroll") for (int t = 0; t < T; ++t) {                                         \
                const int n = n0 + t;                                                               \
                const int ri_ = n < a.nt ? rec_index(n, g.st) : -1;                                 \
                if (ri_ >= 0) {                                                                     \
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rv[t]), SKR, vrec, ri_ * ng4, 0); \
                    unsigned rm_ = rmulti;                                                          \
                    LAUNDER(rm_);                                                                   \
                    if (rm_ && rec) {                        /* several receivers in one column */  \
                        float *SK = a.seis + ((size_t)bs * g.nrec + ri_) * g.ng;                    \
                        for (int j = rs + 1; j < re; ++j) SK[g.rcv_list[j]] = rv[t];                \
                    }                                                                               \
                }                                                                                   \
            }                                                                                       \
        }                                                                                           \
    }

// Row r of a row-pair array.  Stacked pairs {i, i+RP} (PT_MIR false: the exact-order adjoint) or
// mirrored pairs {i, R-1-i} (PT_MIR true: the barrier-free kernels).  In the mirrored form the four
// boundary rows 0, 1, R-2, R-1 are pairs 0 and 1 alone, so a step can finish (and publish) them
// before its interior pairs; the vertical neighbours of pair i are still pairs i-1 / i+1 / i-2 /
// i+2 (the .y half runs the other way, and the stencil's sums are symmetric), except at the slab
// ends (halo rows) and in the middle, where a pair meets itself swapped.
template <int RP, bool M>
__device__ constexpr int pt_pair(int r) { return M ? (r < RP ? r : 2 * RP - 1 - r) : r % RP; }
template <int RP, bool M>
__device__ constexpr int pt_half(int r) { return M ? (r < RP ? 0 : 1) : r / RP; }
#define PT_AT(V, r) V[pt_pair<RP, PT_MIR>(r)][pt_half<RP, PT_MIR>(r)]
__device__ __forceinline__ f32x2 swp(f32x2 v) { return f32x2{v.y, v.x}; }
// vertical neighbours (rows -1, +1, -2, +2) of mirrored pair i of X; E1 = rows {-1, R}, E2 = {-2, R+1}
#define MIR_VERT(X, i, m1, p1, m2, p2)                                                              \
    const f32x2 m1 = (i) >= 1 ? X[(i) - 1] : E1;                                                    \
    const f32x2 p1 = (i) <= RP - 2 ? X[(i) + 1] : swp(X[RP - 1]);                                   \
    const f32x2 m2 = (i) >= 2 ? X[(i) - 2] : ((i) == 1 ? E1 : E2);                                  \
    const f32x2 p2 = (i) <= RP - 3 ? X[(i) + 2] : ((i) == RP - 2 ? swp(X[RP - 1]) : swp(X[RP - 2]));

// Barrier-free forward step: the halo-free work of every pair (DPP shifts, time
// terms) first, then the wait for the neighbours' boundary rows, the two boundary pairs, their
// publication for the next step, and the interior pairs after it.  Per row the operations and
// their order are the reference's (bit-exact).
#define FWD_PAIRS_NB(CUR, PRV, LO, HI)                                                                        \
    {                                                                                               \
        _Pragma("unroll") for (int i = (LO); i < (HI); ++i) {                                        \
            MIR_VERT(CUR, i, m1, p1, m2, p2)                                                        \
            f32x2 s1 = m1 + p1; s1 = s1 + xl1[i]; s1 = s1 + xr1[i];                                 \
            const f32x2 la = kC2 * s1;                                                              \
            f32x2 s2 = m2 + p2;                        /* x -+ 2 taps: fused v_add_f32_dpp */       \
            s2.x = s2.x + dpp_shr1(xl1[i].x); s2.y = s2.y + dpp_shr1(xl1[i].y);                     \
            s2.x = s2.x + dpp_shl1(xr1[i].x); s2.y = s2.y + dpp_shl1(xr1[i].y);                     \
            const f32x2 l2 = kC3 * s2; const f32x2 lap = la + l2;                                   \
            const f32x2 a3 = A[i] * lap;                                                            \
            PRV[i] = tt[i] + a3;                                                                    \
        }                                                                                           \
        if constexpr (RL_SR >= 0) {                  /* source role: the one row's pair is RL_SR */ \
            if constexpr ((HI) > (LO) && SRP >= (LO) && SRP < (HI)) {                               \
                float wt_ = wv[t];                                                                  \
                asm volatile("" : "+s"(wt_));                                                       \
                const float add = scol ? bsrc * wt_ : -0.0f;                                        \
                PRV[SRP] = PRV[SRP] + (shalf ? f32x2{-0.0f, add} : f32x2{add, -0.0f});              \
            }                                                                                       \
        } else if constexpr (!RL_PLAIN) {            /* (plain role: no source row) */              \
        unsigned sm0_ = (HI) > (LO) ? smask : 0u;                                                  \
        LAUNDER(sm0_);                               /* scalar branch; nothing of it hoisted */     \
        if (sm0_) {                                  /* pde.py:80-81 (uniform: source row waves) */ \
            float wt_ = wv[t];                                                                      \
            asm volatile("" : "+s"(wt_));                                                           \
            const float add = scol ? bsrc * wt_ : -0.0f;                                            \
            unsigned one_ = s1row;                                                                  \
            LAUNDER(one_);                                                                          \
            if (one_) {                                                                             \
                const f32x2 av = shalf ? f32x2{-0.0f, add} : f32x2{add, -0.0f};                     \
                int sp_ = spair;                                                                    \
                LAUNDER(sp_);                                                                       \
                _Pragma("unroll") for (int i = (LO); i < (HI); ++i)                                  \
                    if (i == sp_) PRV[i] = PRV[i] + av;                                             \
            } else {                                                                                \
                unsigned sm_ = smask;                                                               \
                LAUNDER(sm_);                                                                       \
                _Pragma("unroll") for (int r = 0; r < R; ++r)                                       \
                    if (pt_pair<RP, PT_MIR>(r) >= (LO) && pt_pair<RP, PT_MIR>(r) < (HI) && ((sm_ >> r) & 1u)) \
                        PT_AT(PRV, r) = PT_AT(PRV, r) + add;                                        \
            }                                                                                       \
        }                                                                                           \
        }                                                                                           \
    }
#define FWD_STEP_NB(CUR, PRV)                                                                       \
    {                                                                                               \
        u32x2 f_;                                                                                   \
        f32x2 E1, E2;                                                                               \
        xm_load<NW>(xm, n & 1, w, lane, f_, E1, E2);                                                \
        f32x2 xl1[RP], xr1[RP], tt[RP];                                                             \
        _Pragma("unroll") for (int i = 0; i < RP; ++i) {                                             \
            const f32x2 c = CUR[i];                                                                 \
            xl1[i] = f32x2{dpp_shr1(c.x), dpp_shr1(c.y)};                                           \
            xr1[i] = f32x2{dpp_shl1(c.x), dpp_shl1(c.y)};                                           \
            f32x2 a1 = C1[i] * c; const f32x2 a2 = C2v[i] * PRV[i]; a1 = a1 - a2;                   \
            tt[i] = a1;                                                                             \
            asm volatile("" : "+v"(tt[i]));          /* computed here, not sunk past the wait */    \
        }                                                                                           \
        xm_wait<NW>(xm, n & 1, w, lane, (unsigned)n + 1u, f_, E1, E2, a.status, live);              \
        FWD_PAIRS_NB(CUR, PRV, 0, 2)                                                                          \
        if (t + 1 < T) xm_put<NW>(xm, (n + 1) & 1, w, lane, (unsigned)n + 2u, PRV[0], PRV[1]);      \
        __builtin_amdgcn_s_setprio(PT_PRIO_BODY);                                                   \
        FWD_PAIRS_NB(CUR, PRV, 2, RP)                                                                         \
        if constexpr (RL_PLAIN) {                    /* steady epoch of a history-keeping launch */ \
            if (t + 1 < T) FWD_HIST(PRV, n)                                                         \
        } else if (a.hist && (t + 1 < T || e + 1 == nep)) FWD_HIST(PRV, n)                          \
        if constexpr (RL_SR >= 0) {                  /* source role: the receiver row is the source row */ \
            rv[t] = shalf ? PRV[SRP].y : PRV[SRP].x;                                                \
        } else if constexpr (!RL_PLAIN) {            /* (plain role: no receiver row) */            \
            int rr_ = rrow;                                                                         \
            LAUNDER(rr_);                                                                           \
            if (rr_ >= 0) {                          /* receiver row: value kept, stored per epoch */ \
                int rp_ = rpair;                                                                    \
                LAUNDER(rp_);                                                                       \
                f32x2 v_ = PRV[0];                                                                  \
                _Pragma("unroll") for (int i = 1; i < RP; ++i) if (i == rp_) v_ = PRV[i];            \
                rv[t] = rhalf ? v_.y : v_.x;                                                        \
            }                                                                                       \
        }                                                                                           \
    }

template <int T, int NW, int RW, bool PROF>
__global__ __launch_bounds__(64 * NW) void k_fwd_pt(FwdPtArgs a)
{
    unsigned long long *const prof = PROF ? a.prof : nullptr;   // phase counters: profiled build only
    constexpr bool PT_MIR = true;                         // mirrored pairs (barrier-free exchange:
                                                          // 1.364 -> 1.287 ms at configs[1])
    constexpr bool PT_PRIO = true;                        // wave priorities (PT_PRIO_*)
    __shared__ XmBox<NW> xm;                              // the waves' inboxes (xm_*)
    const TBGeo &g = a.g;
    PT_REGION_INIT(NW, RW)
    const float *AL = a.coeffs + (size_t)b * g.slice;
    f32x2 A[RP], C1[RP], C2v[RP], P0[RP], P1[RP];         // row pairs {r, r+RP}: PT_AT(X, r)
    const f32x2 kC2 = {C2, C2}, kC3 = {C3, C3};
    unsigned smask = 0;
    int rrow = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int gz = wrap_row(uz0 + r, g.Hp);
        const int o = gz * g.ld + gx;
        PT_AT(A, r) = AL[o]; PT_AT(C1, r) = AL[g.cstride + o]; PT_AT(C2v, r) = AL[2 * g.cstride + o];
        PT_AT(P0, r) = 0.0f; PT_AT(P1, r) = 0.0f;         // P_{-1} = P_0 = 0 (pde.py:74-75)
        if (gz == g.isz) smask |= 1u << r;
        if (gz == g.igz && ((rin >> r) & 1u)) rrow = r;
    }
    smask = __builtin_amdgcn_readfirstlane(smask);        // wave-uniform (row-only): scalar branches,
    rrow = __builtin_amdgcn_readfirstlane(rrow);          // no per-lane masks held across the loop
    const int isx = g.isx[s];
    const bool scol = gx == isx;
    const float bsrc = (smask != 0) ? AL[4 * g.cstride + (size_t)g.isz * g.ld + isx] : 0.0f;

    int rs = 0, re = 0, rcv0 = -1;
    if (rrow >= 0) {
        rs = g.rcv_start[gx]; re = g.rcv_start[gx + 1];
        rcv0 = rs < re ? g.rcv_list[rs] : -1;             // the (usually only) receiver of this column
    }
    const bool rec = rrow >= 0 && xin && rcv0 >= 0;
    const unsigned rmulti = __any(re - rs > 1);           // wave-uniform: a column with several receivers
    const __amdgpu_buffer_rsrc_t SKR = rsrc_of(a.seis + (size_t)bs * g.nrec * g.ng);   // FWD_RECORD
    const int vrec = rec ? rcv0 * 4 : OOB, ng4 = g.ng * 4;
    // source / receiver rows as (row pair, half): the step touches one pair, not all eight rows
    const unsigned s1row = smask != 0 && (smask & (smask - 1u)) == 0;   // one source row in the slab
    const int sr1 = smask ? __builtin_ctz(smask) : 0;
    // wave-uniform by construction; readfirstlane makes that visible to the compiler (LAUNDER "+s")
    const int spair = __builtin_amdgcn_readfirstlane(PT_MIR ? (sr1 < RP ? sr1 : R - 1 - sr1) : sr1 % RP);
    const int rpair = __builtin_amdgcn_readfirstlane(rrow < 0 ? 0 : PT_MIR ? (rrow < RP ? rrow : R - 1 - rrow) : rrow % RP);
    const bool shalf = sr1 >= RP, rhalf = rrow >= RP;     // the half is r >= RP in both pairings
    float rv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) rv[t] = 0.0f;
    const size_t L = g.level;
    const int L4 = (int)(L * 4);                          // bytes per history slot (< 2 GB: resident surveys)
    int hv[R];                                            // history store offset of (row, lane), OOB if not own
#pragma unroll
    for (int r = 0; r < R; ++r) hv[r] = (((rin >> r) & 1u) && xin) ? (PT_ROFS(r) + gx) * 4 : OOB;
    const int nep = (a.nt + T - 1) / T;
    bool live = true;
    PT_PROF_VARS
    // The next epoch's wavelet samples (FWD_ISSUE) are scalar loads issued right after the publish: the
    // source row's first step no longer waits for them behind the deferred history stores.
    float wv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) wv[t] = wav_s(a.wav, min(t, a.nt - 1));
    __builtin_amdgcn_s_waitcnt(0x0F70);                   // vmcnt(0)
#define FWD_ISSUE _Pragma("unroll") for (int t = 0; t < T; ++t) wv[t] = wav_s(a.wav, min(n0 + T + t, a.nt - 1));
    xm_init<NW>(xm, w, lane);                             // no flag matches a tag until written
    __syncthreads();
    xm_put<NW>(xm, 0, w, lane, 1u, f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f});   // P_0 = 0, step 0's tag
// One epoch e, for the role (RL_PLAIN, RL_SR) in scope.  A role's epoch is steady (never the last: all T
// steps exist, the hand-off follows) and belongs to a history-keeping launch.  After the steps: keep
// "P1 = newest"; publish; the next epoch's wavelet samples (scalar loads, wav_s: their latency hides in the
// delay and the sweep, and no vector op waits on them); the sweep; the epoch's last step's history (own
// cells: the sweep reloads halo cells only); the next step's boundary rows, with the halo cells the sweep
// reloaded; the epoch's receiver values.
#define FWD_EPOCH                                                                                   \
    {                                                                                               \
        const int n0 = e * T;                                                                       \
        const __amdgpu_buffer_rsrc_t HFe = rsrc_of(a.hist + (size_t)(n0 + 2) * L + so);   /* FWD_HIST */ \
        PT_PROF_TAIL                                                                                \
        _Pragma("unroll") for (int t = 0; t < T; ++t) {                                             \
            const int n = n0 + t;                                                                   \
            if (!RL_PLAIN && n >= a.nt) break;                                                      \
            if (t & 1) FWD_STEP_NB(P0, P1)                                                          \
            else FWD_STEP_NB(P1, P0)                                                                \
        }                                                                                           \
        if (T & 1) {                                                                                \
            _Pragma("unroll") for (int i = 0; i < RP; ++i) { const f32x2 tmp = P0[i]; P0[i] = P1[i]; P1[i] = tmp; } \
        }                                                                                           \
        PT_PROF(tst)                                                                                \
        if (RL_PLAIN || e + 1 < nep) {                                                              \
            const unsigned tag = (unsigned)(e + 1);                                                 \
            const __amdgpu_buffer_rsrc_t GR = rsrc_of(a.gran + (size_t)(2 * ((e + 1) & 1)) * L + 2 * so); \
            PT_PUBLISH(GR, tag, P0, P1)                                                             \
            PT_PROF(tpb)                                                                            \
            if constexpr (!RL_PLAIN || RL_SR >= 0) { FWD_ISSUE }                                    \
            PT_SWEEP_DELAY()                                                                        \
            PT_SWEEP(GR, tag, P0, P1, R)                                                            \
            if (RL_PLAIN || a.hist) FWD_HIST(P1, n0 + T - 1)                                        \
            xm_put<NW>(xm, (n0 + T) & 1, w, lane, (unsigned)(n0 + T) + 1u, P1[0], P1[1]);           \
        }                                                                                           \
        FWD_RECORD                                                                                  \
    }
    // Source role (rdq_fwi_set_source_role), at PT_ROLES_T steps per epoch and 6 rows per wave, in a launch
    // that keeps its history: a wave branches once, here, into a loop of its own over every epoch but the
    // last.  A plain wave (no source row, no receiver row) runs steps with no source / receiver / a.hist /
    // n >= nt test and loads no wavelet samples; the source/receiver wave (its slab owns the one source
    // row, and that row is its receiver row: isz == igz; every step recorded, the host's test) runs the
    // plain body plus its own work with the row's pair a compile-time constant: one packed add of the
    // source term into that pair, the receiver value from it, FWD_ISSUE and FWD_RECORD.  Every other wave
    // (a source row's halo copy, source and receiver in different rows) and the last epoch of all run the
    // generic loop.  Mailbox, publish, sweep, zeroing, tags and priorities are the same text, and per cell
    // the operations and their order: results are bit for bit those of mode 0.
    int e = 0;
    constexpr bool RL_PLAIN = false;                      // the generic role (shadowed in the role loops)
    constexpr int RL_SR = -1, SRP = 0;                    // source role: the row's pair (SRP = max(RL_SR, 0))
    if constexpr (T == PT_ROLES_T && RW == PT_SROLE_RW) {
        int role = 0;                                     // 0 generic, 1 plain, 2 + pair: source/receiver
        if (a.srole && a.hist) {
            if (smask == 0 && rrow < 0) role = 1;
            else if (s1row && rrow == sr1) role = 2 + spair;
        }
        role = __builtin_amdgcn_readfirstlane(role);
        if (role == 1) {
            constexpr bool RL_PLAIN = true;
            for (; e + 1 < nep; ++e) FWD_EPOCH            // (no source row: the generic epoch reads no sample)
        } else if (role == 2) {
            constexpr bool RL_PLAIN = true;
            constexpr int RL_SR = 0, SRP = 0;
            for (; e + 1 < nep; ++e) FWD_EPOCH
        } else if (role == 3) {
            constexpr bool RL_PLAIN = true;
            constexpr int RL_SR = 1, SRP = 1;
            for (; e + 1 < nep; ++e) FWD_EPOCH
        } else if (role == 4) {
            constexpr bool RL_PLAIN = true;
            constexpr int RL_SR = 2, SRP = 2;
            for (; e + 1 < nep; ++e) FWD_EPOCH
        }
        // Where the loops meet the samples must stay scalars: without this the compiler merges them in VGPRs
        // and the generic step's SGPR constraint on wv[t] does not compile ("illegal VGPR to SGPR copy").
        // Uniform by construction; once per launch.
#pragma unroll
        for (int t = 0; t < T; ++t) wv[t] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wv[t])));
    }
    for (; e < nep; ++e) FWD_EPOCH
#undef FWD_EPOCH
#undef FWD_ISSUE
    PT_PROF_TAIL
    PT_PROF_FLUSH
}

#undef FWD_HIST
#undef FWD_RECORD

// The adjoint keeps the forward's row-pair packing (PT_AT(V, r) = V[r % RP][r / RP]): every add /
// mul / fma of the step and of the gradient is one v_pk_*_f32 for two rows.

struct AdjPtArgs {
    TBGeo g;
    const float *coeffs;                 // alpha, temp1, temp2, kappa at 0..3 x cstride
    const float *wav;
    const float *hist;                   // slot k = P_{k-1}
    const float *dseis;
    float *gA;                           // [B][ns][Hp][ld]
    double *gk_part;                     // [B*ns][nblk]
    float *gbeta;                        // [B*ns]
    unsigned long long *gran;
    unsigned *status;
    unsigned long long *prof;            // nullable, as FwdPtArgs
    int nt, nblk;
    int xcd_mode;
    int sweep_delay;                     // as FwdPtArgs
    int roles;                           // wave roles: 0 every wave runs the generic loop, 1 plain waves their own
};

__device__ __forceinline__ float bload_nt(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, CP_NT));
}

// P_{k-1}, rows uz0-2 .. uz0+9 of one step: slab rows 0..7 as row pairs PC[i] = {i, i+4}, the
// stencil's halo rows as PH = {-2, -1, 8, 9}.  HR = the epoch's history descriptor, SOFF = the
// step's slot offset inside it (bytes): one 64-bit descriptor per epoch, not per step.
#define ADJ_PLOAD(PC, PH, HR, SOFF)                                                                 \
    {                                                                                               \
        const int so_ = (SOFF);                                                                     \
        _Pragma("unroll") for (int i = 0; i < RP; ++i) {                                             \
            PC[i].x = bload_nt(HR, pv[i + 2], so_);                                                 \
            PC[i].y = bload_nt(HR, pv[i + 6], so_);                                                 \
        }                                                                                           \
        PH[0] = bload_nt(HR, pv[0], so_); PH[1] = bload_nt(HR, pv[1], so_);                         \
        PH[2] = bload_nt(HR, pv[10], so_); PH[3] = bload_nt(HR, pv[11], so_);                       \
    }

// vertical neighbours of row pair i in a row-pair field X whose four outer rows are in
// eU1 = {-1, RP-1}, eU2 = {-2, RP-2}, eD1 = {RP, R}, eD2 = {RP+1, R+1}
#define PAIR_VERT(X, i, m1, p1, m2, p2)                                                             \
    const f32x2 m1 = (i) >= 1 ? X[(i) - 1] : eU1;                                                   \
    const f32x2 p1 = (i) <= RP - 2 ? X[(i) + 1] : eD1;                                              \
    const f32x2 m2 = (i) >= 2 ? X[(i) - 2] : ((i) == 1 ? eU1 : eU2);                                \
    const f32x2 p2 = (i) <= RP - 3 ? X[(i) + 2] : ((i) == RP - 2 ? eD1 : eD2);

// gradient accumulation of one step (interior rows are the ones stored; every row of a wave that
// has interior rows is computed: no per-row branch).  CU = L_{k+1}, LN = L_k, P / PH = P_{k-1}.
//   gA_s += L_k (2c1 P + c2 S1(P) + c3 S2(P)),  GK += P (L_{k+1} - L_k)  (x K once at the end),
//   gbeta[s] += L_k(src) w[k-1]
#define ADJ_GRAD(CU, LN, P, PH, WK)                                                                 \
    if (grad) {                                                                                     \
        const f32x2 eU1 = {PH[1], P[RP - 1].x}, eU2 = {PH[0], P[RP - 2].x};                         \
        const f32x2 eD1 = {P[0].y, PH[2]}, eD2 = {P[1].y, PH[3]};                                   \
        _Pragma("unroll") for (int i = 0; i < RP; ++i) {                                             \
            PAIR_VERT(P, i, m1, p1, m2, p2)                                                         \
            const f32x2 c = P[i];                                                                   \
            const f32x2 xl1 = {dpp_shr1(c.x), dpp_shr1(c.y)}, xr1 = {dpp_shl1(c.x), dpp_shl1(c.y)}; \
            f32x2 s1 = m1 + p1; s1 = s1 + xl1; s1 = s1 + xr1;                                       \
            f32x2 s2 = m2 + p2;                        /* x -+ 2 taps: fused v_add_f32_dpp */       \
            s2.x = s2.x + dpp_shr1(xl1.x); s2.y = s2.y + dpp_shr1(xl1.y);                           \
            s2.x = s2.x + dpp_shl1(xr1.x); s2.y = s2.y + dpp_shl1(xr1.y);                           \
            const f32x2 l = LN[i];                                                                  \
            f32x2 lap = kC2 * s1; const f32x2 lq = kC3 * s2; lap = lap + lq;                        \
            f32x2 d = kC1X2 * c; d = d + lap;                                                       \
            const f32x2 cc = l * d;                                                                 \
            GA[i] = GA[i] + cc;                                                                     \
            f32x2 kk = KP[i] * c; const f32x2 dl = CU[i] - l; kk = kk * dl;   /* fp32 term */       \
            if (xin) {                                                       /* fp64 sum */        \
                if ((rin >> i) & 1u) ksum += (double)kk.x;                                          \
                if ((rin >> (i + RP)) & 1u) ksum += (double)kk.y;                                   \
            }                                                                                       \
        }                                                                                           \
        if (srow >= 0) {                             /* gbeta: the source cell's lane only */      \
            int sr_ = srow;                                                                         \
            LAUNDER(sr_);                                                                           \
            float ls_ = 0.0f;                                                                       \
            _Pragma("unroll") for (int r = 0; r < R; ++r) if (r == sr_) ls_ = PT_AT(LN, r);         \
            const float gb = scol ? ls_ * (WK) : -0.0f;                                             \
            gbacc = gbacc + gb;                                                                     \
        }                                                                                           \
    }

// one adjoint step k: CUR = L_{k+1}, PRV = L_{k+2} -> L_k; P / PH = P_{k-1}; the
// next step's P_{k-2} is prefetched into PN / PHN.  The gradient of the epoch's last step is
// deferred past the publish (see k_adj_pt).
#define ADJ_STEP(CUR, PRV, P, PH, PN, PHN)                                                          \
    {                                                                                               \
        if (t + 1 < T) ADJ_PLOAD(PN, PHN, HRe, (T - 2 - t) * L4)                                    \
        const float dcur = dv[t];                                                                   \
        f32x2 q[RP];                                                                                \
        _Pragma("unroll") for (int i = 0; i < RP; ++i) q[i] = A[i] * CUR[i];                         \
        const Halo4 h4 = exchange_nw<NW>(xch, j & 1, w, lane, q[0].x, q[1].x, q[RP - 2].y, q[RP - 1].y); \
        const f32x2 eU1 = {h4.u1, q[RP - 1].x}, eU2 = {h4.u2, q[RP - 2].x};                         \
        const f32x2 eD1 = {q[0].y, h4.d1}, eD2 = {q[1].y, h4.d2};                                   \
        _Pragma("unroll") for (int i = 0; i < RP; ++i) {                                             \
            PAIR_VERT(q, i, m1, p1, m2, p2)                                                         \
            const f32x2 c = q[i];                                                                   \
            const f32x2 xl1 = {dpp_shr1(c.x), dpp_shr1(c.y)}, xr1 = {dpp_shl1(c.x), dpp_shl1(c.y)}; \
            f32x2 n1 = m1 + p1; n1 = n1 + xl1; n1 = n1 + xr1;                                       \
            f32x2 n2 = m2 + p2;                        /* x -+ 2 taps: fused v_add_f32_dpp */       \
            n2.x = n2.x + dpp_shr1(xl1.x); n2.y = n2.y + dpp_shr1(xl1.y);                           \
            n2.x = n2.x + dpp_shl1(xr1.x); n2.y = n2.y + dpp_shl1(xr1.y);                           \
            f32x2 nb = kC2 * n1; const f32x2 nb2 = kC3 * n2; nb = nb + nb2;                         \
            f32x2 l = T1v[i] * CUR[i]; const f32x2 l2 = T2v[i] * PRV[i]; l = l - l2; l = l + nb;     \
            PRV[i] = l;                                                                             \
        }                                                                                           \
        if (rrow >= 0 && rec_index(k - 1, g.st) >= 0) {   /* uniform: the receiver row's wave */    \
            int rr_ = rrow;                                                                         \
            LAUNDER(rr_);                                                                           \
            _Pragma("unroll") for (int r = 0; r < R; ++r)                                           \
                if (r == rr_) PT_AT(PRV, r) = PT_AT(PRV, r) + dcur;   /* -0 off the receivers */     \
        }                                                                                           \
        if (t + 1 < T || last) ADJ_GRAD(CUR, PRV, P, PH, wv[t])                                     \
    }

// Adjoint, persistent, in the oracle's exact fp32 operation order (rdq_fwi_set_variant flag 2: the
// bitwise tests; the default build is k_adj_pr below).  Per step k = nt..1:
//   L_k = T1 L_{k+1} - T2 L_{k+2} + (c2 N1(A L_{k+1}) + c3 N2(A L_{k+1})) [+ R^T dseis[k-1]]
//   gA_s += L_k (2c1 P_{k-1} + c2 S1(P_{k-1}) + c3 S2(P_{k-1})),  gk += (K P_{k-1})(L_{k+1} - L_k),
//   gbeta[s] += L_k(src) w[k-1]        (interior cells; accumulators in registers for all nt steps)
// P_{k-1} comes from the history: each wave loads its rows +-2 one step ahead into alternating
// register arrays and needs no LDS exchange for it.  Per epoch of T steps: steps, publish of the
// border, then the LAST step's gradient (it needs no neighbour data: the interior L_k, L_{k+1} and
// the wave's own history rows), and only then the hand-off sweep — the gradient's VALU work fills
// the time the neighbours' granules take to arrive.
template <int T, int NW, bool PROF>
__global__ __launch_bounds__(64 * NW) void k_adj_pt(AdjPtArgs a)
{
    unsigned long long *const prof = PROF ? a.prof : nullptr;   // phase counters: profiled build only
    constexpr bool PT_MIR = false;                        // stacked pairs {i, i+4} (ADJ_PLOAD / ADJ_GRAD)
    constexpr bool PT_PRIO = false;                       // (barrier-synchronised steps: PT_PRIO_*)
    __shared__ float xch[2][NW][4][64];
    __shared__ double red[64 * NW];
    const TBGeo &g = a.g;
    PT_REGION_INIT(NW, TB_R)
    const float *AL = a.coeffs + (size_t)b * g.slice;
    f32x2 A[RP], T1v[RP], T2v[RP], KP[RP], L0[RP], L1[RP], GA[RP];
    const f32x2 kC2 = {C2, C2}, kC3 = {C3, C3}, kC1X2 = {C1X2, C1X2};
    int srow = -1, rrow = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int gz = wrap_row(uz0 + r, g.Hp);
        const int o = gz * g.ld + gx;
        PT_AT(A, r) = AL[o]; PT_AT(T1v, r) = AL[g.cstride + o]; PT_AT(T2v, r) = AL[2 * g.cstride + o];
        PT_AT(KP, r) = AL[3 * g.cstride + o];
        PT_AT(L0, r) = 0.0f; PT_AT(L1, r) = 0.0f;         // L_{nt+1} = L_{nt+2} = 0
        PT_AT(GA, r) = 0.0f;
        if (gz == g.isz && ((rin >> r) & 1u)) srow = r;
        if (gz == g.igz) rrow = r;
    }
    const bool scol = xin && gx == g.isx[s];
    // residual of this lane's column: one receiver's dseis, or several receivers' folded sum
    const int rcv0 = rrow >= 0 ? g.rlane[gx] : -1;
    const float *DSb = a.dseis + (size_t)bs * g.nrec * g.dstride;
    const __amdgpu_buffer_rsrc_t DSR = rsrc_of(DSb);
    // dseis[k-1] of this lane's receiver; -0 (x + -0 == x bitwise) where there is none.  An
    // unconditional buffer load (OOB offset: no memory access) keeps every wave's vmcnt count equal.
#define DLOAD(KK)                                                                                   \
    ({                                                                                              \
        const int ri_ = (KK) >= 1 ? rec_index((KK) - 1, g.st) : -1;                                 \
        const bool ok_ = rcv0 >= 0 && ri_ >= 0;                                                     \
        const float v_ = bload(DSR, ok_ ? (ri_ * g.dstride + rcv0) * 4 : OOB, 0);                   \
        ok_ ? v_ : -0.0f;                                                                           \
    })
    const bool grad = rin != 0;                           // uniform: this wave has interior rows
    double ksum = 0.0;
    float gbacc = 0.0f;
    const size_t L = g.level;
    const int L4 = (int)(L * 4);                          // bytes per history slot (< 2 GB: resident surveys)
    f32x2 PA[RP], PB[RP];
    float PHA[4], PHB[4];
    int pv[12];                                           // P row (uz0 - 2 + i) offset of this lane
#pragma unroll
    for (int i = 0; i < 12; ++i) pv[i] = grad ? (wrap_row(uz0 + i - 2, g.Hp) * g.ld + gx) * 4 : OOB;
    // history descriptor of the epoch whose first step is KN: slots KN - T + 1 .. KN (step t of the
    // epoch reads slot KN - t at byte offset (T - 1 - t) * L4)
#define HIST_RSRC(KN) rsrc_of(a.hist + (ptrdiff_t)((KN) - (T - 1)) * (ptrdiff_t)L + (ptrdiff_t)so)
    // Per-epoch inputs (the first step's history slice P, the receiver residuals dseis[k-1] and the
    // wavelet w[k-1] of the epoch's T steps) are issued right behind the hand-off loads of the
    // previous epoch's sweep (ADJ_ISSUE), so the sweep does not wait for this HBM traffic; inside an
    // epoch a step waits only for its own P (prefetched one step ahead).
    float wv[T], dv[T];
    {
        const __amdgpu_buffer_rsrc_t H0 = HIST_RSRC(a.nt);
        ADJ_PLOAD(PA, PHA, H0, (T - 1) * L4)
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        wv[t] = a.wav[max(a.nt - t - 1, 0)];
        dv[t] = DLOAD(a.nt - t);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                   // vmcnt(0)
#define ADJ_ISSUE                                                                                   \
    {                                                                                               \
        const __amdgpu_buffer_rsrc_t HN = HIST_RSRC(kn);                                            \
        ADJ_PLOAD(PA, PHA, HN, (T - 1) * L4)                                                        \
        _Pragma("unroll") for (int t = 0; t < T; ++t) {                                             \
            wv[t] = a.wav[max(kn - t - 1, 0)];                                                      \
            dv[t] = DLOAD(kn - t);                                                                  \
        }                                                                                           \
    }
    const int nep = (a.nt + T - 1) / T;
    bool live = true;
    PT_PROF_VARS
    for (int e = 0; e < nep; ++e) {
        const int ke = a.nt - e * T;                      // first step k of this epoch
        const bool last = e + 1 == nep;
        const __amdgpu_buffer_rsrc_t HRe = HIST_RSRC(ke);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int j = e * T + t;
            if (j >= a.nt) break;
            const int k = ke - t;
            if (t & 1) ADJ_STEP(L0, L1, PB, PHB, PA, PHA)
            else ADJ_STEP(L1, L0, PA, PHA, PB, PHB)
        }
        if (T & 1) {   // keep "L1 = newest, PB = the last step's P, PA = free" at every epoch boundary
#pragma unroll
            for (int i = 0; i < RP; ++i) {
                const f32x2 tl = L0[i]; L0[i] = L1[i]; L1[i] = tl;
                const f32x2 tp = PA[i]; PA[i] = PB[i]; PB[i] = tp;
                const float th = PHA[i]; PHA[i] = PHB[i]; PHB[i] = th;
            }
        }
        PT_PROF(tst)
        if (!last) {
            const unsigned tag = (unsigned)(e + 1);
            const __amdgpu_buffer_rsrc_t GR = rsrc_of(a.gran + (size_t)(2 * ((e + 1) & 1)) * L + 2 * so);
            PT_PUBLISH(GR, tag, L0, L1)
            PT_PROF(tpb)
            ADJ_GRAD(L0, L1, PB, PHB, wv[T - 1])          // the deferred last step (no neighbour data)
            const int kn = ke - T;                        // first step k of the next epoch
            PT_PROF(tgr)
            PT_SWEEP_DELAY()
            PT_SWEEP(GR, tag, L0, L1, PT_ADJ_SG)
            ADJ_ISSUE
            PT_PROF_TAIL
        }
    }
#undef DLOAD
#undef ADJ_ISSUE
#undef HIST_RSRC
    PT_PROF_FLUSH
    if (xin) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if ((rin >> r) & 1u) a.gA[so + (size_t)PT_ROFS(r) + gx] = PT_AT(GA, r);
    }
    if (srow >= 0 && scol) a.gbeta[bs] = gbacc;
    // deterministic workgroup reduction of the sponge-coefficient partial sum
    const int tid = threadIdx.x;
    red[tid] = ksum;
    __syncthreads();
    for (int w2 = 512; w2 > 0; w2 >>= 1) {
        if (tid < w2 && tid + w2 < 64 * NW) red[tid] += red[tid + w2];
        __syncthreads();
    }
    if (tid == 0) a.gk_part[(size_t)bs * a.nblk + tile] = red[0];
}
// ---- FMA build of the persistent adjoint: the gradient from the history's time recurrence.
// The forward's own update P_k = T1 P_{k-1} - T2 P_{k-2} + A lap'(P_{k-1}) (+ beta w[k-1] at the
// source cell, pde.py:79-81) gives the stencil term the gradient needs without a stencil:
//   lap'(P_{k-1}) = (P_k - T1 P_{k-1} + T2 P_{k-2} - src) / A,   d = 2c1 P_{k-1} + lap'(P_{k-1})
// so a step's gradient is 7 packed ops per row pair (no DPP, no P halo rows, 8 history rows per
// wave and step instead of 12).  The history values are the forward's own, so the identity holds
// up to the rounding of P_k's last add (fp32 tolerance, like the FMA contraction of the step).
// The window lives in four row-pair buffers Q0..Q3 that rotate by one per step (step t of an
// epoch: P_k, P_{k-1}, P_{k-2} = Q[t], Q[t+1], Q[t+2] mod 4, prefetch into Q[t+3]): no copies for
// T = 4; other depths restore the order once per epoch.

#define ADJR_LOAD(PD, HR, SOFF)                                                                     \
    {                                                                                               \
        const int so_ = (SOFF);                                                                     \
        _Pragma("unroll") for (int i = 0; i < RP; ++i) {                                             \
            if constexpr (PR_S) {                    /* one lane offset, the row in the scalar offset */ \
                PD[i].x = bload_nt(HR, pl, so_ + prs[i]);                                           \
                PD[i].y = bload_nt(HR, pl, so_ + prs[R - 1 - i]);                                   \
            } else {                                                                                \
                PD[i].x = bload_nt(HR, pr[i], so_);                                                 \
                PD[i].y = bload_nt(HR, pr[R - 1 - i], so_);   /* mirrored pairs {i, R-1-i} */      \
            }                                                                                       \
        }                                                                                           \
    }

// gradient of step k (CU = L_{k+1}, LN = L_k; wavelet sample WK = w[k-1]; window P0 = P_k,
// P1 = P_{k-1}, P2 = P_{k-2}): u = lap'(P_{k-1}) x A from the history (the forward's source add undone
// on the source row), d = 2c1 P_{k-1} + lap'(P_{k-1}), then the accumulations with L_k; the source
// row's two terms share one scalar branch.
#define ADJR_GRAD(CU, LN, WK, P0, P1, P2)                                                           \
    if (grad) {                                                                                     \
        f32x2 u[RP];                                                                                \
        _Pragma("unroll") for (int i = 0; i < RP; ++i) {                                             \
            u[i] = fma2(-T1v[i], P1[i], P0[i]);                                                     \
            u[i] = fma2(T2v[i], P2[i], u[i]);                                                       \
        }                                                                                           \
        int sg_ = RL_PLAIN ? -1 : srow;              /* one scalar branch for both source terms */  \
        if constexpr (!RL_PLAIN) LAUNDER(sg_);       /* (plain role: no source row) */              \
        if constexpr (RL_SR >= 0) {                  /* source/receiver role: the row's pair is RL_SR */ \
            const float sa_ = scol ? bsrc * (WK) : 0.0f;                                            \
            const f32x2 sv_ = shalf ? f32x2{0.0f, sa_} : f32x2{sa_, 0.0f};                          \
            u[SRP] = u[SRP] - sv_;                                                                  \
            const float ls_ = shalf ? LN[SRP].y : LN[SRP].x;                                        \
            const float gb = scol ? ls_ * (WK) : -0.0f;                                             \
            gbacc = gbacc + gb;                                                                     \
        } else if (sg_ >= 0) {                                                                      \
            int sp_ = spair;                                                                        \
            LAUNDER(sp_);                                                                           \
            const float sa_ = scol ? bsrc * (WK) : 0.0f;  /* the forward's source add, undone */    \
            const f32x2 sv_ = shalf ? f32x2{0.0f, sa_} : f32x2{sa_, 0.0f};                          \
            f32x2 lp_ = LN[0];                                                                      \
            _Pragma("unroll") for (int i = 0; i < RP; ++i) {                                         \
                if (i == sp_) u[i] = u[i] - sv_;                                                    \
                if (i > 0 && i == sp_) lp_ = LN[i];                                                 \
            }                                                                                       \
            const float ls_ = shalf ? lp_.y : lp_.x;                                                \
            const float gb = scol ? ls_ * (WK) : -0.0f;  /* gbeta: the source cell's lane only */   \
            gbacc = gbacc + gb;                                                                     \
        }                                                                                           \
        /* A d = A 2c1 P_{k-1} + u: the 1/A is applied once to the sum (gA = sum L A d / A) */     \
        _Pragma("unroll") for (int i = 0; i < RP; ++i) {                                             \
            const f32x2 dd = fma2(A[i], kC1X2 * P1[i], u[i]);                                       \
            GA[i] = fma2(LN[i], dd, GA[i]);                                                         \
            GK[i] = fma2(P1[i], CU[i] - LN[i], GK[i]);                                              \
        }                                                                                           \
    }

// One adjoint step k: CUR = L_{k+1}, PRV = L_{k+2} -> L_k; window P0 / P1 / P2 as ADJR_GRAD; history
// slot k-2 (the next step's P_{k-3}) prefetched into PN.  Barrier-free (mirrored pairs, the forward's
// LDS mailbox xm_*): the wave waits only for its two neighbours' A L_{k+1} boundary rows, computes its
// two boundary pairs (receiver residual included), publishes their A L_k rows for the next step, then
// its interior pair.  Per row the operations and their order are those of the barrier-synchronised step
// it replaced in round 6 (m1 + p1 commutes: same bits; 1.646 -> 1.577 ms at configs[1],
// profiles/r6/adj_nb_ab.txt).  (The gradient's history half ahead of the wait, as the forward's time
// terms, needs 6 more VGPRs: 84 B/lane scratch.)
#define ADJR_PAIRS_NB(CUR, PRV, LO, HI)                                                             \
    {                                                                                               \
        _Pragma("unroll") for (int i = (LO); i < (HI); ++i) {                                        \
            MIR_VERT(q, i, m1, p1, m2, p2)                                                          \
            const f32x2 c = q[i];                                                                   \
            const f32x2 xl1 = {dpp_shr1(c.x), dpp_shr1(c.y)}, xr1 = {dpp_shl1(c.x), dpp_shl1(c.y)}; \
            f32x2 n1 = m1 + p1; n1 = n1 + xl1; n1 = n1 + xr1;                                       \
            f32x2 n2 = m2 + p2;                        /* x -+ 2 taps: fused v_add_f32_dpp */       \
            n2.x = n2.x + dpp_shr1(xl1.x); n2.y = n2.y + dpp_shr1(xl1.y);                           \
            n2.x = n2.x + dpp_shl1(xr1.x); n2.y = n2.y + dpp_shl1(xr1.y);                           \
            const f32x2 nb = fma2(kC3, n2, kC2 * n1);                                               \
            PRV[i] = fma2(T1v[i], CUR[i], fma2(-T2v[i], PRV[i], nb));                               \
        }                                                                                           \
        int rr_ = RL_PLAIN ? 0 : (LO) == 0 ? rlo : rhi;   /* the receiver's pair is in this half */ \
        if constexpr (!RL_PLAIN) LAUNDER(rr_);       /* (plain role: no receiver row) */            \
        if constexpr (RL_SR >= 0) {                  /* source/receiver role: every step is recorded */ \
            if constexpr ((HI) > (LO) && SRP >= (LO) && SRP < (HI))                                 \
                PRV[SRP] = PRV[SRP] + (shalf ? f32x2{-0.0f, dcur} : f32x2{dcur, -0.0f});            \
        } else if ((HI) > (LO) && rr_ && rec_index(k - 1, g.st) >= 0) {                             \
            int rp_ = rpair;                                                                        \
            LAUNDER(rp_);                                                                           \
            const f32x2 dv_ = rhalf ? f32x2{-0.0f, dcur} : f32x2{dcur, -0.0f};   /* -0: no-op */     \
            _Pragma("unroll") for (int i = (LO); i < (HI); ++i) if (i == rp_) PRV[i] = PRV[i] + dv_; \
        }                                                                                           \
    }
#define ADJR_STEP_NB(CUR, PRV, P0, P1, P2, PN)                                                      \
    {                                                                                               \
        if constexpr (RL_SR >= 0 && SA) {            /* step-ahead fetch: the next step's residual */ \
            dv[(t + 1) % T] = DLOAD(k - 1);                                                         \
            /* the history prefetch without its `grad` test (the role's wave owns an interior row; a halo    \
               lane's offset is out of range and loads 0): under the test the in-order wait for the load     \
               above is placed for the path without the six loads, vmcnt(3) at the next step's head, and     \
               the wave waits there for history it needs a step later (1.366 -> 1.401 ms) */                 \
            ADJR_LOAD(PN, HRe, (T - 1 - t) * L4)                                                    \
        } else if constexpr (RL_PLAIN) {             /* steady epoch: every prefetched slot exists */ \
            if (grad) ADJR_LOAD(PN, HRe, (T - 1 - t) * L4)                                          \
        } else if (ldall || (grad && k >= 2)) ADJR_LOAD(PN, HRe, (T - 1 - t) * L4)                  \
        const float dcur = dv[t];                                                                   \
        u32x2 f_;                                                                                   \
        f32x2 E1, E2;                                                                               \
        xm_load<NW>(xm, j & 1, w, lane, f_, E1, E2);                                                \
        f32x2 q[RP];                                                                                \
        _Pragma("unroll") for (int i = 0; i < RP; ++i) q[i] = A[i] * CUR[i];                         \
        xm_wait<NW>(xm, j & 1, w, lane, (unsigned)j + 1u, f_, E1, E2, a.status, live);              \
        ADJR_PAIRS_NB(CUR, PRV, 0, 2)                                                               \
        if (t + 1 < T) xm_put<NW>(xm, (j + 1) & 1, w, lane, (unsigned)j + 2u, A[0] * PRV[0], A[1] * PRV[1]); \
        __builtin_amdgcn_s_setprio(PT_PRIO_BODY);                                                   \
        ADJR_PAIRS_NB(CUR, PRV, 2, RP)                                                              \
        if (t + 1 < T || (!RL_PLAIN && last)) ADJR_GRAD(CUR, PRV, wv[t], P0, P1, P2)                \
    }

// OV (rdq_fwi_set_handoff_overlap): 0 = PT_SWEEP; 1 = the dead cells are zeroed while the sweep's first
// pass is in flight (PT_SWEEP_SHADOW), in the lean form: 1.4897 -> 1.4579 ms at configs[1], modes
// alternated x9 (profiles/r9/kernel_ab_lean_zeroing.jsonl; with PT_SWEEP_ZERO's form in the round trip
// 1.4911 -> 1.4722, kernel_ab_adj_shadow_fwd_xmfirst.jsonl).  In the forward the zeroing in the round
// trip was slower (1.011 -> 1.035 ms: more stale first passes) and the lean form after the sweep no
// faster, so the forward has the one order.
// SA (rdq_fwi_set_adjoint_fetch), with a role only (SR >= 0): false = the role's loop loads its T residuals and
// wavelet samples an epoch ahead, after the sweep (ADJ_ISSUE); true = the residuals a step ahead: step k loads
// step k - 1's ahead of its own history prefetch, the epoch's last step the next epoch's first (ADJR_STEP_NB),
// so a step's head, where the residual goes into the boundary rows its neighbours wait for, finds a value
// issued a whole step earlier instead of one issued a few instructions earlier, at the end of the tail.  The
// wavelet samples, read at a step's end, stay an epoch ahead: with them a step ahead too the overlap-1 builds
// spill two VGPR values (profiles/r26/resource_usage.txt).  The bound (no such loads at all) is 84-86 of the 1360
// us, the residuals alone take 81: 1.3599 -> 1.2784 ms at configs[1] (profiles/r26/kernel_ab_adj_fetch.jsonl).
template <int T, int NW, int RW, bool PROF, int OV = 0, int SR = -1, bool SA = false>
__global__ __launch_bounds__(64 * NW) void k_adj_pr(AdjPtArgs a)
{
    unsigned long long *const prof = PROF ? a.prof : nullptr;   // phase counters: profiled build only
    constexpr bool PT_PRIO = true;                        // wave priorities (PT_PRIO_*)
    constexpr bool PT_MIR = true;                         // mirrored pairs for the exchange's boundary rows
    constexpr bool RL_PLAIN = false;                      // the generic wave role (shadowed in the plain epochs)
    constexpr int RL_SR = -1, SRP = 0;                    // source/receiver role: the row's pair (SRP = max(RL_SR, 0))
    constexpr bool PR_S = SR >= 0;                        // history row offsets as scalars (ADJR_LOAD)
    static_assert(SR < RW / 2 && (SR < 0 || (T == PT_ROLES_T && RW == PT_SROLE_RW)), "k_adj_pr: the role's row pair");
    static_assert(SR >= 0 || !SA, "k_adj_pr: the step-ahead fetch belongs to the role's loop");
    __shared__ XmBox<NW> xm;                              // the waves' inboxes (xm_*)
    __shared__ double red[64 * NW];
    // the LDS the residency decision (resident_capacity) depends on: the mailboxes and the reduction
    static_assert(sizeof(XmBox<NW>) + sizeof(double) * 64 * NW == (size_t)NW * 4608 && NW <= 16,
                  "k_adj_pr: 4 KB of mailboxes + 512 B of reduction per wave (72 KB at 16 waves)");
    const TBGeo &g = a.g;
    PT_REGION_INIT(NW, RW)
    const float *AL = a.coeffs + (size_t)b * g.slice;
    f32x2 A[RP], T1v[RP], T2v[RP], L0[RP], L1[RP], GA[RP], GK[RP];   // GA accumulates A x the gradient
    const f32x2 kC2 = {C2, C2}, kC3 = {C3, C3}, kC1X2 = {C1X2, C1X2};
    int srow = -1, rrow = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int gz = wrap_row(uz0 + r, g.Hp);
        const int o = gz * g.ld + gx;
        PT_AT(A, r) = AL[o]; PT_AT(T1v, r) = AL[g.cstride + o]; PT_AT(T2v, r) = AL[2 * g.cstride + o];
        PT_AT(L0, r) = 0.0f; PT_AT(L1, r) = 0.0f;         // L_{nt+1} = L_{nt+2} = 0
        PT_AT(GA, r) = 0.0f; PT_AT(GK, r) = 0.0f;
        if (gz == g.isz && ((rin >> r) & 1u)) srow = r;
        if (gz == g.igz) rrow = r;
    }
    const int isx = g.isx[s];
    const bool scol = xin && gx == isx;
    const float bsrc = srow >= 0 ? AL[4 * g.cstride + (size_t)g.isz * g.ld + isx] : 0.0f;   // beta at the source
    const int rcv0 = rrow >= 0 ? g.rlane[gx] : -1;
    const float *DSb = a.dseis + (size_t)bs * g.nrec * g.dstride;
    const __amdgpu_buffer_rsrc_t DSR = rsrc_of(DSb);
    // source / receiver rows as (row pair, half): a step touches one pair, not all eight rows
    const int spair = __builtin_amdgcn_readfirstlane(srow < 0 ? 0 : srow < RP ? srow : R - 1 - srow);
    const int rpair = __builtin_amdgcn_readfirstlane(rrow < 0 ? 0 : rrow < RP ? rrow : R - 1 - rrow);
    const bool shalf = srow >= RP, rhalf = rrow >= RP;   // the half is r >= RP
    // the receiver's row pair among the boundary pairs 0, 1 (rlo) or the interior ones (rhi): wave-uniform
    const int rlo = __builtin_amdgcn_readfirstlane(rrow >= 0 && rpair < 2 ? 1 : 0);
    const int rhi = __builtin_amdgcn_readfirstlane(rrow >= 0 && rpair >= 2 ? 1 : 0);
#define DLOAD(KK)                                                                                   \
    ({                                                                                              \
        const int ri_ = (KK) >= 1 ? rec_index((KK) - 1, g.st) : -1;                                 \
        const bool ok_ = rcv0 >= 0 && ri_ >= 0;                                                     \
        const float v_ = bload(DSR, ok_ ? (ri_ * g.dstride + rcv0) * 4 : OOB, 0);                   \
        ok_ ? v_ : -0.0f;                                                                           \
    })
    const bool grad = rin != 0;                           // uniform: this wave has interior rows
    float gbacc = 0.0f;
    const size_t L = g.level;
    const int L4 = (int)(L * 4);                          // bytes per history slot (< 2 GB: resident surveys)
    f32x2 Q0[RP], Q1[RP], Q2[RP], Q3[RP];
    // History offsets of ADJR_LOAD, in two forms, of which a build reads one (`if constexpr (PR_S)` there) and
    // the compiler drops the other.  Builds without a source/receiver role (SR = -1) read pr[r]: the offset of
    // (own row r, lane), a VGPR each.
    int pr[R];                                            // history offset of (own row r, lane)
#pragma unroll
    for (int r = 0; r < R; ++r)   // every lane (own cells only, halo lanes at OOB: 1.66 -> 1.73 ms)
        pr[r] = grad ? (PT_ROFS(r) + gx) * 4 : OOB;
    // Builds with a role (PR_S) read the same offsets as one lane offset pl and a wave-uniform row offset
    // prs[r] that goes into the load's scalar offset: six VGPRs less, six SGPRs more.  (Both forms are written
    // out unguarded on purpose: with each under its own `if constexpr` the SR >= 0 builds come out as a
    // different text, 133 SGPR spills for 131, and the text here is the one that was timed.)
    const int pl = grad ? gx * 4 : OOB;
    int prs[R];
#pragma unroll
    for (int r = 0; r < R; ++r) prs[r] = __builtin_amdgcn_readfirstlane(PT_ROFS(r) * 4);
#pragma unroll
    for (int i = 0; i < RP; ++i) { Q0[i] = 0.0f; Q1[i] = 0.0f; Q2[i] = 0.0f; Q3[i] = 0.0f; }
    // history descriptor of the epoch whose first step is KN: its prefetches read slots
    // KN - 2 .. KN - T - 1, step t at byte offset (T - 1 - t) * L4
#define HIST_RSRC(KN) rsrc_of(a.hist + (ptrdiff_t)((KN) - T - 1) * (ptrdiff_t)L + (ptrdiff_t)so)
    float wv[T], dv[T];
    if (grad) {   // window of the first step k = nt: slots nt + 1, nt, nt - 1
        const __amdgpu_buffer_rsrc_t H0 = rsrc_of(a.hist + (ptrdiff_t)(a.nt - 1) * (ptrdiff_t)L + (ptrdiff_t)so);
        ADJR_LOAD(Q0, H0, 2 * L4)
        ADJR_LOAD(Q1, H0, L4)
        ADJR_LOAD(Q2, H0, 0)
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        wv[t] = a.wav[max(a.nt - t - 1, 0)];
        dv[t] = DLOAD(a.nt - t);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                   // vmcnt(0)
// the next epoch's wavelet samples and receiver residuals, issued after the sweep as vector loads:
// ahead of it the residual loads make the sweep wait for their round trip (1.65 -> 1.78 ms), and the
// wavelet as scalar loads (wav_s) is slower here too, before the sweep (1.64 -> 1.77 ms: an outstanding
// s_load holds every lgkmcnt wait of the LDS exchange) or after it (1.66 ms; profiles/r6/
// presweep_reorder_ab.txt, wav_scalar_ab.txt)
#define ADJ_ISSUE                                                                                   \
    _Pragma("unroll") for (int t = 0; t < T; ++t) {                                                 \
        wv[t] = a.wav[max(kn - t - 1, 0)];                                                          \
        dv[t] = DLOAD(kn - t);                                                                      \
    }
    const int nep = (a.nt + T - 1) / T;
    bool live = true;
    PT_PROF_VARS
    xm_init<NW>(xm, w, lane);                             // no flag matches a tag until written
    __syncthreads();
    xm_put<NW>(xm, 0, w, lane, 1u, f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f});   // A L_{nt+1} = 0, step 0's tag
    int plain = (T == PT_ROLES_T) && a.roles && srow < 0 && rrow < 0;   // wave role, decided once
    plain = __builtin_amdgcn_readfirstlane(plain);
// the T steps of one epoch, for the role RL_PLAIN in scope (a plain epoch is steady: all its steps exist)
#define ADJR_EPOCH_STEPS                                                                            \
    _Pragma("unroll") for (int t = 0; t < T; ++t) {                                                 \
        const int j = e * T + t;                                                                    \
        if (!RL_PLAIN && j >= a.nt) break;                                                          \
        const int k = ke - t;                                                                       \
        if ((t & 3) == 0) ADJR_STEP_NB(L1, L0, Q0, Q1, Q2, Q3)                                      \
        else if ((t & 3) == 1) ADJR_STEP_NB(L0, L1, Q1, Q2, Q3, Q0)                                 \
        else if ((t & 3) == 2) ADJR_STEP_NB(L1, L0, Q2, Q3, Q0, Q1)                                 \
        else ADJR_STEP_NB(L0, L1, Q3, Q0, Q1, Q2)                                                   \
    }
// the last step's window (step T - 1: Q[T-1], Q[T], Q[T+1] mod 4), for the deferred gradient
#define QW(o) (((T - 1 + (o)) & 3) == 0 ? Q0 : ((T - 1 + (o)) & 3) == 1 ? Q1 : ((T - 1 + (o)) & 3) == 2 ? Q2 : Q3)
// One epoch e, for the role RL_PLAIN in scope (plain: never the last epoch).  ldall: every step of the
// epoch prefetches a history slot that exists (k >= 2), one scalar test per epoch instead of per step (the
// barrier-free step, ADJR_STEP_NB).  After the steps: keep "L1 = newest" at every epoch boundary; publish;
// the deferred last step's gradient (no neighbour data); the sweep; the next step's boundary rows, with
// the halo cells the sweep reloaded; restore Q0 = the next epoch's P_k.
#define ADJR_EPOCH                                                                                  \
    {                                                                                               \
        const int ke = a.nt - e * T;                      /* first step k of this epoch */          \
        const bool last = !RL_PLAIN && e + 1 == nep;                                                \
        const __amdgpu_buffer_rsrc_t HRe = HIST_RSRC(ke);                                           \
        int ldall = grad && ke >= T + 1;                                                            \
        LAUNDER(ldall);                                                                             \
        ADJR_EPOCH_STEPS                                                                            \
        if (T & 1) {                                                                                \
            _Pragma("unroll") for (int i = 0; i < RP; ++i) { const f32x2 tl = L0[i]; L0[i] = L1[i]; L1[i] = tl; } \
        }                                                                                           \
        PT_PROF(tst)                                                                                \
        if (!last) {                                                                                \
            const unsigned tag = (unsigned)(e + 1);                                                 \
            const __amdgpu_buffer_rsrc_t GR = rsrc_of(a.gran + (size_t)(2 * ((e + 1) & 1)) * L + 2 * so); \
            PT_PUBLISH(GR, tag, L0, L1)                                                             \
            PT_PROF(tpb)                                                                            \
            const int kn = ke - T;                        /* first step k of the next epoch */      \
            ADJR_GRAD(L0, L1, wv[T - 1], QW(0), QW(1), QW(2))                                       \
            PT_PROF(tgr)                                                                            \
            PT_SWEEP_DELAY()                                                                        \
            if constexpr (OV == 0) PT_SWEEP(GR, tag, L0, L1, PT_ADJ_SG)                             \
            else PT_SWEEP_SHADOW(GR, tag, L0, L1, PT_ADJ_SG, (PT_ADJ_SG < R ? PT_ADJ_SG : R))       \
            xm_put<NW>(xm, (e + 1) * T & 1, w, lane, (unsigned)((e + 1) * T) + 1u, A[0] * L1[0], A[1] * L1[1]); \
            if constexpr (!RL_PLAIN || (RL_SR >= 0 && !SA)) ADJ_ISSUE                               \
            else if constexpr (RL_SR >= 0) {         /* step-ahead: the residuals come with the steps */ \
                _Pragma("unroll") for (int t = 0; t < T; ++t) wv[t] = a.wav[max(kn - t - 1, 0)];     \
            }                                                                                       \
            PT_PROF_TAIL                                                                            \
        }                                                                                           \
        if constexpr ((T & 3) != 0) {                                                               \
            _Pragma("unroll") for (int i = 0; i < RP; ++i) {                                         \
                const f32x2 a0 = QW(1)[i], a1 = QW(2)[i], a2 = QW(3)[i], a3 = QW(4)[i];             \
                Q0[i] = a0; Q1[i] = a1; Q2[i] = a2; Q3[i] = a3;                                     \
            }                                                                                       \
        }                                                                                           \
    }
    // Wave roles (rdq_fwi_set_wave_roles): a plain wave (no source row, no receiver row) branches once,
    // here, into a loop of its own over every epoch but the last (steady: all T steps exist, every step's
    // history prefetch reads an existing slot, the epoch's last gradient is the deferred one), whose steps
    // carry no per-step source / receiver / j >= nt / last / prefetch test and whose epochs load no wavelet
    // samples or residuals (they are loaded once, after the loop, for the generic epoch); `grad` stays a
    // scalar test, so the all-halo waves share that loop.  The generic loop runs the rest: every epoch of
    // the other waves and the last epoch of all.  Mailbox, publish, sweep, zeroing and tags are the same
    // text in both, and per cell the arithmetic is the same: results are bit for bit those of mode 0.
    // configs[1]: 1.4464 -> 1.4193 ms (profiles/r11/kernel_ab_adj_roles.jsonl).  (One loop choosing a body
    // per epoch spilled 107 VGPRs; the same split of the forward's steps alone was no faster: the forward has
    // it with its source role, k_fwd_pt.)
    // Source/receiver role (rdq_fwi_set_adjoint_role), SR >= 0: the wave whose rows own the source row, that row
    // being the receiver row too, in mirrored pair SR (the host's choice, adjoint_role_pair: the pair is the same
    // for every tile, shot and model of a launch, so it is a template parameter and each build carries one such
    // body).  That wave branches once into a loop of its own over every epoch but the last: the plain epoch plus
    // the row's work with the pair a compile-time index and the half a scalar (the receiver add in
    // ADJR_PAIRS_NB, the source undo and the gbeta term in ADJR_GRAD, ADJ_ISSUE after the sweep).  The host
    // runs it only where every step is recorded and the row has no live halo copy (source_role_fits).  With the
    // pair a run-time value or one body per pair in one kernel the role spilled 11 to 413 VGPR values
    // (profiles/r13/resource_usage.txt); as built it needs the history row offsets as scalars (PR_S) to spill
    // none (profiles/r18/resource_usage.txt).  The waves that enter count themselves into status word
    // PT_ROLE_WORD, once per launch.  Same text per cell as the generic step: bit for bit the results of SR = -1.
    int e = 0;
    if constexpr (T == PT_ROLES_T) {
        if (plain) {
            constexpr bool RL_PLAIN = true;
            for (; e + 1 < nep; ++e) ADJR_EPOCH
            const int kn = a.nt - e * T;                  // the generic epoch's samples and residuals
            ADJ_ISSUE
        }
        // (a test of its own after the plain branch, which a plain wave fails: as the plain branch's `else`
        // the same text spills 24 to 54 VGPR values around the loops, profiles/r18/resource_usage.txt)
        int srw = SR >= 0 && a.roles && srow >= 0 && rrow == srow && spair == SR;
        srw = __builtin_amdgcn_readfirstlane(srw);
        if (srw) {
            constexpr bool RL_PLAIN = true;
            constexpr int RL_SR = SR, SRP = SR;
            if (lane == 0)                                // once per wave and launch: the role ran
                __hip_atomic_fetch_add(a.status + PT_ROLE_WORD, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (; e + 1 < nep; ++e) ADJR_EPOCH
            if constexpr (SA) {                           // the generic epoch's samples and residuals, as the plain branch
                const int kn = a.nt - e * T;
                ADJ_ISSUE
            }
        }
    }
    for (; e < nep; ++e) ADJR_EPOCH
#undef ADJR_EPOCH
#undef ADJR_EPOCH_STEPS
#undef QW
#undef DLOAD
#undef ADJ_ISSUE
#undef HIST_RSRC
    PT_PROF_FLUSH
    double ksum = 0.0;                                    // gk = sum K * (sum_k P (L_{k+1} - L_k))
    if (xin) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if ((rin >> r) & 1u) {
                a.gA[so + (size_t)PT_ROFS(r) + gx] = PT_AT(GA, r) / PT_AT(A, r);
                const float kp = AL[3 * g.cstride + PT_ROFS(r) + gx];
                ksum += (double)kp * (double)PT_AT(GK, r);
            }
    }
    if (srow >= 0 && scol) a.gbeta[bs] = gbacc;
    // deterministic workgroup reduction of the sponge-coefficient partial sum
    const int tid = threadIdx.x;
    red[tid] = ksum;
    __syncthreads();
    for (int w2 = 512; w2 > 0; w2 >>= 1) {
        if (tid < w2 && tid + w2 < 64 * NW) red[tid] += red[tid + w2];
        __syncthreads();
    }
    if (tid == 0) a.gk_part[(size_t)bs * a.nblk + tile] = red[0];
}
#undef ADJR_STEP_NB
#undef ADJR_PAIRS_NB
#undef FWD_STEP_NB
#undef FWD_PAIRS_NB
#undef MIR_VERT
#undef ADJR_GRAD
#undef ADJR_LOAD
#undef ADJ_STEP
#undef ADJ_GRAD
#undef ADJ_PLOAD
#undef PAIR_VERT
#undef PT_AT
#undef PT_SWEEP
#undef PT_SWEEP_PASSES
#undef PT_SWEEP_ZERO
#undef PT_SWEEP_ZERO_LEAN
#undef PT_SWEEP_ROW_OFS
#undef PT_SWEEP_EARLY
#undef PT_SWEEP_MERGE
#undef PT_SWEEP_OV
#undef PT_SWEEP_SHADOW
#undef PT_PUBLISH
#undef PT_PROF
#undef PT_PROF_VARS
#undef PT_PROF_TAIL
#undef PT_PROF_FLUSH
#undef PT_SWEEP_DELAY
#undef PT_ROFS
#undef PT_REGION_INIT
#undef PT_REGION_HEAD
#undef PT_REGION_GEOM
#undef LAUNDER

// Receivers sharing a padded column (ng > nx, or repeated gx): their residuals at one (model, shot,
// record) summed in receiver order into one value per column, the gradient the reference's
// indexing backward builds (index_put with accumulate into zeros, pde.py:82-83), so the time-loop
// kernels inject one value per lane and step with no per-receiver loop.
__global__ __launch_bounds__(256) void k_rcv_fold(const float *__restrict__ ds, float *__restrict__ out,
                                                  const int *__restrict__ colx, const int *__restrict__ rcv_start,
                                                  const int *__restrict__ rcv_list, int ng, int ncolr, size_t rows)
{
    const size_t n = rows * (size_t)ncolr;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / ncolr;
        const int c = (int)(i - row * ncolr), x = colx[c];
        const float *d = ds + row * ng;
        const int r0 = rcv_start[x], r1 = rcv_start[x + 1];
        float v = d[rcv_list[r0]];
        for (int j = r0 + 1; j < r1; ++j) v = v + d[rcv_list[j]];
        out[i] = v;
    }
}

// --------------------------------------------------------------------------------------- K4
struct FinArgs {
    int B, ns, nz, nx, nbc, Hp, Wp, ld, isz, nblk;
    float dt, dx;
    double scale;     // d(v)/d(input): 1500 for normalised input, 1 for physical velocity
    size_t cstride, slice;
    const float *coeffs, *gA, *gbeta, *vmin;
    const int64_t *amin;
    const double *gk_part;
    const int *isx;
    double *colsum;   // [B][Hp][nx]
    float *out;       // [B][nz][nx]
};
// rdq_fwi_grad_finalize_enc: ne supershots; gA [B][ne][Hp][ld], gk_part [B][ne][nblk], gbeta [B][ne][ns]
struct FinEncArgs : FinArgs {
    int ne;
};

// Stage 1: per padded row z and model column ix, sum g_vpad over the padded columns that
// replicate ix (F.pad replicate backward).  g_vpad is formed per point exactly as autograd
// chains it: alpha = (v*dt/dx)^2 -> ((gA*(2*a1))/dx)*dt; beta = (v*dt)^2 at the sources;
// the sponge term sum(gK*K)/vmin lands on the first argmin of the padded field.
// One workgroup per padded row (z, b): every padded cell's d(loss)/d(v_pad) (fp64) into LDS, all
// cells in parallel; then the replicate-pad fold along x: interior columns take their own cell,
// the two edge columns sum their nbc+1-wide strips (one wave each, fixed-order shuffle tree).
// ENC: the accumulators of an encoded call.  The ne wavefield planes of gA and gk_part are summed in order where
// the plain call sums its ns shot planes, and source s takes sum_e gbeta[b, e, s] (fp32, ascending e).
constexpr int FIN_MAXW = 4096;
template <class Args>
__global__ __launch_bounds__(256) void k_fin_rows(Args p)
{
    constexpr bool ENC = std::is_same_v<Args, FinEncArgs>;
    int nw;                                           // wavefields per model
    if constexpr (ENC) nw = p.ne; else nw = p.ns;
    __shared__ double gv_s[FIN_MAXW];
    const int z = blockIdx.x, b = blockIdx.y;
    const size_t ro = (size_t)b * p.slice + (size_t)z * p.ld;
    const float *GA = p.gA + (size_t)b * nw * p.slice + (size_t)z * p.ld;   // [B][ns][Hp][ld]
    const float *V = p.coeffs + 5 * p.cstride + ro;
    const int amz = (int)(p.amin[b] / p.nx), amx = (int)(p.amin[b] - (int64_t)amz * p.nx);
    const int apz = amz == 0 ? 0 : amz + p.nbc, apx = amx == 0 ? 0 : amx + p.nbc;
    // sponge term sum(gk_part) of the argmin row: a fixed-order two-level fp64 sum (256 contiguous
    // segments, then the segment sums in order) instead of one thread's serial loop of dependent
    // loads (ns * nblk round trips)
    __shared__ double gk_s[256];
    if (z == apz) {
        const int cnt = nw * p.nblk, per = (cnt + 255) / 256;
        const double *GK = p.gk_part + (size_t)b * cnt;
        double acc = 0.0;
        const int j0 = threadIdx.x * per, j1 = min(cnt, j0 + per);
        for (int j = j0; j < j1; j += 4) {
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = GK[min(j + u, cnt - 1)];   // independent loads
#pragma unroll
            for (int u = 0; u < 4; ++u) if (j + u < j1) acc += v[u];
        }
        gk_s[threadIdx.x] = acc;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < p.Wp; x += blockDim.x) {
        float a1 = V[x] * p.dt; a1 = a1 / p.dx;
        float ga = 0.0f;
        {   // shots in order (the oracle's order); the loads are issued 4 at a time
            int s = 0;
            for (; s + 4 <= nw; s += 4) {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = GA[(size_t)(s + u) * p.slice + x];
#pragma unroll
                for (int u = 0; u < 4; ++u) ga = ga + v[u];
            }
            for (; s < nw; ++s) ga = ga + GA[(size_t)s * p.slice + x];
        }
        float t = ga * (2.0f * a1); t = t / p.dx; t = t * p.dt;
        double gv = (double)t;
        if (z == p.isz) {
            for (int s = 0; s < p.ns; ++s)
                if (p.isx[s] == x) {
                    const float b1 = V[x] * p.dt;
                    float gb;
                    if constexpr (ENC) {
                        gb = 0.0f;
                        for (int e = 0; e < p.ne; ++e) gb = gb + p.gbeta[((size_t)b * p.ne + e) * p.ns + s];
                    } else gb = p.gbeta[b * p.ns + s];
                    float u = gb * (2.0f * b1); u = u * p.dt;
                    gv += (double)u;
                }
        }
        if (z == apz && x == apx) {
            double gk = 0.0;
            for (int j = 0; j < 256; ++j) gk += gk_s[j];
            gv += gk / (double)p.vmin[b];
        }
        gv_s[x] = gv;
    }
    __syncthreads();
    double *CS = p.colsum + ((size_t)b * p.Hp + z) * p.nx;
    for (int ix = 1 + threadIdx.x; ix < p.nx - 1; ix += blockDim.x) CS[ix] = gv_s[ix + p.nbc];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (w < 2) {   // wave 0: columns [0, nbc] -> ix 0; wave 1: [nbc+nx-1, Wp) -> ix nx-1
        const int x0 = w == 0 ? 0 : p.nbc + p.nx - 1, x1 = w == 0 ? p.nbc + 1 : p.Wp;
        double acc = 0.0;
        for (int x = x0 + lane; x < x1; x += 64) acc += gv_s[x];
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if (lane == 0) {
            if (p.nx == 1) { if (w == 0) { double t2 = acc; for (int x = p.nbc + 1; x < p.Wp; ++x) t2 += gv_s[x]; CS[0] = t2; } }
            else CS[w == 0 ? 0 : p.nx - 1] = acc;
        }
    }
}
__global__ __launch_bounds__(256) void k_fin_cols(FinArgs p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= p.nz * p.nx) return;
    const int iz = i / p.nx, ix = i - iz * p.nx;
    const int z0 = iz == 0 ? 0 : iz + p.nbc;
    const int z1 = iz == p.nz - 1 ? p.Hp : iz + p.nbc + 1;
    // the first / last model rows fold nbc + 1 padded rows (121 at OpenFWI): loads issued 16 at a time,
    // then added in row order (the same sum bit for bit; one dependent load per row made this 31 us)
    const double *cs = p.colsum + (size_t)b * p.Hp * p.nx + ix;
    double acc = 0.0;
    int z = z0;
    for (; z + 16 <= z1; z += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = cs[(size_t)(z + u) * p.nx];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += v[u];
    }
    for (; z < z1; ++z) acc += cs[(size_t)z * p.nx];
    p.out[(size_t)b * p.nz * p.nx + i] = (float)(acc * p.scale);
}

// Illumination finalize (rdq_fwi_illum_finalize): H[b, iz, ix] = (dA/dv)^2 sum_{(z, x) -> (iz, ix)} sum_w hA[b, w, z, x],
// dA/dv = 2 v (dt/dx)^2 (x 1500 for normalised input), v the model cell's fp32 velocity (field 5 of K3: every padded
// cell of the fold holds the same value).  Everything in fp64: the wavefield planes in ascending w, then K4's
// two-stage replicate fold (rows into colsum [B][Hp][nx], then columns), one cast to fp32 at the end.  Two square
// factors of dA/dv, which is why this is not K4 with zeroed gk / gbeta.
struct IllumFinArgs {
    int B, nwf, nz, nx, nbc, Hp, Wp, ld;
    float dt, dx;
    double scale;     // d(v)/d(input): 1500 for normalised input, 1 for physical velocity
    size_t cstride, slice;
    const float *coeffs, *hA;
    double *colsum;   // [B][Hp][nx]
    float *out;       // [B][nz][nx]
};
__global__ __launch_bounds__(256) void k_illum_fin_rows(IllumFinArgs p)
{
    __shared__ double hs[FIN_MAXW];
    const int z = blockIdx.x, b = blockIdx.y;
    const float *HA = p.hA + (size_t)b * p.nwf * p.slice + (size_t)z * p.ld;
    for (int x = threadIdx.x; x < p.Wp; x += blockDim.x) {
        double acc = 0.0;
        int s = 0;
        for (; s + 4 <= p.nwf; s += 4) {     // loads issued 4 at a time, added in order
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = HA[(size_t)(s + u) * p.slice + x];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += (double)v[u];
        }
        for (; s < p.nwf; ++s) acc += (double)HA[(size_t)s * p.slice + x];
        hs[x] = acc;
    }
    __syncthreads();
    double *CS = p.colsum + ((size_t)b * p.Hp + z) * p.nx;
    for (int ix = threadIdx.x; ix < p.nx; ix += blockDim.x) {
        const int x0 = ix == 0 ? 0 : ix + p.nbc, x1 = ix == p.nx - 1 ? p.Wp : ix + p.nbc + 1;
        double acc = 0.0;
        for (int x = x0; x < x1; ++x) acc += hs[x];
        CS[ix] = acc;
    }
}
__global__ __launch_bounds__(256) void k_illum_fin(IllumFinArgs p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= p.nz * p.nx) return;
    const int iz = i / p.nx, ix = i - iz * p.nx;
    const int z0 = iz == 0 ? 0 : iz + p.nbc;
    const int z1 = iz == p.nz - 1 ? p.Hp : iz + p.nbc + 1;
    const double *cs = p.colsum + (size_t)b * p.Hp * p.nx + ix;
    double acc = 0.0;
    for (int z = z0; z < z1; ++z) acc += cs[(size_t)z * p.nx];
    const double v = (double)p.coeffs[5 * p.cstride + (size_t)b * p.slice + (size_t)(iz + p.nbc) * p.ld + (ix + p.nbc)];
    const double r = (double)p.dt / (double)p.dx;
    const double d = 2.0 * v * (r * r) * p.scale;
    p.out[(size_t)b * p.nz * p.nx + i] = (float)((d * d) * acc);
}

// --------------------------------------------------------------------------------------- K5
constexpr int L1_BLOCK = 256;
constexpr int L1_ITEMS = 16;   // elements per thread per block tile

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

// pass 1: per (model, chunk) partial sums of |y - pred| * mask and of mask (fp64, fixed order)
__global__ __launch_bounds__(L1_BLOCK) void k_l1_partial(int64_t n, const float *__restrict__ pred,
                                                         const float *__restrict__ y,
                                                         const float *__restrict__ mask,
                                                         double *__restrict__ part, int nchunk)
{
    __shared__ double sh[L1_BLOCK];
    const int b = blockIdx.y, c = blockIdx.x;
    const int64_t base = (int64_t)b * n;
    const int64_t c0 = (int64_t)c * L1_BLOCK * L1_ITEMS;
    double se = 0.0, sm = 0.0;
    float dv[L1_ITEMS], mv[L1_ITEMS];
#pragma unroll
    for (int k = 0; k < L1_ITEMS; ++k) {      // all loads first (clamped index, no branch per element)
        const int64_t j = min(c0 + (int64_t)k * L1_BLOCK + threadIdx.x, n - 1);
        mv[k] = mask ? mask[base + j] : 1.0f;
        dv[k] = fabsf(y[base + j] - pred[base + j]);
    }
#pragma unroll
    for (int k = 0; k < L1_ITEMS; ++k) {
        const int64_t j = c0 + (int64_t)k * L1_BLOCK + threadIdx.x;
        if (j < n) {
            se += (double)(dv[k] * mv[k]);
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

// pass 2: one workgroup per model; thread t sums chunks t, t + 256, ... in chunk order, then a fixed
// tree (deterministic).  (One thread per model summed 11.7 k chunks serially at configs[4]: 250 us.)
__global__ __launch_bounds__(L1_BLOCK) void k_l1_final(int B, int nchunk, const double *__restrict__ part,
                                                       float *loss, float *nobs)
{
    __shared__ double sh[L1_BLOCK];
    const int b = blockIdx.x;
    const double *pb = part + (size_t)b * nchunk * 2;
    double se = 0.0, sm = 0.0;
    int c = threadIdx.x;
    for (; c + 7 * L1_BLOCK < nchunk; c += 8 * L1_BLOCK) {   // eight independent loads in flight
        double e[8], m[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { e[u] = pb[(c + u * L1_BLOCK) * 2]; m[u] = pb[(c + u * L1_BLOCK) * 2 + 1]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { se += e[u]; sm += m[u]; }
    }
    for (; c < nchunk; c += L1_BLOCK) { se += pb[c * 2]; sm += pb[c * 2 + 1]; }
    se = block_sum(se, sh);
    sm = block_sum(sm, sh);
    if (threadIdx.x == 0) {
        const float no = fmaxf((float)sm, 1.0f);
        nobs[b] = no;
        loss[b] = (float)(se / (double)no);
    }
}

__global__ __launch_bounds__(256) void k_l1_backward(int B, int64_t n, const float *__restrict__ pred,
                                                     const float *__restrict__ y,
                                                     const float *__restrict__ mask,
                                                     const float *__restrict__ nobs,
                                                     const float *__restrict__ gout,
                                                     float *__restrict__ dpred)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (j >= n) return;
    const int64_t i = (int64_t)b * n + j;
    const float g = gout[b] / nobs[b];
    const float m = mask ? mask[i] : 1.0f;
    const float d = pred[i] - y[i];
    const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    dpred[i] = sg * (m * g);
}

// --------------------------------------------------------------------------------------- K6
__global__ __launch_bounds__(256) void k_smooth_fwd(int kind, int H, int W, const float *__restrict__ mu,
                                                    float *loss)
{
    __shared__ double sh[256];
    const int b = blockIdx.x;
    const float *m = mu + (size_t)b * H * W;
    double sx = 0.0, sy = 0.0;
    const int n = H * W;
    // each thread's elements in its original order, their loads issued 8 at a time (same sums)
    constexpr int CH = 8;
    for (int base = threadIdx.x; base < n; base += CH * blockDim.x) {
        float c[CH], r[CH], d[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int i = base + u * blockDim.x;
            const int z = i / W, x = i - z * W;
            c[u] = i < n ? m[i] : 0.0f;
            r[u] = (i < n && x + 1 < W) ? m[i + 1] : 0.0f;
            d[u] = (i < n && z + 1 < H) ? m[i + W] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int i = base + u * blockDim.x;
            if (i >= n) break;
            const int z = i / W, x = i - z * W;
            if (x + 1 < W) { const float e = r[u] - c[u]; sx += kind == 0 ? (double)fabsf(e) : (double)(e * e); }
            if (z + 1 < H) { const float e = d[u] - c[u]; sy += kind == 0 ? (double)fabsf(e) : (double)(e * e); }
        }
    }
    sx = block_sum(sx, sh);
    sy = block_sum(sy, sh);
    if (threadIdx.x == 0) {
        const float tx = (float)(sx / (double)((size_t)H * (W - 1)));
        const float ty = (float)(sy / (double)((size_t)(H - 1) * W));
        loss[b] = tx + ty;
    }
}

__global__ __launch_bounds__(256) void k_smooth_bwd(int kind, int H, int W, const float *__restrict__ mu,
                                                    const float *__restrict__ gout, float *__restrict__ grad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= H * W) return;
    const float *m = mu + (size_t)b * H * W;
    const int z = i / W, x = i - z * W;
    const float gx = gout[b] / (float)((size_t)H * (W - 1));
    const float gy = gout[b] / (float)((size_t)(H - 1) * W);
    auto dterm = [&](float d, float g) {
        if (kind == 0) return d > 0.0f ? g : (d < 0.0f ? -g : 0.0f);
        return 2.0f * d * g;
    };
    float acc = 0.0f;
    if (x + 1 < W) acc -= dterm(m[i + 1] - m[i], gx);
    if (x > 0) acc += dterm(m[i] - m[i - 1], gx);
    if (z + 1 < H) acc -= dterm(m[i + W] - m[i], gy);
    if (z > 0) acc += dterm(m[i] - m[i - W], gy);
    grad[(size_t)b * H * W + i] = acc;
}

}  // namespace

// ======================================================================================= plan
struct GraphEntry {
    int kind;                 // 0 fwd-history, 1 fwd-ring, 2 adjoint, 3 fwd-checkpoint, 4 adjoint-checkpoint, 5 born,
                              // 6 fused forward + born; + 8: the same pass with the call's own wavelets;
                              // + 16: with an encoding (rdq_fwi_*_enc)
    int B;
    int K;                    // checkpoint interval (kinds 3, 4, 6; else 0): it shapes the launch sequence
    const void *ptrs[10];     // the call's buffers; a per-call source adds its wav and gwav
    long long strides[4];     // and its wavelet strides (else 0); an encoding: its three strides and ne
    hipGraphExec_t exec;
    uint64_t last_use;
};

// default pre-sweep delays of the persistent forward / adjoint, 10 ns ticks (PT_SWEEP_DELAY)
constexpr int RDQ_SWEEP_DELAY_FWD = 15, RDQ_SWEEP_DELAY_ADJ = 0;
// default hand-off overlap mode of the persistent adjoint (rdq_fwi_set_handoff_overlap); mode 1 exists at
// PT_OV_T steps per epoch
constexpr int RDQ_OVERLAP_ADJ = 1, PT_OV_T = 4;
// default source-role mode of the persistent forward (rdq_fwi_set_source_role)
constexpr int RDQ_SROLE_FWD = 1;
// default fetch mode of the adjoint's source/receiver role (rdq_fwi_set_adjoint_fetch): the residuals a step ahead
constexpr int RDQ_ADJ_FETCH = 1;

struct rdq_fwi_plan {
    rdq_fwi_geom g;
    std::vector<int32_t> isx, igx;
    std::vector<double> wav;
    std::vector<float> wavf;
    int Hp, Wp, ld, nrec;
    int *d_isx = nullptr, *d_rcv_start = nullptr, *d_rcv_list = nullptr;
    int *d_src_table = nullptr; // sources by padded column, as the receivers: {src_start [Wp + 1], src_list [ns]} (FwdTBArgs)
    int *d_rlane = nullptr;     // [Wp] adjoint residual index per column (receiver id, or folded column)
    int *d_colx = nullptr;      // [ncolr] padded column of each receiver column (fold)
    int ncolr = 0;              // columns holding a receiver
    bool rmulti = false;        // some column holds several receivers: residuals folded per column
    float *d_wav = nullptr;     // fp32 wavelet [nt] (persistent kernels)
    unsigned *d_status = nullptr;   // status words in use: d_status_own or a caller buffer (rdq_fwi_set_status_buffer)
    unsigned *d_status_own = nullptr;
    unsigned long long *d_prof = nullptr;   // phase counters (rdq_fwi_set_profile): fwd, then adj
    std::vector<unsigned long long> prof_host;
    bool graphs = true;
    int persist = 1;            // 0 off, 1 auto, 8 / 12: persistent kernels with that region height (waves),
                                // -1: persistent launches oversubscribed 2x past residency (fault-path test)
    int xcd_mode = 1;           // persistent kernels: XCD-local slices with L2 hand-offs (pt_assign)
    std::vector<std::pair<const void *, int>> resident;   // resident workgroups per persistent kernel
                                                          // queried so far (resident_capacity)
    int fwd_rw = 6, adj_rw = 6;   // rows per wave of the 96-row persistent kernels (rdq_fwi_set_rows_per_wave;
                                  // adjoint 6: 1.649 vs 1.672 ms for 8, profiles/r3/adj_rows_nb_ab.txt)
    int fwd_T = 4, adj_T = 4;   // time steps per launch (temporal blocking depth), <= TB_MAXT
    int fwd_delay = RDQ_SWEEP_DELAY_FWD, adj_delay = RDQ_SWEEP_DELAY_ADJ;   // persistent kernels' pre-sweep delay (ticks)
    int adj_ov = RDQ_OVERLAP_ADJ;   // the persistent (recurrence) adjoint's hand-off overlap mode
    int adj_roles = 1;              // wave roles of the persistent (recurrence) adjoint (rdq_fwi_set_wave_roles)
    int fwd_srole = RDQ_SROLE_FWD;  // source role of the persistent forward (rdq_fwi_set_source_role)
    int adj_srole = 1;              // source/receiver role of the persistent adjoint (rdq_fwi_set_adjoint_role)
    int adj_fetch = RDQ_ADJ_FETCH;  // that role's residual / sample fetch: 0 an epoch ahead, 1 a step ahead (rdq_fwi_set_adjoint_fetch)
    int adj_Tw = 0;             // the wide chunked adjoint's depth (<= TW_ADJ_MAXT); 0 = auto, see wide_adj_depth
    int fwd_Tw = 0;             // the wide chunked forward's depth (<= TW_FWD_MAXT); 0 = auto, see wide_fwd_depth
    int adj_spw = 0;            // the wide chunked adjoint's shots per workgroup, 0 = auto (wide_spw)
    int fwd_spw = 0;            // the wide chunked forward's, 0 = auto
    int chains = 0;             // independent shot groups launched as concurrent chains; 0 = auto (chain_count)
    bool fwd_gen = true;        // chunked forward regenerates coefficients from the model (vs loading K3)
    bool adj_fma = true;        // persistent adjoint with FMA contraction (vs the oracle's exact op order)
    bool adj_tw_fma = false;    // wide chunked adjoint with FMA contraction (RDQ_VARIANT_CHUNKED_ADJ_FMA; default:
                                // the oracle's exact order, bitwise gA / gbeta / gk terms)
    bool wide = true;           // chunked kernels on 128-column regions (k_fwd_tw / k_adj_tw) vs 64-column
    hipStream_t cap = nullptr;
    std::vector<hipStream_t> aux;
    std::vector<hipEvent_t> evs;   // [0] fork, [1..] joins (inside graph capture: graph edges)
    std::vector<GraphEntry> cache;
    uint64_t tick = 0;
    // One call in flight per plan: the host state above (graph cache, chain streams and events) is
    // guarded by `mu`, and a time-loop call on another stream than the previous one first waits on an
    // event recorded on that stream at this point (`handover`), so calls on one plan from several
    // streams run one after the other on the device (the persistent launches share the plan's arrival
    // counters and each needs the whole chip; the chunked launches share the chain streams).
    std::mutex mu;
    hipStream_t last = nullptr;
    bool have_last = false;
    hipEvent_t handover = nullptr;
};

namespace {

int tiles_x(int Wp, int T) { return (Wp + (64 - 4 * T) - 1) / (64 - 4 * T); }
int tiles_y(int Hp, int T) { return (Hp + (TB_RH - 4 * T) - 1) / (TB_RH - 4 * T); }


// nwf: wavefields per model, the plan's shots or an encoded call's supershots
TBGeo tb_geo(const rdq_fwi_plan *p, int B, int nwf)
{
    TBGeo g;
    g.B = B; g.ns = nwf; g.Hp = p->Hp; g.Wp = p->Wp; g.ld = p->ld;
    g.isz = p->g.isz; g.igz = p->g.igz; g.ng = p->g.ng; g.nrec = p->nrec; g.st = p->g.sample_temporal;
    g.slice = (size_t)p->Hp * p->ld;
    g.cstride = (size_t)B * g.slice;
    g.level = (size_t)B * g.ns * g.slice;
    g.isx = p->d_isx; g.rcv_start = p->d_rcv_start; g.rcv_list = p->d_rcv_list;
    g.rlane = p->d_rlane; g.dstride = p->rmulti ? p->ncolr : p->g.ng;
    g.s_off = 0; g.ns_grp = nwf;
    g.sl_off = 0; g.nsl = B * nwf;
    return g;
}
TBGeo tb_geo(const rdq_fwi_plan *p, int B) { return tb_geo(p, B, p->g.ns); }

// Shots split into `chains` groups, each a dependent chain of launches on its own stream, forked
// from and joined back into `st` with events (inside graph capture this records parallel graph
// branches).  Concurrent chains overlap each launch's fixed latency (prologue loads, store
// drain, dispatch) with the other chains' compute.
// Concurrent launch chains of a chunked time loop.  Auto: two for the wide kernels (each chain's
// launches fill the other's tail rounds: configs[4] forward 54.7 -> 49.0-50.0 ms, adjoint 93.8 ->
// 91.0-91.6; 3 / 4 / 8 chains 51.7 / 53.9 / 58.0 and 93.1 / 95.1 / 101.2; profiles/r5/configs4_chains.jsonl),
// one for the 64-column kernels.
int chain_count(const rdq_fwi_plan *p, bool wide, int nwf)
{
    const int c = p->chains > 0 ? p->chains : (wide ? 2 : 1);
    return std::max(1, std::min(c, nwf));
}
int chain_count(const rdq_fwi_plan *p, bool wide) { return chain_count(p, wide, p->g.ns); }
int chain_count(const rdq_fwi_plan *p) { return chain_count(p, p->wide); }

// Default depth of the wide chunked adjoint, measured at configs[4] (profiles/r5/configs4_wide_adj_depth.jsonl):
// 5 steps per launch is the fastest for both forms (exact order 116.1-116.3 ms vs 120.4 at 4 and 120.6
// at 6; contracted 111.2 ms vs 115.1-115.7 at 6).
constexpr int TW_ADJ_DEFAULT = 5;
int wide_adj_depth(const rdq_fwi_plan *p) { return p->adj_Tw > 0 ? p->adj_Tw : TW_ADJ_DEFAULT; }
// Default depth of the wide chunked forward: rdq_fwi_set_tuning's fwd_steps (the persistent kernels'
// depth, <= 4) unless rdq_fwi_set_wide_fwd_steps chose one (<= TW_FWD_MAXT)
int wide_fwd_depth(const rdq_fwi_plan *p) { return p->fwd_Tw > 0 ? p->fwd_Tw : p->fwd_T; }

// Compute units of the device the plan's launches run on, cached per device (a process may drive
// several GPUs; the count is queried once per device id).
int device_cus()
{
    constexpr int MAXDEV = 64;
    static std::atomic<int> cache[MAXDEV];               // 0 = not queried yet
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev >= 0 && dev < MAXDEV && (n = cache[dev].load(std::memory_order_relaxed)) > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    if (dev >= 0 && dev < MAXDEV) cache[dev].store(n, std::memory_order_relaxed);
    return n;
}

// Shots per workgroup of a wide forward / adjoint launch over `regions` (models x tiles) of `ns` shots.  A
// workgroup generates its region's coefficients once for all its shots and pays its fixed start-up
// once, so more is cheaper per shot, but a workgroup of many shots is a long indivisible unit.  Cost
// model: rounds of one workgroup per CU x (shots per workgroup + kappa), kappa = a workgroup's fixed
// cost in shots, fitted at configs[4] (profiles/r5/configs4_adj_spw.jsonl, configs4_fwd_spw.jsonl):
// forward 0.6, adjoint 0.25; the cheapest of 16 / 8 / 4 / 2 / 1 (ties: more shots).  `chains` launch
// chains run concurrently and share the CUs, so one chain's launch gets cus / chains of them.
// configs[4] (16 shots in two chains of 8, 203 forward / 510 adjoint regions): 8 for both; with one
// chain, 16 for both (forward 57.5 -> 54.9 ms, adjoint 94.9 -> 94.1 against 8: configs4_spw16.jsonl); a
// small grid (20 regions) keeps 1 for parallelism.
int wide_spw(int setting, int regions, int ns, bool adj, int chains)
{
    if (setting > 0) return std::max(1, std::min(setting, ns));
    const int cus = std::max(1, device_cus() / std::max(1, chains));
    const double kappa = adj ? 0.25 : 0.6;
    int pick = 1;
    double best = 1e300;
    for (const int c : {16, 8, 4, 2, 1}) {
        const int spw = std::min(c, ns), groups = (ns + spw - 1) / spw;
        const long long wgs = (long long)regions * groups, rounds = (wgs + cus - 1) / cus;
        const double cost = (double)rounds * (spw + kappa);
        if (cost < best - 1e-9) { best = cost; pick = spw; }
    }
    return pick;
}

// A time-loop call on `st` (caller holds p->mu): when the plan's previous call went to another
// stream, `st` first waits for everything that stream had queued by now (which includes that call),
// so calls on one plan never overlap on the device whatever streams they come on.  A steady caller
// (one stream) pays nothing.  Skipped while either stream is being captured into a graph: a captured
// stream cannot wait on an event recorded outside the capture (the caller orders captured work).
int plan_enter(rdq_fwi_plan *p, hipStream_t st)
{
    if (p->have_last && p->last != st) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone, cl = hipStreamCaptureStatusNone;
        RDQ_CHECK(hipStreamIsCapturing(st, &cs));
        RDQ_CHECK(hipStreamIsCapturing(p->last, &cl));
        if (cs == hipStreamCaptureStatusNone && cl == hipStreamCaptureStatusNone) {
            if (!p->handover) RDQ_CHECK(hipEventCreateWithFlags(&p->handover, hipEventDisableTiming));
            RDQ_CHECK(hipEventRecord(p->handover, p->last));
            RDQ_CHECK(hipStreamWaitEvent(st, p->handover, 0));
        }
    }
    p->last = st;
    p->have_last = true;
    return 0;
}

// The chunked adjoints accumulate each workgroup's sponge partial into gk_part[(b * ns + shot) * nblk
// + tile]: the narrow kernel with a load-add-store, the wide one with a no-return fp64 atomic add.  Both
// are deterministic (and the load-add-store race-free) only if every slot has ONE writer per launch
// (the adds of a slot then arrive launch after launch, in stream order) and no slot is written by two
// concurrent launch chains.  GkWriters replays the kernels' own block decode (decode_tile, the
// shot-group split of k_adj_tw / k_adj_tb) for every launch of a time loop on the host, when the loop
// is enqueued (once per captured graph), and refuses the call (RDQ_E_INVALID) on a violation or on a
// slot outside the caller's gk_part buffer.
struct GkWriters {
    std::vector<int> chain;          // chain that owns the slot (-1: none yet)
    std::vector<unsigned> stamp;     // last launch that wrote it
    unsigned launch = 0;
    int nblk;
    GkWriters(size_t slices, int nblk_) : chain(slices * nblk_, -1), stamp(slices * nblk_, 0u), nblk(nblk_) {}
    // one launch of chain c: grid blocks, tile grid, B models x ns shots, shot group [s_off, s_off + ns_sh)
    // split in groups of spw shots (ns_grp groups)
    bool add(int c, unsigned grid, int tiles_x, int ntiles, int B, int ns, int ns_grp, int s_off, int spw, int ns_sh)
    {
        ++launch;
        const int nsg = B * ns_grp;
        for (unsigned L = 0; L < grid; ++L) {
            const TileId ti = decode_tile((int)L, tiles_x, ntiles, nsg);
            if (!ti.valid) continue;
            if (ti.tile >= nblk) return false;
            const int b = ti.sl / ns_grp, jg = ti.sl - b * ns_grp;
            const int s_first = s_off + jg * spw, nsh = std::min(spw, ns_sh - jg * spw);
            for (int sh = 0; sh < nsh; ++sh) {
                const size_t slot = (size_t)(b * ns + s_first + sh) * nblk + ti.tile;
                if (s_first + sh >= ns || slot >= chain.size()) return false;
                if (stamp[slot] == launch || (chain[slot] >= 0 && chain[slot] != c)) return false;
                stamp[slot] = launch;
                chain[slot] = c;
            }
        }
        return true;
    }
};

int ensure_aux(rdq_fwi_plan *p, int S)
{
    while ((int)p->aux.size() < S - 1) {
        hipStream_t s;
        RDQ_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        p->aux.push_back(s);
    }
    while ((int)p->evs.size() < S) {
        hipEvent_t e;
        RDQ_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        p->evs.push_back(e);
    }
    return 0;
}

int fork_chains(rdq_fwi_plan *p, hipStream_t st, int S)
{
    if (S == 1) return 0;
    RDQ_TRY(ensure_aux(p, S));
    RDQ_CHECK(hipEventRecord(p->evs[0], st));
    for (int c = 1; c < S; ++c) RDQ_CHECK(hipStreamWaitEvent(p->aux[c - 1], p->evs[0], 0));
    return 0;
}

int join_chains(rdq_fwi_plan *p, hipStream_t st, int S)
{
    for (int c = 1; c < S; ++c) {
        RDQ_CHECK(hipEventRecord(p->evs[c], p->aux[c - 1]));
        RDQ_CHECK(hipStreamWaitEvent(st, p->evs[c], 0));
    }
    return 0;
}

// coeffs buffer: [6][B][Hp][ld] fields, then v_model [B][nz][nx], then ks [B]
CoefGen coef_gen(const rdq_fwi_plan *p, int B, const float *coeffs)
{
    CoefGen c;
    const size_t cstride = (size_t)B * p->Hp * p->ld;
    c.vmod = coeffs + 6 * cstride;
    c.ks = c.vmod + (size_t)B * p->g.nz * p->g.nx;
    c.nz = p->g.nz; c.nx = p->g.nx; c.nbc = p->g.nbc; c.Hp = p->Hp; c.Wp = p->Wp;
    c.dt = p->g.dt; c.dx = p->g.dx;
    c.a = (float)((double)(p->g.nbc - 1) * (double)p->g.dx);
    return c;
}

// ---- Kernel tables.  One function per kernel family maps the plan's settings to an instantiation:
// the kernel and its workgroup size.  Every launch and every occupancy query goes through them, so the
// two cannot disagree about which kernel a setting means.
template <class Args>
struct KernelRef {
    void (*fn)(Args);
    int threads;
};

template <class Args>
void launch_kernel(KernelRef<Args> k, unsigned grid, hipStream_t st, const Args &a)
{
    void *argv[] = {const_cast<Args *>(&a)};
    (void)hipLaunchKernel(reinterpret_cast<const void *>(k.fn), dim3(grid), dim3(k.threads), argv, 0, st);
}   // (a failed launch is reported by the caller's hipGetLastError)

// f(std::integral_constant<int, T>) for the run-time depth T in 1 .. N (the setters admit no other):
// the compile-time depth of a kernel instantiation
template <int N, class F>
auto with_depth(int T, F &&f)
{
    if constexpr (N == 1) return f(std::integral_constant<int, 1>{});
    else return T >= N ? f(std::integral_constant<int, N>{}) : with_depth<N - 1>(T, f);
}

// narrow chunked kernels (64 x 64 regions), instantiated at the plan's depth T
KernelRef<FwdTBArgs> fwd_tb_kernel(int T, bool gen)
{
    return with_depth<TB_MAXT>(T, [&](auto t) -> KernelRef<FwdTBArgs> {
        return {gen ? k_fwd_tb<t(), true> : k_fwd_tb<t(), false>, 64 * TB_NW};
    });
}
KernelRef<AdjTBArgs> adj_tb_kernel(int T)
{
    return with_depth<TB_MAXT>(T, [](auto t) -> KernelRef<AdjTBArgs> { return {k_adj_tb<t()>, 64 * TB_NW}; });
}
// the same two with the call's own wavelets (rdq_fwi_*_src)
KernelRef<FwdTBArgs> fwd_tb_src_kernel(int T, bool gen)
{
    return with_depth<TB_MAXT>(T, [&](auto t) -> KernelRef<FwdTBArgs> {
        return {gen ? k_fwd_tb<t(), true, SRC_CALL> : k_fwd_tb<t(), false, SRC_CALL>, 64 * TB_NW};
    });
}
KernelRef<AdjTBArgs> adj_tb_src_kernel(int T)
{
    return with_depth<TB_MAXT>(T, [](auto t) -> KernelRef<AdjTBArgs> { return {k_adj_tb<t(), SRC_CALL>, 64 * TB_NW}; });
}
// and with an encoding (rdq_fwi_*_enc)
KernelRef<FwdTBArgs> fwd_tb_enc_kernel(int T, bool gen)
{
    return with_depth<TB_MAXT>(T, [&](auto t) -> KernelRef<FwdTBArgs> {
        return {gen ? k_fwd_tb<t(), true, SRC_ENC> : k_fwd_tb<t(), false, SRC_ENC>, 64 * TB_NW};
    });
}
KernelRef<AdjTBArgs> adj_tb_enc_kernel(int T)
{
    return with_depth<TB_MAXT>(T, [](auto t) -> KernelRef<AdjTBArgs> { return {k_adj_tb<t(), SRC_ENC>, 64 * TB_NW}; });
}
KernelRef<BornTBArgs> born_tb_kernel(int T, bool gen)
{
    return with_depth<TB_MAXT>(T, [&](auto t) -> KernelRef<BornTBArgs> {
        return {gen ? k_born_tb<t(), true> : k_born_tb<t(), false>, 64 * TB_NW};
    });
}
KernelRef<FwdBornTBArgs> fwd_born_tb_kernel(int T, bool gen)
{
    return with_depth<TB_MAXT>(T, [&](auto t) -> KernelRef<FwdBornTBArgs> {
        return {gen ? k_fwd_born_tb<t(), true> : k_fwd_born_tb<t(), false>, 64 * TB_NW};
    });
}

// wide chunked regions: forward 16 waves x 8 rows (128 x 128), adjoint 16 waves x 4 rows (128 x 64:
// its seven two-column fields per row fill the 128 VGPRs of a 1024-thread workgroup)
constexpr int TW_FWD_NW = 16, TW_FWD_R = 8, TW_ADJ_NW = 16, TW_ADJ_R = 4;
static_assert(ADJ_W_MAX >= TW_ADJ_MAXT && ADJ_W_MAX >= TB_MAXT, "AdjTBArgs::w holds one sample per step of a launch");
int tw_tiles_x(int Wp, int T) { return (Wp + (TW_W - 4 * T) - 1) / (TW_W - 4 * T); }
int tw_tiles_y(int Hp, int T, bool adj)
{
    const int ih = (adj ? TW_ADJ_NW * TW_ADJ_R : TW_FWD_NW * TW_FWD_R) - 4 * T;
    return (Hp + ih - 1) / ih;
}

static_assert(FWD_W_MAX >= TW_FWD_MAXT && FWD_W_MAX >= TB_MAXT, "FwdTBArgs::w holds one sample per step of a launch");

// wide chunked kernels, instantiated at the launch's own step count (a short tail runs as its own depth);
// `pair`: an even padded width (two-column loads)
KernelRef<FwdTBArgs> fwd_tw_kernel(int T, bool gen, bool pair)
{
    constexpr int N = TW_FWD_NW, R = TW_FWD_R;
    return with_depth<TW_FWD_MAXT>(T, [&](auto t) -> KernelRef<FwdTBArgs> {
        if (gen) return {pair ? k_fwd_tw<t(), N, R, true, true> : k_fwd_tw<t(), N, R, true, false>, 64 * N};
        return {pair ? k_fwd_tw<t(), N, R, false, true> : k_fwd_tw<t(), N, R, false, false>, 64 * N};
    });
}
KernelRef<AdjTBArgs> adj_tw_kernel(int T, bool pair, bool exact)
{
    constexpr int N = TW_ADJ_NW, R = TW_ADJ_R;
    return with_depth<TW_ADJ_MAXT>(T, [&](auto t) -> KernelRef<AdjTBArgs> {
        if (exact) return {pair ? k_adj_tw<t(), N, R, true, true> : k_adj_tw<t(), N, R, false, true>, 64 * N};
        return {pair ? k_adj_tw<t(), N, R, true, false> : k_adj_tw<t(), N, R, false, false>, 64 * N};
    });
}

// Depth T of the chunked kernels a plan runs, and the kernel of one chunked launch of `nsteps` steps: the
// narrow kernels are instantiated at T whatever the launch's step count, the wide ones at `nsteps`.  (The
// wide adjoint runs the exact order unless RDQ_VARIANT_CHUNKED_ADJ_FMA asked for the contracted stencils,
// and only where nbc >= 20: a thin sponge's standing modes amplify the contraction.)
int chunk_depth(const rdq_fwi_plan *p, bool adj)
{
    if (p->wide) return adj ? wide_adj_depth(p) : wide_fwd_depth(p);
    return adj ? p->adj_T : p->fwd_T;
}
KernelRef<FwdTBArgs> chunk_fwd_kernel(const rdq_fwi_plan *p, int nsteps)
{
    return p->wide ? fwd_tw_kernel(nsteps, p->fwd_gen, (p->Wp & 1) == 0) : fwd_tb_kernel(p->fwd_T, p->fwd_gen);
}
KernelRef<AdjTBArgs> chunk_adj_kernel(const rdq_fwi_plan *p, int nsteps)
{
    return p->wide ? adj_tw_kernel(nsteps, (p->Wp & 1) == 0, !p->adj_tw_fma) : adj_tb_kernel(p->adj_T);
}

// Persistent kernels.  `NW` is the region class: 12 = 64 x 96 regions at the plan's rows per wave (6, 8,
// 12 or 24 rows: 16, 12, 8 or 4 waves per workgroup), 8 = 64 x 64 regions of 8 waves x 8 rows, 16 = 64 x 64
// regions of 16 waves x 4 rows.  The phase-profiled build exists only at T = 4.
template <int T, bool PROF>
KernelRef<FwdPtArgs> fwd_pt_T(int NW, int rw)
{
    if (NW == 16) return {k_fwd_pt<T, 16, 4, PROF>, 64 * 16};
    if (NW != 12) return {k_fwd_pt<T, 8, 8, PROF>, 64 * 8};
    switch (rw) {
    case 24: return {k_fwd_pt<T, 4, 24, PROF>, 64 * 4};
    case 12: return {k_fwd_pt<T, 8, 12, PROF>, 64 * 8};
    case 6: return {k_fwd_pt<T, 16, 6, PROF>, 64 * 16};
    default: return {k_fwd_pt<T, 12, 8, PROF>, 64 * 12};
    }
}
KernelRef<FwdPtArgs> fwd_pt_kernel(const rdq_fwi_plan *p, int NW, int T, bool prof)
{
    if (prof && T == 4) return fwd_pt_T<4, true>(NW, p->fwd_rw);
    return with_depth<TB_MAXT>(T, [&](auto t) { return fwd_pt_T<t(), false>(NW, p->fwd_rw); });
}
// The persistent adjoint: the FMA / recurrence build (k_adj_pr, the plan's rows per wave for 96-row
// regions) or the oracle's exact operation order (k_adj_pt, 8 rows per wave: the 16-wave class of 64-row
// regions pairs with its 8-wave kernel).
template <int T, bool PROF, int OV = 0>
KernelRef<AdjPtArgs> adj_pt_T(int NW, int rw, bool fma)
{
    if (!fma) {
        if (NW != 12) return {k_adj_pt<T, 8, PROF>, 64 * 8};
        return {k_adj_pt<T, 12, PROF>, 64 * 12};
    }
    if (NW == 16) return {k_adj_pr<T, 16, 4, PROF, OV>, 64 * 16};
    if (NW != 12) return {k_adj_pr<T, 8, 8, PROF, OV>, 64 * 8};
    switch (rw) {
    case 12: return {k_adj_pr<T, 8, 12, PROF, OV>, 64 * 8};
    case 6: return {k_adj_pr<T, 16, 6, PROF, OV>, 64 * 16};
    default: return {k_adj_pr<T, 12, 8, PROF, OV>, 64 * 12};
    }
}
// The hand-off overlap mode the persistent adjoint runs (0 = the plain order): mode 1 is built at PT_OV_T
// steps per epoch, for the recurrence adjoint.
int adj_overlap(const rdq_fwi_plan *p) { return p->adj_T == PT_OV_T && p->adj_fma ? p->adj_ov : 0; }
// The wave-role mode the persistent adjoint runs (0 = every wave the generic loop): the plain role is built
// at PT_ROLES_T steps per epoch, in the recurrence adjoint.
int adj_wave_roles(const rdq_fwi_plan *p) { return p->adj_T == PT_ROLES_T && p->adj_fma ? p->adj_roles : 0; }
// Whether a persistent launch of region class NW at depth T and `rw` rows per wave has a source/receiver
// wave (the source role, rdq_fwi_set_source_role): 96-row regions at PT_SROLE_RW rows per wave and PT_ROLES_T
// steps per epoch, source and receivers in one padded row, every step recorded, and the source row held by
// its owning region alone.  A live halo copy of it in the neighbouring region (a row of that region's
// dependence cone: PT_REGION_GEOM's rcy) repeats the source add in the generic loop every step, on the same
// path, so there the role is not run.
bool source_role_fits(const rdq_fwi_plan *p, int NW, int T, int rw)
{
    if (NW != 12 || T != PT_ROLES_T || rw != PT_SROLE_RW) return false;
    if (p->g.isz != p->g.igz || p->g.sample_temporal != 1) return false;
    const int H = 2 * T, RH = 96, IH = RH - 2 * H;       // the 96-row class (region_rows)
    for (int ty = 0; ty * IH < p->Hp; ++ty) {
        const int vh = std::min(IH, p->Hp - ty * IH);
        for (int rr = 0; rr < RH; ++rr) {
            const int uz = ty * IH - H + rr;
            const bool own = rr >= H && rr < RH - H && uz < p->Hp;
            if (((uz % p->Hp) + p->Hp) % p->Hp == p->g.isz && !own && rr - H < vh + H) return false;
        }
    }
    return true;
}
// The source-role mode a persistent forward launch runs (0 = none); it covers the plain loop too.  (A no-grad
// call keeps no history and runs the generic loop whatever the mode.)
int fwd_source_role(const rdq_fwi_plan *p, int NW) { return p->fwd_srole && source_role_fits(p, NW, p->fwd_T, p->fwd_rw); }
// Mirrored row pair (k_adj_pr's SR) of padded row `row` in the region that owns it: 96-row regions at
// PT_ROLES_T steps per epoch and PT_SROLE_RW rows per wave.  The owning tile row, the wave and the row in the
// wave depend on the row alone (PT_REGION_GEOM: own rows are region rows H .. RH - H - 1 of tile row row / IH),
// so the pair is the same for every tile, shot and model of a launch.
int role_row_pair(int row)
{
    constexpr int H = 2 * PT_ROLES_T, IH = 96 - 2 * H, R = PT_SROLE_RW;
    const int r = (row % IH + H) % R;                    // row in wave of region row (row - ty IH) + H
    return r < R / 2 ? r : R - 1 - r;
}
// Whether the persistent adjoint of region class NW runs its source/receiver role (rdq_fwi_set_adjoint_role),
// and with which row pair (-1 = no role): the recurrence adjoint with wave roles on, in a launch the source
// role fits (source_role_fits); the phase-profiled build has no role.  The one place that decides it: the
// kernel table, the capacity query and rdq_fwi_adjoint_role_info all ask here.
int adjoint_role_pair(const rdq_fwi_plan *p, int NW, bool prof)
{
    if (!p->adj_srole || prof || !p->adj_fma || adj_wave_roles(p) != 1) return -1;
    if (!source_role_fits(p, NW, p->adj_T, p->adj_rw)) return -1;
    return role_row_pair(p->g.isz);
}
// The fetch mode of the role's residuals and wavelet samples (rdq_fwi_set_adjoint_fetch; k_adj_pr's SA) that a
// launch with the role runs.
int adjoint_fetch(const rdq_fwi_plan *p, int NW, bool prof) { return adjoint_role_pair(p, NW, prof) >= 0 ? p->adj_fetch : 0; }
template <int OV, bool SA>
KernelRef<AdjPtArgs> adj_pr_role(int sr)
{
    constexpr int T = PT_ROLES_T, RW = PT_SROLE_RW;
    if (sr == 0) return {k_adj_pr<T, 16, RW, false, OV, 0, SA>, 64 * 16};
    if (sr == 1) return {k_adj_pr<T, 16, RW, false, OV, 1, SA>, 64 * 16};
    return {k_adj_pr<T, 16, RW, false, OV, 2, SA>, 64 * 16};
}
KernelRef<AdjPtArgs> adj_pt_kernel(const rdq_fwi_plan *p, int NW, int T, bool fma, bool prof)
{
    static_assert(PT_OV_T == 4, "the profiled and the overlap builds share their depth");
    static_assert(PT_ROLES_T == 4 && PT_SROLE_RW / 2 == 3, "adj_pr_role: the role's depth and its three row pairs");
    if (T == p->adj_T && fma == p->adj_fma) {
        const int sr = adjoint_role_pair(p, NW, prof);
        if (sr >= 0 && adjoint_fetch(p, NW, prof)) return adj_overlap(p) ? adj_pr_role<1, true>(sr) : adj_pr_role<0, true>(sr);
        if (sr >= 0) return adj_overlap(p) ? adj_pr_role<1, false>(sr) : adj_pr_role<0, false>(sr);
    }
    if (T == 4 && fma && adj_overlap(p))
        return prof ? adj_pt_T<4, true, 1>(NW, p->adj_rw, true) : adj_pt_T<4, false, 1>(NW, p->adj_rw, true);
    if (prof && T == 4) return adj_pt_T<4, true>(NW, p->adj_rw, fma);
    return with_depth<TB_MAXT>(T, [&](auto t) { return adj_pt_T<t(), false>(NW, p->adj_rw, fma); });
}

// Workgroups of a persistent kernel the device holds at once (occupancy query x CUs), remembered per
// kernel in the plan.
template <class Args>
int resident_capacity(rdq_fwi_plan *p, KernelRef<Args> k)
{
    const void *fn = reinterpret_cast<const void *>(k.fn);
    for (const auto &e : p->resident)
        if (e.first == fn) return e.second;
    int dev = 0, cus = 0, nb = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, k.threads, 0) != hipSuccess) return -1;
    if (cus * nb) p->resident.emplace_back(fn, cus * nb);
    return cus * nb;
}

// Resident capacity of the persistent kernel a call would launch.  The adjoint's launch must fit both
// adjoint variants of the class, whichever one adj_fma selects; each is asked for as launch_adjoint_pt asks
// (the phase-profiled build while the profile is on: it has no source/receiver role).
int capacity_nw(rdq_fwi_plan *p, int NW, bool adj, int T)
{
    if (!adj) return resident_capacity(p, fwd_pt_kernel(p, NW, T, false));
    const bool prof = p->d_prof != nullptr;
    return std::min(resident_capacity(p, adj_pt_kernel(p, NW, T, false, prof)),
                    resident_capacity(p, adj_pt_kernel(p, NW, T, true, prof)));
}

// rows of a persistent region of class NW (fwd_pt_T)
static int region_rows(int NW) { return NW == 12 ? 96 : 64; }

// tiles (padded to the 8-XCD deal) of one (model, shot) slice at depth T with NW-wave regions
unsigned pt_tiles_padded(const rdq_fwi_plan *p, int T, int NW)
{
    const int ih = region_rows(NW) - 4 * T;
    const int nt_ = tiles_x(p->Wp, T) * ((p->Hp + ih - 1) / ih);
    return (unsigned)((nt_ + 7) / 8 * 8);
}

// Per-(model, shot) slots of the sponge-term partials gk_part: one per tile of whichever kernel runs
// the adjoint (persistent classes, narrow or wide chunked, every depth T), sized to the largest tile
// count over all of them, so no region shape can outgrow the buffer the caller allocated
// (rdq_fwi_sizes) and the finalize sums (k_fin_rows: unused slots stay zero).
int gk_blocks(const rdq_fwi_plan *p)
{
    int n = 0;
    for (int T = 1; T <= TW_ADJ_MAXT; ++T)                                       // wide chunked (128 x 64)
        n = std::max(n, tw_tiles_x(p->Wp, T) * tw_tiles_y(p->Hp, T, true));
    for (int T = 1; T <= TB_MAXT; ++T) {
        n = std::max(n, tiles_x(p->Wp, T) * tiles_y(p->Hp, T));                  // narrow chunked (64 x 64)
        n = std::max(n, tw_tiles_x(p->Wp, T) * tw_tiles_y(p->Hp, T, true));      // wide chunked (128 x 64)
        for (int NW : {8, 12, 16}) {                                             // persistent region classes
            const int ih = region_rows(NW) - 4 * T;
            n = std::max(n, tiles_x(p->Wp, T) * ((p->Hp + ih - 1) / ih));
        }
    }
    return n;
}

// Slices (model x shot) per persistent launch: every slice of one launch must be resident at once,
// so a batch larger than the chip (e.g. 32 OpenFWI shots = 4 x 224 workgroups, or the reference's
// OpenFWI config of 25 models x 5 shots = 125 slices) runs as ceil(B ns / per) launches over
// consecutive runs of the flat slice index b * ns + s, of near-equal size; 0 = not even one slice fits.
int pt_slices_per_launch(const rdq_fwi_plan *p, int B, int T, int NW, int cap)
{
    if (cap <= 0) return 0;
    const unsigned per = (unsigned)cap / pt_tiles_padded(p, T, NW);
    if (per < 1) return 0;
    const int total = B * p->g.ns, groups = (total + (int)per - 1) / (int)per;
    return (total + groups - 1) / groups;
}

// grid of a persistent launch covering S slices.  A slice is XCD-local (L2 hand-offs,
// pt_assign) only if one XCD received all its Tt workgroups; blocks are dealt round-robin over the
// 8 XCDs, so a launch of S slices gets that for every slice only with >= 8 Tt ceil(S / 8) blocks.
// Launches of fewer than 8 slices (e.g. the reference's 5-shot survey: 5 x 32 = 160 blocks, 20 per
// XCD) are padded up to it when the chip holds that many; the surplus blocks find no slice and exit.
unsigned pt_grid(const rdq_fwi_plan *p, int T, int NW, int nsl, bool adj)
{
    const unsigned S = (unsigned)nsl;
    unsigned grid = pt_tiles_padded(p, T, NW) * S;
    if (p->xcd_mode) {
        const int ih = region_rows(NW) - 4 * T;
        const unsigned Tt = (unsigned)(tiles_x(p->Wp, T) * ((p->Hp + ih - 1) / ih));
        const unsigned want = 8u * Tt * ((S + 7u) / 8u);
        const int cap = capacity_nw(const_cast<rdq_fwi_plan *>(p), NW, adj, T);
        if (want > grid && (int)want <= cap) grid = want;
    }
    if (p->persist == -1) {   // fault-path test: a grid the device cannot hold resident at once
        const int cap = capacity_nw(const_cast<rdq_fwi_plan *>(p), NW, adj, T);
        grid = std::max(grid, 2u * (unsigned)std::max(cap, 1));
    }
    return grid;
}

// region height (waves) of the persistent kernel for this call, 0 = not resident -> chunked.
// Taller regions first: one workgroup per CU and less halo (64 x 96 vs 64 x 64).  `per` = slices
// per launch (the batch runs as ceil(B ns / per) launches).
// Small surveys first: a launch of at most PT_SMALL_WG workgroups in 64 x 64 regions of 16 waves x
// 4 rows runs each step with 2/3 of the 96-row kernels' per-wave work on CUs the 96-row launch leaves
// idle (profiles/r3/pt64_ab.txt, configs[1] geometry: 3 shots = 168 workgroups, forward 1.30 -> 1.14
// ms, adjoint 1.65 -> 1.44; at 5 shots, 280, no slice fits one XCD and it is slower).
constexpr unsigned PT_SMALL_WG = 200;
int persistent_nw(rdq_fwi_plan *p, int B, bool adj, int *per = nullptr)
{
    if (!p->persist) return 0;
    const int T = adj ? p->adj_T : p->fwd_T;
    const int want = p->persist == -1 ? 1 : p->persist;   // 1 = auto, 8 / 12 / 16 = forced
    if (want == 1 || want == 16) {
        const int k = pt_slices_per_launch(p, B, T, 16, capacity_nw(p, 16, adj, T));
        const bool small = k >= B * p->g.ns && pt_tiles_padded(p, T, 16) * (unsigned)(B * p->g.ns) <= PT_SMALL_WG;
        if (k > 0 && (want == 16 || small)) { if (per) *per = k; return 16; }
    }
    if (want == 1 || want == 12) {
        const int k = pt_slices_per_launch(p, B, T, 12, capacity_nw(p, 12, adj, T));
        if (k > 0) { if (per) *per = k; return 12; }
    }
    if (want == 1 || want == 8) {
        const int k = pt_slices_per_launch(p, B, T, 8, capacity_nw(p, 8, adj, T));
        if (k > 0) { if (per) *per = k; return 8; }
    }
    return 0;
}

// The buffers a launch needs zeroed (granules, accumulators, history slots, adjoint levels, pt_assign's
// arrival counters) in ONE stream-ordered kernel instead of a memset each (each memset is a separate
// ~5 us dispatch on the step's critical path).  Sizes are multiples of 4 B; 16-byte-aligned regions are
// cleared with 16-byte stores, others with 4-byte ones.
// The chunked launchers run inside hipGraph capture (run_cached), and they must not use
// hipMemsetAsync there: on this ROCm (7.2) the captured memset node (present and first in the chain:
// profiles/r5/graph_replay/captured_memset_node.dot.txt) takes effect on the graph exec's first launch
// but not on its replays, which then read whatever the buffer held (tools/diag_graph_rawmem.py on
// hipMalloc'd buffers; the minimal memset + kernel-chain graphs of tools/repro/graph_kernarg.hip
// replay correctly, so the trigger is not isolated).  The zeroing kernel replays correctly.
constexpr int ZERO_MAXR = 6;
struct ZeroArgs {
    void *p[ZERO_MAXR];
    size_t n[ZERO_MAXR];      // bytes
    int nr;
};
__global__ __launch_bounds__(256) void k_zero_regions(ZeroArgs z)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int r = 0; r < z.nr; ++r) {
        if ((reinterpret_cast<uintptr_t>(z.p[r]) & 15) == 0) {
            uint4 *q = static_cast<uint4 *>(z.p[r]);
            const size_t n4 = z.n[r] / 16;
            for (size_t i = t; i < n4; i += stride) q[i] = make_uint4(0u, 0u, 0u, 0u);
            const size_t tail = (z.n[r] - n4 * 16) / 4;
            if (t < tail) reinterpret_cast<unsigned *>(q + n4)[t] = 0u;
        } else {
            unsigned *q = static_cast<unsigned *>(z.p[r]);
            for (size_t i = t; i < z.n[r] / 4; i += stride) q[i] = 0u;
        }
    }
}
static int zero_regions(std::initializer_list<std::pair<void *, size_t>> regs, hipStream_t st)
{
    ZeroArgs z{};
    size_t tot = 0;
    auto flush = [&]() -> int {
        if (!z.nr) return 0;
        const size_t blocks = std::min<size_t>(2048, std::max<size_t>(1, (tot / 16 + 255) / 256));
        hipLaunchKernelGGL(k_zero_regions, dim3((unsigned)blocks), dim3(256), 0, st, z);
        RDQ_CHECK(hipGetLastError());
        z = ZeroArgs{};
        tot = 0;
        return 0;
    };
    for (const auto &r : regs)                   // every region is 4-byte words: checked before any launch
        if (r.first && (r.second & 3)) return RDQ_E_INVALID;
    for (const auto &r : regs) {
        if (!r.first || !r.second) continue;
        if (z.nr == ZERO_MAXR) RDQ_TRY(flush());
        z.p[z.nr] = r.first;
        z.n[z.nr++] = r.second;
        tot += r.second;
    }
    return flush();
}

int launch_forward_pt(rdq_fwi_plan *p, int B, int NW, int per, const float *coeffs, float *seis, float *hist, float *ring,
                      hipStream_t st)
{
    FwdPtArgs a{};
    a.g = tb_geo(p, B);
    const int T = p->fwd_T;
    const size_t L = a.g.level;
    // granules, the history's first two slots and the first group's arrival counters: one launch
    if (int e = zero_regions({{hist, hist ? 2 * L * sizeof(float) : 0}, {ring, 4 * L * sizeof(unsigned long long)},
                              {p->d_status + 16, 8 * sizeof(unsigned)}}, st))
        return e;
    const int ih = region_rows(NW) - 4 * T;
    a.g.tiles_x = tiles_x(p->Wp, T);
    a.g.ntiles = a.g.tiles_x * ((p->Hp + ih - 1) / ih);
    a.coeffs = coeffs; a.wav = p->d_wav; a.hist = hist; a.seis = seis;
    a.gran = reinterpret_cast<unsigned long long *>(ring);
    a.status = p->d_status; a.nt = p->g.nt; a.prof = p->d_prof; a.xcd_mode = p->xcd_mode;
    a.sweep_delay = p->fwd_delay;
    a.srole = fwd_source_role(p, NW);
    // consecutive slice groups, one resident launch each (granules live at per-slice offsets, so
    // one zeroing serves every group)
    for (int s0 = 0; s0 < B * p->g.ns; s0 += per) {
        a.g.sl_off = s0;
        a.g.nsl = std::min(per, B * p->g.ns - s0);
        const unsigned grid = pt_grid(p, T, NW, a.g.nsl, false);
        if (s0 > 0) RDQ_TRY(zero_regions({{p->d_status + 16, 8 * sizeof(unsigned)}}, st));   // pt_assign arrivals
        launch_kernel(fwd_pt_kernel(p, NW, T, a.prof != nullptr), grid, st, a);
        RDQ_CHECK(hipGetLastError());
    }
    return 0;
}

int launch_adjoint_pt(rdq_fwi_plan *p, int B, int NW, int per, const float *coeffs, const float *hist, const float *dseis,
                      float *ring, float *gA, double *gk, float *gbeta, hipStream_t st)
{
    AdjPtArgs a{};
    a.g = tb_geo(p, B);
    const int T = p->adj_T;
    const size_t L = a.g.level;
    const int nblk_alloc = gk_blocks(p);
    if (int e = zero_regions({{ring, 4 * L * sizeof(unsigned long long)}, {gA, L * sizeof(float)},
                              {gk, (size_t)B * p->g.ns * nblk_alloc * sizeof(double)},
                              {gbeta, (size_t)B * p->g.ns * sizeof(float)},
                              // the arrival counters and, behind them, the call's role-wave count (PT_ROLE_WORD)
                              {p->d_status + 16, (PT_ROLE_WORD + 1 - 16) * sizeof(unsigned)}},
                             st))
        return e;
    const int ih = region_rows(NW) - 4 * T;
    a.g.tiles_x = tiles_x(p->Wp, T);
    a.g.ntiles = a.g.tiles_x * ((p->Hp + ih - 1) / ih);
    a.coeffs = coeffs; a.wav = p->d_wav; a.hist = hist; a.dseis = dseis;
    a.gA = gA; a.gk_part = gk; a.gbeta = gbeta;
    a.gran = reinterpret_cast<unsigned long long *>(ring);
    a.status = p->d_status; a.nt = p->g.nt; a.nblk = nblk_alloc; a.prof = p->d_prof ? p->d_prof + PROF_WORDS : nullptr;
    a.xcd_mode = p->xcd_mode;
    a.sweep_delay = p->adj_delay;
    a.roles = adj_wave_roles(p);
    for (int s0 = 0; s0 < B * p->g.ns; s0 += per) {
        a.g.sl_off = s0;
        a.g.nsl = std::min(per, B * p->g.ns - s0);
        const unsigned grid = pt_grid(p, T, NW, a.g.nsl, true);
        if (s0 > 0) RDQ_TRY(zero_regions({{p->d_status + 16, 8 * sizeof(unsigned)}}, st));   // pt_assign arrivals
        launch_kernel(adj_pt_kernel(p, NW, T, p->adj_fma, a.prof != nullptr), grid, st, a);
        RDQ_CHECK(hipGetLastError());
    }
    return 0;
}

// ---- Checkpointed gradient (rdq_fwi_forward_ckpt / rdq_fwi_adjoint_ckpt): the history bounded by
// recomputation.  Segments of K steps are counted from the END of the record: boundaries b_c =
// max(nt - c K, 0), c = 0 .. nseg = ceil(nt / K); segment c is the steps [b_{c+1}, b_c), the first one in
// time being the short one, so the adjoint's launches (k0 = nt, nt - T, ...) are those of a store-all run
// whenever K is a multiple of its depth.  Checkpoint c (0 < c < nseg) is the two levels {P_{b_c - 1},
// P_{b_c}} = the history's slots {b_c, b_c + 1}, pair c - 1 of the store; the boundary at 0 is two zero
// levels, produced by zeroing.
struct CkptPlan {
    int K, nseg;
    int lo(int c) const { return hi(c + 1); }                                   // segment c = steps [lo, hi)
    int hi(int c) const { return (int)std::max<long long>(nt - (long long)c * K, 0); }
    int nt;
};
CkptPlan ckpt_plan(const rdq_fwi_plan *p, int K)
{
    CkptPlan c;
    c.nt = p->g.nt;
    c.K = std::min(K, c.nt);
    c.nseg = (c.nt + c.K - 1) / c.K;
    return c;
}

// Levels {0, 1} of a segment buffer from a checkpoint pair (src == nullptr: zeros, the boundary at step
// 0), for the shots [s_off, s_off + ns_sh) of every model: each launch chain fills its own shots' slices,
// so the copy needs no ordering against the other chains.  (A kernel, not hipMemcpyAsync: the call is
// captured into a graph, see zero_regions.)  grid.y = 2 levels x B models.
__global__ __launch_bounds__(256) void k_ckpt_levels(const float *src, float *dst, size_t level, size_t model,
                                                     size_t off, size_t run, int B)
{
    const int lvl = blockIdx.y / B, b = blockIdx.y - lvl * B;
    const size_t base = (size_t)lvl * level + (size_t)b * model + off;   // (run <= model - off: inside the level)
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < run; i += stride)
        dst[base + i] = src ? src[base + i] : 0.0f;
}

// ---- The chunked time loops as data.  A chunked call is a schedule: per launch chain, the ordered list of
// its launches, built by chunked_schedule from the segments of a CkptPlan (store-all = the one-segment plan)
// and the plan's settings.  enqueue_chunked checks and launches it; rdq_fwi_launch_info, rdq_fwi_wide_info
// and rdq_fwi_ckpt_info count it.  The four passes:
//   fwd_ring  the no-grad forward (ring ping-pong, seismograms), its launches cut at the segment
//             boundaries: the launch that ends on an interior boundary writes its two output levels into
//             the checkpoint store instead of the ring, and the next launch reads them from there (no copy);
//   fwd_hist  the history form over one segment: level j of the buffer = slot hbase + j, levels 0 and 1
//             given (zeroed for the whole record, hbase = 0), every launch writes its steps' levels;
//   adj_hist  the adjoint over a stored history (one segment, hbase = 0);
//   adj_ckpt  per segment, from the last to the first: the segment buffer's levels 0 and 1 from the
//             checkpoint (k_ckpt_levels), the fwd_hist launches of the segment (hbase = lo: the recompute,
//             no seismograms), then its adjoint launches (dseis, wavelet and record indices stay absolute).
//   born      the linearised forward: the launches of fwd_ring over the one-segment plan (dP ping-pongs in the
//             ring), each also reading the stored history (hbase = 0).  Always the narrow kernels (k_born_tb) at
//             the forward's narrow depth, whatever the plan's wide or persistent settings are.
//   fwd_born  the forward and its tangent in one loop, no history (k_fwd_born_tb): the launches of fwd_ring over a
//             CkptPlan, cut at the segment boundaries.  The P pair follows fwd_ring's rule (ring levels 0-3, the
//             launch ending on an interior boundary writes its pair into the checkpoint store and the next reads
//             it there); the dP pair (in2 / out2) always ping-pongs in ring levels 4-7.  Narrow kernels at the
//             forward's narrow depth and chains, as born.
//   illum_hist  the illumination pass over a stored history: one k_illum_tb launch per chain over slots 1 .. nt;
//   illum_ckpt  adj_ckpt's schedule with the adjoint launches of a segment replaced by one illumination launch
//             over slots lo + 1 .. hi: the levels, the fwd_hist recompute, then illum (the first segment visited,
//             the last in time, starts the accumulator from zero).
// A call with its own wavelets (`src`: rdq_fwi_*_src) runs the same four passes on the narrow kernels' SRC
// instantiations at the narrow depths and chains, as born does; the wavelet and gwav indices are absolute, so a
// segment's recompute reads the samples the first pass read.
// The adjoint's levels stay in the ring between launches and the ring parity runs on across segments.
// Every launch of a chain is ordered on the chain's stream, so a segment's recompute overwrites the
// segment buffer only after the previous segment's adjoint has read it.
enum class Pass { fwd_ring, fwd_hist, adj_hist, adj_ckpt, born, fwd_born, illum_hist, illum_ckpt };
enum class Store { none, ring, ckpt, hist };
struct LevelPair {                   // two consecutive levels {slot, slot + 1} of a store (none: nullptr)
    Store store;
    int slot;
};
struct Launch {
    enum Kind { levels, fwd, adj, born, fwd_born, illum } kind;
    int chain, s_off, ns_sh;         // launch chain and its shots [s_off, s_off + ns_sh) of every model
    int first, nsteps;               // fwd: steps first, first + 1, ...; adj: steps first, first - 1, ...
    int seg, hbase;                  // segment, and the slot held by the history buffer's first level
    int tiles_x, ntiles, spw, ns_grp;   // tile grid of the launch's depth, shots per workgroup, shot groups
    unsigned grid;
    LevelPair in, out;               // levels read and written (fwd into a history: out = none)
    LevelPair in2, out2;             // fwd_born: the dP levels (in / out are its P levels)
};

// passes that always run the narrow (64-column) kernels at the forward's narrow depth
bool narrow_pass(Pass pass) { return pass == Pass::born || pass == Pass::fwd_born; }

// src: a call with its own wavelets or an encoding (narrow kernels); nwf: its wavefields per model, 0 = the plan's shots
std::vector<Launch> chunked_schedule(const rdq_fwi_plan *p, int B, Pass pass, const CkptPlan &cp, bool src = false,
                                     int nwf = 0)
{
    const bool wide = p->wide && !narrow_pass(pass) && !src, wide_pass = wide;
    const bool illum = pass == Pass::illum_hist || pass == Pass::illum_ckpt;
    const int Tf = wide ? wide_fwd_depth(p) : p->fwd_T, Ta = wide ? wide_adj_depth(p) : p->adj_T;
    const int ns = nwf > 0 ? nwf : p->g.ns, S = chain_count(p, wide, ns);
    std::vector<Launch> sched;
    auto add = [&](Launch::Kind kind, int c, int sg, int first, int nsteps, LevelPair in, LevelPair out) {
        Launch l{};
        l.kind = kind; l.chain = c; l.seg = sg; l.first = first; l.nsteps = nsteps; l.in = in; l.out = out;
        l.hbase = pass == Pass::fwd_ring || narrow_pass(pass) ? 0 : cp.lo(sg);
        l.s_off = c * ns / S;
        l.ns_sh = (c + 1) * ns / S - l.s_off;
        if (kind != Launch::levels) {
            // tile grid of this launch's depth (the wide kernels run a short tail as its own depth); wide
            // kernels: spw shots of one region per workgroup (the decode's slice groups are shot groups)
            const bool adj = kind == Launch::adj, wide = wide_pass && kind != Launch::illum;   // (k_illum_tb: the narrow depth-1 grid)
            const int Tl = kind == Launch::illum ? 1 : wide ? nsteps : (adj ? Ta : Tf);
            l.tiles_x = wide ? tw_tiles_x(p->Wp, Tl) : tiles_x(p->Wp, Tl);
            l.ntiles = l.tiles_x * (wide ? tw_tiles_y(p->Hp, Tl, adj) : tiles_y(p->Hp, Tl));
            l.spw = wide ? wide_spw(adj ? p->adj_spw : p->fwd_spw, B * l.ntiles, l.ns_sh, adj, S) : 1;
            l.ns_grp = (l.ns_sh + l.spw - 1) / l.spw;
            l.grid = (unsigned)((l.ntiles + 7) / 8 * 8 * B * l.ns_grp);
        }
        sched.push_back(l);
    };
    for (int c = 0; c < S; ++c) {
        int i = 0;                                               // ring parity: runs on across segments
        if (pass == Pass::fwd_ring || narrow_pass(pass)) {
            const Launch::Kind kind = pass == Pass::born       ? Launch::born
                                      : pass == Pass::fwd_born ? Launch::fwd_born
                                                               : Launch::fwd;
            for (int sg = cp.nseg - 1; sg >= 0; --sg) {
                const int lo = cp.lo(sg), hi = cp.hi(sg);
                for (int n0 = lo; n0 < hi; n0 += Tf, ++i) {
                    const int n = std::min(Tf, hi - n0), pin = i & 1, pout = pin ^ 1;
                    add(kind, c, sg, n0, n,
                        n0 == lo && lo > 0 ? LevelPair{Store::ckpt, 2 * sg} : LevelPair{Store::ring, 2 * pin},
                        n0 + n == hi && hi < cp.nt ? LevelPair{Store::ckpt, 2 * (sg - 1)} : LevelPair{Store::ring, 2 * pout});
                    sched.back().in2 = LevelPair{Store::ring, 4 + 2 * pin};
                    sched.back().out2 = LevelPair{Store::ring, 4 + 2 * pout};
                }                                                // (checkpoint sg = pair sg - 1 of the store)
            }
            continue;
        }
        for (int sg = 0; sg < cp.nseg; ++sg) {
            const int lo = cp.lo(sg), hi = cp.hi(sg);
            if (pass == Pass::adj_ckpt || pass == Pass::illum_ckpt)   // slots lo, lo + 1: checkpoint sg + 1 = pair sg, or zeros at the record's start
                add(Launch::levels, c, sg, lo, 0, lo > 0 ? LevelPair{Store::ckpt, 2 * sg} : LevelPair{Store::none, 0},
                    LevelPair{Store::hist, 0});
            if (pass != Pass::adj_hist && pass != Pass::illum_hist)   // slot n0 = P_{n0-1}, slot n0 + 1 = P_{n0}; writes slots lo + 2 .. hi + 1
                for (int n0 = lo; n0 < hi; n0 += Tf)
                    add(Launch::fwd, c, sg, n0, std::min(Tf, hi - n0), LevelPair{Store::hist, n0 - lo},
                        LevelPair{Store::none, 0});
            if (illum)                    // steps k = hi .. lo + 1 in one launch: slots lo + 1 .. hi
                add(Launch::illum, c, sg, hi, hi - lo, LevelPair{Store::none, 0}, LevelPair{Store::none, 0});
            else if (pass != Pass::fwd_hist)   // adjoint steps k = hi .. lo + 1: slots lo + 1 .. hi
                for (int k0 = hi; k0 > lo; k0 -= Ta, ++i) {
                    const int pin = i & 1, pout = pin ^ 1;
                    add(Launch::adj, c, sg, k0, std::min(Ta, k0 - lo), LevelPair{Store::ring, 2 * pin},
                        LevelPair{Store::ring, 2 * pout});
                }
        }
    }
    return sched;
}

// launches of one kind that chain 0 runs (every chain runs the same number)
int count_launches(const std::vector<Launch> &sched, Launch::Kind kind)
{
    int n = 0;
    for (const Launch &l : sched) n += l.chain == 0 && l.kind == kind;
    return n;
}

// The buffers of a chunked call; a pass leaves the ones it does not use null.  `hist` is the stored
// history or the checkpointed segment buffer.
struct ChunkBufs {
    const float *coeffs;
    float *seis, *hist, *ckpt, *ring;
    const float *dseis;
    float *gA;                       // (illum passes: hA)
    double *gk;
    float *gbeta;
    const float *dwork;              // born: the perturbation workspace (`seis` is then the linearised record)
    float *dseis_out;                // fwd_born: the linearised record (`seis` is the forward's)
    const rdq_fwi_source *src;       // the call's own wavelets (rdq_fwi_*_src), or nullptr: the plan's
    const rdq_fwi_encoding *enc;     // the call's encoding (rdq_fwi_*_enc): ne wavefields per model, every buffer
                                     // above with ns replaced by ne, gbeta [B][ne][ns]; or nullptr
    int nwf;                         // illum_hist: the history's wavefields per model (0: the plan's shots, or enc's ne)
};

// What every time-loop launch sets the same way in its kernel arguments: the launch's shots and tile grid, and the
// wavelet samples of its steps (forward kinds: w[first + t]; adjoint: w[first - 1 - t]; zero past nsteps).
template <int N>
void launch_geo_and_wavelet(TBGeo &g, float (&w)[N], const Launch &l, const std::vector<float> &wavf)
{
    g.s_off = l.s_off; g.ns_grp = l.ns_grp; g.tiles_x = l.tiles_x; g.ntiles = l.ntiles;
    const bool adj = l.kind == Launch::adj;
    for (int t = 0; t < N; ++t) w[t] = t < l.nsteps ? wavf[adj ? l.first - 1 - t : l.first + t] : 0.0f;
}

// an encoded launch's supershot stride, as the bits of w[0], w[1] (FwdTBArgs; the kernels' enc_stride)
void enc_stride_bits(float *w, long long stride)
{
    std::memcpy(w, &stride, sizeof(stride));
}

int enqueue_chunked(rdq_fwi_plan *p, int B, Pass pass, int K, const ChunkBufs &b, hipStream_t st)
{
    const bool enc = b.enc != nullptr, src = b.src != nullptr || enc;
    const int ns = enc ? b.enc->ne : b.nwf > 0 ? b.nwf : p->g.ns;        // wavefields per model
    const std::vector<Launch> sched = chunked_schedule(p, B, pass, ckpt_plan(p, K), src, ns);
    FwdTBArgs f{};
    AdjTBArgs a{};
    BornTBArgs d{};
    FwdBornTBArgs u{};
    f.g = a.g = d.g = u.g = tb_geo(p, B, ns);
    const size_t L = a.g.level, slice = a.g.slice;
    const int S = chain_count(p, p->wide && !narrow_pass(pass) && !src, ns), nblk_alloc = gk_blocks(p);
    const bool adjoint = pass == Pass::adj_hist || pass == Pass::adj_ckpt;
    const bool illum = pass == Pass::illum_hist || pass == Pass::illum_ckpt;
    IllumTBArgs il{};
    il.g = a.g; il.hist = b.hist; il.hA = b.gA;
    if (illum) {     // every illumination launch before anything is enqueued: its levels lie in the buffer it reads
        // (a stored history: slots 0 .. nt + 1; a segment buffer: K + 2 levels from hbase), its grid is the
        // depth-1 tile grid of its shots, and each chain's first launch (and only that one) starts hA from zero
        const int levels = pass == Pass::illum_hist ? p->g.nt + 2 : ckpt_plan(p, K).K + 2;
        for (const Launch &l : sched)
            if (l.kind == Launch::illum &&
                (l.nsteps < 1 || l.first - l.nsteps + 1 - l.hbase < 1 || l.first - l.hbase >= levels || l.spw != 1 ||
                 l.s_off < 0 || l.ns_sh < 1 || l.s_off + l.ns_sh > ns ||
                 l.ntiles != tiles_x(p->Wp, 1) * tiles_y(p->Hp, 1) ||
                 l.grid != (unsigned)((l.ntiles + 7) / 8 * 8 * B * l.ns_sh)))
                return RDQ_E_INVALID;
    }
    if (adjoint) {   // the gk_part one-writer invariant, on every adjoint launch, before anything is enqueued
        GkWriters writers((size_t)B * ns, nblk_alloc);
        for (const Launch &l : sched)
            if (l.kind == Launch::adj &&
                !writers.add(l.chain, l.grid, l.tiles_x, l.ntiles, B, ns, l.ns_grp, l.s_off, l.spw, l.ns_sh))
                return RDQ_E_INVALID;
    }
    // zeroed once, ahead of the chains (no hipMemsetAsync under graph capture: see zero_regions)
    if (adjoint)
        RDQ_TRY(zero_regions({{b.ring, 4 * L * sizeof(float)}, {b.gA, L * sizeof(float)},
                              {b.gk, (size_t)B * ns * nblk_alloc * sizeof(double)},
                              {b.gbeta, (size_t)B * ns * (enc ? p->g.ns : 1) * sizeof(float)}}, st));
    else if (pass == Pass::fwd_hist) RDQ_TRY(zero_regions({{b.hist, 2 * L * sizeof(float)}}, st));
    else if (illum) {}               // nothing to zero: k_ckpt_levels fills a segment's first levels, k_illum_tb starts hA
    else RDQ_TRY(zero_regions({{b.ring, (pass == Pass::fwd_born ? 8 : 4) * L * sizeof(float)}}, st));   // P, and dP in 4-7
    f.coeffs = a.coeffs = d.coeffs = u.coeffs = b.coeffs;
    f.cg = a.cg = d.cg = u.cg = coef_gen(p, B, b.coeffs);
    d.hist = b.hist; d.dseis = b.seis;
    d.dam = b.dwork;
    d.ratio = b.dwork ? b.dwork + (size_t)B * p->g.nz * p->g.nx : nullptr;
    d.dbeta = b.dwork ? d.ratio + B : nullptr;
    d.oscale = b.dwork ? d.dbeta + (size_t)B * p->g.ns : nullptr;
    u.dam = d.dam; u.ratio = d.ratio; u.dbeta = d.dbeta; u.oscale = d.oscale;
    u.seis = b.seis; u.dseis = b.dseis_out;
    f.seis = b.seis; f.hist = b.hist;
    a.hist = b.hist; a.dseis = b.dseis; a.gA = b.gA; a.gk_part = b.gk; a.gbeta = b.gbeta;
    a.nblk = nblk_alloc;
    if (enc) {
        f.wav = a.wav = b.enc->wav;
        f.wms = a.wms = b.enc->model_stride; f.wss = a.wss = b.enc->source_stride;
        f.g.isx = a.g.isx = p->d_src_table;          // (the source table; the supershot stride goes with each launch's w below)
        a.gwav = b.enc->gwav; a.nt = p->g.nt;
    } else if (src) {
        f.wav = a.wav = b.src->wav;
        f.wms = a.wms = b.src->model_stride; f.wss = a.wss = b.src->shot_stride;
        a.gwav = b.src->gwav; a.nt = p->g.nt;
    }
    auto level = [&](LevelPair lp, int j) -> float * {
        float *base = lp.store == Store::ring ? b.ring : lp.store == Store::ckpt ? b.ckpt
                      : lp.store == Store::hist ? b.hist : nullptr;
        return base ? base + (size_t)(lp.slot + j) * L : nullptr;
    };
    RDQ_TRY(fork_chains(p, st, S));
    for (const Launch &l : sched) {
        const hipStream_t cs = l.chain == 0 ? st : p->aux[l.chain - 1];
        if (l.kind == Launch::levels) {
            const size_t run = (size_t)l.ns_sh * slice;
            const unsigned gx = (unsigned)std::min<size_t>((run + 255) / 256, 1024);
            hipLaunchKernelGGL(k_ckpt_levels, dim3(gx, 2 * B), dim3(256), 0, cs, level(l.in, 0), level(l.out, 0), L,
                               (size_t)ns * slice, (size_t)l.s_off * slice, run, B);
        } else if (l.kind == Launch::fwd) {
            launch_geo_and_wavelet(f.g, f.w, l, p->wavf);
            if (enc) enc_stride_bits(f.w, b.enc->enc_stride);
            f.ns_sh = l.ns_sh; f.spw = l.spw;
            f.n0 = l.first; f.nsteps = l.nsteps; f.hbase = l.hbase;
            f.in_prev = level(l.in, 0); f.in_cur = level(l.in, 1);
            f.out_prev = level(l.out, 0); f.out_cur = level(l.out, 1);
            launch_kernel(enc   ? fwd_tb_enc_kernel(p->fwd_T, p->fwd_gen)
                          : src ? fwd_tb_src_kernel(p->fwd_T, p->fwd_gen)
                                : chunk_fwd_kernel(p, l.nsteps), l.grid, cs, f);
        } else if (l.kind == Launch::born) {
            launch_geo_and_wavelet(d.g, d.w, l, p->wavf);
            d.n0 = l.first; d.nsteps = l.nsteps;
            d.in_prev = level(l.in, 0); d.in_cur = level(l.in, 1);
            d.out_prev = level(l.out, 0); d.out_cur = level(l.out, 1);
            launch_kernel(born_tb_kernel(p->fwd_T, p->fwd_gen), l.grid, cs, d);
        } else if (l.kind == Launch::fwd_born) {
            launch_geo_and_wavelet(u.g, u.w, l, p->wavf);
            u.n0 = l.first; u.nsteps = l.nsteps;
            u.p_in_prev = level(l.in, 0); u.p_in_cur = level(l.in, 1);
            u.p_out_prev = level(l.out, 0); u.p_out_cur = level(l.out, 1);
            u.in_prev = level(l.in2, 0); u.in_cur = level(l.in2, 1);
            u.out_prev = level(l.out2, 0); u.out_cur = level(l.out2, 1);
            launch_kernel(fwd_born_tb_kernel(p->fwd_T, p->fwd_gen), l.grid, cs, u);
        } else if (l.kind == Launch::illum) {
            il.g.s_off = l.s_off; il.g.ns_grp = l.ns_grp; il.g.tiles_x = l.tiles_x; il.g.ntiles = l.ntiles;
            il.first = l.first; il.nsteps = l.nsteps; il.hbase = l.hbase; il.init = l.seg == 0;
            launch_kernel(KernelRef<IllumTBArgs>{k_illum_tb, 64 * TB_NW}, l.grid, cs, il);
        } else {
            launch_geo_and_wavelet(a.g, a.w, l, p->wavf);
            if (enc) enc_stride_bits(a.w, b.enc->enc_stride);
            a.ns_sh = l.ns_sh; a.spw = l.spw;
            a.k0 = l.first; a.nsteps = l.nsteps; a.hbase = l.hbase;
            a.in_l1 = level(l.in, 0); a.in_l2 = level(l.in, 1);
            a.out_l1 = level(l.out, 0); a.out_l2 = level(l.out, 1);
            launch_kernel(enc ? adj_tb_enc_kernel(p->adj_T) : src ? adj_tb_src_kernel(p->adj_T) : chunk_adj_kernel(p, l.nsteps),
                          l.grid, cs, a);
        }
    }
    RDQ_CHECK(hipGetLastError());
    return join_chains(p, st, S);
}

// destroy every cached graph; a graph may still be queued or running (asynchronous launches), so
// the device is drained first
void drop_graphs(rdq_fwi_plan *p)
{
    if (p->cache.empty()) return;
    (void)hipDeviceSynchronize();
    for (auto &e : p->cache) (void)hipGraphExecDestroy(e.exec);
    p->cache.clear();
}

// A setting that shapes the launches (cached graphs encode them): changing it drops the graphs.
// Caller holds p->mu.
template <class T>
void set_knob(rdq_fwi_plan *p, T &knob, T value)
{
    if (knob != value) drop_graphs(p);
    knob = value;
}

// Several receivers in one padded column: their residuals folded per column into the ring's tail
// (k_rcv_fold), which the adjoint kernels then read in place of the caller's dseis.
int fold_residuals(const rdq_fwi_plan *p, int B, const float *&dseis, float *ring, hipStream_t st, int nwf = 0)
{
    if (!p->rmulti) return 0;
    const size_t ns = nwf > 0 ? nwf : p->g.ns;       // wavefields per model
    float *fold = ring + 8 * (size_t)B * ns * p->Hp * p->ld;
    const size_t rows = (size_t)B * ns * p->nrec, n = rows * p->ncolr;
    hipLaunchKernelGGL(k_rcv_fold, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st,
                       dseis, fold, p->d_colx, p->d_rcv_start, p->d_rcv_list, p->g.ng, p->ncolr, rows);
    RDQ_CHECK(hipGetLastError());
    dseis = fold;
    return 0;
}

template <class F>
int run_cached(rdq_fwi_plan *p, int kind, int B, std::initializer_list<const void *> key, hipStream_t st, F &&launch,
               int K = 0, const rdq_fwi_source *src = nullptr, const rdq_fwi_encoding *enc = nullptr)
{
    if (!p->graphs) return launch(st);
    const void *k[10] = {nullptr};
    long long ks[4] = {0, 0, 0, 0};
    int n = 0;
    for (const void *v : key) k[n++] = v;
    if (src) { k[8] = src->wav; k[9] = src->gwav; ks[0] = src->model_stride; ks[1] = src->shot_stride; }
    if (enc) {
        k[8] = enc->wav; k[9] = enc->gwav;
        ks[0] = enc->model_stride; ks[1] = enc->source_stride; ks[2] = enc->enc_stride; ks[3] = enc->ne;
    }
    for (auto &e : p->cache)
        if (e.kind == kind && e.B == B && e.K == K && std::equal(k, k + 10, e.ptrs) && std::equal(ks, ks + 4, e.strides)) {
            e.last_use = ++p->tick;
            RDQ_CHECK(hipGraphLaunch(e.exec, st));
            return 0;
        }
    if (!p->cap) RDQ_CHECK(hipStreamCreateWithFlags(&p->cap, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    RDQ_CHECK(hipStreamBeginCapture(p->cap, hipStreamCaptureModeThreadLocal));
    const int rc = launch(p->cap);
    const hipError_t ee = hipStreamEndCapture(p->cap, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    RDQ_CHECK(ee);
    GraphEntry e{};
    e.kind = kind; e.B = B; e.K = K;
    std::copy(k, k + 10, e.ptrs);
    std::copy(ks, ks + 4, e.strides);
    const hipError_t ie = hipGraphInstantiate(&e.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    RDQ_CHECK(ie);
    e.last_use = ++p->tick;
    if (p->cache.size() >= 16) {
        auto old = std::min_element(p->cache.begin(), p->cache.end(),
                                    [](const GraphEntry &a, const GraphEntry &b) { return a.last_use < b.last_use; });
        // the evicted graph may still be queued or running on `st` (everything here is
        // asynchronous): destroying an executing graph frees its kernel-argument storage under the
        // running persistent kernel, so drain the stream first (evictions are rare: a steady loop
        // replays cached graphs)
        RDQ_CHECK(hipStreamSynchronize(st));
        (void)hipGraphExecDestroy(old->exec);
        p->cache.erase(old);
    }
    p->cache.push_back(e);
    RDQ_CHECK(hipGraphLaunch(e.exec, st));
    return 0;
}

}  // namespace

// ======================================================================================= C ABI
extern "C" {

// The recurrence adjoint (k_adj_pr) recovers lap'(P_{k-1}) = (P_k - T1 P_{k-1} + T2 P_{k-2} - src) / A
// from three history levels: a difference of nearly equal values whenever the field is smooth on
// the grid scale.  With an absorbing sponge (the reference's nbc = 120) the field keeps its
// wavelength and the gradient stays within ~1e-5 of the exact order (profiles/r3/
// small_dt_adjoint.jsonl: 1.0e-5 at dt = 1 ms, 3.9e-5 at dt / 4); a thin sponge lets the wave wrap
// round the periodic grid into long standing modes and the cancellation costs 5e-3 (tests/
// golden/fwd_wrap: nbc = 4).  Below RDQ_RECURRENCE_MIN_NBC the plan runs the exact-order adjoint.
constexpr int RDQ_RECURRENCE_MIN_NBC = 20;
static bool recurrence_ok(const rdq_fwi_plan *p) { return p->g.nbc >= RDQ_RECURRENCE_MIN_NBC; }

int rdq_fwi_plan_create(const rdq_fwi_geom *geom, rdq_fwi_plan **out)
{
    if (!geom || !out || geom->nz < 1 || geom->nx < 1 || geom->nbc < 0 || geom->nt < 1 || geom->ns < 1 ||
        geom->ng < 1 || geom->sample_temporal < 1 || !geom->isx || !geom->igx || !geom->wavelet)
        return RDQ_E_INVALID;
    rdq_fwi_plan *p = new (std::nothrow) rdq_fwi_plan();
    if (!p) return RDQ_E_NOMEM;
    p->g = *geom;
    p->Hp = geom->nz + 2 * geom->nbc;
    p->Wp = geom->nx + 2 * geom->nbc;
    p->ld = (p->Wp + 63) / 64 * 64;
    p->nrec = (geom->nt + geom->sample_temporal - 1) / geom->sample_temporal;
    p->isx.assign(geom->isx, geom->isx + geom->ns);
    p->igx.assign(geom->igx, geom->igx + geom->ng);
    p->wav.assign(geom->wavelet, geom->wavelet + geom->nt);
    p->wavf.resize(geom->nt);
    for (int i = 0; i < geom->nt; ++i) p->wavf[i] = (float)p->wav[i];   // pde.py:81 casts to fp32
    for (int v : p->isx) if (v < 0 || v >= p->Wp) { delete p; return RDQ_E_INVALID; }
    for (int v : p->igx) if (v < 0 || v >= p->Wp) { delete p; return RDQ_E_INVALID; }
    if (geom->isz < 0 || geom->isz >= p->Hp || geom->igz < 0 || geom->igz >= p->Hp) { delete p; return RDQ_E_INVALID; }
    if (p->Wp > FIN_MAXW) { delete p; return RDQ_E_INVALID; }   // gradient finalize holds a padded row in LDS
    p->g.isx = p->isx.data();
    p->g.igx = p->igx.data();
    p->g.wavelet = p->wav.data();
    // receivers grouped by column (stable -> ascending receiver id within a column)
    std::vector<int> order(geom->ng), start(p->Wp + 1, 0);
    for (int r = 0; r < geom->ng; ++r) order[r] = r;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p->igx[a] < p->igx[b]; });
    for (int r = 0; r < geom->ng; ++r) start[p->igx[r] + 1]++;
    for (int x = 0; x < p->Wp; ++x) start[x + 1] += start[x];
    // adjoint residual per column: the receiver's own dseis, or (several receivers in one column)
    // their residuals folded in receiver order into one value per column (k_rcv_fold)
    std::vector<int> rlane(p->Wp, -1), colx;
    for (int x = 0; x < p->Wp; ++x) {
        if (start[x + 1] - start[x] > 1) p->rmulti = true;
        if (start[x + 1] > start[x]) colx.push_back(x);
    }
    p->ncolr = (int)colx.size();
    for (int c = 0; c < p->ncolr; ++c) rlane[colx[c]] = p->rmulti ? c : order[start[colx[c]]];
    // sources grouped by column the same way (encoded calls: a lane injects its column's sources in ascending index)
    std::vector<int> sorder(geom->ns), sstart(p->Wp + 1, 0);
    for (int j = 0; j < geom->ns; ++j) sorder[j] = j;
    std::stable_sort(sorder.begin(), sorder.end(), [&](int a, int b) { return p->isx[a] < p->isx[b]; });
    for (int j = 0; j < geom->ns; ++j) sstart[p->isx[j] + 1]++;
    for (int x = 0; x < p->Wp; ++x) sstart[x + 1] += sstart[x];
    hipError_t e = hipMalloc(&p->d_isx, sizeof(int) * geom->ns);
    sstart.insert(sstart.end(), sorder.begin(), sorder.end());
    if (e == hipSuccess) e = hipMalloc(&p->d_src_table, sizeof(int) * sstart.size());
    if (e == hipSuccess) e = hipMemcpy(p->d_src_table, sstart.data(), sizeof(int) * sstart.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&p->d_rcv_start, sizeof(int) * (p->Wp + 1));
    if (e == hipSuccess) e = hipMalloc(&p->d_rcv_list, sizeof(int) * geom->ng);
    if (e == hipSuccess) e = hipMemcpy(p->d_isx, p->isx.data(), sizeof(int) * geom->ns, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_rcv_start, start.data(), sizeof(int) * (p->Wp + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_rcv_list, order.data(), sizeof(int) * geom->ng, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&p->d_rlane, sizeof(int) * p->Wp);
    if (e == hipSuccess) e = hipMemcpy(p->d_rlane, rlane.data(), sizeof(int) * p->Wp, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&p->d_colx, sizeof(int) * std::max(p->ncolr, 1));
    if (e == hipSuccess && p->ncolr)
        e = hipMemcpy(p->d_colx, colx.data(), sizeof(int) * p->ncolr, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&p->d_wav, sizeof(float) * geom->nt);
    if (e == hipSuccess) e = hipMemcpy(p->d_wav, p->wavf.data(), sizeof(float) * geom->nt, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&p->d_status_own, 256);
    if (e == hipSuccess) e = hipMemset(p->d_status_own, 0, 256);
    p->d_status = p->d_status_own;
    p->adj_fma = recurrence_ok(p);
    if (e != hipSuccess) { rdq_fwi_plan_destroy(p); return -(int)e; }
    *out = p;
    return 0;
}

int rdq_fwi_plan_destroy(rdq_fwi_plan *p)
{
    if (!p) return 0;
    drop_graphs(p);
    if (p->cap) (void)hipStreamDestroy(p->cap);
    for (auto st : p->aux) (void)hipStreamDestroy(st);
    for (auto e : p->evs) (void)hipEventDestroy(e);
    if (p->handover) (void)hipEventDestroy(p->handover);
    if (p->d_isx) (void)hipFree(p->d_isx);
    if (p->d_rcv_start) (void)hipFree(p->d_rcv_start);
    if (p->d_rcv_list) (void)hipFree(p->d_rcv_list);
    if (p->d_src_table) (void)hipFree(p->d_src_table);
    if (p->d_rlane) (void)hipFree(p->d_rlane);
    if (p->d_colx) (void)hipFree(p->d_colx);
    if (p->d_wav) (void)hipFree(p->d_wav);
    if (p->d_status_own) (void)hipFree(p->d_status_own);
    if (p->d_prof) (void)hipFree(p->d_prof);
    delete p;
    return 0;
}

int rdq_fwi_set_graphs(rdq_fwi_plan *p, int32_t enable)
{
    if (!p) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    p->graphs = enable != 0;
    return 0;
}

int rdq_fwi_set_tuning(rdq_fwi_plan *p, int32_t fwd_steps, int32_t adj_steps, int32_t chains)
{
    if (!p || fwd_steps < 1 || fwd_steps > TB_MAXT || adj_steps < 1 || adj_steps > TB_MAXT || chains < 0 ||
        chains > 16)
        return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->fwd_T, fwd_steps);
    set_knob(p, p->adj_T, adj_steps);
    set_knob(p, p->chains, chains);
    return 0;
}

int rdq_fwi_set_wide_fwd_steps(rdq_fwi_plan *p, int32_t steps)
{
    if (!p || steps < 0 || steps > TW_FWD_MAXT) return RDQ_E_INVALID;   // 0 = set_tuning's fwd_steps
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->fwd_Tw, steps);
    return 0;
}

int rdq_fwi_set_wide_fwd_shots(rdq_fwi_plan *p, int32_t shots)
{
    if (!p || shots < 0 || shots > 64) return RDQ_E_INVALID;   // 0 = auto (wide_spw)
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->fwd_spw, shots);
    return 0;
}

int rdq_fwi_set_wide_adj_shots(rdq_fwi_plan *p, int32_t shots)
{
    if (!p || shots < 0 || shots > 64) return RDQ_E_INVALID;   // 0 = auto (wide_spw)
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->adj_spw, shots);
    return 0;
}

int rdq_fwi_set_wide_adj_steps(rdq_fwi_plan *p, int32_t steps)
{
    if (!p || steps < 0 || steps > TW_ADJ_MAXT) return RDQ_E_INVALID;   // 0 = auto (wide_adj_depth)
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->adj_Tw, steps);
    return 0;
}

int rdq_fwi_set_variant(rdq_fwi_plan *p, int32_t flags)
{
    if (!p || (flags & ~31)) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const bool gen = (flags & RDQ_VARIANT_FWD_GEN) != 0;
    const bool fma = (flags & RDQ_VARIANT_ADJ_EXACT) == 0 && recurrence_ok(p);
    const bool twfma = (flags & RDQ_VARIANT_CHUNKED_ADJ_FMA) != 0 && (flags & RDQ_VARIANT_ADJ_EXACT) == 0 &&
                       recurrence_ok(p);
    const int xcd = (flags & RDQ_VARIANT_NO_XCD_LOCAL) ? 0 : 1;
    const bool wide = (flags & RDQ_VARIANT_NARROW_CHUNKED) == 0;
    set_knob(p, p->fwd_gen, gen);
    set_knob(p, p->adj_fma, fma);
    set_knob(p, p->adj_tw_fma, twfma);
    set_knob(p, p->xcd_mode, xcd);
    set_knob(p, p->wide, wide);
    return 0;
}

int rdq_fwi_set_rows_per_wave(rdq_fwi_plan *p, int32_t fwd_rows, int32_t adj_rows)
{
    if (!p || (fwd_rows != 6 && fwd_rows != 8 && fwd_rows != 12 && fwd_rows != 24) ||
        (adj_rows != 6 && adj_rows != 8 && adj_rows != 12))
        return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->fwd_rw, fwd_rows);
    set_knob(p, p->adj_rw, adj_rows);
    return 0;
}
int rdq_fwi_set_persistent(rdq_fwi_plan *p, int32_t mode)
{
    if (!p || (mode != 0 && mode != 1 && mode != 8 && mode != 12 && mode != 16 && mode != -1)) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->persist, mode);
    return 0;
}

int rdq_fwi_launch_info(rdq_fwi_plan *p, int32_t B, int32_t out[10])
{
    if (!p || !out || B < 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    int perf = 0, pera = 0;
    out[0] = persistent_nw(p, B, false, &perf);
    out[1] = persistent_nw(p, B, true, &pera);
    out[2] = out[0] ? p->fwd_T : chunk_depth(p, false);   // chunked: the wide kernels' depth
    out[3] = out[1] ? p->adj_T : chunk_depth(p, true);
    // persistent: one launch per slice group; chunked: the store-all schedule's launches per chain
    const int ns = B * p->g.ns;
    const CkptPlan all = ckpt_plan(p, p->g.nt);
    out[4] = out[0] ? (ns + perf - 1) / perf : count_launches(chunked_schedule(p, B, Pass::fwd_ring, all), Launch::fwd);
    out[5] = out[1] ? (ns + pera - 1) / pera : count_launches(chunked_schedule(p, B, Pass::adj_hist, all), Launch::adj);
    out[6] = 0;   // the forward has the one order
    out[7] = out[1] ? adj_overlap(p) : 0;
    out[8] = 0;   // the forward has the generic loop only
    out[9] = out[1] ? adj_wave_roles(p) : 0;
    return 0;
}

int rdq_fwi_set_sweep_delay(rdq_fwi_plan *p, int32_t fwd_ticks, int32_t adj_ticks)
{
    if (!p || fwd_ticks < 0 || fwd_ticks > 100000 || adj_ticks < 0 || adj_ticks > 100000) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    p->fwd_delay = fwd_ticks;   // (persistent launches are direct, not graphs: nothing cached to drop)
    p->adj_delay = adj_ticks;
    return 0;
}

int rdq_fwi_set_handoff_overlap(rdq_fwi_plan *p, int32_t fwd_mode, int32_t adj_mode)
{
    if (!p || fwd_mode != 0 || adj_mode < 0 || adj_mode > 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    p->adj_ov = adj_mode;   // (persistent launches are direct, not graphs: nothing cached to drop)
    return 0;
}

int rdq_fwi_set_wave_roles(rdq_fwi_plan *p, int32_t fwd_mode, int32_t adj_mode)
{
    if (!p || fwd_mode != 0 || adj_mode < 0 || adj_mode > 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->adj_roles, adj_mode);   // (drops the cached graphs when the value changes)
    return 0;
}

int rdq_fwi_set_source_role(rdq_fwi_plan *p, int32_t fwd_mode, int32_t adj_mode)
{
    if (!p || fwd_mode < 0 || fwd_mode > 1 || adj_mode != 0) return RDQ_E_INVALID;   // the adjoint's role has its own setter (rdq_fwi_set_adjoint_role)
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->fwd_srole, fwd_mode);   // (drops the cached graphs when the value changes)
    return 0;
}

int rdq_fwi_source_role_info(rdq_fwi_plan *p, int32_t B, int32_t out[2])
{
    if (!p || !out || B < 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const int nwf = persistent_nw(p, B, false);
    out[0] = nwf ? fwd_source_role(p, nwf) : 0;
    out[1] = 0;   // the adjoint's role has a setting of its own (rdq_fwi_set_adjoint_role)
    return 0;
}

int rdq_fwi_set_adjoint_role(rdq_fwi_plan *p, int32_t mode)
{
    if (!p || mode < 0 || mode > 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->adj_srole, mode);   // (drops the cached graphs when the value changes)
    return 0;
}

int rdq_fwi_adjoint_role_info(rdq_fwi_plan *p, int32_t B, int32_t out[2])
{
    if (!p || !out || B < 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const int nwa = persistent_nw(p, B, true);
    out[1] = nwa ? adjoint_role_pair(p, nwa, p->d_prof != nullptr) : -1;
    out[0] = out[1] >= 0 ? 1 : 0;
    return 0;
}

int rdq_fwi_set_adjoint_fetch(rdq_fwi_plan *p, int32_t mode)
{
    if (!p || mode < 0 || mode > 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->adj_fetch, mode);   // (drops the cached graphs when the value changes)
    return 0;
}

int rdq_fwi_adjoint_fetch_info(rdq_fwi_plan *p, int32_t B, int32_t *out)
{
    if (!p || !out || B < 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const int nwa = persistent_nw(p, B, true);
    *out = nwa ? adjoint_fetch(p, nwa, p->d_prof != nullptr) : 0;
    return 0;
}

int rdq_fwi_role_row_pair(int32_t padded_row) { return padded_row < 0 ? RDQ_E_INVALID : role_row_pair(padded_row); }

int rdq_fwi_wide_info(rdq_fwi_plan *p, int32_t B, int32_t out[4])
{
    if (!p || !out || B < 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    // the first launch of chain 0 (shots [0, ns / S), the smallest group) of the store-all schedules
    const CkptPlan all = ckpt_plan(p, p->g.nt);
    const Launch f = chunked_schedule(p, B, Pass::fwd_ring, all).front();
    const Launch a = chunked_schedule(p, B, Pass::adj_hist, all).front();
    out[0] = chain_count(p);
    out[1] = f.spw;
    out[2] = a.spw;
    out[3] = f.ns_sh;
    return 0;
}

int rdq_fwi_set_profile(rdq_fwi_plan *p, int32_t enable)
{
    if (!p) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    drop_graphs(p);   // graphs bake the pointer in
    if (enable && !p->d_prof) {
        RDQ_CHECK(hipMalloc(&p->d_prof, 2 * PROF_WORDS * sizeof(unsigned long long)));
        RDQ_CHECK(hipMemset(p->d_prof, 0, 2 * PROF_WORDS * sizeof(unsigned long long)));
    } else if (!enable && p->d_prof) {
        RDQ_CHECK(hipFree(p->d_prof));
        p->d_prof = nullptr;
    }
    return 0;
}

int rdq_fwi_read_profile(rdq_fwi_plan *p, uint64_t out[12])
{
    if (!p || !out) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->d_prof) { for (int i = 0; i < 8; ++i) out[i] = 0; return 0; }
    RDQ_CHECK(hipDeviceSynchronize());
    p->prof_host.resize(2 * PROF_WORDS);
    RDQ_CHECK(hipMemcpy(p->prof_host.data(), p->d_prof, 2 * PROF_WORDS * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost));
    RDQ_CHECK(hipMemset(p->d_prof, 0, 2 * PROF_WORDS * sizeof(unsigned long long)));
    for (int i = 0; i < 6; ++i) { out[i] = p->prof_host[i]; out[6 + i] = p->prof_host[PROF_WORDS + i]; }
    return 0;
}

int rdq_fwi_profile_split(rdq_fwi_plan *p, uint64_t out[10])
{
    if (!p || !out) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    for (int i = 0; i < 5; ++i) {
        out[i] = p->prof_host.empty() ? 0 : p->prof_host[6 + i];
        out[5 + i] = p->prof_host.empty() ? 0 : p->prof_host[PROF_WORDS + 6 + i];
    }
    return 0;
}

int rdq_fwi_profile_waves(rdq_fwi_plan *p, int32_t adj, uint64_t *out, size_t count)
{
    if (!p || !out || (adj != 0 && adj != 1)) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const size_t n = std::min(count, PROF_WAVES * 3);
    for (size_t i = 0; i < n; ++i)   // the first three words of each wave's record
        out[i] = p->prof_host.empty() ? 0 : p->prof_host[(adj ? PROF_WORDS : 0) + PROF_RAW + i / 3 * PROF_REC + i % 3];
    return 0;
}

int rdq_fwi_profile_waves_split(rdq_fwi_plan *p, int32_t adj, uint64_t *out, size_t count)
{
    if (!p || !out || (adj != 0 && adj != 1)) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const size_t n = std::min(count, PROF_WAVES * PROF_REC);
    for (size_t i = 0; i < n; ++i)
        out[i] = p->prof_host.empty() ? 0 : p->prof_host[(adj ? PROF_WORDS : 0) + PROF_RAW + i];
    return 0;
}

int rdq_fwi_status(rdq_fwi_plan *p, hipStream_t st)
{
    if (!p) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    unsigned v = 0;
    RDQ_CHECK(hipMemcpyAsync(&v, p->d_status, sizeof(v), hipMemcpyDeviceToHost, st));
    RDQ_CHECK(hipStreamSynchronize(st));
    if (v) {
        RDQ_CHECK(hipMemsetAsync(p->d_status, 0, sizeof(v), st));
        RDQ_CHECK(hipStreamSynchronize(st));
        return RDQ_E_HANDOFF;
    }
    return 0;
}

int rdq_fwi_set_status_buffer(rdq_fwi_plan *p, uint32_t *words)
{
    if (!p) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    set_knob(p, p->d_status, words ? words : p->d_status_own);
    return 0;
}

int rdq_fwi_debug_words(rdq_fwi_plan *p, uint32_t out[32])
{
    if (!p || !out) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    RDQ_CHECK(hipDeviceSynchronize());
    RDQ_CHECK(hipMemcpy(out, p->d_status, 32 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

// buffer sizes for nwf wavefields per model (the plan's shots, or an encoded call's supershots); gbeta is sized by the caller
static void sizes_for(const rdq_fwi_plan *p, int32_t B, size_t ns, rdq_fwi_sizes_t *o)
{
    const size_t slice = (size_t)p->Hp * p->ld;
    o->Hp = p->Hp; o->Wp = p->Wp; o->ld = p->ld; o->nrec = p->nrec;
    o->coeffs = (6 * (size_t)B * slice + (size_t)B * p->g.nz * p->g.nx + B + 4) * sizeof(float);
    o->vstat = (size_t)B * (sizeof(float) + sizeof(int64_t)) + 16;
    o->seis = (size_t)B * ns * p->nrec * p->g.ng * sizeof(float);
    o->history = (size_t)(p->g.nt + 2) * B * ns * slice * sizeof(float);
    o->ring = 4 * (size_t)B * ns * slice * sizeof(unsigned long long);   // = 8 float levels (fwd_born: P in 0-3, dP in 4-7)
    if (p->rmulti) o->ring += (size_t)B * ns * p->nrec * p->ncolr * sizeof(float);   // folded residuals
    o->gA = (size_t)B * ns * slice * sizeof(float);
    o->gk_part = (size_t)B * ns * gk_blocks(p) * sizeof(double);
    o->gbeta = (size_t)B * ns * sizeof(float);
    o->colsum = (size_t)B * p->Hp * p->g.nx * sizeof(double);
}

int rdq_fwi_sizes(const rdq_fwi_plan *p, int32_t B, rdq_fwi_sizes_t *o)
{
    if (!p || !o || B < 1) return RDQ_E_INVALID;
    sizes_for(p, B, (size_t)p->g.ns, o);
    return 0;
}

int rdq_fwi_sizes_enc(const rdq_fwi_plan *p, int32_t B, int32_t ne, rdq_fwi_sizes_t *o)
{
    if (!p || !o || B < 1 || ne < 1) return RDQ_E_INVALID;
    sizes_for(p, B, (size_t)ne, o);
    o->gbeta = (size_t)B * ne * p->g.ns * sizeof(float);   // [B][ne][ns]
    return 0;
}

static void vstat_ptrs(const void *vstat, int B, float **vmin, int64_t **amin)
{
    char *base = (char *)vstat;
    *vmin = (float *)base;
    *amin = (int64_t *)(base + (((size_t)B * sizeof(float) + 15) / 16) * 16);
}

int rdq_fwi_coeffs(const rdq_fwi_plan *p, int32_t B, const float *vn, const int64_t strides[4],
                   int32_t vel_mode, float *coeffs, void *vstat, hipStream_t st)
{
    if (!p || !vn || !strides || !coeffs || !vstat || B < 1 || (vel_mode != 0 && vel_mode != 1))
        return RDQ_E_INVALID;
    float *vmin; int64_t *amin;
    vstat_ptrs(vstat, B, &vmin, &amin);
    CoefArgs a;
    a.cg = coef_gen(p, B, coeffs);
    const double ad = (double)(p->g.nbc - 1) * (double)p->g.dx;   // a = (nbc-1)*dx, pde.py:42
    {   // partials in field 5 of `coeffs` (the model copy, written by k_coeff_fields afterwards)
        const int n = p->g.nz * p->g.nx, parts = std::max(1, std::min(256, (n + 8191) / 8192));
        const int chunk = (n + parts - 1) / parts;
        float *pv = coeffs + 5 * (size_t)B * p->Hp * p->ld;
        int64_t *pi = reinterpret_cast<int64_t *>(pv + (((size_t)B * parts + 3) / 4) * 4);
        hipLaunchKernelGGL(k_vstat_part, dim3(B, parts), dim3(256), 0, st, vn, strides[0], strides[2], strides[3],
                           p->g.nz, p->g.nx, vel_mode, chunk, pv, pi);
        hipLaunchKernelGGL(k_vstat_final, dim3(B), dim3(256), 0, st, pv, pi, parts, (float)std::log(10000000.0),
                           (float)(2.0 * ad), vmin, amin, const_cast<float *>(a.cg.ks));
    }
    a.vn = vn; a.s0 = strides[0]; a.s2 = strides[2]; a.s3 = strides[3];
    a.vel_mode = vel_mode; a.ld = p->ld;
    a.vmod_out = const_cast<float *>(a.cg.vmod);
    a.coeffs = coeffs;
    a.cstride = (size_t)B * p->Hp * p->ld;
    hipLaunchKernelGGL(k_coeffs, dim3((p->ld + 255) / 256, p->Hp, B), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_coeff_fields, dim3((p->ld + 255) / 256, p->Hp, B), dim3(256), 0, st, a);
    RDQ_CHECK(hipGetLastError());
    return 0;
}

// a call's source: usable (a wavelet, strides >= 0), or absent (nullptr: the plan's wavelet)
static bool source_ok(const rdq_fwi_source *src)
{
    return src && src->wav && src->model_stride >= 0 && src->shot_stride >= 0;
}
static bool encoding_ok(const rdq_fwi_encoding *enc)
{
    return enc && enc->wav && enc->ne >= 1 && enc->model_stride >= 0 && enc->enc_stride >= 0 && enc->source_stride >= 0;
}

// K1, with the plan's wavelet (src == nullptr) or the call's own (always the narrow chunked kernels)
static int forward_call(rdq_fwi_plan *p, int32_t B, const float *coeffs, const rdq_fwi_source *src, float *seis,
                        float *hist, float *ring, hipStream_t st, const rdq_fwi_encoding *enc = nullptr)
{
    if (!p || !coeffs || !seis || (!hist && !ring) || B < 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    RDQ_TRY(plan_enter(p, st));
    int per = 0;
    if (const int nw = src || enc ? 0 : persistent_nw(p, B, false, &per)) {
        if (!ring) return RDQ_E_INVALID;   // the persistent kernel's hand-off granules live in `ring`
        // direct launch (one kernel + memsets per shot group: nothing for a graph to amortise; the
        // arrival counters of pt_assign are zeroed by a stream-ordered memset right before it)
        return launch_forward_pt(p, B, nw, per, coeffs, seis, hist, ring, st);
    }
    // chunked: the store-all schedule, writing the history or (no-grad) ping-ponging in the ring
    ChunkBufs b{};
    b.coeffs = coeffs; b.seis = seis; b.hist = hist; b.ring = ring; b.src = src; b.enc = enc;
    return run_cached(p, (hist ? 0 : 1) + (src ? 8 : 0) + (enc ? 16 : 0), B, {coeffs, seis, hist, ring}, st, [&](hipStream_t s) {
        return enqueue_chunked(p, B, hist ? Pass::fwd_hist : Pass::fwd_ring, p->g.nt, b, s);
    }, 0, src, enc);
}

int rdq_fwi_forward(const rdq_fwi_plan *pc, int32_t B, const float *coeffs, float *seis, float *hist,
                    float *ring, hipStream_t st)
{
    return forward_call(const_cast<rdq_fwi_plan *>(pc), B, coeffs, nullptr, seis, hist, ring, st);
}

int rdq_fwi_forward_src(const rdq_fwi_plan *pc, int32_t B, const float *coeffs, const rdq_fwi_source *src,
                        float *seis, float *hist, float *ring, hipStream_t st)
{
    if (!source_ok(src)) return RDQ_E_INVALID;
    return forward_call(const_cast<rdq_fwi_plan *>(pc), B, coeffs, src, seis, hist, ring, st);
}

int rdq_fwi_forward_enc(const rdq_fwi_plan *pc, int32_t B, const float *coeffs, const rdq_fwi_encoding *enc,
                        float *seis, float *hist, float *ring, hipStream_t st)
{
    if (!encoding_ok(enc)) return RDQ_E_INVALID;
    return forward_call(const_cast<rdq_fwi_plan *>(pc), B, coeffs, nullptr, seis, hist, ring, st, enc);
}

static int adjoint_call(rdq_fwi_plan *p, int32_t B, const float *coeffs, const rdq_fwi_source *src,
                        const float *hist, const float *dseis, float *ring, float *gA, double *gk, float *gbeta,
                        hipStream_t st, const rdq_fwi_encoding *enc = nullptr)
{
    if (!p || !coeffs || !hist || !dseis || !ring || !gA || !gk || !gbeta || B < 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    RDQ_TRY(plan_enter(p, st));
    RDQ_TRY(fold_residuals(p, B, dseis, ring, st, enc ? enc->ne : 0));
    int per = 0;
    if (const int nw = src || enc ? 0 : persistent_nw(p, B, true, &per))
        return launch_adjoint_pt(p, B, nw, per, coeffs, hist, dseis, ring, gA, gk, gbeta, st);
    ChunkBufs b{};
    b.coeffs = coeffs; b.hist = const_cast<float *>(hist); b.ring = ring; b.dseis = dseis;
    b.gA = gA; b.gk = gk; b.gbeta = gbeta; b.src = src; b.enc = enc;
    return run_cached(p, 2 + (src ? 8 : 0) + (enc ? 16 : 0), B, {coeffs, hist, dseis, ring, gA, gk, gbeta}, st,
                      [&](hipStream_t s) { return enqueue_chunked(p, B, Pass::adj_hist, p->g.nt, b, s); }, 0, src, enc);
}

int rdq_fwi_adjoint(const rdq_fwi_plan *pc, int32_t B, const float *coeffs, const float *hist,
                    const float *dseis, float *ring, float *gA, double *gk, float *gbeta, hipStream_t st)
{
    return adjoint_call(const_cast<rdq_fwi_plan *>(pc), B, coeffs, nullptr, hist, dseis, ring, gA, gk, gbeta, st);
}

int rdq_fwi_adjoint_src(const rdq_fwi_plan *pc, int32_t B, const float *coeffs, const rdq_fwi_source *src,
                        const float *hist, const float *dseis, float *ring, float *gA, double *gk, float *gbeta,
                        hipStream_t st)
{
    if (!source_ok(src)) return RDQ_E_INVALID;
    return adjoint_call(const_cast<rdq_fwi_plan *>(pc), B, coeffs, src, hist, dseis, ring, gA, gk, gbeta, st);
}

int rdq_fwi_adjoint_enc(const rdq_fwi_plan *pc, int32_t B, const float *coeffs, const rdq_fwi_encoding *enc,
                        const float *hist, const float *dseis, float *ring, float *gA, double *gk, float *gbeta,
                        hipStream_t st)
{
    if (!encoding_ok(enc)) return RDQ_E_INVALID;
    return adjoint_call(const_cast<rdq_fwi_plan *>(pc), B, coeffs, nullptr, hist, dseis, ring, gA, gk, gbeta, st, enc);
}

// perturbation workspace: dam [B][nz][nx], ratio [B], dbeta [B][ns], oscale [B], dmax [B] (k_dcoeffs)
int rdq_fwi_born_sizes(const rdq_fwi_plan *p, int32_t B, size_t *bytes)
{
    if (!p || !bytes || B < 1) return RDQ_E_INVALID;
    *bytes = ((size_t)B * p->g.nz * p->g.nx + 3 * (size_t)B + (size_t)B * p->g.ns + 4) * sizeof(float);
    return 0;
}

int rdq_fwi_dcoeffs(const rdq_fwi_plan *p, int32_t B, const float *dv, const int64_t strides[4], int32_t vel_mode,
                    const float *coeffs, const void *vstat, float *dwork, hipStream_t st)
{
    if (!p || !dv || !strides || !coeffs || !vstat || !dwork || B < 1 || (vel_mode != 0 && vel_mode != 1))
        return RDQ_E_INVALID;
    float *vmin; int64_t *amin;
    vstat_ptrs(vstat, B, &vmin, &amin);
    DCoefArgs a;
    a.dv = dv; a.s0 = strides[0]; a.s2 = strides[2]; a.s3 = strides[3];
    a.vel_mode = vel_mode; a.B = B; a.nz = p->g.nz; a.nx = p->g.nx; a.ns = p->g.ns; a.nbc = p->g.nbc;
    a.isz = p->g.isz; a.ld = p->ld; a.dt = p->g.dt; a.dx = p->g.dx;
    a.slice = (size_t)p->Hp * p->ld; a.cstride = (size_t)B * a.slice;
    a.coeffs = coeffs; a.vmod = coef_gen(p, B, coeffs).vmod; a.vmin = vmin; a.amin = amin; a.isx = p->d_isx;
    a.dam = dwork; a.ratio = dwork + (size_t)B * p->g.nz * p->g.nx; a.dbeta = a.ratio + B;
    a.oscale = a.dbeta + (size_t)B * p->g.ns;
    a.dmax = reinterpret_cast<unsigned *>(a.oscale + B);
    const size_t n = (size_t)B * p->g.nz * p->g.nx + (size_t)B + (size_t)B * p->g.ns;
    if (n > 0x7fffffffu) return RDQ_E_INVALID;
    RDQ_TRY(zero_regions({{a.dmax, (size_t)B * sizeof(unsigned)}}, st));
    const int cells = p->g.nz * p->g.nx;
    hipLaunchKernelGGL(k_dmax, dim3((unsigned)std::max(1, std::min(64, (cells + 2047) / 2048)), B), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_dcoeffs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    RDQ_CHECK(hipGetLastError());
    return 0;
}

int rdq_fwi_born(const rdq_fwi_plan *pc, int32_t B, const float *coeffs, const float *dwork, const float *hist,
                 float *dseis, float *ring, hipStream_t st)
{
    rdq_fwi_plan *p = const_cast<rdq_fwi_plan *>(pc);
    if (!p || !coeffs || !dwork || !hist || !dseis || !ring || B < 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    RDQ_TRY(plan_enter(p, st));
    ChunkBufs b{};
    b.coeffs = coeffs; b.dwork = dwork; b.hist = const_cast<float *>(hist); b.seis = dseis; b.ring = ring;
    return run_cached(p, 5, B, {coeffs, dwork, hist, dseis, ring}, st,
                      [&](hipStream_t s) { return enqueue_chunked(p, B, Pass::born, p->g.nt, b, s); });
}

int rdq_fwi_born_fused(const rdq_fwi_plan *pc, int32_t B, int32_t K, const float *coeffs, const float *dwork,
                       float *seis, float *dseis_out, float *ckpt, float *ring, hipStream_t st)
{
    rdq_fwi_plan *p = const_cast<rdq_fwi_plan *>(pc);
    if (!p || !coeffs || !dwork || !seis || !dseis_out || !ring || B < 1 || (ckpt && K < 1)) return RDQ_E_INVALID;
    const int Ke = ckpt ? ckpt_plan(p, K).K : p->g.nt;   // no store: one segment
    std::lock_guard<std::mutex> lk(p->mu);
    RDQ_TRY(plan_enter(p, st));
    ChunkBufs b{};
    b.coeffs = coeffs; b.dwork = dwork; b.seis = seis; b.dseis_out = dseis_out; b.ckpt = ckpt; b.ring = ring;
    return run_cached(p, 6, B, {coeffs, dwork, seis, dseis_out, ckpt, ring}, st,
                      [&](hipStream_t s) { return enqueue_chunked(p, B, Pass::fwd_born, Ke, b, s); }, Ke);
}

static void ckpt_sizes_for(const rdq_fwi_plan *p, int32_t B, size_t ns, int32_t K, rdq_fwi_ckpt_sizes_t *o)
{
    const CkptPlan cp = ckpt_plan(p, K);
    const size_t level = (size_t)B * ns * p->Hp * p->ld * sizeof(float);
    o->nseg = cp.nseg;
    o->seg_levels = cp.K + 2;
    o->ckpt = 2 * (size_t)(cp.nseg - 1) * level;
    o->seg = (size_t)(cp.K + 2) * level;
}

int rdq_fwi_ckpt_sizes(const rdq_fwi_plan *p, int32_t B, int32_t K, rdq_fwi_ckpt_sizes_t *o)
{
    if (!p || !o || B < 1 || K < 1) return RDQ_E_INVALID;
    ckpt_sizes_for(p, B, (size_t)p->g.ns, K, o);
    return 0;
}

int rdq_fwi_ckpt_sizes_enc(const rdq_fwi_plan *p, int32_t B, int32_t ne, int32_t K, rdq_fwi_ckpt_sizes_t *o)
{
    if (!p || !o || B < 1 || ne < 1 || K < 1) return RDQ_E_INVALID;
    ckpt_sizes_for(p, B, (size_t)ne, K, o);
    return 0;
}

int rdq_fwi_ckpt_info(rdq_fwi_plan *p, int32_t B, int32_t K, int32_t out[4])
{
    if (!p || !out || B < 1 || K < 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    const CkptPlan cp = ckpt_plan(p, K);
    const std::vector<Launch> bwd = chunked_schedule(p, B, Pass::adj_ckpt, cp);
    out[0] = 0;            // the first pass runs the chunked kernels
    out[1] = cp.nseg;
    out[2] = count_launches(chunked_schedule(p, B, Pass::fwd_ring, cp), Launch::fwd);
    out[3] = count_launches(bwd, Launch::fwd) + count_launches(bwd, Launch::adj);   // every segment: its recompute, then its adjoint
    return 0;
}

static int forward_ckpt_call(rdq_fwi_plan *p, int32_t B, int32_t K, const float *coeffs, const rdq_fwi_source *src,
                             float *seis, float *ckpt, float *ring, hipStream_t st,
                             const rdq_fwi_encoding *enc = nullptr)
{
    if (!p || !coeffs || !seis || !ring || B < 1 || K < 1) return RDQ_E_INVALID;
    if (!ckpt && ckpt_plan(p, K).nseg > 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    RDQ_TRY(plan_enter(p, st));
    ChunkBufs b{};
    b.coeffs = coeffs; b.seis = seis; b.ckpt = ckpt; b.ring = ring; b.src = src; b.enc = enc;
    return run_cached(p, 3 + (src ? 8 : 0) + (enc ? 16 : 0), B, {coeffs, seis, ckpt, ring}, st,
                      [&](hipStream_t s) { return enqueue_chunked(p, B, Pass::fwd_ring, K, b, s); }, ckpt_plan(p, K).K,
                      src, enc);
}

int rdq_fwi_forward_ckpt(const rdq_fwi_plan *pc, int32_t B, int32_t K, const float *coeffs, float *seis,
                         float *ckpt, float *ring, hipStream_t st)
{
    return forward_ckpt_call(const_cast<rdq_fwi_plan *>(pc), B, K, coeffs, nullptr, seis, ckpt, ring, st);
}

int rdq_fwi_forward_ckpt_src(const rdq_fwi_plan *pc, int32_t B, int32_t K, const float *coeffs,
                             const rdq_fwi_source *src, float *seis, float *ckpt, float *ring, hipStream_t st)
{
    if (!source_ok(src)) return RDQ_E_INVALID;
    return forward_ckpt_call(const_cast<rdq_fwi_plan *>(pc), B, K, coeffs, src, seis, ckpt, ring, st);
}

int rdq_fwi_forward_ckpt_enc(const rdq_fwi_plan *pc, int32_t B, int32_t K, const float *coeffs,
                             const rdq_fwi_encoding *enc, float *seis, float *ckpt, float *ring, hipStream_t st)
{
    if (!encoding_ok(enc)) return RDQ_E_INVALID;
    return forward_ckpt_call(const_cast<rdq_fwi_plan *>(pc), B, K, coeffs, nullptr, seis, ckpt, ring, st, enc);
}

static int adjoint_ckpt_call(rdq_fwi_plan *p, int32_t B, int32_t K, const float *coeffs, const rdq_fwi_source *src,
                             const float *ckpt, float *seg, const float *dseis, float *ring, float *gA, double *gk,
                             float *gbeta, hipStream_t st, const rdq_fwi_encoding *enc = nullptr)
{
    if (!p || !coeffs || !seg || !dseis || !ring || !gA || !gk || !gbeta || B < 1 || K < 1) return RDQ_E_INVALID;
    if (!ckpt && ckpt_plan(p, K).nseg > 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    RDQ_TRY(plan_enter(p, st));
    RDQ_TRY(fold_residuals(p, B, dseis, ring, st, enc ? enc->ne : 0));
    ChunkBufs b{};
    b.coeffs = coeffs; b.hist = seg; b.ckpt = const_cast<float *>(ckpt); b.ring = ring; b.dseis = dseis;
    b.gA = gA; b.gk = gk; b.gbeta = gbeta; b.src = src; b.enc = enc;
    return run_cached(p, 4 + (src ? 8 : 0) + (enc ? 16 : 0), B, {coeffs, ckpt, seg, dseis, ring, gA, gk, gbeta}, st,
                      [&](hipStream_t s) { return enqueue_chunked(p, B, Pass::adj_ckpt, K, b, s); }, ckpt_plan(p, K).K,
                      src, enc);
}

int rdq_fwi_adjoint_ckpt(const rdq_fwi_plan *pc, int32_t B, int32_t K, const float *coeffs, const float *ckpt,
                         float *seg, const float *dseis, float *ring, float *gA, double *gk, float *gbeta,
                         hipStream_t st)
{
    return adjoint_ckpt_call(const_cast<rdq_fwi_plan *>(pc), B, K, coeffs, nullptr, ckpt, seg, dseis, ring, gA, gk,
                             gbeta, st);
}

int rdq_fwi_adjoint_ckpt_src(const rdq_fwi_plan *pc, int32_t B, int32_t K, const float *coeffs,
                             const rdq_fwi_source *src, const float *ckpt, float *seg, const float *dseis, float *ring,
                             float *gA, double *gk, float *gbeta, hipStream_t st)
{
    if (!source_ok(src)) return RDQ_E_INVALID;
    return adjoint_ckpt_call(const_cast<rdq_fwi_plan *>(pc), B, K, coeffs, src, ckpt, seg, dseis, ring, gA, gk, gbeta,
                             st);
}

int rdq_fwi_adjoint_ckpt_enc(const rdq_fwi_plan *pc, int32_t B, int32_t K, const float *coeffs,
                             const rdq_fwi_encoding *enc, const float *ckpt, float *seg, const float *dseis, float *ring,
                             float *gA, double *gk, float *gbeta, hipStream_t st)
{
    if (!encoding_ok(enc)) return RDQ_E_INVALID;
    return adjoint_ckpt_call(const_cast<rdq_fwi_plan *>(pc), B, K, coeffs, nullptr, ckpt, seg, dseis, ring, gA, gk,
                             gbeta, st, enc);
}

// Illumination over a stored history: one k_illum_tb launch per chain (graph kind 32; the key's K slot holds nwf)
int rdq_fwi_illum(const rdq_fwi_plan *pc, int32_t B, int32_t nwf, const float *history, float *hA, hipStream_t st)
{
    rdq_fwi_plan *p = const_cast<rdq_fwi_plan *>(pc);
    if (!p || !history || !hA || B < 1 || nwf < 0) return RDQ_E_INVALID;
    const int nw = nwf > 0 ? nwf : p->g.ns;
    std::lock_guard<std::mutex> lk(p->mu);
    RDQ_TRY(plan_enter(p, st));
    ChunkBufs b{};
    b.hist = const_cast<float *>(history); b.gA = hA;
    b.nwf = nw;
    return run_cached(p, 32, B, {history, hA}, st,
                      [&](hipStream_t s) { return enqueue_chunked(p, B, Pass::illum_hist, p->g.nt, b, s); }, nw);
}

// Illumination over a checkpoint store: per segment the recompute the matching adjoint_ckpt call runs, then one
// k_illum_tb launch (graph kinds 33, + 8 / + 16 as the other passes)
int rdq_fwi_illum_ckpt(const rdq_fwi_plan *pc, int32_t B, int32_t K, const float *coeffs, const rdq_fwi_source *src,
                       const rdq_fwi_encoding *enc, const float *ckpt, float *seg, float *ring, float *hA,
                       hipStream_t st)
{
    rdq_fwi_plan *p = const_cast<rdq_fwi_plan *>(pc);
    if (!p || !coeffs || !seg || !ring || !hA || B < 1 || K < 1 || (src && enc)) return RDQ_E_INVALID;
    if ((src && !source_ok(src)) || (enc && !encoding_ok(enc))) return RDQ_E_INVALID;
    if (!ckpt && ckpt_plan(p, K).nseg > 1) return RDQ_E_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);
    RDQ_TRY(plan_enter(p, st));
    ChunkBufs b{};
    b.coeffs = coeffs; b.hist = seg; b.ckpt = const_cast<float *>(ckpt); b.ring = ring; b.gA = hA; b.src = src; b.enc = enc;
    return run_cached(p, 33 + (src ? 8 : 0) + (enc ? 16 : 0), B, {coeffs, ckpt, seg, ring, hA}, st,
                      [&](hipStream_t s) { return enqueue_chunked(p, B, Pass::illum_ckpt, K, b, s); }, ckpt_plan(p, K).K,
                      src, enc);
}

int rdq_fwi_illum_finalize(const rdq_fwi_plan *p, int32_t B, int32_t nwf, const float *coeffs, const float *hA,
                           int32_t vel_mode, double *colsum, float *H, hipStream_t st)
{
    if (!p || !coeffs || !hA || !colsum || !H || B < 1 || nwf < 0 || (vel_mode != 0 && vel_mode != 1))
        return RDQ_E_INVALID;
    if (p->Wp > FIN_MAXW) return RDQ_E_INVALID;
    IllumFinArgs a;
    a.B = B; a.nwf = nwf > 0 ? nwf : p->g.ns; a.nz = p->g.nz; a.nx = p->g.nx; a.nbc = p->g.nbc;
    a.Hp = p->Hp; a.Wp = p->Wp; a.ld = p->ld; a.dt = p->g.dt; a.dx = p->g.dx;
    a.scale = vel_mode == 0 ? 1500.0 : 1.0;
    a.slice = (size_t)p->Hp * p->ld; a.cstride = (size_t)B * a.slice;
    a.coeffs = coeffs; a.hA = hA; a.colsum = colsum; a.out = H;
    hipLaunchKernelGGL(k_illum_fin_rows, dim3(p->Hp, B), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_illum_fin, dim3((p->g.nz * p->g.nx + 255) / 256, B), dim3(256), 0, st, a);
    RDQ_CHECK(hipGetLastError());
    return 0;
}

// K4 of the plain call (ne == 0) or of an encoded one
static int finalize_call(const rdq_fwi_plan *p, int32_t B, int32_t ne, const float *coeffs, const void *vstat,
                         const float *gA, const double *gk, const float *gbeta, int32_t vel_mode,
                         double *colsum, float *out, hipStream_t st)
{
    if (!p || !coeffs || !vstat || !gA || !gk || !gbeta || !colsum || !out || B < 1 ||
        (vel_mode != 0 && vel_mode != 1))
        return RDQ_E_INVALID;
    float *vmin; int64_t *amin;
    vstat_ptrs(vstat, B, &vmin, &amin);
    FinEncArgs a;
    a.B = B; a.ns = p->g.ns; a.nz = p->g.nz; a.nx = p->g.nx; a.nbc = p->g.nbc; a.Hp = p->Hp; a.Wp = p->Wp;
    a.ld = p->ld; a.isz = p->g.isz; a.nblk = gk_blocks(p); a.dt = p->g.dt; a.dx = p->g.dx;
    a.scale = vel_mode == 0 ? 1500.0 : 1.0;
    a.slice = (size_t)p->Hp * p->ld; a.cstride = (size_t)B * a.slice;
    a.coeffs = coeffs; a.gA = gA; a.gbeta = gbeta; a.vmin = vmin; a.amin = amin; a.gk_part = gk;
    a.isx = p->d_isx; a.colsum = colsum; a.out = out; a.ne = ne;
    if (p->Wp > FIN_MAXW) return RDQ_E_INVALID;
    if (ne) hipLaunchKernelGGL(k_fin_rows<FinEncArgs>, dim3(p->Hp, B), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_fin_rows<FinArgs>, dim3(p->Hp, B), dim3(256), 0, st, static_cast<const FinArgs &>(a));
    hipLaunchKernelGGL(k_fin_cols, dim3((p->g.nz * p->g.nx + 255) / 256, B), dim3(256), 0, st, a);
    RDQ_CHECK(hipGetLastError());
    return 0;
}

int rdq_fwi_grad_finalize(const rdq_fwi_plan *p, int32_t B, const float *coeffs, const void *vstat,
                          const float *gA, const double *gk, const float *gbeta, int32_t vel_mode,
                          double *colsum, float *out, hipStream_t st)
{
    return finalize_call(p, B, 0, coeffs, vstat, gA, gk, gbeta, vel_mode, colsum, out, st);
}

int rdq_fwi_grad_finalize_enc(const rdq_fwi_plan *p, int32_t B, int32_t ne, const float *coeffs, const void *vstat,
                              const float *gA, const double *gk, const float *gbeta, int32_t vel_mode,
                              double *colsum, float *out, hipStream_t st)
{
    if (ne < 1) return RDQ_E_INVALID;
    return finalize_call(p, B, ne, coeffs, vstat, gA, gk, gbeta, vel_mode, colsum, out, st);
}

size_t rdq_l1_partial_bytes(int32_t B, int64_t n)
{
    const int64_t nchunk = (n + L1_BLOCK * L1_ITEMS - 1) / (L1_BLOCK * L1_ITEMS);
    return (size_t)B * nchunk * 2 * sizeof(double);
}

int rdq_l1_forward(int32_t B, int64_t n, const float *pred, const float *y, const float *mask, float *loss,
                   float *nobs, void *partial, hipStream_t st)
{
    if (B < 1 || n < 1 || !pred || !y || !loss || !nobs || !partial) return RDQ_E_INVALID;
    const int nchunk = (int)((n + L1_BLOCK * L1_ITEMS - 1) / (L1_BLOCK * L1_ITEMS));
    hipLaunchKernelGGL(k_l1_partial, dim3(nchunk, B), dim3(L1_BLOCK), 0, st, n, pred, y, mask, (double *)partial, nchunk);
    hipLaunchKernelGGL(k_l1_final, dim3(B), dim3(L1_BLOCK), 0, st, B, nchunk, (const double *)partial, loss, nobs);
    RDQ_CHECK(hipGetLastError());
    return 0;
}

int rdq_l1_backward(int32_t B, int64_t n, const float *pred, const float *y, const float *mask,
                    const float *nobs, const float *gout, float *dpred, hipStream_t st)
{
    if (B < 1 || n < 1 || !pred || !y || !nobs || !gout || !dpred) return RDQ_E_INVALID;
    hipLaunchKernelGGL(k_l1_backward, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, st, B, n, pred, y, mask,
                       nobs, gout, dpred);
    RDQ_CHECK(hipGetLastError());
    return 0;
}

int rdq_smooth_reg_forward(int32_t kind, int32_t B, int32_t H, int32_t W, const float *mu, float *loss,
                           hipStream_t st)
{
    if ((kind != 0 && kind != 1) || B < 1 || H < 2 || W < 2 || !mu || !loss) return RDQ_E_INVALID;
    hipLaunchKernelGGL(k_smooth_fwd, dim3(B), dim3(256), 0, st, kind, H, W, mu, loss);
    RDQ_CHECK(hipGetLastError());
    return 0;
}

int rdq_smooth_reg_backward(int32_t kind, int32_t B, int32_t H, int32_t W, const float *mu,
                            const float *gout, float *grad, hipStream_t st)
{
    if ((kind != 0 && kind != 1) || B < 1 || H < 2 || W < 2 || !mu || !gout || !grad) return RDQ_E_INVALID;
    hipLaunchKernelGGL(k_smooth_bwd, dim3((H * W + 255) / 256, B), dim3(256), 0, st, kind, H, W, mu, gout, grad);
    RDQ_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
