// Guided matching on gfx950: the matcher's fused GEMM + top-2 (match_kernels.hip) with a geometric gate in the
// epilogue.  A similarity counts only where the pair of key points agrees with the pair's F (Sampson error without the division) or H
// (one-sided transfer error); elsewhere it is -inf, so the running top-2, the split merge (match_reduce_kernel) and the ratio /
// distance / mutual tests see the masked matrix and nothing else.
//
// The gate works on one 16-byte record per key point, computed once in fp64 from the double matrix and rounded to fp32
// (guided_prep_kernel).  guided_gate decides a pair from (record of the image-0 point, record of the image-1 point) and is called
// with its arguments in THAT order from both sweeps: the forward sweep (a lane keeps an image-0 point, image-1 candidates come
// through LDS) and the reverse sweep (the roles swapped) evaluate the same expression on the same bits, so the two directions of
// the mutual check see one mask.
//
// Orientation and work mapping are match_top2_kernel's: candidates are the MFMA A operand staged through LDS (64 rows per stage,
// double buffered), the kept side sits in registers as B, a lane holds 16 candidates of ONE query per 32 x 32 tile and its running
// top-2 is lane-local.  The candidates' records are staged with their tile (64 x 16 B per stage); for a given accumulator register
// all 32 lanes of a half-wave read the same record (an LDS broadcast).  No tile is skipped: at a pass rate of 1 - 1.5 % and key
// points in no spatial order a 32 x 32 tile without a passing pair practically never occurs.
#include "sfd2_internal.h"
#include "../../include/sfd2_hip.h"
#include <math.h>

#define NT 256
#define KD 128        // descriptor dimension
#define TA 64         // candidate rows per LDS stage
#define APITCH 136    // fp16 per staged row: 128 + 8 pad (272 B)

// ---------------------------------------------------------------- per-point records
// F, image-0 point: l = F (x0, y0, 1)        -> (l0, l1, l2, l0^2 + l1^2)
// F, image-1 point: m = F^T (x1, y1, 1)      -> (x1, y1, m0^2 + m1^2, 0)
// H, image-0 point: p = pi(H (x0, y0, 1))    -> (px, py, valid, 0); valid = 0 when p is not finite (as fp32)
// H, image-1 point:                          -> (x1, y1, 0, 0)
__global__ __launch_bounds__(NT)
void guided_prep_kernel(const GuidedProbDev *__restrict__ probs, const float *__restrict__ xy0, const float *__restrict__ xy1,
                        float4 *__restrict__ rec0, float4 *__restrict__ rec1)
{
    const GuidedProbDev p = probs[blockIdx.y];
    const int side = blockIdx.z;
    const int n = side == 0 ? p.n0 : p.n1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t at = (size_t)(side == 0 ? p.off0 : p.off1) + i;
    const float *xy = (side == 0 ? xy0 : xy1) + 2 * at;
    const float xf = xy[0], yf = xy[1];
    const double x = (double)xf, y = (double)yf;
    const double *M = p.M;
    float4 r;
    if (side == 1) {
        r.x = xf;
        r.y = yf;
        r.z = 0.0f;
        r.w = 0.0f;
        if (p.model == SFD2_GUIDE_F) {
            const double m0 = M[0] * x + M[3] * y + M[6], m1 = M[1] * x + M[4] * y + M[7];
            r.z = (float)(m0 * m0 + m1 * m1);
        }
        rec1[at] = r;
        return;
    }
    const double l0 = M[0] * x + M[1] * y + M[2], l1 = M[3] * x + M[4] * y + M[5], l2 = M[6] * x + M[7] * y + M[8];
    if (p.model == SFD2_GUIDE_F) {
        r.x = (float)l0;
        r.y = (float)l1;
        r.z = (float)l2;
        r.w = (float)(l0 * l0 + l1 * l1);
    } else {
        const float px = (float)(l0 / l2), py = (float)(l1 / l2);
        const bool valid = isfinite(px) && isfinite(py);
        r.x = valid ? px : 0.0f;
        r.y = valid ? py : 0.0f;
        r.z = valid ? 1.0f : 0.0f;
        r.w = 0.0f;
    }
    rec0[at] = r;
}

void launch_guided_prep(hipStream_t st, const GuidedProbDev *probs_dev, int k, int max_n, const float *xy0, const float *xy1,
                        float4 *rec0, float4 *rec1)
{
    if (k <= 0 || max_n <= 0) return;
    hipLaunchKernelGGL(guided_prep_kernel, dim3((max_n + NT - 1) / NT, k, 2), dim3(NT), 0, st, probs_dev, xy0, xy1, rec0, rec1);
}

// ---------------------------------------------------------------- the gate
// THE decision on one pair of key points; r0 = record of the image-0 point, r1 = record of the image-1 point, t2 = max_error^2.
// F: the four-term Sampson error r^2 / (n_l + n_m) <= t2 without the division.  H: the squared transfer error in image 1.
template <int MODEL>
__device__ __forceinline__ bool guided_gate(const float4 r0, const float4 r1, float t2)
{
    if (MODEL == SFD2_GUIDE_F) {
        const float r = fmaf(r1.x, r0.x, fmaf(r1.y, r0.y, r0.z));
        return r * r <= t2 * (r0.w + r1.z);
    }
    const float dx = r1.x - r0.x, dy = r1.y - r0.y;
    return r0.z != 0.0f && fmaf(dx, dx, dy * dy) <= t2;
}

__device__ __forceinline__ void top2_update(float v, int j, float &b1, float &b2, int &i1)
{
    // strict '>' keeps the first (lowest) index among equal maxima (match_kernels.hip)
    b2 = __builtin_amdgcn_fmed3f(b1, b2, v);
    i1 = v > b1 ? j : i1;
    b1 = fmaxf(b1, v);
}

// ---------------------------------------------------------------- fused GEMM + gate + top-2
// One direction of one pair over the candidates [ja0, ja1) of this split.  DIR 0: the lane keeps an image-0 point (forward), DIR 1:
// an image-1 point (reverse).
template <int MODEL, int DIR>
__device__ __forceinline__ void guided_sweep(const GuidedJob &job, half_t *As, float4 *Rs, const h8_t (&bh)[8], const float4 mine, int ja0,
                                             int ja1, float &b1, float &b2, int &i1)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int lcol = lane & 31, lk = (lane >> 5) * 8;
    const float t2 = job.t2;
    const int nst = (ja1 - ja0 + TA - 1) / TA;
    uint4 rh[4];
    float4 rr = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // descriptor piece p (0..1023): row = p >> 4, part = p & 15 (16 bytes each); the first 64 threads carry one record each
#define LOAD_A(stage_)                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                    \
        const int p = tid + i * NT, row = p >> 4, part = p & 15;                                       \
        const int ja = ja0 + (stage_)*TA + row;                                                        \
        rh[i] = make_uint4(0, 0, 0, 0);                                                                \
        if (ja < ja1) rh[i] = *reinterpret_cast<const uint4 *>(job.a_hi + (size_t)ja * KD + part * 8); \
    }                                                                                                  \
    if (tid < TA) {                                                                                    \
        const int ja = ja0 + (stage_)*TA + tid;                                                        \
        rr = make_float4(0.0f, 0.0f, 0.0f, 0.0f);                                                      \
        if (ja < ja1) rr = job.a_rec[ja];                                                              \
    }
#define STORE_A(buf_)                                                                                  \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                    \
        const int p = tid + i * NT, row = p >> 4, part = p & 15;                                       \
        *reinterpret_cast<uint4 *>(As + ((buf_)*TA + row) * APITCH + part * 8) = rh[i];                \
    }                                                                                                  \
    if (tid < TA) Rs[(buf_)*TA + tid] = rr;
    LOAD_A(0)
    STORE_A(0)
    __syncthreads();
    for (int s = 0; s < nst; ++s) {
        const int buf = s & 1;
        const bool has_next = s + 1 < nst;
        if (has_next) { LOAD_A(s + 1) }
#pragma unroll
        for (int sub = 0; sub < TA / 32; ++sub) {
            f32x16_t acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            const half_t *arow = As + (buf * TA + sub * 32 + lcol) * APITCH + lk;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const h8_t ah = *reinterpret_cast<const h8_t *>(arow + ks * 16);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[ks], acc, 0, 0, 0);
            }
            const int rbase = buf * TA + sub * 32 + 4 * (lane >> 5);
            const int jbase = ja0 + s * TA + sub * 32 + 4 * (lane >> 5);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = (r & 3) + 8 * (r >> 2);
                const int j = jbase + o;
                const float4 cand = Rs[rbase + o];
                const bool pass = DIR == 0 ? guided_gate<MODEL>(mine, cand, t2) : guided_gate<MODEL>(cand, mine, t2);
                const float v = (pass && j < ja1) ? acc[r] : -INFINITY;
                top2_update(v, j, b1, b2, i1);
            }
        }
        if (has_next) { STORE_A(buf ^ 1) }
        __syncthreads();
    }
#undef LOAD_A
#undef STORE_A
}

__global__ __launch_bounds__(NT, 2)
void guided_top2_kernel(const GuidedJob *__restrict__ jobs, int splits)
{
    __shared__ __attribute__((aligned(16))) half_t As[2 * TA * APITCH];
    __shared__ __attribute__((aligned(16))) float4 Rs[2 * TA];
    const GuidedJob job = jobs[blockIdx.z];
    const int na = job.na, nb = job.nb;
    const int i_base = blockIdx.x * 128;
    if (i_base >= nb) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lcol = lane & 31, lk = (lane >> 5) * 8;

    // candidate range of this split, a multiple of 32 so that sub-tiles never straddle splits
    int chunk = (na + splits - 1) / splits;
    chunk = (chunk + 31) & ~31;
    const int ja0 = blockIdx.y * chunk;
    int ja1 = ja0 + chunk;
    if (ja1 > na) ja1 = na;

    const int my_i = i_base + wave * 32 + lcol;
    h8_t bh[8];
    float4 mine = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        h8_t z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (half_t)0.0f;
        bh[ks] = z;
        if (my_i < nb) bh[ks] = *reinterpret_cast<const h8_t *>(job.b_hi + (size_t)my_i * KD + ks * 16 + lk);
    }
    if (my_i < nb) mine = job.b_rec[my_i];

    float b1 = -INFINITY, b2 = -INFINITY;
    int i1 = 0;
    if (ja0 < ja1) {   // (block-uniform, like the model and the direction: every thread reaches guided_sweep's barriers)
        if (job.model == SFD2_GUIDE_F) {
            if (job.dir == 0) guided_sweep<SFD2_GUIDE_F, 0>(job, As, Rs, bh, mine, ja0, ja1, b1, b2, i1);
            else guided_sweep<SFD2_GUIDE_F, 1>(job, As, Rs, bh, mine, ja0, ja1, b1, b2, i1);
        } else {
            if (job.dir == 0) guided_sweep<SFD2_GUIDE_H, 0>(job, As, Rs, bh, mine, ja0, ja1, b1, b2, i1);
            else guided_sweep<SFD2_GUIDE_H, 1>(job, As, Rs, bh, mine, ja0, ja1, b1, b2, i1);
        }
    }
    // merge the two half-waves (same query, interleaved candidate rows)
    const float c1 = __shfl_xor(b1, 32), c2 = __shfl_xor(b2, 32);
    const int j1 = __shfl_xor(i1, 32);
    float n1v, n2v;
    int n1i;
    if (c1 > b1 || (c1 == b1 && j1 < i1)) { n1v = c1; n1i = j1; n2v = fmaxf(b1, c2); }
    else { n1v = b1; n1i = i1; n2v = fmaxf(b2, c1); }
    if (lane < 32 && my_i < nb) {
        const size_t o = (size_t)blockIdx.y * nb + my_i;
        job.part_v1[o] = n1v;
        job.part_v2[o] = n2v;
        job.part_i1[o] = n1i;
    }
}

void launch_guided_top2(hipStream_t st, const GuidedJob *jobs_dev, int njobs, int max_nb, int splits)
{
    if (njobs <= 0 || max_nb <= 0) return;
    hipLaunchKernelGGL(guided_top2_kernel, dim3((max_nb + 127) / 128, splits, njobs), dim3(NT), 0, st, jobs_dev, splits);
}
