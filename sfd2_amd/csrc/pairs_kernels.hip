// Image-pair selection (hloc/pairs_from_retrieval.py, pairs_from_covisibility.py, pairs_from_poses.py) on gfx950.
//
// The three selections share one step, the k best of n scored candidates of a row, written once (pairs_topk_scan below) and used by
// every kernel of this file.  The order is total: the larger score first, then the smaller candidate index.  A row's list therefore
// depends on the row's candidates alone -- not on the tile or split that offered them, nor on the order in which they were offered.
//
//   retrieval     query . db^T on the f32-input MFMA (v_mfma_f32_16x16x4_f32: bit for bit an fmaf chain over ascending k), operands
//                 tiled in LDS, ragged edges zero-padded there; the running top-k of the block's 64 query rows lives in LDS and is fed
//                 from the accumulators after every 64 x 128 tile, so the nq x nd matrix is never written.  The db range is split over
//                 blockIdx.y; pairs_retrieval_merge folds the partial lists (always: one split is the trivial case).
//   covisibility  one workgroup per image, an int32 counter per other image (LDS, or a row of a global scratch buffer), integer
//                 atomics over observation -> point -> track, then the k largest counts > 0.
//   poses         fp64 throughout: per image the rotation and the position, per pair distance and relative rotation angle, the k
//                 nearest candidates with angle < threshold (score = -distance).
// No floating-point atomics anywhere.
#include "sfd2_internal.h"
#include <algorithm>

namespace {

#define PAIRS_WAVE 64

// Lanes of one wave hand values to each other through LDS below: the fences keep the compiler from moving LDS accesses across the
// hand-over (the hardware serves one wave's LDS instructions in order).
__device__ __forceinline__ void pairs_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

template <class S> __device__ __forceinline__ bool pairs_better(S sa, int ia, S sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// lane moves of one 32-bit word: a (wave-uniform) lane's value to everybody; every lane its left neighbour's (lane 0 keeps its own)
__device__ __forceinline__ int pairs_lane_w(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ int pairs_shr1_w(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ int pairs_lane(int v, int l) { return pairs_lane_w(v, l); }
__device__ __forceinline__ float pairs_lane(float v, int l) { return __int_as_float(pairs_lane_w(__float_as_int(v), l)); }
__device__ __forceinline__ double pairs_lane(double v, int l)
{
    return __hiloint2double(pairs_lane_w(__double2hiint(v), l), pairs_lane_w(__double2loint(v), l));
}
__device__ __forceinline__ int pairs_shr1(int v) { return pairs_shr1_w(v); }
__device__ __forceinline__ float pairs_shr1(float v) { return __int_as_float(pairs_shr1_w(__float_as_int(v))); }
__device__ __forceinline__ double pairs_shr1(double v) { return __hiloint2double(pairs_shr1_w(__double2hiint(v)), pairs_shr1_w(__double2loint(v))); }

// THE shared step.  One wave offers the candidates j = n0 .. n1 - 1 to its list (sorted, best first, len <= k entries, in LDS);
// gen(j, score, index) returns whether j is a candidate at all.  For the length of the call the list lives in registers, entry p in
// lane p & 63 of register p >> 6 (k <= 64 MAXCH), and goes back to LDS only when it changed.  The list's k-th entry is the
// threshold: only candidates that beat it are inserted -- rank by ballot + popcount, the tail one lane to the right.
template <class S, int MAXCH, class Gen>
__device__ __forceinline__ void pairs_topk_scan(S *ls, int *li, int &len, int k, int n0, int n1, int lane, Gen gen)
{
    S rs[MAXCH];
    int ri[MAXCH];
#pragma unroll
    for (int c = 0; c < MAXCH; ++c) {
        const int p = c * PAIRS_WAVE + lane;
        rs[c] = S(0);
        ri[c] = 0;
        if (p < len) { rs[c] = ls[p]; ri[c] = li[p]; }
    }
    const int kc = (k - 1) >> 6, kl = (k - 1) & 63;               // where the k-th entry sits
    bool full = len == k, dirty = false;
    S thr_s = S(0);
    int thr_i = 0;
#pragma unroll
    for (int c = 0; c < MAXCH; ++c)
        if (c == kc) { thr_s = pairs_lane(rs[c], kl); thr_i = pairs_lane(ri[c], kl); }
    for (int j0 = n0; j0 < n1; j0 += PAIRS_WAVE) {
        const int j = j0 + lane;
        S s = S(0);
        int id = 0;
        bool ok = false;
        if (j < n1) ok = gen(j, s, id);
        if (ok && full) ok = pairs_better(s, id, thr_s, thr_i);
        unsigned long long m = __ballot(ok);
        while (m) {
            const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
            m &= m - 1;
            const S cs = pairs_lane(s, src);
            const int ci = pairs_lane(id, src);
            if (full && !pairs_better(cs, ci, thr_s, thr_i)) continue;
            int pos = 0;                                           // entries that stay in front of the candidate
#pragma unroll
            for (int c = 0; c < MAXCH; ++c) {
                const int p = c * PAIRS_WAVE + lane;
                pos += __popcll(__ballot(p < len && pairs_better(rs[c], ri[c], cs, ci)));
            }
            if (pos >= k) continue;
#pragma unroll
            for (int c = MAXCH - 1; c >= 0; --c) {                 // from the tail: register c - 1 is still the old one
                const int p = c * PAIRS_WAVE + lane;
                S us = pairs_shr1(rs[c]);
                int ui = pairs_shr1(ri[c]);
                if (c > 0) {
                    const S ws = pairs_lane(rs[c - 1], 63);
                    const int wi = pairs_lane(ri[c - 1], 63);
                    if (lane == 0) { us = ws; ui = wi; }
                }
                if (p > pos) { rs[c] = us; ri[c] = ui; }
                if (p == pos) { rs[c] = cs; ri[c] = ci; }
            }
            len = min(len + 1, k);
            dirty = true;
            full = len == k;
#pragma unroll
            for (int c = 0; c < MAXCH; ++c)
                if (c == kc) { thr_s = pairs_lane(rs[c], kl); thr_i = pairs_lane(ri[c], kl); }
        }
    }
    if (dirty) {
#pragma unroll
        for (int c = 0; c < MAXCH; ++c) {
            const int p = c * PAIRS_WAVE + lane;
            if (p < len) { ls[p] = rs[c]; li[p] = ri[c]; }
        }
    }
    pairs_wave_sync();
}

// ------------------------------------------------------------------------------------------------ retrieval
#define RT_BM 64                       // query rows of a block: 4 waves x 16
#define RT_BN 128                      // db rows of a tile: 8 accumulators of 16 x 16 per wave
#define RT_KC 32                       // descriptor elements of a staged chunk
#define RT_LD 36                       // floats of an LDS operand row: 16 lanes' float4 reads at this stride touch every bank once
#define RT_SLD 68                      // floats of a row of the similarity staging (64 columns): rows 4 apart sit 16 banks apart
#define RT_UNITS ((RT_BM + RT_BN) * (RT_KC / 16))

// 16 consecutive elements of a row (zero beyond the row's end or for a row that does not exist)
__device__ __forceinline__ void rt_load16(const float *row, int k0, int d, bool vec, float (&v)[16])
{
    if (row && vec && k0 + 16 <= d) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 t = *reinterpret_cast<const float4 *>(row + k0 + 4 * q);
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = (row && k0 + q < d) ? row[k0 + q] : 0.0f;
    }
}

// In LDS a group of 16 elements is stored transposed as 4 x 4: position 4 g + s holds element 4 s + g, so that lane group g's one
// float4 holds its operand of the four MFMA steps s = 0..3 and every step multiplies the elements 4 s .. 4 s + 3: ascending k.
__device__ __forceinline__ void rt_store16(float *dst, const float (&v)[16])
{
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<float4 *>(dst + 4 * g) = make_float4(v[g], v[4 + g], v[8 + g], v[12 + g]);
}

__global__ __launch_bounds__(256) void pairs_retrieval_kernel(const float *__restrict__ query, int nq, const float *__restrict__ db, int nd, int d,
                                                              int k, int splits, int tiles, int vec, float *__restrict__ part_s,
                                                              int *__restrict__ part_i)
{
    extern __shared__ __align__(16) unsigned char pairs_smem[];
    float *As = reinterpret_cast<float *>(pairs_smem);            // [RT_BM][RT_LD]
    float *Bs = As + RT_BM * RT_LD;                               // [RT_BN][RT_LD]
    float *ls = As + (RT_BM + RT_BN) * RT_LD;                     // [RT_BM][k]
    int *li = reinterpret_cast<int *>(ls + RT_BM * k);            // [RT_BM][k]
    int *lens = li + RT_BM * k;                                   // [RT_BM]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * RT_BM, split = blockIdx.y;
    const int t0 = (int)((long long)split * tiles / splits), t1 = (int)((long long)(split + 1) * tiles / splits);
    float *Sw = As + wave * 16 * RT_SLD;                          // this wave's similarity staging, over the operand tiles
    if (tid < RT_BM) lens[tid] = 0;
    __syncthreads();

    // what this thread stages: unit u = (row of the 192 operand rows, 16-element group of the chunk)
    const float *src[2];
    int ugrp[2], urow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int u = tid + i * 256;
        urow[i] = u >> 1;
        ugrp[i] = u & 1;
        src[i] = nullptr;
        if (u < RT_UNITS && urow[i] < RT_BM && row0 + urow[i] < nq) src[i] = query + (size_t)(row0 + urow[i]) * d;
    }
    const int nchunks = (d + RT_KC - 1) / RT_KC;
    const int arow = wave * 16 + (lane & 15), lg = lane >> 4;
    float v[2][16];

    for (int t = t0; t < t1; ++t) {
        const int col0 = t * RT_BN;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = tid + i * 256;
            if (u < RT_UNITS && urow[i] >= RT_BM) {
                const int c = col0 + urow[i] - RT_BM;
                src[i] = c < nd ? db + (size_t)c * d : nullptr;
            }
        }
        f32x4_t acc[8];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[a][r] = 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (tid + i * 256 < RT_UNITS) rt_load16(src[i], ugrp[i] * 16, d, vec != 0, v[i]);
        for (int c = 0; c < nchunks; ++c) {
            __syncthreads();                                       // the operand tiles (and the staging over them) are free
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (tid + i * 256 < RT_UNITS) rt_store16(As + urow[i] * RT_LD + ugrp[i] * 16, v[i]);
            __syncthreads();
            if (c + 1 < nchunks) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    if (tid + i * 256 < RT_UNITS) rt_load16(src[i], (c + 1) * RT_KC + ugrp[i] * 16, d, vec != 0, v[i]);
            }
#pragma unroll
            for (int kg = 0; kg < RT_KC / 16; ++kg) {
                const float4 a = *reinterpret_cast<const float4 *>(As + arow * RT_LD + kg * 16 + lg * 4);
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    const float4 b = *reinterpret_cast<const float4 *>(Bs + (n * 16 + (lane & 15)) * RT_LD + kg * 16 + lg * 4);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[n], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                           // every wave is past its operand reads
        // epilogue: accumulator (column = lane & 15, row = 4 (lane >> 4) + register) -> this wave's staging, 64 columns at a time,
        // then one scan per row
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) Sw[(lg * 4 + r) * RT_SLD + n * 16 + (lane & 15)] = acc[4 * h + n][r];
            pairs_wave_sync();
            const int cbase = col0 + h * 64;
            for (int rr = 0; rr < 16; ++rr) {
                const int lrow = wave * 16 + rr;
                if (row0 + lrow >= nq) break;
                int len = lens[lrow];
                const float *srow = Sw + rr * RT_SLD;
                pairs_topk_scan<float, 4>(ls + lrow * k, li + lrow * k, len, k, 0, 64, lane, [&](int j, float &s, int &id) {
                    s = srow[j];
                    id = cbase + j;
                    return id < nd;
                });
                if (lane == 0) lens[lrow] = len;
            }
            pairs_wave_sync();
        }
    }
    pairs_wave_sync();
    for (int rr = 0; rr < 16; ++rr) {                              // the partial lists; unused slots carry index -1
        const int lrow = wave * 16 + rr;
        if (row0 + lrow >= nq) break;
        const int len = lens[lrow];
        const size_t o = ((size_t)(row0 + lrow) * splits + split) * k;
        for (int p = lane; p < k; p += PAIRS_WAVE) {
            part_s[o + p] = p < len ? ls[lrow * k + p] : 0.0f;
            part_i[o + p] = p < len ? li[lrow * k + p] : -1;
        }
    }
}

// one wave per query row folds the row's splits * k partial entries into the final list
__global__ __launch_bounds__(256) void pairs_retrieval_merge(const float *__restrict__ part_s, const int *__restrict__ part_i, int nq, int splits,
                                                             int k, int *__restrict__ idx, float *__restrict__ sim)
{
    extern __shared__ __align__(16) unsigned char pairs_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *ls = reinterpret_cast<float *>(pairs_smem) + wave * k;
    int *li = reinterpret_cast<int *>(pairs_smem) + 4 * k + wave * k;
    const int row = blockIdx.x * 4 + wave;
    if (row >= nq) return;
    const size_t o = (size_t)row * splits * k;
    int len = 0;
    pairs_topk_scan<float, 4>(ls, li, len, k, 0, splits * k, lane, [&](int j, float &s, int &id) {
        s = part_s[o + j];
        id = part_i[o + j];
        return id >= 0;
    });
    for (int p = lane; p < k; p += PAIRS_WAVE) {
        idx[(size_t)row * k + p] = p < len ? li[p] : -1;
        sim[(size_t)row * k + p] = p < len ? ls[p] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void pairs_finite_kernel(const float *__restrict__ a, size_t na, const float *__restrict__ b, size_t nb, int *flag)
{
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (size_t)gridDim.x * 256) {
        const float x = i < na ? a[i] : b[i - na];
        bad |= !(fabsf(x) <= 3.402823466e38f);
    }
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// ------------------------------------------------------------------------------------------------ covisibility
template <bool GLOBAL>
__global__ __launch_bounds__(256) void pairs_covis_kernel(const int64_t *__restrict__ obs_off, const int32_t *__restrict__ obs_point, int n_images,
                                                          const int64_t *__restrict__ trk_off, const int32_t *__restrict__ trk_img, int k,
                                                          int *scratch, int32_t *__restrict__ out_idx, int32_t *__restrict__ out_cnt,
                                                          int32_t *__restrict__ out_n)
{
    extern __shared__ __align__(16) unsigned char pairs_smem[];
    int *ls = reinterpret_cast<int *>(pairs_smem), *li = ls + k;
    int *cnt = GLOBAL ? scratch + (size_t)blockIdx.x * n_images : li + k;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = blockIdx.x; i < n_images; i += gridDim.x) {
        for (int j = tid; j < n_images; j += 256) {
            if (GLOBAL) __hip_atomic_store(cnt + j, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else cnt[j] = 0;
        }
        if (GLOBAL) __threadfence();
        __syncthreads();
        for (int64_t o = obs_off[i] + tid; o < obs_off[i + 1]; o += 256) {
            const int p = obs_point[o];
            for (int64_t t = trk_off[p]; t < trk_off[p + 1]; ++t) {
                const int im = trk_img[t];
                if (im != i) atomicAdd(cnt + im, 1);
            }
        }
        if (GLOBAL) __threadfence();
        __syncthreads();
        if (tid < PAIRS_WAVE) {
            int len = 0;
            pairs_topk_scan<int, 4>(ls, li, len, k, 0, n_images, lane, [&](int j, int &s, int &id) {
                s = GLOBAL ? __hip_atomic_load(cnt + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : cnt[j];
                id = j;
                return s > 0;
            });
            for (int p = lane; p < k; p += PAIRS_WAVE) {
                out_idx[(size_t)i * k + p] = p < len ? li[p] : -1;
                out_cnt[(size_t)i * k + p] = p < len ? ls[p] : 0;
            }
            if (lane == 0) out_n[i] = len;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ poses
// per image: R of the quaternion as stored (COLMAP's qvec2rotmat: no normalisation), rows 0..8, and the position, 9..11:
// -R t as hloc/pairs_from_poses.py:25 has it (it multiplies before it transposes), or the camera centre -R^T t (centres != 0)
__global__ __launch_bounds__(256) void pairs_pose_prep_kernel(const double *__restrict__ qvec, const double *__restrict__ tvec, int n, int centres,
                                                              double *__restrict__ rc)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double w = qvec[4 * i], x = qvec[4 * i + 1], y = qvec[4 * i + 2], z = qvec[4 * i + 3];
    double R[9];
    R[0] = 1 - 2 * y * y - 2 * z * z; R[1] = 2 * x * y - 2 * w * z;     R[2] = 2 * z * x + 2 * w * y;
    R[3] = 2 * x * y + 2 * w * z;     R[4] = 1 - 2 * x * x - 2 * z * z; R[5] = 2 * y * z - 2 * w * x;
    R[6] = 2 * z * x - 2 * w * y;     R[7] = 2 * y * z + 2 * w * x;     R[8] = 1 - 2 * x * x - 2 * y * y;
    const double t0 = tvec[3 * i], t1 = tvec[3 * i + 1], t2 = tvec[3 * i + 2];
    double *o = rc + (size_t)i * 12;
    for (int a = 0; a < 9; ++a) o[a] = R[a];
    for (int a = 0; a < 3; ++a)
        o[9 + a] = centres ? -(R[a] * t0 + R[3 + a] * t1 + R[6 + a] * t2) : -(R[3 * a] * t0 + R[3 * a + 1] * t1 + R[3 * a + 2] * t2);
}

__global__ __launch_bounds__(256) void pairs_pose_kernel(const double *__restrict__ rc, int n, int k, double thr_deg, int32_t *__restrict__ out_idx,
                                                         double *__restrict__ out_dist, int32_t *__restrict__ out_n)
{
    extern __shared__ __align__(16) unsigned char pairs_smem[];
    double *ls_all = reinterpret_cast<double *>(pairs_smem);      // [4][k]
    int *li_all = reinterpret_cast<int *>(ls_all + 4 * k);        // [4][k]
    int *lens = li_all + 4 * k;                                   // [4]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = blockIdx.x;
    double me[12];
    for (int a = 0; a < 12; ++a) me[a] = rc[(size_t)i * 12 + a];
    double *ls = ls_all + wave * k;
    int *li = li_all + wave * k;
    int len = 0;
    const int j0 = (int)((long long)wave * n / 4), j1 = (int)((long long)(wave + 1) * n / 4);
    pairs_topk_scan<double, 16>(ls, li, len, k, j0, j1, lane, [&](int j, double &s, int &id) {
        const double *o = rc + (size_t)j * 12;
        double tr = 0;
        for (int a = 0; a < 9; ++a) tr += me[a] * o[a];
        const double dx = me[9] - o[9], dy = me[10] - o[10], dz = me[11] - o[11];
        const double c = fmin(fmax((tr - 1) / 2, -1.0), 1.0);
        const double dr = fabs(acos(c)) * (180.0 / 3.14159265358979323846);
        s = -sqrt(dx * dx + dy * dy + dz * dz);
        id = j;
        return j != i && dr < thr_deg;
    });
    if (lane == 0) lens[wave] = len;
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 4; ++w) {
        const double *os = ls_all + w * k;
        const int *oi = li_all + w * k;
        pairs_topk_scan<double, 16>(ls, li, len, k, 0, lens[w], lane, [&](int j, double &s, int &id) {
            s = os[j];
            id = oi[j];
            return true;
        });
    }
    for (int p = lane; p < k; p += PAIRS_WAVE) {
        out_idx[(size_t)i * k + p] = p < len ? li[p] : -1;
        out_dist[(size_t)i * k + p] = p < len ? -ls[p] : __builtin_inf();
    }
    if (lane == 0) out_n[i] = len;
}

}  // namespace

size_t pairs_retrieval_lds(int k) { return ((size_t)(RT_BM + RT_BN) * RT_LD + RT_BM) * 4 + (size_t)RT_BM * k * 8; }

hipError_t launch_pairs_finite(hipStream_t st, const float *a, size_t na, const float *b, size_t nb, int *flag)
{
    const size_t blocks = std::min<size_t>((na + nb + 255) / 256, 2048);
    pairs_finite_kernel<<<dim3((unsigned)std::max<size_t>(blocks, 1)), dim3(256), 0, st>>>(a, na, b, nb, flag);
    return hipGetLastError();
}

hipError_t launch_pairs_retrieval(hipStream_t st, const float *query, int nq, const float *db, int nd, int d, int k, int splits, float *part_s,
                                  int *part_i, int32_t *idx, float *sim)
{
    const size_t lds = pairs_retrieval_lds(k);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(pairs_retrieval_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int tiles = (nd + RT_BN - 1) / RT_BN;
    const int vec = (d % 4 == 0 && (reinterpret_cast<uintptr_t>(query) & 15) == 0 && (reinterpret_cast<uintptr_t>(db) & 15) == 0) ? 1 : 0;
    pairs_retrieval_kernel<<<dim3((nq + RT_BM - 1) / RT_BM, splits), dim3(256), lds, st>>>(query, nq, db, nd, d, k, splits, tiles, vec, part_s, part_i);
    pairs_retrieval_merge<<<dim3((nq + 3) / 4), dim3(256), (size_t)k * 32, st>>>(part_s, part_i, nq, splits, k, idx, sim);
    return hipGetLastError();
}

int pairs_retrieval_tiles(int nd) { return (nd + RT_BN - 1) / RT_BN; }
int pairs_retrieval_strips(int nq) { return (nq + RT_BM - 1) / RT_BM; }

hipError_t launch_pairs_covis(hipStream_t st, const int64_t *obs_off, const int32_t *obs_point, int n_images, const int64_t *trk_off,
                              const int32_t *trk_img, int k, int global_counters, int blocks, int *scratch, int32_t *idx, int32_t *cnt, int32_t *n_found)
{
    if (global_counters) {
        pairs_covis_kernel<true><<<dim3(blocks), dim3(256), (size_t)k * 8, st>>>(obs_off, obs_point, n_images, trk_off, trk_img, k, scratch, idx, cnt,
                                                                                n_found);
    } else {
        const size_t lds = (size_t)k * 8 + (size_t)n_images * 4;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(pairs_covis_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        pairs_covis_kernel<false><<<dim3(blocks), dim3(256), lds, st>>>(obs_off, obs_point, n_images, trk_off, trk_img, k, nullptr, idx, cnt, n_found);
    }
    return hipGetLastError();
}

hipError_t launch_pairs_poses(hipStream_t st, const double *qvec, const double *tvec, int n, int k, double thr_deg, int centres, double *rc,
                              int32_t *idx, double *dist, int32_t *n_found)
{
    pairs_pose_prep_kernel<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(qvec, tvec, n, centres, rc);
    pairs_pose_kernel<<<dim3(n), dim3(256), (size_t)k * 48 + 16, st>>>(rc, n, k, thr_deg, idx, dist, n_found);
    return hipGetLastError();
}
