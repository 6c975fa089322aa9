// Global descriptors on gfx950: VLAD over the 128-d local descriptors (include/sfd2_hip.h, "global descriptors").
//
//   half norms   h_j = 0.5f * |c_j|^2 as an fmaf chain over ascending e, one thread per centroid.
//   assignment   x . c^T on the f32-input MFMA (v_mfma_f32_16x16x4_f32: bit for bit an fmaf chain over ascending e), operands tiled in
//                LDS in pairs_retrieval_kernel's layout.  The centroids (zero rows up to the kernel's 16 NT columns) stay in LDS for
//                the life of the block, which walks 64-row tiles of x; the rows are staged 32 elements at a time.  The running arg-max
//                of s_j = dot_j - h_j lives in the tile epilogue (per lane over its columns, then over the 16 lanes of a row): the
//                n x k matrix is never written.  The larger s first, a tie to the smaller j.
//   aggregation  one workgroup per segment (an image, or a chunk of k-means rows), the k x 128 fp32 accumulators in LDS, every (j, e)
//                owned by ONE thread -- thread t owns element t & 127 of the centroids j with (j & 1) == t >> 7 -- which walks the
//                segment's rows in ascending order: no floating-point atomics, the sum's order is the row order.  Rows are staged
//                through LDS in coalesced 32-row tiles.  Residual mode normalises in fp64 from LDS and rounds each component once.
//   update       per (j, e) the chunks' partial sums added in ascending chunk order in fp64, centroid = (float)(sum / count).
// A row's / an image's result depends on that row / image and the centroids alone, not on the batch, its order or the grid.
#include "sfd2_internal.h"
#include "../../include/sfd2_hip.h"
#include <algorithm>

namespace {

#define VL_D SFD2_VLAD_DIM
#define VL_BM 64                       // rows of a tile: 4 waves x 16
#define VL_KC 32                       // row elements of a staged chunk
#define VL_LDA 36                      // floats of a staged row chunk: 16 lanes' float4 reads at this stride touch every bank once
#define VL_LDC 132                     // floats of a resident centroid row (132 = 4 mod 64: the same property)
#define VL_TR 32                       // rows of an aggregation tile

__global__ __launch_bounds__(256) void vlad_half_norms_kernel(const float *__restrict__ c, int k, float *__restrict__ half)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    const float *row = c + (size_t)j * VL_D;
    float s = 0.0f;
    for (int e = 0; e < VL_D; ++e) s = fmaf(row[e], row[e], s);
    half[j] = 0.5f * s;
}

// In LDS a group of 16 elements is stored transposed as 4 x 4 (pairs_kernels.hip, rt_store16): position 4 g + s holds element 4 s + g,
// so that lane group g's one float4 holds its operand of the four MFMA steps s = 0..3 and step s multiplies the elements 4 s .. 4 s + 3.
// Here a thread carries 8 consecutive elements, the half hf of a group: elements 8 hf + j -> step 2 hf + (j >> 2), lane group j & 3.
__device__ __forceinline__ void vlad_store8(float *grp, int hf, const float4 &lo, const float4 &hi)
{
    *reinterpret_cast<float2 *>(grp + 0 + 2 * hf) = make_float2(lo.x, hi.x);
    *reinterpret_cast<float2 *>(grp + 4 + 2 * hf) = make_float2(lo.y, hi.y);
    *reinterpret_cast<float2 *>(grp + 8 + 2 * hf) = make_float2(lo.z, hi.z);
    *reinterpret_cast<float2 *>(grp + 12 + 2 * hf) = make_float2(lo.w, hi.w);
}

// NT: 16-column accumulator tiles a wave carries; the centroid rows k .. 16 NT - 1 are zero in LDS and take part in no arg-max
template <int NT>
__global__ __launch_bounds__(256) void vlad_assign_kernel(const float *__restrict__ x, long long n, const float *__restrict__ cen,
                                                          const float *__restrict__ half, int k, long long tiles, int32_t *assign,
                                                          float *__restrict__ score, unsigned long long *moved)
{
    extern __shared__ __align__(16) unsigned char vlad_smem[];
    constexpr int kpad = NT * 16;
    float *Cs = reinterpret_cast<float *>(vlad_smem);             // [kpad][VL_LDC]
    float *As = Cs + (size_t)kpad * VL_LDC;                       // [VL_BM][VL_LDA]
    float *Hs = As + VL_BM * VL_LDA;                              // [kpad]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lg = lane >> 4;

    // the centroids, once: unit = (row, 8 elements), zero rows beyond k
    for (int u = tid; u < kpad * (VL_D / 8); u += 256) {
        const int row = u >> 4, oct = u & 15;
        float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
        if (row < k) {
            const float4 *p = reinterpret_cast<const float4 *>(cen + (size_t)row * VL_D + oct * 8);
            lo = p[0];
            hi = p[1];
        }
        vlad_store8(Cs + row * VL_LDC + (oct >> 1) * 16, oct & 1, lo, hi);
    }
    for (int j = tid; j < kpad; j += 256) Hs[j] = j < k ? half[j] : 0.0f;

    const int srow = tid >> 2, soct = tid & 3;                     // what this thread stages of a chunk: (row of the tile, 8 elements)
    const int arow = wave * 16 + lc;
    unsigned long long changed = 0;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long row0 = t * VL_BM;
        const bool live = row0 + srow < n;
        const float4 *src = reinterpret_cast<const float4 *>(x + (size_t)(live ? row0 + srow : 0) * VL_D + soct * 8);
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        f32x4_t acc[NT];
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[a][r] = 0.0f;
        float4 lo = live ? src[0] : zero, hi = live ? src[1] : zero;
#pragma unroll 1
        for (int c = 0; c < VL_D / VL_KC; ++c) {
            __syncthreads();                                       // the row chunk is free (and, the first time, the centroids are there)
            vlad_store8(As + srow * VL_LDA + (soct >> 1) * 16, soct & 1, lo, hi);
            __syncthreads();
            if (c + 1 < VL_D / VL_KC) {
                lo = live ? src[(c + 1) * (VL_KC / 4)] : zero;
                hi = live ? src[(c + 1) * (VL_KC / 4) + 1] : zero;
            }
#pragma unroll
            for (int kg = 0; kg < VL_KC / 16; ++kg) {
                const float4 a = *reinterpret_cast<const float4 *>(As + arow * VL_LDA + kg * 16 + lg * 4);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const float4 b = *reinterpret_cast<const float4 *>(Cs + (nt * 16 + lc) * VL_LDC + c * VL_KC + kg * 16 + lg * 4);
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[nt], 0, 0, 0);
                }
            }
        }
        // epilogue: accumulator (column = lane & 15, row = 4 (lane >> 4) + register).  Per lane the best of its columns in ascending
        // order (a later one must be strictly larger), then the best of the row's 16 lanes; -1 marks a lane without a column.
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float bs = 0.0f;
            int bi = -1;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int j = nt * 16 + lc;
                if (j < k) {
                    const float s = acc[nt][r] - Hs[j];
                    if (bi < 0 || s > bs) { bs = s; bi = j; }
                }
            }
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) {
                const float os = __shfl_xor(bs, m, 64);
                const int oi = __shfl_xor(bi, m, 64);
                if (oi >= 0 && (bi < 0 || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; }
            }
            const long long row = row0 + wave * 16 + lg * 4 + r;
            if (lc == 0 && row < n) {
                bi = min(max(bi, 0), k - 1);                      // (column 0 always exists: a clamp for non-finite input only)
                if (moved && assign[row] != bi) ++changed;
                assign[row] = bi;
                if (score) score[row] = bs;
            }
        }
    }
    if (moved) {                                                   // integer atomics: one per wave
        for (int m = 32; m >= 1; m >>= 1) changed += __shfl_xor(changed, m, 64);
        if (lane == 0 && changed) atomicAdd(moved, changed);
    }
}

__device__ __forceinline__ double vlad_wave_sum(double v)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the value a component takes before the global L2 norm
__device__ __forceinline__ double vlad_pre(float v, int norm, double bn)
{
    const double d = (double)v;
    if (norm == SFD2_VLAD_NORM_INTRA) return bn > 0.0 ? d / bn : 0.0;
    if (norm == SFD2_VLAD_NORM_SSR) return d < 0.0 ? -sqrt(-d) : sqrt(d);
    return d;
}

__global__ __launch_bounds__(256) void vlad_aggregate_kernel(const float *__restrict__ x, long long n, const long long *__restrict__ offsets,
                                                             const float *__restrict__ cen, int k, const int32_t *__restrict__ assign, int norm,
                                                             float *__restrict__ out, int32_t *__restrict__ cnt_out)
{
    extern __shared__ __align__(16) unsigned char vlad_smem[];
    float *V = reinterpret_cast<float *>(vlad_smem);              // [k][VL_D]
    float *Xs = V + (size_t)k * VL_D;                             // [VL_TR][VL_D]
    double *blk = reinterpret_cast<double *>(Xs + VL_TR * VL_D);  // [k] a block's L2 norm, [k] its share of the squared global norm
    int *cnt = reinterpret_cast<int *>(blk + 2 * k);              // [k]
    int *As = cnt + k;                                            // [VL_TR]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, e = tid & (VL_D - 1), hf = tid >> 7;
    const long long seg = blockIdx.x;
    const bool sums = norm < 0;
    long long r0, r1;
    if (offsets) {
        r0 = offsets[seg];
        r1 = offsets[seg + 1];
    } else {
        r0 = seg * SFD2_VLAD_CHUNK;
        r1 = r0 + SFD2_VLAD_CHUNK;
    }
    r0 = max(r0, 0LL);
    r1 = min(r1, n);                                               // the entry point checked the offsets; a row outside x is never read
    for (int i = tid; i < k * VL_D; i += 256) V[i] = 0.0f;
    for (int j = tid; j < k; j += 256) cnt[j] = 0;
    for (long long t0 = r0; t0 < r1; t0 += VL_TR) {
        const int rows = (int)min((long long)VL_TR, r1 - t0);
        __syncthreads();                                           // the tile is free (and, the first time, the accumulators are zero)
        for (int u = tid; u < rows * (VL_D / 4); u += 256)
            reinterpret_cast<float4 *>(Xs)[u] = reinterpret_cast<const float4 *>(x + (size_t)t0 * VL_D)[u];
        if (tid < VL_TR) {                                         // -1: no row, an assignment outside [0, k)
            const int a = tid < rows ? assign[t0 + tid] : -1;
            As[tid] = (a >= 0 && a < k) ? a : -1;
        }
        __syncthreads();
        float cv[VL_TR];                                           // the tile's centroid values first: 32 loads in flight, not one per row
#pragma unroll
        for (int i = 0; i < VL_TR; ++i) {
            const int a = As[i];
            cv[i] = (!sums && a >= 0 && (a & 1) == hf) ? cen[(size_t)a * VL_D + e] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < VL_TR; ++i) {                          // ascending rows; the branch is uniform over a wave
            const int a = As[i];
            if (a >= 0 && (a & 1) == hf) {
                const float v = Xs[i * VL_D + e];
                V[a * VL_D + e] += sums ? v : v - cv[i];
                if (e == 0) ++cnt[a];
            }
        }
    }
    __syncthreads();
    float *o = out + (size_t)seg * k * VL_D;
    if (sums) {
        for (int i = tid; i < k * VL_D; i += 256) o[i] = V[i];
        for (int j = tid; j < k; j += 256) cnt_out[(size_t)seg * k + j] = cnt[j];
        return;
    }
    // fp64 from here: per centroid (one wave each) the block norm and the block's share of the squared global norm
    for (int j = wave; j < k; j += 4) {
        const float v0 = V[j * VL_D + lane], v1 = V[j * VL_D + 64 + lane];
        double bn = 0.0;
        if (norm == SFD2_VLAD_NORM_INTRA) bn = sqrt(vlad_wave_sum((double)v0 * (double)v0 + (double)v1 * (double)v1));
        const double w0 = vlad_pre(v0, norm, bn), w1 = vlad_pre(v1, norm, bn);
        const double share = vlad_wave_sum(w0 * w0 + w1 * w1);
        if (lane == 0) { blk[j] = bn; blk[k + j] = share; }
    }
    __syncthreads();
    double total = 0.0;
    for (int j = 0; j < k; ++j) total += blk[k + j];               // ascending, the same in every thread
    const double gn = sqrt(total);
    for (int i = tid; i < k * VL_D; i += 256) {
        const double w = vlad_pre(V[i], norm, blk[i / VL_D]);
        o[i] = gn > 0.0 ? (float)(w / gn) : 0.0f;
    }
}

__global__ __launch_bounds__(256) void vlad_update_kernel(const float *__restrict__ part_sum, const int32_t *__restrict__ part_cnt, long long n_chunks,
                                                          int k, float *__restrict__ cen, long long *__restrict__ counts)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k * VL_D) return;
    const int j = i / VL_D;
    double s = 0.0;
    long long c = 0;
    for (long long ch = 0; ch < n_chunks; ++ch) {
        s += (double)part_sum[(size_t)ch * k * VL_D + i];
        c += part_cnt[(size_t)ch * k + j];
    }
    if (c > 0) cen[i] = (float)(s / (double)c);
    if ((i & (VL_D - 1)) == 0) counts[j] = c;
}

size_t vlad_assign_lds(int nt) { return ((size_t)nt * 16 * (VL_LDC + 1) + VL_BM * VL_LDA) * 4; }
size_t vlad_aggregate_lds(int k) { return (size_t)k * VL_D * 4 + VL_TR * VL_D * 4 + (size_t)k * 16 + (size_t)k * 4 + VL_TR * 4; }

template <int NT>
hipError_t vlad_assign_go(hipStream_t st, const float *x, long long n, const float *cen, const float *half, int k, int32_t *assign, float *score,
                          unsigned long long *moved)
{
    const size_t lds = vlad_assign_lds(NT);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(vlad_assign_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const long long tiles = (n + VL_BM - 1) / VL_BM;
    const unsigned blocks = (unsigned)std::min<long long>(tiles, 1024);   // the centroids are loaded once per block
    vlad_assign_kernel<NT><<<dim3(blocks), dim3(256), lds, st>>>(x, n, cen, half, k, tiles, assign, score, moved);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_vlad_half_norms(hipStream_t st, const float *centroids, int k, float *half)
{
    vlad_half_norms_kernel<<<dim3((k + 255) / 256), dim3(256), 0, st>>>(centroids, k, half);
    return hipGetLastError();
}

hipError_t launch_vlad_assign(hipStream_t st, const float *x, int64_t n, const float *centroids, const float *half, int k, int32_t *assign,
                              float *score, unsigned long long *moved)
{
#define VLAD_GO(NT) \
    if (k <= 16 * NT) return vlad_assign_go<NT>(st, x, n, centroids, half, k, assign, score, moved)
    VLAD_GO(1);
    VLAD_GO(2);
    VLAD_GO(3);
    VLAD_GO(4);
    VLAD_GO(6);
    VLAD_GO(8);
    VLAD_GO(12);
    return vlad_assign_go<16>(st, x, n, centroids, half, k, assign, score, moved);
#undef VLAD_GO
}

hipError_t launch_vlad_aggregate(hipStream_t st, const float *x, int64_t n, const int64_t *offsets, int64_t n_seg, const float *centroids, int k,
                                 const int32_t *assign, int norm, float *out, int32_t *cnt)
{
    const size_t lds = vlad_aggregate_lds(k);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(vlad_aggregate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    vlad_aggregate_kernel<<<dim3((unsigned)n_seg), dim3(256), lds, st>>>(x, n, reinterpret_cast<const long long *>(offsets), centroids, k, assign,
                                                                       norm, out, cnt);
    return hipGetLastError();
}

hipError_t launch_vlad_update(hipStream_t st, const float *part_sum, const int32_t *part_cnt, int64_t n_chunks, int k, float *centroids,
                              long long *counts)
{
    vlad_update_kernel<<<dim3((k * VL_D + 255) / 256), dim3(256), 0, st>>>(part_sum, part_cnt, n_chunks, k, centroids, counts);
    return hipGetLastError();
}
