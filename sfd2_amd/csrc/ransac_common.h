// libsfd2hip: what the two-view RANSAC kernels (two_view_kernels.hip, fundamental_kernels.hip, homography_kernels.hip) share -- the workgroup reductions in a
// fixed order (wave butterflies, then the waves in index order), the support order and the sampler.  A workgroup is SFD2_TV_WG threads.
#pragma once
#include "sfd2_internal.h"

#ifndef SFD2_PD
#define SFD2_PD __host__ __device__ __forceinline__
#endif

namespace {

constexpr int kRcWaves = SFD2_TV_WG / 64;

// ---------------------------------------------------------------------------------------------------------------- reductions
// red: kRcWaves * N doubles of LDS
template <int N>
__device__ __forceinline__ void wg_sum(double (&v)[N], double *red)
{
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v[i] += __shfl_xor(v[i], m, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) red[w * N + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = red[i];
#pragma unroll
        for (int q = 1; q < kRcWaves; ++q) s += red[q * N + i];
        v[i] = s;
    }
}

struct Support {
    int cnt;          // -1: no hypothesis
    double sum;
    long long trial;
};
__device__ __forceinline__ bool better(const Support &a, const Support &b)
{
    if (a.cnt != b.cnt) return a.cnt > b.cnt;
    if (a.sum != b.sum) return a.sum < b.sum;
    return a.trial < b.trial;
}
// red: kRcWaves entries of LDS
__device__ __forceinline__ Support wg_best(Support s, Support *red)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        Support o;
        o.cnt = __shfl_xor(s.cnt, m, 64);
        o.sum = __shfl_xor(s.sum, m, 64);
        o.trial = __shfl_xor(s.trial, m, 64);
        if (better(o, s)) s = o;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = s;
    __syncthreads();
    Support b = red[0];
#pragma unroll
    for (int q = 1; q < kRcWaves; ++q)
        if (better(red[q], b)) b = red[q];
    return b;
}

// ---------------------------------------------------------------------------------------------------------------- sampling
SFD2_PD uint64_t mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// K distinct indices in [0, n), n >= K, from (seed, trial) only: draw k is h_k mod (n - k) from the chain h_0 = mix64(seed ^
// mix64(trial)), h_k = mix64(h_k-1), then stepped over the earlier indices in ascending order (sample3's scheme, pose_kernels.hip)
template <int K>
SFD2_PD void sample_k(uint64_t seed, int64_t trial, int n, int (&id)[K])
{
    uint64_t h = mix64(seed ^ mix64((uint64_t)trial));
    int srt[K];                                         // the earlier indices, ascending
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k) h = mix64(h);
        int v = (int)(h % (uint64_t)(n - k));
#pragma unroll
        for (int p = 0; p < k; ++p)
            if (v >= srt[p]) ++v;
        id[k] = v;
        int ins = v;                                    // insert v into srt[0 .. k]
#pragma unroll
        for (int p = 0; p < k; ++p) {
            const int lo = min(srt[p], ins), hi = max(srt[p], ins);
            srt[p] = lo;
            ins = hi;
        }
        srt[k] = ins;
    }
}
SFD2_PD void sample5(uint64_t seed, int64_t trial, int n, int (&id)[5]) { sample_k<5>(seed, trial, n, id); }

}  // namespace
