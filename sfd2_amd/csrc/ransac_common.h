// libsfd2hip: what the four LO-RANSAC kernels (pose_kernels.hip, two_view_kernels.hip, fundamental_kernels.hip, homography_kernels.hip)
// share, the one header they include.  The arithmetic (sampler, normal equations, Cholesky solve, stopping rule) is in ransac_math.h;
// here is what needs the device: the workgroup reductions in a fixed order (wave butterflies, then the waves in index order), the
// fp64 support and its scoring, and for the matrix estimators (F, H) the output convention.  A workgroup is SFD2_TV_WG =
// SFD2_POSE_WG threads.
// Not here, on purpose: the final Levenberg-Marquardt loop, the Hartley preparation and the LO step stay in each
// kernel, and fundamental_kernels.hip keeps its own scoring loops.  Moved into a shared function they compile to other basic blocks,
// the compiler fuses other multiply-add pairs, and the results change in their last bits; every entry point returns the bytes it did.
#pragma once
#include "sfd2_internal.h"
#include "ransac_math.h"

static_assert(SFD2_POSE_WG == SFD2_TV_WG, "the reductions assume one workgroup size");

namespace {

constexpr int kRcWG = SFD2_TV_WG;
constexpr int kRcWaves = kRcWG / 64;

// ---------------------------------------------------------------------------------------------------------------- reductions
// Sum over the workgroup in a fixed order; every thread receives the same totals.  red: kRcWaves * N doubles of LDS
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

// The best support of the workgroup.  S supplies better(a, b), a total order (so the result does not depend on the reduction's
// shape), and shfl_support(s, m), its lane shuffle.  red: kRcWaves entries of LDS
template <class S>
__device__ __forceinline__ S wg_best(S s, S *red)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const S o = shfl_support(s, m);
        if (better(o, s)) s = o;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = s;
    __syncthreads();
    S b = red[0];
#pragma unroll
    for (int q = 1; q < kRcWaves; ++q)
        if (better(red[q], b)) b = red[q];
    return b;
}

// ---------------------------------------------------------------------------------------------------------------- fp64 support (E, F, H)
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
__device__ __forceinline__ Support shfl_support(const Support &s, int m)
{
    Support o;
    o.cnt = __shfl_xor(s.cnt, m, 64);
    o.sum = __shfl_xor(s.sum, m, 64);
    o.trial = __shfl_xor(s.trial, m, 64);
    return o;
}

// one matrix scored by one lane over all correspondences in point order (j is wave-uniform: one load per wave and point)
template <class Err>
__device__ __forceinline__ void score_lane(Err err, const double (&M)[9], const double2 *x0, const double2 *x1, int n, double th2, int &cnt,
                                           double &sum)
{
    cnt = 0;
    sum = 0.0;
    for (int j = 0; j < n; ++j) {
        const double e = err(M, x0[j], x1[j]);
        const bool in = e <= th2;
        cnt += in ? 1 : 0;
        sum += in ? e : 0.0;
    }
}
// one matrix scored by the whole workgroup (strided), totals in a fixed order.  red: kRcWaves * 2 doubles of LDS
template <class Err>
__device__ __forceinline__ void score_wg(Err err, const double (&M)[9], const double2 *x0, const double2 *x1, int n, double th2, double *red,
                                         int &cnt, double &sum)
{
    double v[2] = {0.0, 0.0};
    for (int j = threadIdx.x; j < n; j += kRcWG) {
        const double e = err(M, x0[j], x1[j]);
        if (e <= th2) { v[0] += 1.0; v[1] += e; }
    }
    wg_sum(v, red);
    cnt = (int)v[0];
    sum = v[1];
}
// the lane whose trial won the round writes its matrix to LDS, everyone reads it.  sh: 9 doubles of LDS
__device__ __forceinline__ void publish_winner(bool winner, const double (&mine)[9], double *sh, double (&best)[9])
{
    if (winner)
#pragma unroll
        for (int i = 0; i < 9; ++i) sh[i] = mine[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 9; ++i) best[i] = sh[i];
}

// ---------------------------------------------------------------------------------------------------------------- matrix estimators (F, H)
// The output convention: P at unit Frobenius norm with its first entry of largest magnitude positive; all zero, and no success, when
// that is not finite.
__device__ __forceinline__ void finish_matrix(const double (&P)[9], int best_cnt, const TvConfDev &conf, FmResDev &out)
{
    double nn = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) nn += P[i] * P[i];
    double inv = 1.0 / sqrt(nn);
    double lead = P[0];
#pragma unroll
    for (int i = 1; i < 9; ++i)
        if (fabs(P[i]) > fabs(lead)) lead = P[i];
    if (lead < 0) inv = -inv;
    bool fin = finite_d(inv);
#pragma unroll
    for (int i = 0; i < 9; ++i) { out.F[i] = P[i] * inv; fin = fin && finite_d(out.F[i]); }
    out.success = (fin && best_cnt >= conf.min_num_inliers) ? 1 : 0;
    if (!fin)
#pragma unroll
        for (int i = 0; i < 9; ++i) out.F[i] = 0.0;
}

}  // namespace
