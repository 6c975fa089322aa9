// libsfd2hip: the arithmetic the four LO-RANSAC kernels (pose_kernels.hip, two_view_kernels.hip, fundamental_kernels.hip,
// homography_kernels.hip) share -- the sampler, the normal equations and their damped Cholesky solve, and COLMAP's stopping rule.
// No HIP include: a plain host compiler builds it too (tests/host/ransac_math_main.cpp).  Everything is a template that unrolls
// completely at its N, so each kernel gets the code it would get from its own copy.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef SFD2_PD
#ifdef __HIPCC__
#define SFD2_PD __host__ __device__ __forceinline__
#else
#define SFD2_PD inline
#endif
#endif

namespace {

SFD2_PD bool finite_d(double v) { return __builtin_isfinite(v); }

// ---------------------------------------------------------------------------------------------------------------- sampling
SFD2_PD uint64_t mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// K distinct indices in [0, n), n >= K, from (seed, trial) only: draw k is h_k mod (n - k) from the chain h_0 = mix64(seed ^
// mix64(trial)), h_k = mix64(h_k-1), then stepped over the earlier indices in ascending order.  Integers only: exact everywhere.
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
            const int lo = srt[p] < ins ? srt[p] : ins, hi = srt[p] < ins ? ins : srt[p];
            srt[p] = lo;
            ins = hi;
        }
        srt[k] = ins;
    }
}

// ---------------------------------------------------------------------------------------------------------------- normal equations
// s: the packed upper triangle of J^T J (NP (NP + 1) / 2 entries, row by row), the gradient J^T r (NP entries), then whatever the
// caller keeps behind them; the cost, by convention, in the last entry.
template <int NP>
constexpr int normal_size() { return NP * (NP + 1) / 2 + NP; }

// one residual r with its derivative J: triangle, gradient, and r^2 into the entry after them
template <int NP, int NS>
SFD2_PD void normal_acc(double (&s)[NS], const double (&J)[NP], double r)
{
    static_assert(NS > normal_size<NP>(), "no room for the cost");
    constexpr int NT = NP * (NP + 1) / 2;
    int k = 0;
#pragma unroll
    for (int a = 0; a < NP; ++a)
#pragma unroll
        for (int b = a; b < NP; ++b, ++k) s[k] += J[a] * J[b];
#pragma unroll
    for (int a = 0; a < NP; ++a) s[NT + a] += J[a] * r;
    s[NT + NP] += r * r;
}

// Solves (H + lambda diag(H) + 1e-15 max diag(H) I) d = -g by Cholesky; false when not positive definite or not finite.
template <int NP, int NS>
SFD2_PD bool chol_solve(const double (&s)[NS], double lambda, double (&d)[NP])
{
    static_assert(NS >= normal_size<NP>(), "triangle and gradient do not fit");
    constexpr int N = NP, NT = NP * (NP + 1) / 2;
    double A[N * N];
    int k = 0;
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = a; b < N; ++b, ++k) { A[a * N + b] = s[k]; A[b * N + a] = s[k]; }
    double mx = 0;
#pragma unroll
    for (int a = 0; a < N; ++a) mx = fmax(mx, A[a * (N + 1)]);
    if (!(mx > 0) || !finite_d(mx)) return false;
#pragma unroll
    for (int a = 0; a < N; ++a) A[a * (N + 1)] += lambda * A[a * (N + 1)] + 1e-15 * mx;
#pragma unroll
    for (int j = 0; j < N; ++j) {                       // A = L L^T in place (lower)
        double dj = A[j * (N + 1)];
#pragma unroll
        for (int p = 0; p < j; ++p) dj -= A[j * N + p] * A[j * N + p];
        if (!(dj > 0)) return false;
        const double l = sqrt(dj);
        A[j * (N + 1)] = l;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = A[i * N + j];
#pragma unroll
            for (int p = 0; p < j; ++p) v -= A[i * N + p] * A[j * N + p];
            A[i * N + j] = v / l;
        }
    }
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = -s[NT + i];
#pragma unroll
        for (int p = 0; p < i; ++p) v -= A[i * N + p] * y[p];
        y[i] = v / A[i * (N + 1)];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int p = i + 1; p < N; ++p) v -= A[p * N + i] * d[p];
        d[i] = v / A[i * (N + 1)];
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; ++i) ok = ok && finite_d(d[i]);
    return ok;
}

// ---------------------------------------------------------------------------------------------------------------- stopping
// After a round: true when RANSAC stops at `trials` -- the limit is reached, or COLMAP's ComputeNumTrials (multiplier 3) on the best
// inlier ratio best_cnt / n asks for no more and min_trials have run.  ratio_pow(ratio): ratio ^ sample size, which every caller
// spells out as a product: (r r)(r r) and ((r r) r) r can differ in the last bit, and that bit goes through log and ceil into the
// trial count, so a generic pow would change results.  Conf: min_trials, max_trials, confidence.
template <class Conf, class Pow>
SFD2_PD bool ransac_enough(int64_t trials, const Conf &conf, int n, int best_cnt, Pow ratio_pow)
{
    if (trials >= conf.max_trials) return true;
    if (!(trials >= conf.min_trials && best_cnt > 0)) return false;
    const double nom = 1.0 - conf.confidence;
    const double den = 1.0 - ratio_pow((double)best_cnt / n);
    double need;
    if (nom <= 0) need = 1e300;
    else if (den <= 0) need = 1.0;
    else if (den == 1.0 || fabs(log(den)) < 1e-16) need = 1e300;
    else need = ceil(log(nom) / log(den) * 3.0);
    return (double)trials >= need;
}

}  // namespace
