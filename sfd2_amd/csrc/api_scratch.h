// libsfd2hip, host side: what the geometry entry points (api_pose / assemble / triangulate / pairs / cluster / frames .hip) share --
// the layout of one scratch block, the checks that stand between a caller's array and an index a kernel follows, and the RANSAC entry
// points' one statement of their trial limits.
// Standard C++ only (no HIP): tests/host/api_scratch_main.cpp runs it under the sanitizers.  The block itself is a ScratchBuf (sfd2_ctx.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Carve {                        // offsets into one block, 256-byte aligned; an empty array still takes a slot of its own
    size_t off = 0;
    size_t take(size_t bytes)
    {
        const size_t o = off;
        off += align256(std::max<size_t>(bytes, 1));
        return o;
    }
};

// the array at a carved offset
template <typename T> T *at(char *base, size_t off) { return reinterpret_cast<T *>(base + off); }

// n + 1 offsets that start at 0 and do not decrease
inline bool monotone(const int64_t *o, int64_t n)
{
    if (o[0] != 0) return false;
    for (int64_t i = 0; i < n; ++i)
        if (o[i + 1] < o[i]) return false;
    return true;
}

// the first of a's n entries outside [0, hi), n when there is none
inline int64_t first_outside(const int32_t *a, int64_t n, int hi)
{
    for (int64_t i = 0; i < n; ++i)
        if (a[i] < 0 || a[i] >= hi) return i;
    return n;
}

inline bool in_range(const int32_t *a, int64_t n, int hi) { return first_outside(a, n, hi) == n; }

template <typename T> bool all_finite(const T *p, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// ---- the trial limits of the RANSAC entry points (absolute pose, its focal sweep, relative pose, the F / H pairs)
// what is wrong with the options every RANSAC entry point takes, nullptr when nothing is; the caller puts its own name in front
inline const char *ransac_conf_error(double confidence, double min_inlier_ratio, int64_t min_num_trials, int64_t max_num_trials)
{
    if (!(confidence >= 0 && confidence <= 1) || !(min_inlier_ratio >= 0 && min_inlier_ratio <= 1))
        return ": confidence and min_inlier_ratio must lie in [0, 1]";
    if (max_num_trials < 1 || max_num_trials > 1000000000 || min_num_trials < 0)
        return ": trial limits out of range (1 <= max_num_trials <= 1e9, min_num_trials >= 0)";
    return nullptr;
}

// COLMAP's RANSAC assumes min_inlier_ratio in steps of 1e-5 (kNumSamples = 100000)
inline double floored_ratio(double min_inlier_ratio) { return std::floor(min_inlier_ratio * 100000) / 100000.0; }

// COLMAP ComputeNumTrials (dyn_num_trials_multiplier 3) on the probability that a sample holds inliers only; 1e300 stands for "never"
inline double num_trials(double p_all_inliers, double confidence)
{
    const double nom = 1.0 - confidence;
    if (nom <= 0) return 1e300;
    const double den = 1.0 - p_all_inliers;
    if (den <= 0) return 1.0;
    if (den == 1.0 || std::fabs(std::log(den)) < 1e-16) return 1e300;
    return std::ceil(std::log(nom) / std::log(den) * 3.0);
}

struct TrialLimits {
    int64_t max_trials, min_trials;
};

// COLMAP's RANSAC: max_num_trials limited by the trial count of the assumed min_inlier_ratio, at least 1; min_num_trials clamped to it;
// both at most cap.  p_all_inliers = floored_ratio(min_inlier_ratio) to the sample size, by the caller: its last bit goes through log
// and ceil into max_trials, so every entry point keeps the power it has always used (ransac_math.h, ransac_enough).
inline TrialLimits trial_limits(double confidence, int64_t min_num_trials, int64_t max_num_trials, int64_t cap, double p_all_inliers)
{
    TrialLimits t;
    t.max_trials = std::max<int64_t>(1, std::min<double>((double)std::min(max_num_trials, cap), num_trials(p_all_inliers, confidence)));
    t.min_trials = std::min(std::min(min_num_trials, cap), t.max_trials);
    return t;
}
