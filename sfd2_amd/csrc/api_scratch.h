// libsfd2hip, host side: what the geometry entry points (api_pose / assemble / triangulate / pairs / cluster / frames .hip) share --
// the layout of one scratch block and the checks that stand between a caller's array and an index a kernel follows.
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
