// libsfd2hip: the bookkeeping of the round-based mapper -- restrict the tracks to the registered views, filter
// the adjusted points, count what every unregistered view sees, assemble the candidates' 2D-3D problems.
//
// Every phase is a launch of its own; none waits on another workgroup.  The compactions are count, scan, scatter (the scans between
// the launches are rocPRIM's, api_mapper.hip).  Atomics are integer adds only, so every result is a function of the inputs.  A track or
// a point is one lane's up to SFD2_MAP_LONG_TRACK observations and one wave's beyond (the host's two lists, as in bundle_kernels.hip);
// the two mappings write the same bytes except the filter's mean error, whose sum runs in observation order (lane) or as 64 strided
// partial sums joined by a fixed tree (wave).  gfx950, wave64.
#include "pose_camera.h"
#include "mapper.h"

namespace {

constexpr int kNone = 0x7fffffff;

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = min(v, __shfl_xor(v, s));
    return v;
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// the track of observation o: the largest t with off[t] <= o (0 <= o < off[n], off[0] = 0; empty tracks are stepped over)
__device__ __forceinline__ int track_of(const int64_t *__restrict__ off, int n, int64_t o)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (off[mid] <= o) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------------------------- restrict
__global__ void __launch_bounds__(SFD2_MAP_WG) mapper_restrict_count_lane_kernel(const int32_t *__restrict__ ids, int n, const int64_t *__restrict__ off,
                                                                                 const int32_t *__restrict__ obs_view, const unsigned char *__restrict__ reg,
                                                                                 int32_t *__restrict__ keep, int32_t *__restrict__ cnt)
{
    const int i = blockIdx.x * SFD2_MAP_WG + threadIdx.x;
    if (i >= n) return;
    const int t = ids[i];
    int first = -1, c = 0;
    bool two = false;
    for (int64_t o = off[t]; o < off[t + 1]; ++o) {
        const int v = obs_view[o];
        if (!reg[v]) continue;
        if (first < 0) first = v;
        else if (v != first) two = true;
        ++c;
    }
    keep[t] = two ? 1 : 0;
    cnt[t] = two ? c : 0;
}

__global__ void __launch_bounds__(64) mapper_restrict_count_wave_kernel(const int32_t *__restrict__ ids, const int64_t *__restrict__ off,
                                                                        const int32_t *__restrict__ obs_view, const unsigned char *__restrict__ reg,
                                                                        int32_t *__restrict__ keep, int32_t *__restrict__ cnt)
{
    const int t = ids[blockIdx.x], lane = threadIdx.x;
    const int64_t b = off[t];
    const int len = (int)(off[t + 1] - b);
    int c = 0, fo = kNone;
    for (int r = lane; r < len; r += 64)
        if (reg[obs_view[b + r]]) {
            ++c;
            if (fo == kNone) fo = r;
        }
    c = wave_sum(c);
    fo = wave_min(fo);
    const int first = fo == kNone ? -1 : obs_view[b + fo];
    bool other = false;
    for (int r = lane; r < len; r += 64) {
        const int v = obs_view[b + r];
        other |= reg[v] && v != first;
    }
    const bool two = __any(other) != 0;
    if (lane == 0) {
        keep[t] = two ? 1 : 0;
        cnt[t] = two ? c : 0;
    }
}

struct RestrictOut {
    int32_t *sub_track, *sub_obs, *sub_view;
    int64_t *sub_off, *totals;
    float2 *sub_xy;
};

// the last track closes the table: the totals and the final offset
__device__ __forceinline__ void restrict_close(int t, int n_tracks, const int32_t *keep, const int32_t *cnt, const int32_t *tpos, const int32_t *opos,
                                               const RestrictOut &R)
{
    if (t != n_tracks - 1) return;
    const int64_t nt = (int64_t)tpos[t] + keep[t], no = (int64_t)opos[t] + cnt[t];
    R.totals[0] = nt;
    R.totals[1] = no;
    R.sub_off[nt] = no;
}

__global__ void __launch_bounds__(SFD2_MAP_WG) mapper_restrict_scatter_lane_kernel(const int32_t *__restrict__ ids, int n, int n_tracks,
                                                                                   const int64_t *__restrict__ off, const int32_t *__restrict__ obs_view,
                                                                                   const float2 *__restrict__ obs_xy, const unsigned char *__restrict__ reg,
                                                                                   const int32_t *__restrict__ keep, const int32_t *__restrict__ cnt,
                                                                                   const int32_t *__restrict__ tpos, const int32_t *__restrict__ opos,
                                                                                   RestrictOut R)
{
    const int i = blockIdx.x * SFD2_MAP_WG + threadIdx.x;
    if (i >= n) return;
    const int t = ids[i];
    restrict_close(t, n_tracks, keep, cnt, tpos, opos, R);
    if (!keep[t]) return;
    const int j = tpos[t];
    int64_t w = opos[t];
    R.sub_track[j] = t;
    R.sub_off[j] = w;
    for (int64_t o = off[t]; o < off[t + 1]; ++o) {
        const int v = obs_view[o];
        if (!reg[v]) continue;
        R.sub_obs[w] = (int32_t)o;
        R.sub_view[w] = v;
        R.sub_xy[w] = obs_xy[o];
        ++w;
    }
}

__global__ void __launch_bounds__(64) mapper_restrict_scatter_wave_kernel(const int32_t *__restrict__ ids, int n_tracks, const int64_t *__restrict__ off,
                                                                          const int32_t *__restrict__ obs_view, const float2 *__restrict__ obs_xy,
                                                                          const unsigned char *__restrict__ reg, const int32_t *__restrict__ keep,
                                                                          const int32_t *__restrict__ cnt, const int32_t *__restrict__ tpos,
                                                                          const int32_t *__restrict__ opos, RestrictOut R)
{
    const int t = ids[blockIdx.x], lane = threadIdx.x;
    if (lane == 0) restrict_close(t, n_tracks, keep, cnt, tpos, opos, R);
    if (!keep[t]) return;
    const int j = tpos[t];
    int64_t w = opos[t];
    if (lane == 0) {
        R.sub_track[j] = t;
        R.sub_off[j] = w;
    }
    const int64_t e = off[t + 1];
    for (int64_t base = off[t]; base < e; base += 64) {      // 64 observations at a time, their order kept by the ballot's prefix count
        const int64_t o = base + lane;
        const int v = o < e ? obs_view[o] : 0;
        const bool r = o < e && reg[v];
        const unsigned long long mask = __ballot(r);
        if (r) {
            const int64_t at = w + __popcll(mask & ((1ull << lane) - 1ull));
            R.sub_obs[at] = (int32_t)o;
            R.sub_view[at] = v;
            R.sub_xy[at] = obs_xy[o];
        }
        w += __popcll(mask);
    }
}

// ---------------------------------------------------------------------------------------------------------------- filter
__global__ void __launch_bounds__(SFD2_MAP_WG) mapper_filter_obs_kernel(const TriViewDev *__restrict__ views, const double *__restrict__ xyz,
                                                                        const int32_t *__restrict__ obs_view, const int32_t *__restrict__ obs_pt,
                                                                        const double2 *__restrict__ obs_xy, int64_t n, double max_err,
                                                                        double *__restrict__ err, unsigned char *__restrict__ keep, double *__restrict__ ray)
{
    const int64_t o = (int64_t)blockIdx.x * SFD2_MAP_WG + threadIdx.x;
    if (o >= n) return;
    const TriViewDev &V = views[obs_view[o]];
    const double *X = xyz + 3 * (int64_t)obs_pt[o];
    const double x = X[0], y = X[1], z = X[2];
    double Pc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) Pc[a] = V.R[3 * a] * x + V.R[3 * a + 1] * y + V.R[3 * a + 2] * z + V.t[a];
    double px, py;
    project_px(V.cam, Pc, px, py);
    const double2 q = obs_xy[o];
    const double dx = px - q.x, dy = py - q.y;
    const double e = sqrt(dx * dx + dy * dy);
    err[o] = e;
    keep[o] = (Pc[2] > 0.0 && e <= max_err) ? 1 : 0;           // a NaN fails both comparisons
    ray[3 * o] = V.C[0] - x;
    ray[3 * o + 1] = V.C[1] - y;
    ray[3 * o + 2] = V.C[2] - z;
}

// the angle between two rays, radians in [0, pi]: atan2 of |a x b| and a . b (well conditioned at small angles, where acos is not)
__device__ __forceinline__ double ray_angle(const double *__restrict__ a, const double *__restrict__ b)
{
    const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
    return atan2(sqrt(cx * cx + cy * cy + cz * cz), a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
}

__device__ __forceinline__ void filter_store(int64_t p, int nk, bool two, double sum, double amax, double min_angle_deg, unsigned char *__restrict__ live,
                                             double *__restrict__ perr, double *__restrict__ pangle)
{
    const double deg = nk >= 2 ? amax * (180.0 / 3.14159265358979323846) : __longlong_as_double(0x7ff8000000000000LL);
    perr[p] = nk ? sum / (double)nk : 0.0;
    pangle[p] = deg;
    live[p] = (two && deg >= min_angle_deg) ? 1 : 0;
}

__global__ void __launch_bounds__(SFD2_MAP_WG) mapper_filter_point_lane_kernel(const int32_t *__restrict__ ids, int n, const int64_t *__restrict__ off,
                                                                               const int32_t *__restrict__ obs_view, const double *__restrict__ err,
                                                                               const unsigned char *__restrict__ keep, const double *__restrict__ ray,
                                                                               double min_angle_deg, unsigned char *__restrict__ live,
                                                                               double *__restrict__ perr, double *__restrict__ pangle)
{
    const int i = blockIdx.x * SFD2_MAP_WG + threadIdx.x;
    if (i >= n) return;
    const int64_t p = ids[i], b = off[p], e = off[p + 1];
    int nk = 0, first = -1;
    bool two = false;
    double sum = 0.0, amax = 0.0;
    for (int64_t o = b; o < e; ++o) {
        if (!keep[o]) continue;
        const int v = obs_view[o];
        if (first < 0) first = v;
        else if (v != first) two = true;
        ++nk;
        sum += err[o];
        for (int64_t u = o + 1; u < e; ++u)
            if (keep[u]) amax = fmax(amax, ray_angle(ray + 3 * o, ray + 3 * u));
    }
    filter_store(p, nk, two, sum, amax, min_angle_deg, live, perr, pangle);
}

__global__ void __launch_bounds__(64) mapper_filter_point_wave_kernel(const int32_t *__restrict__ ids, const int64_t *__restrict__ off,
                                                                      const int32_t *__restrict__ obs_view, const double *__restrict__ err,
                                                                      const unsigned char *__restrict__ keep, const double *__restrict__ ray,
                                                                      double min_angle_deg, unsigned char *__restrict__ live, double *__restrict__ perr,
                                                                      double *__restrict__ pangle)
{
    const int lane = threadIdx.x;
    const int64_t p = ids[blockIdx.x], b = off[p];
    const int len = (int)(off[p + 1] - b);
    int nk = 0, fo = kNone;
    double sum = 0.0, amax = 0.0;
    for (int r = lane; r < len; r += 64)
        if (keep[b + r]) {
            ++nk;
            sum += err[b + r];
            if (fo == kNone) fo = r;
        }
    nk = wave_sum(nk);
    fo = wave_min(fo);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) sum += __shfl_down(sum, s);   // the fixed tree: lane l += lane l + s; lane 0 ends with the sum
    const int first = fo == kNone ? -1 : obs_view[b + fo];
    bool other = false;
    // the len (len - 1) / 2 pairs, spread evenly: row r pairs with the next len / 2 observations round the circle (for an even len the
    // last distance names every pair twice, so only the first half of the rows takes it)
    const int half = len / 2;
    for (int r = lane; r < len; r += 64) {
        if (!keep[b + r]) continue;
        other |= obs_view[b + r] != first;
        for (int d = 1; d <= half; ++d) {
            if (2 * d == len && r >= half) break;
            int u = r + d;
            if (u >= len) u -= len;
            if (keep[b + u]) amax = fmax(amax, ray_angle(ray + 3 * (b + r), ray + 3 * (b + u)));
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) amax = fmax(amax, __shfl_xor(amax, s));
    const bool two = __any(other) != 0;
    if (lane == 0) filter_store(p, nk, two, sum, amax, min_angle_deg, live, perr, pangle);
}

// ---------------------------------------------------------------------------------------------------------------- visible
__global__ void __launch_bounds__(SFD2_MAP_WG) mapper_track_points_kernel(const int32_t *__restrict__ point_track, const unsigned char *__restrict__ point_live,
                                                                          int n, int32_t *__restrict__ tlive, int32_t *__restrict__ tfirst)
{
    const int p = blockIdx.x * SFD2_MAP_WG + threadIdx.x;
    if (p >= n) return;
    const int t = point_track[p];
    if (point_live[p]) atomicAdd(&tlive[t], 1);
    if (tfirst && (p == 0 || point_track[p - 1] != t)) tfirst[t] = p;
}

__global__ void __launch_bounds__(SFD2_MAP_WG) mapper_visible_kernel(const int64_t *__restrict__ off, int n_tracks, const int32_t *__restrict__ obs_view,
                                                                     int64_t n, const unsigned char *__restrict__ reg, const int32_t *__restrict__ tlive,
                                                                     unsigned long long *__restrict__ counts)
{
    const int64_t o = (int64_t)blockIdx.x * SFD2_MAP_WG + threadIdx.x;
    if (o >= n) return;
    const int v = obs_view[o];
    if (reg[v]) return;
    const int c = tlive[track_of(off, n_tracks, o)];
    if (c) atomicAdd(&counts[v], (unsigned long long)c);
}

// ---------------------------------------------------------------------------------------------------------------- assemble
// exclusive scan of v over the block's 256 threads in thread order; total = the block's sum; sh: 4 ints
__device__ __forceinline__ int block_scan(int v, int *sh, int &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) sh[w] = x;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) base += i < w ? sh[i] : 0;
    total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return base + x - v;
}

__global__ void __launch_bounds__(SFD2_MAP_WG) mapper_assemble_count_kernel(const int32_t *__restrict__ cand, const int64_t *__restrict__ view_off,
                                                                            const int32_t *__restrict__ view_obs, const int64_t *__restrict__ off,
                                                                            int n_tracks, const int32_t *__restrict__ tlive, int64_t *__restrict__ total)
{
    __shared__ int sh[4];
    const int v = cand[blockIdx.x];
    int64_t sum = 0;
    const int64_t b = view_off[v], e = view_off[v + 1];
    for (int64_t base = b; base < e; base += SFD2_MAP_WG) {   // uniform trip count: the scan's barriers are reached by every thread
        const int64_t i = base + threadIdx.x;
        const int c = i < e ? tlive[track_of(off, n_tracks, view_obs[i])] : 0;
        int chunk;
        (void)block_scan(c, sh, chunk);
        sum += chunk;
    }
    if (threadIdx.x == 0) total[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(SFD2_MAP_WG) mapper_assemble_scatter_kernel(const int32_t *__restrict__ cand, const int64_t *__restrict__ view_off,
                                                                              const int32_t *__restrict__ view_obs, const int64_t *__restrict__ off,
                                                                              int n_tracks, const float2 *__restrict__ obs_xy, const int32_t *__restrict__ tfirst,
                                                                              const int32_t *__restrict__ point_track, const unsigned char *__restrict__ point_live,
                                                                              int n_points, const double *__restrict__ xyz, const int64_t *__restrict__ offsets,
                                                                              double2 *__restrict__ p2, double *__restrict__ p3, int32_t *__restrict__ src_obs,
                                                                              int32_t *__restrict__ src_point)
{
    __shared__ int sh[4];
    const int v = cand[blockIdx.x];
    int64_t w = offsets[blockIdx.x];
    const int64_t b = view_off[v], e = view_off[v + 1];
    for (int64_t base = b; base < e; base += SFD2_MAP_WG) {
        const int64_t i = base + threadIdx.x;
        int o = -1, t = -1, p0 = -1, c = 0;
        if (i < e) {
            o = view_obs[i];
            t = track_of(off, n_tracks, o);
            p0 = tfirst[t];
            if (p0 >= 0)
                for (int p = p0; p < n_points && point_track[p] == t; ++p) c += point_live[p] ? 1 : 0;
        }
        int chunk;
        int64_t at = w + block_scan(c, sh, chunk);
        if (c) {
            const float2 q = obs_xy[o];
            const double2 q2 = make_double2((double)q.x + 0.5, (double)q.y + 0.5);
            for (int p = p0; p < n_points && point_track[p] == t; ++p) {
                if (!point_live[p]) continue;
                p2[at] = q2;
                p3[3 * at] = xyz[3 * (int64_t)p];
                p3[3 * at + 1] = xyz[3 * (int64_t)p + 1];
                p3[3 * at + 2] = xyz[3 * (int64_t)p + 2];
                src_obs[at] = o;
                src_point[at] = p;
                ++at;
            }
        }
        w += chunk;
    }
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + SFD2_MAP_WG - 1) / SFD2_MAP_WG); }

}  // namespace

void launch_mapper_restrict_count(hipStream_t st, const int32_t *short_ids, int n_short, const int32_t *long_ids, int n_long, const int64_t *off,
                                  const int32_t *obs_view, const unsigned char *reg, int32_t *keep, int32_t *cnt)
{
    if (n_short) mapper_restrict_count_lane_kernel<<<blocks_of(n_short), SFD2_MAP_WG, 0, st>>>(short_ids, n_short, off, obs_view, reg, keep, cnt);
    if (n_long) mapper_restrict_count_wave_kernel<<<(unsigned)n_long, 64, 0, st>>>(long_ids, off, obs_view, reg, keep, cnt);
}

void launch_mapper_restrict_scatter(hipStream_t st, const int32_t *short_ids, int n_short, const int32_t *long_ids, int n_long, int n_tracks,
                                    const int64_t *off, const int32_t *obs_view, const float2 *obs_xy, const unsigned char *reg, const int32_t *keep,
                                    const int32_t *cnt, const int32_t *tpos, const int32_t *opos, int32_t *sub_track, int64_t *sub_off, int32_t *sub_obs,
                                    int32_t *sub_view, float2 *sub_xy, int64_t *totals)
{
    RestrictOut R;
    R.sub_track = sub_track; R.sub_obs = sub_obs; R.sub_view = sub_view; R.sub_off = sub_off; R.totals = totals; R.sub_xy = sub_xy;
    if (n_short)
        mapper_restrict_scatter_lane_kernel<<<blocks_of(n_short), SFD2_MAP_WG, 0, st>>>(short_ids, n_short, n_tracks, off, obs_view, obs_xy, reg, keep, cnt,
                                                                                         tpos, opos, R);
    if (n_long) mapper_restrict_scatter_wave_kernel<<<(unsigned)n_long, 64, 0, st>>>(long_ids, n_tracks, off, obs_view, obs_xy, reg, keep, cnt, tpos, opos, R);
}

void launch_mapper_filter_obs(hipStream_t st, const TriViewDev *views, const double *xyz, const int32_t *obs_view, const int32_t *obs_pt,
                              const double2 *obs_xy, int64_t n, double max_err, double *err, unsigned char *keep, double *ray)
{
    if (n) mapper_filter_obs_kernel<<<blocks_of(n), SFD2_MAP_WG, 0, st>>>(views, xyz, obs_view, obs_pt, obs_xy, n, max_err, err, keep, ray);
}

void launch_mapper_filter_points(hipStream_t st, const int32_t *short_ids, int n_short, const int32_t *long_ids, int n_long, const int64_t *off,
                                 const int32_t *obs_view, const double *err, const unsigned char *keep, const double *ray, double min_angle_deg,
                                 unsigned char *live, double *perr, double *pangle)
{
    if (n_short)
        mapper_filter_point_lane_kernel<<<blocks_of(n_short), SFD2_MAP_WG, 0, st>>>(short_ids, n_short, off, obs_view, err, keep, ray, min_angle_deg, live,
                                                                                     perr, pangle);
    if (n_long) mapper_filter_point_wave_kernel<<<(unsigned)n_long, 64, 0, st>>>(long_ids, off, obs_view, err, keep, ray, min_angle_deg, live, perr, pangle);
}

void launch_mapper_track_points(hipStream_t st, const int32_t *point_track, const unsigned char *point_live, int n_points, int32_t *tlive, int32_t *tfirst)
{
    if (n_points) mapper_track_points_kernel<<<blocks_of(n_points), SFD2_MAP_WG, 0, st>>>(point_track, point_live, n_points, tlive, tfirst);
}

void launch_mapper_visible(hipStream_t st, const int64_t *off, int n_tracks, const int32_t *obs_view, int64_t n_obs, const unsigned char *reg,
                           const int32_t *tlive, unsigned long long *counts)
{
    if (n_obs) mapper_visible_kernel<<<blocks_of(n_obs), SFD2_MAP_WG, 0, st>>>(off, n_tracks, obs_view, n_obs, reg, tlive, counts);
}

void launch_mapper_assemble_count(hipStream_t st, const int32_t *cand, int k, const int64_t *view_off, const int32_t *view_obs, const int64_t *off,
                                  int n_tracks, const int32_t *tlive, int64_t *total)
{
    if (k) mapper_assemble_count_kernel<<<(unsigned)k, SFD2_MAP_WG, 0, st>>>(cand, view_off, view_obs, off, n_tracks, tlive, total);
}

void launch_mapper_assemble_scatter(hipStream_t st, const int32_t *cand, int k, const int64_t *view_off, const int32_t *view_obs, const int64_t *off,
                                    int n_tracks, const float2 *obs_xy, const int32_t *tfirst, const int32_t *point_track,
                                    const unsigned char *point_live, int n_points, const double *xyz, const int64_t *offsets, double2 *p2, double *p3,
                                    int32_t *src_obs, int32_t *src_point)
{
    if (k)
        mapper_assemble_scatter_kernel<<<(unsigned)k, SFD2_MAP_WG, 0, st>>>(cand, view_off, view_obs, off, n_tracks, obs_xy, tfirst, point_track, point_live,
                                                                             n_points, xyz, offsets, p2, p3, src_obs, src_point);
}
