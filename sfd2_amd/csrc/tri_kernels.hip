// libsfd2hip: the SfM map from matches and known poses, the device side of sfd2_verify_matches_batch, sfd2_build_tracks and
// sfd2_triangulate_tracks (api_triangulate.hip).  Replaces what hloc/triangulation.py gets from `colmap matches_importer` and
// `colmap point_triangulator` with the poses and intrinsics fixed (triangulation.py:134-142).
//
// (a) verification.  Every key point is normalised once through its camera (img_to_norm, pose_camera.h) into a table that stays
//     in HBM; a block owns SFD2_TRI_WG matches of one pair and measures the point-to-epipolar-line distance in either image with
//     the pair's essential matrix (from the given poses, built by the host in fp64).  Rejected matches become (-1, -1) in place;
//     the block's survivor count is a ballot + popcount, a pair's count the sum of its blocks, and a third launch clears the
//     pairs below min_num_inliers.  Nothing is compacted, so no position depends on anything but the input order.
// (b) tracks.  Connected components of the graph node = key point, edge = surviving match, by atomic-min hooking
//     (parent[max(pu, pv)] <- min(pu, pv), a vector atomic on global memory) and pointer jumping, a round = one launch of each.
//     parent[v] <= v always holds and only decreases; a round that changes nothing proves parent[v] = the smallest node of v's
//     component, a definition free of the execution order.  The host stops at the first quiet round or at the ceiling
//     (SFD2_TRI_ST_NOT_CONVERGED).  The CSR then comes from a stable radix sort of (label, node) and two exclusive scans
//     (api_triangulate.hip, rocPRIM); tri_cc_flags / tri_cc_scatter are the element-wise steps between them.
// (c) triangulation.  One wave owns one track (a block is one wave, so a long track delays no other; the host launches the
//     long tracks first).  Up to SFD2_TRI_MAX_POINTS passes over the observations no point has taken yet:
//       hypotheses   lane h = pair h of the free observations when there are at most 64 pairs, else the pair drawn from
//                    mix64(seed, track label, 64 * pass + h); midpoint triangulation of the two rays in fp64, positive depth in
//                    both views, triangulation angle >= min_tri_angle;
//       scoring      every lane walks the free observations (uniform loads): tan(angular error) <= tan(create_max_angle_error)
//                    and positive depth, one observation per image (smallest error, then smallest index); support order more
//                    observations, smaller error sum (accumulated in observation order), smaller lane;
//       refinement   lanes = observations: Levenberg-Marquardt on the three coordinates, squared reprojection error in pixels
//                    through the camera model, sums by per-lane order then an xor butterfly (every lane gets the same bits);
//       completion   free observations within filter_max_reproj_error join (one per image), one more refinement;
//       filter       observations beyond the bound return to the free set, a point with fewer than two observations or with
//                    no pair of views at >= min_tri_angle is dropped (and ends the track's passes).
//     Membership lives in obs_point (global, -1 = free), so a track's length has no ceiling and no LDS is used.  A track's
//     result depends on its observations, its label and the seed only.  Every loop is bounded by the track length, the 64
//     hypotheses, SFD2_TRI_MAX_POINTS or the iteration limits.
#include "sfd2_internal.h"
#include "pose_camera.h"

namespace {

constexpr int kWG = SFD2_TRI_WG;
constexpr int kWave = SFD2_TRI_WAVE;
constexpr int kJumpSteps = 64;        // pointer jumping steps per node and round

SFD2_PD bool tri_finite(double v) { return __builtin_isfinite(v); }

SFD2_PD uint64_t tri_mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---------------------------------------------------------------------------------------------------------------- verification
__global__ __launch_bounds__(kWG) void tri_normalise_kernel(const TriViewDev *__restrict__ views, int n_views, const int64_t *__restrict__ offsets,
                                                            const float *__restrict__ kp, int64_t n, double2 *__restrict__ xn)
{
    const int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = n_views;                                // the image with offsets[lo] <= i < offsets[lo + 1]
    for (int s = 0; s < 32 && hi - lo > 1; ++s) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    double u, v;
    img_to_norm(views[lo].cam, (double)kp[2 * i] + 0.5, (double)kp[2 * i + 1] + 0.5, u, v);   // the COLMAP origin, triangulation.py:64
    xn[i] = make_double2(u, v);
}

__global__ __launch_bounds__(kWG) void tri_verify_kernel(const TriPairDev *__restrict__ pairs, const int32_t *__restrict__ blk_pair,
                                                         const double2 *__restrict__ xn, int32_t *__restrict__ matches,
                                                         int32_t *__restrict__ blk_cnt, int32_t *pair_status)
{
    __shared__ int wcnt[kWG / 64];
    const int p = blk_pair[blockIdx.x];
    const TriPairDev &P = pairs[p];
    const int idx = ((int)blockIdx.x - P.blk0) * kWG + (int)threadIdx.x;
    bool ok = false;
    if (idx < P.n) {
        int32_t *m = matches + 2 * (P.moff + idx);
        const int a = m[0], b = m[1];
        if (a >= 0 && b >= 0) {
            if (a >= P.n_i || b >= P.n_j) {
                atomicOr(&pair_status[p], SFD2_TRI_ST_RANGE);
            } else {
                const double2 xi = xn[P.kp_i + a], xj = xn[P.kp_j + b];
                const double l0 = P.E[0] * xi.x + P.E[1] * xi.y + P.E[2], l1 = P.E[3] * xi.x + P.E[4] * xi.y + P.E[5],
                             l2 = P.E[6] * xi.x + P.E[7] * xi.y + P.E[8];               // E x_i: the line in image j
                const double k0 = P.E[0] * xj.x + P.E[3] * xj.y + P.E[6], k1 = P.E[1] * xj.x + P.E[4] * xj.y + P.E[7],
                             k2 = P.E[2] * xj.x + P.E[5] * xj.y + P.E[8];               // E^T x_j: the line in image i
                const double dj = fabs(xj.x * l0 + xj.y * l1 + l2) / sqrt(l0 * l0 + l1 * l1);
                const double di = fabs(xi.x * k0 + xi.y * k1 + k2) / sqrt(k0 * k0 + k1 * k1);
                ok = di <= P.thr_i && dj <= P.thr_j;                                    // (a NaN distance rejects)
            }
        }
        if (!ok) { m[0] = -1; m[1] = -1; }
    }
    const unsigned long long bal = __ballot(ok);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kWG / 64; ++w) s += wcnt[w];
        blk_cnt[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kWG) void tri_pair_count_kernel(const TriPairDev *__restrict__ pairs, int n_pairs, const int32_t *__restrict__ blk_cnt,
                                                             int32_t *__restrict__ pair_cnt)
{
    const int p = blockIdx.x * kWG + threadIdx.x;
    if (p >= n_pairs) return;
    const int nb = (pairs[p].n + kWG - 1) / kWG;
    int s = 0;
    for (int b = 0; b < nb; ++b) s += blk_cnt[pairs[p].blk0 + b];
    pair_cnt[p] = s;
}

__global__ __launch_bounds__(kWG) void tri_verify_drop_kernel(const TriPairDev *__restrict__ pairs, const int32_t *__restrict__ blk_pair,
                                                              const int32_t *__restrict__ pair_cnt, int min_inliers, int32_t *__restrict__ matches)
{
    const int p = blk_pair[blockIdx.x];
    if (pair_cnt[p] >= min_inliers) return;
    const TriPairDev &P = pairs[p];
    const int idx = ((int)blockIdx.x - P.blk0) * kWG + (int)threadIdx.x;
    if (idx >= P.n) return;
    matches[2 * (P.moff + idx)] = -1;
    matches[2 * (P.moff + idx) + 1] = -1;
}

// ---------------------------------------------------------------------------------------------------------------- tracks
__global__ __launch_bounds__(kWG) void tri_iota_kernel(int32_t *__restrict__ p, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (i < n) p[i] = (int32_t)i;
}

__global__ __launch_bounds__(kWG) void tri_cc_hook_kernel(const int32_t *__restrict__ edges, int64_t n_edges, int32_t *parent, int64_t n,
                                                          int32_t *words)
{
    const int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (e >= n_edges) return;
    const int u = edges[2 * e], v = edges[2 * e + 1];
    if (u < 0 || v < 0) return;                               // a rejected match
    if (u >= n || v >= n) { atomicOr(&words[1], SFD2_TRI_ST_RANGE); return; }
    const int pu = parent[u], pv = parent[v];
    if (pu == pv) return;
    const int hi = max(pu, pv), lo = min(pu, pv);
    if (atomicMin(&parent[hi], lo) > lo) words[0] = 1;
}

__global__ __launch_bounds__(kWG) void tri_cc_jump_kernel(int32_t *parent, int64_t n, int32_t *words)
{
    const int64_t v = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (v >= n) return;
    int p = parent[v];
    bool moved = false;
    for (int s = 0; s < kJumpSteps; ++s) {
        const int pp = parent[p];
        if (pp == p) break;
        p = pp;
        moved = true;
    }
    if (moved) { parent[v] = p; words[0] = 1; }
}

__global__ __launch_bounds__(kWG) void tri_cc_flags_kernel(const int32_t *__restrict__ sl, int64_t n, int32_t *__restrict__ keep, int32_t *__restrict__ head)
{
    const int64_t k = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (k >= n) return;
    const int l = sl[k];
    const bool first = k == 0 || sl[k - 1] != l;
    const bool kp = !first || (k + 1 < n && sl[k + 1] == l);  // a component of two or more nodes
    keep[k] = kp ? 1 : 0;
    head[k] = kp && first ? 1 : 0;
}

__global__ __launch_bounds__(kWG) void tri_cc_scatter_kernel(const int32_t *__restrict__ sn, int64_t n, const int32_t *__restrict__ keep,
                                                             const int32_t *__restrict__ head, const int32_t *__restrict__ pos,
                                                             const int32_t *__restrict__ tid, int32_t *__restrict__ track_offsets,
                                                             int32_t *__restrict__ track_nodes, int32_t *__restrict__ totals)
{
    const int64_t k = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (k >= n) return;
    if (keep[k]) track_nodes[pos[k]] = sn[k];
    if (head[k]) track_offsets[tid[k]] = pos[k];
    if (k == n - 1) {
        const int nt = tid[k] + head[k], nn = pos[k] + keep[k];
        track_offsets[nt] = nn;
        totals[0] = nt;
        totals[1] = nn;
    }
}

// ---------------------------------------------------------------------------------------------------------------- triangulation
__global__ __launch_bounds__(kWG) void tri_obs_prep_kernel(const TriViewDev *__restrict__ views, const int32_t *__restrict__ obs_view,
                                                           const float *__restrict__ xy, int64_t n, double2 *__restrict__ px, double2 *__restrict__ xn)
{
    const int64_t o = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (o >= n) return;
    const double x = (double)xy[2 * o] + 0.5, y = (double)xy[2 * o + 1] + 0.5;
    double u, v;
    img_to_norm(views[obs_view[o]].cam, x, y, u, v);
    px[o] = make_double2(x, y);
    xn[o] = make_double2(u, v);
}

struct TriTrack {
    const TriViewDev *views;
    const int32_t *view;              // per observation
    const double2 *px, *xn;
    signed char *point;               // -1 free, else the pass that took the observation
    unsigned char *tmp;
    int64_t lo, hi;
};

__device__ __forceinline__ void to_cam(const TriViewDev &V, const double X[3], double Pc[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) Pc[a] = V.R[3 * a] * X[0] + V.R[3 * a + 1] * X[1] + V.R[3 * a + 2] * X[2] + V.t[a];
}

// tan of the angle between the ray to X and the observation's ray; false behind the camera
__device__ __forceinline__ bool err_angle(const TriTrack &T, int64_t o, const double X[3], double &e)
{
    double Pc[3];
    to_cam(T.views[T.view[o]], X, Pc);
    const double2 b = T.xn[o];
    const double c0 = Pc[1] - Pc[2] * b.y, c1 = Pc[2] * b.x - Pc[0], c2 = Pc[0] * b.y - Pc[1] * b.x;
    const double dot = Pc[0] * b.x + Pc[1] * b.y + Pc[2];
    e = sqrt(c0 * c0 + c1 * c1 + c2 * c2) / dot;
    return Pc[2] > 0 && dot > 0;
}

// reprojection error in pixels; false behind the camera
__device__ __forceinline__ bool err_pixel(const TriTrack &T, int64_t o, const double X[3], double &e)
{
    double Pc[3], x, y;
    const TriViewDev &V = T.views[T.view[o]];
    to_cam(V, X, Pc);
    project_px(V.cam, Pc, x, y);
    const double2 p = T.px[o];
    const double dx = x - p.x, dy = y - p.y;
    e = sqrt(dx * dx + dy * dy);
    return Pc[2] > 0;
}

template <bool kPixel>
__device__ __forceinline__ bool obs_ok(const TriTrack &T, int64_t o, const double X[3], double thr, double &e)
{
    const bool front = kPixel ? err_pixel(T, o, X, e) : err_angle(T, o, X, e);
    return front && e <= thr;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v = fmin(v, __shfl_xor(v, m));
    return v;
}

// free observations within thr of X join point p: at most one per image, none for an image p already holds; the smallest error wins,
// ties go to the smaller index.  Decisions are taken on the state before the call (tmp), then written.  Returns how many joined.
template <bool kPixel>
__device__ int tri_select(const TriTrack &T, int p, const double X[3], double thr)
{
    const int lane = threadIdx.x;
    for (int64_t o = T.lo + lane; o < T.hi; o += kWave) {
        bool win = false;
        double e;
        if (T.point[o] == -1 && obs_ok<kPixel>(T, o, X, thr, e)) {
            const int im = T.view[o];
            win = true;
            for (int64_t q = o - 1; q >= T.lo && win && T.view[q] == im; --q) {
                double eq;
                const int s = T.point[q];
                if (s == p || (s == -1 && obs_ok<kPixel>(T, q, X, thr, eq) && eq <= e)) win = false;
            }
            for (int64_t q = o + 1; q < T.hi && win && T.view[q] == im; ++q) {
                double eq;
                const int s = T.point[q];
                if (s == p || (s == -1 && obs_ok<kPixel>(T, q, X, thr, eq) && eq < e)) win = false;
            }
        }
        T.tmp[o] = win ? 1 : 0;
    }
    __syncthreads();
    int joined = 0;
    for (int64_t o = T.lo + lane; o < T.hi; o += kWave)
        if (T.tmp[o]) { T.point[o] = (signed char)p; ++joined; }
    __syncthreads();
    return wave_sum(joined);
}

// normal equations of the squared reprojection error over the observations of point p at X: s = H (xx xy xz yy yz zz), g (3), cost;
// a member behind the camera makes the cost infinite
__device__ void tri_normal(const TriTrack &T, int p, const double X[3], double s[10])
{
#pragma unroll
    for (int k = 0; k < 10; ++k) s[k] = 0.0;
    for (int64_t o = T.lo + threadIdx.x; o < T.hi; o += kWave) {
        if (T.point[o] != p) continue;
        const TriViewDev &V = T.views[T.view[o]];
        double Pc[3];
        to_cam(V, X, Pc);
        const double iz = 1.0 / Pc[2], u = Pc[0] * iz, v = Pc[1] * iz;
        double ud, vd, D[4];
        distort(V.cam, u, v, ud, vd, D);
        const double2 px = T.px[o];
        const double r0 = V.cam.f[0] * ud + V.cam.c[0] - px.x, r1 = V.cam.f[1] * vd + V.cam.c[1] - px.y;
        // d pixel / d Pc = diag(f) D [[1/z, 0, -u/z], [0, 1/z, -v/z]], then d Pc / d X = R
        const double a00 = V.cam.f[0] * D[0] * iz, a01 = V.cam.f[0] * D[1] * iz, a02 = -(a00 * u + a01 * v);
        const double a10 = V.cam.f[1] * D[2] * iz, a11 = V.cam.f[1] * D[3] * iz, a12 = -(a10 * u + a11 * v);
        double j0[3], j1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            j0[c] = a00 * V.R[c] + a01 * V.R[3 + c] + a02 * V.R[6 + c];
            j1[c] = a10 * V.R[c] + a11 * V.R[3 + c] + a12 * V.R[6 + c];
        }
        s[0] += j0[0] * j0[0] + j1[0] * j1[0];
        s[1] += j0[0] * j0[1] + j1[0] * j1[1];
        s[2] += j0[0] * j0[2] + j1[0] * j1[2];
        s[3] += j0[1] * j0[1] + j1[1] * j1[1];
        s[4] += j0[1] * j0[2] + j1[1] * j1[2];
        s[5] += j0[2] * j0[2] + j1[2] * j1[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) s[6 + c] += j0[c] * r0 + j1[c] * r1;
        s[9] += Pc[2] > 0 ? r0 * r0 + r1 * r1 : (double)INFINITY;
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) s[k] = wave_sum(s[k]);
}

// Levenberg-Marquardt on X over the observations of point p; false when it leaves the finite numbers
__device__ bool tri_refine(const TriTrack &T, int p, double X[3], int iters)
{
    double s[10], lambda = 1e-3;
    tri_normal(T, p, X, s);
    if (!tri_finite(s[9])) return false;
    for (int it = 0; it < iters; ++it) {
        const double h0 = s[0] * (1.0 + lambda), h3 = s[3] * (1.0 + lambda), h5 = s[5] * (1.0 + lambda);
        const double c00 = h3 * h5 - s[4] * s[4], c01 = s[2] * s[4] - s[1] * h5, c02 = s[1] * s[4] - s[2] * h3;
        const double det = h0 * c00 + s[1] * c01 + s[2] * c02;
        bool stepped = false;
        if (tri_finite(det) && fabs(det) > 0) {
            const double c11 = h0 * h5 - s[2] * s[2], c12 = s[1] * s[2] - h0 * s[4], c22 = h0 * h3 - s[1] * s[1];
            const double d[3] = {-(c00 * s[6] + c01 * s[7] + c02 * s[8]) / det, -(c01 * s[6] + c11 * s[7] + c12 * s[8]) / det,
                                 -(c02 * s[6] + c12 * s[7] + c22 * s[8]) / det};
            const double Xn[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
            double sn[10];
            tri_normal(T, p, Xn, sn);
            if (tri_finite(sn[9]) && sn[9] <= s[9]) {
                const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], xx = Xn[0] * Xn[0] + Xn[1] * Xn[1] + Xn[2] * Xn[2];
#pragma unroll
                for (int k = 0; k < 3; ++k) X[k] = Xn[k];
#pragma unroll
                for (int k = 0; k < 10; ++k) s[k] = sn[k];
                lambda = fmax(lambda * 0.1, 1e-15);
                stepped = true;
                if (dd <= 1e-28 * xx) break;
            }
        }
        if (!stepped) {
            lambda *= 10.0;
            if (lambda > 1e15) break;
        }
    }
    return tri_finite(X[0]) && tri_finite(X[1]) && tri_finite(X[2]);
}

__global__ __launch_bounds__(kWave) void tri_track_kernel(const TriViewDev *__restrict__ views, const TriConfDev conf,
                                                          const int64_t *__restrict__ offsets, const int64_t *__restrict__ labels,
                                                          const int32_t *__restrict__ order, const int32_t *__restrict__ obs_view,
                                                          const double2 *__restrict__ px, const double2 *__restrict__ xn, signed char *obs_point,
                                                          unsigned char *obs_tmp, double *__restrict__ xyz, double *__restrict__ err,
                                                          int32_t *__restrict__ n_obs, int32_t *__restrict__ status)
{
    const int t = order[blockIdx.x], lane = threadIdx.x;
    TriTrack T;
    T.views = views; T.view = obs_view; T.px = px; T.xn = xn; T.point = obs_point; T.tmp = obs_tmp;
    T.lo = offsets[t]; T.hi = offsets[t + 1];
    if (T.hi - T.lo < 2) {
        if (lane == 0) status[t] = SFD2_TRI_ST_SHORT;
        return;
    }
    const uint64_t key = tri_mix64(conf.seed ^ tri_mix64((uint64_t)labels[t]));
    int st = 0;
    for (int p = 0; p < SFD2_TRI_MAX_POINTS; ++p) {
        // ---- the free observations and this lane's pair of them
        int m = 0;
        for (int64_t o = T.lo; o < T.hi; ++o) m += T.point[o] == -1 ? 1 : 0;
        if (m < 2) break;
        const int64_t n_pairs = (int64_t)m * (m - 1) / 2;
        int a = -1, b = -1;
        if (n_pairs <= kWave) {
            if (lane < n_pairs) {
                int rem = lane;
                a = 0;
                for (int s = 0; s < kWave && rem >= m - 1 - a; ++s) { rem -= m - 1 - a; ++a; }
                b = a + 1 + rem;
            }
        } else {
            const uint64_t h0 = tri_mix64(key ^ tri_mix64((uint64_t)(kWave * p + lane))), h1 = tri_mix64(h0);
            const int i0 = (int)(h0 % (uint64_t)m);
            int i1 = (int)(h1 % (uint64_t)(m - 1));
            if (i1 >= i0) ++i1;
            a = min(i0, i1);
            b = max(i0, i1);
        }
        int64_t oa = -1, ob = -1;
        {
            int c = 0;
            for (int64_t o = T.lo; o < T.hi; ++o) {
                if (T.point[o] != -1) continue;
                if (c == a) oa = o;
                if (c == b) ob = o;
                ++c;
            }
        }
        // ---- midpoint of the two rays
        double X[3] = {0, 0, 0};
        bool valid = oa >= 0 && ob >= 0 && T.view[oa] != T.view[ob];
        if (valid) {
            const TriViewDev &A = views[T.view[oa]], &B = views[T.view[ob]];
            const double2 xa = xn[oa], xb = xn[ob];
            double da[3], db[3], w[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                da[c] = A.R[c] * xa.x + A.R[3 + c] * xa.y + A.R[6 + c];      // R^T (u, v, 1)
                db[c] = B.R[c] * xb.x + B.R[3 + c] * xb.y + B.R[6 + c];
                w[c] = A.C[c] - B.C[c];
            }
            const double aa = da[0] * da[0] + da[1] * da[1] + da[2] * da[2], ab = da[0] * db[0] + da[1] * db[1] + da[2] * db[2],
                         bb = db[0] * db[0] + db[1] * db[1] + db[2] * db[2], aw = da[0] * w[0] + da[1] * w[1] + da[2] * w[2],
                         bw = db[0] * w[0] + db[1] * w[1] + db[2] * w[2];
            const double den = aa * bb - ab * ab;
            const double sa = (ab * bw - bb * aw) / den, sb = (aa * bw - ab * aw) / den;
            double va[3], vb[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                X[c] = 0.5 * ((A.C[c] + sa * da[c]) + (B.C[c] + sb * db[c]));
                va[c] = A.C[c] - X[c];
                vb[c] = B.C[c] - X[c];
            }
            double Pa[3], Pb[3];
            to_cam(A, X, Pa);
            to_cam(B, X, Pb);
            const double cs = (va[0] * vb[0] + va[1] * vb[1] + va[2] * vb[2]) /
                              sqrt((va[0] * va[0] + va[1] * va[1] + va[2] * va[2]) * (vb[0] * vb[0] + vb[1] * vb[1] + vb[2] * vb[2]));
            valid = den > 0 && tri_finite(X[0]) && tri_finite(X[1]) && tri_finite(X[2]) && Pa[2] > 0 && Pb[2] > 0 &&
                    fabs(cs) <= conf.cos_min_angle;                          // min(angle, pi - angle) >= min_tri_angle
        }
        // ---- support of this lane's hypothesis over the free observations (observations of an image are consecutive)
        int cnt = -1;
        double sum = 0.0;
        if (valid) {
            cnt = 0;
            int cur = -1;
            bool have = false;
            double best = 0.0;
            for (int64_t o = T.lo; o < T.hi; ++o) {
                if (T.point[o] != -1) continue;
                const int im = T.view[o];
                if (im != cur) {
                    if (have) { ++cnt; sum += best; }
                    have = false;
                    cur = im;
                }
                double e;
                if (obs_ok<false>(T, o, X, conf.tan_create, e) && (!have || e < best)) { best = e; have = true; }
            }
            if (have) { ++cnt; sum += best; }
        }
        // ---- the best lane: more observations, smaller sum, smaller lane (a total order, so the butterfly's order is immaterial)
        int bc = cnt, bl = lane;
        double bs = sum;
#pragma unroll
        for (int msk = 1; msk < kWave; msk <<= 1) {
            const int oc = __shfl_xor(bc, msk), ol = __shfl_xor(bl, msk);
            const double os = __shfl_xor(bs, msk);
            if (oc > bc || (oc == bc && (os < bs || (os == bs && ol < bl)))) { bc = oc; bs = os; bl = ol; }
        }
        if (bc < 2) break;
#pragma unroll
        for (int c = 0; c < 3; ++c) X[c] = __shfl(X[c], bl);
        // ---- inliers, refinement, completion, filter
        tri_select<false>(T, p, X, conf.tan_create);
        bool fin = tri_refine(T, p, X, conf.lm_iters);
        if (fin && tri_select<true>(T, p, X, conf.max_reproj) > 0) fin = tri_refine(T, p, X, conf.lm_iters);
        int members = 0;
        double esum = 0.0;
        if (fin) {
            for (int64_t o = T.lo + lane; o < T.hi; o += kWave) {
                if (T.point[o] != p) continue;
                double e;
                if (obs_ok<true>(T, o, X, conf.max_reproj, e)) { ++members; esum += e; }
                else T.point[o] = -1;
            }
            __syncthreads();
            members = wave_sum(members);
            esum = wave_sum(esum);
        }
        // the largest triangulation angle over the pairs of views = the smallest |cos|
        double mc = 2.0;
        if (fin && members >= 2) {
            for (int64_t o = T.lo + lane; o < T.hi; o += kWave) {
                if (T.point[o] != p) continue;
                const TriViewDev &A = views[T.view[o]];
                const double va[3] = {A.C[0] - X[0], A.C[1] - X[1], A.C[2] - X[2]};
                const double na = va[0] * va[0] + va[1] * va[1] + va[2] * va[2];
                for (int64_t q = o + 1; q < T.hi; ++q) {
                    if (T.point[q] != p) continue;
                    const TriViewDev &B = views[T.view[q]];
                    const double vb[3] = {B.C[0] - X[0], B.C[1] - X[1], B.C[2] - X[2]};
                    const double cs = (va[0] * vb[0] + va[1] * vb[1] + va[2] * vb[2]) / sqrt(na * (vb[0] * vb[0] + vb[1] * vb[1] + vb[2] * vb[2]));
                    mc = fmin(mc, fabs(cs));                                 // (fmin drops a NaN)
                }
            }
            mc = wave_min(mc);
        }
        if (!fin) st |= SFD2_TRI_ST_NONFINITE;
        if (!fin || members < 2 || !(mc <= conf.cos_min_angle)) {           // the point is dropped: its observations are free again
            for (int64_t o = T.lo + lane; o < T.hi; o += kWave)
                if (T.point[o] == p) T.point[o] = -1;
            break;
        }
        if (lane == 0) {
            const int64_t r = (int64_t)t * SFD2_TRI_MAX_POINTS + p;
            xyz[3 * r] = X[0]; xyz[3 * r + 1] = X[1]; xyz[3 * r + 2] = X[2];
            err[r] = esum / members;
            n_obs[r] = members;
        }
        __syncthreads();
    }
    if (lane == 0) status[t] = st;
}

template <typename... A>
void flat(void (*k)(A...), hipStream_t st, int64_t n, A... args)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k, dim3((unsigned)((n + kWG - 1) / kWG)), dim3(kWG), 0, st, args...);
}

}  // namespace

void launch_tri_normalise(hipStream_t st, const TriViewDev *views, int n_views, const int64_t *offsets, const float *kp, int64_t n, double2 *xn)
{
    flat(tri_normalise_kernel, st, n, views, n_views, offsets, kp, n, xn);
}

void launch_tri_verify(hipStream_t st, const TriPairDev *pairs, int n_pairs, const int32_t *blk_pair, int n_blocks, const double2 *xn,
                       int32_t *matches, int32_t *blk_cnt, int32_t *pair_cnt, int32_t *pair_status, int min_inliers)
{
    if (n_blocks > 0) hipLaunchKernelGGL(tri_verify_kernel, dim3((unsigned)n_blocks), dim3(kWG), 0, st, pairs, blk_pair, xn, matches, blk_cnt, pair_status);
    flat(tri_pair_count_kernel, st, (int64_t)n_pairs, pairs, n_pairs, (const int32_t *)blk_cnt, pair_cnt);
    if (n_blocks > 0)
        hipLaunchKernelGGL(tri_verify_drop_kernel, dim3((unsigned)n_blocks), dim3(kWG), 0, st, pairs, blk_pair, (const int32_t *)pair_cnt, min_inliers, matches);
}

void launch_tri_iota(hipStream_t st, int32_t *p, int64_t n) { flat(tri_iota_kernel, st, n, p, n); }

void launch_tri_cc_round(hipStream_t st, const int32_t *edges, int64_t n_edges, int32_t *parent, int64_t n, int32_t *words)
{
    flat(tri_cc_hook_kernel, st, n_edges, edges, n_edges, parent, n, words);
    flat(tri_cc_jump_kernel, st, n, parent, n, words);
}

void launch_tri_cc_flags(hipStream_t st, const int32_t *sorted_labels, int64_t n, int32_t *keep, int32_t *head)
{
    flat(tri_cc_flags_kernel, st, n, sorted_labels, n, keep, head);
}

void launch_tri_cc_scatter(hipStream_t st, const int32_t *sorted_labels, const int32_t *sorted_nodes, int64_t n, const int32_t *keep,
                           const int32_t *head, const int32_t *pos, const int32_t *tid, int32_t *track_offsets, int32_t *track_nodes, int32_t *totals)
{
    (void)sorted_labels;
    flat(tri_cc_scatter_kernel, st, n, sorted_nodes, n, keep, head, pos, tid, track_offsets, track_nodes, totals);
}

void launch_tri_obs_prep(hipStream_t st, const TriViewDev *views, const int32_t *obs_view, const float *obs_xy, int64_t n, double2 *px, double2 *xn)
{
    flat(tri_obs_prep_kernel, st, n, views, obs_view, obs_xy, n, px, xn);
}

void launch_tri_tracks(hipStream_t st, const TriViewDev *views, const TriConfDev &conf, const int64_t *offsets, const int64_t *labels,
                       const int32_t *order, int n_tracks, const int32_t *obs_view, const double2 *px, const double2 *xn, signed char *obs_point,
                       unsigned char *obs_tmp, double *xyz, double *err, int32_t *n_obs, int32_t *status)
{
    if (n_tracks <= 0) return;
    hipLaunchKernelGGL(tri_track_kernel, dim3((unsigned)n_tracks), dim3(kWave), 0, st, views, conf, offsets, labels, order, obs_view, px, xn,
                       obs_point, obs_tmp, xyz, err, n_obs, status);
}
