// libsfd2hip: sfd2_mapper_restrict / _filter / _visible / _assemble -- checks and packs the inputs, the launches of mapper_kernels.hip on the
// context's stream, results back.  The scans between a count and its scatter are rocPRIM's integer scans, as in
// api_triangulate.hip; the by-view order of sfd2_mapper_assemble is api_bundle.hip's stable counting sort.
#include "sfd2_ctx.h"
#include "api_scratch.h"
#include "pose_camera.h"
#include "mapper.h"
#include <rocprim/rocprim.hpp>

namespace {

template <typename T> int64_t first_nonfinite(const T *p, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return i;
    return n;
}

// the first i with o[i + 1] < o[i], n when there is none
int64_t first_decrease(const int64_t *o, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (o[i + 1] < o[i]) return i;
    return n;
}

bool mapping_flags_ok(int flags)
{
    const int both = SFD2_MAPPER_FLAG_TRACK_LANE | SFD2_MAPPER_FLAG_TRACK_WAVE;
    return !(flags & ~both) && flags != both;
}

// items by mapping: a lane each up to SFD2_MAP_LONG_TRACK observations, beyond that a wave each (the flags force either side)
void split_by_length(const int64_t *off, int n, int flags, std::vector<int32_t> &short_ids, std::vector<int32_t> &long_ids)
{
    for (int j = 0; j < n; ++j) {
        const int64_t len = off[j + 1] - off[j];
        const bool wave = (flags & SFD2_MAPPER_FLAG_TRACK_WAVE) || (!(flags & SFD2_MAPPER_FLAG_TRACK_LANE) && len > SFD2_MAP_LONG_TRACK);
        (wave ? long_ids : short_ids).push_back(j);
    }
}

// the checks the track table shares: offsets, the observation count, the view indices; why names the first offending index
bool check_tracks(const int64_t *off, int n_tracks, const int32_t *obs_view, int n_views, std::string &why)
{
    if (off[0] != 0) { why = "track_offsets must start at 0"; return false; }
    if (const int64_t t = first_decrease(off, n_tracks); t < n_tracks) { why = "track " + std::to_string(t) + ": track_offsets decrease"; return false; }
    const int64_t O = off[n_tracks];
    if (O > 0x7fffffffLL) { why = "more than 2^31 - 1 observations"; return false; }
    if (O > 0 && !obs_view) { why = "null observations"; return false; }
    if (const int64_t o = first_outside(obs_view, O, n_views); o < O) { why = "observation " + std::to_string(o) + ": view index out of range"; return false; }
    return true;
}

// point_track: ascending, inside the track table, at most SFD2_TRI_MAX_POINTS points per track
bool check_points(const int32_t *point_track, int n_points, int n_tracks, std::string &why)
{
    int run = 0;
    for (int p = 0; p < n_points; ++p) {
        if (point_track[p] < 0 || point_track[p] >= n_tracks) { why = "point " + std::to_string(p) + ": track index out of range"; return false; }
        if (p > 0 && point_track[p] < point_track[p - 1]) { why = "point " + std::to_string(p) + ": point_track must be ascending"; return false; }
        run = (p > 0 && point_track[p] == point_track[p - 1]) ? run + 1 : 1;
        if (run > SFD2_TRI_MAX_POINTS) { why = "point " + std::to_string(p) + ": more than SFD2_TRI_MAX_POINTS points of one track"; return false; }
    }
    return true;
}

}  // namespace

extern "C" int sfd2_mapper_restrict(sfd2_ctx *c, const int64_t *track_offsets, int n_tracks, const int32_t *obs_view, const float *obs_xy,
                                    const uint8_t *registered, int n_views, int32_t *sub_track, int64_t *sub_offsets, int32_t *sub_obs, int32_t *sub_view,
                                    float *sub_xy, int64_t *n_sub_tracks, int64_t *n_sub_obs, int flags)
{
    const std::string F("sfd2_mapper_restrict: ");
    if (!c || !track_offsets || !registered || !sub_offsets || !n_sub_tracks || !n_sub_obs || (n_tracks > 0 && !sub_track)) return fail(F + "null argument");
    if (n_views < 1 || n_tracks < 0) return fail(F + "n_views must be positive and n_tracks non-negative");
    if (!mapping_flags_ok(flags)) return fail(F + "unknown flags (at most one of SFD2_MAPPER_FLAG_TRACK_LANE, SFD2_MAPPER_FLAG_TRACK_WAVE)");
    std::string why;
    if (!check_tracks(track_offsets, n_tracks, obs_view, n_views, why)) return fail(F + why);
    const int64_t O = track_offsets[n_tracks];
    if (O > 0 && (!obs_xy || !sub_obs || !sub_view || !sub_xy)) return fail(F + "null observations");
    *n_sub_tracks = *n_sub_obs = 0;
    sub_offsets[0] = 0;
    if (n_tracks == 0) return 0;
    std::vector<int32_t> short_ids, long_ids;
    split_by_length(track_offsets, n_tracks, flags, short_ids, long_ids);

    HIPCHECK(hipSetDevice(c->device));
    const size_t T = (size_t)n_tracks, no = (size_t)O, nv = (size_t)n_views;
    size_t tmp_scan = 0;
    {
        int32_t *nil = nullptr;
        HIPCHECK(rocprim::exclusive_scan(nullptr, tmp_scan, nil, nil, 0, T, rocprim::plus<int32_t>(), c->stream));
    }
    Carve in, ws;
    const size_t o_off = in.take(8 * (T + 1)), o_ov = in.take(4 * no), o_xy = in.take(8 * no), o_reg = in.take(nv), o_sh = in.take(4 * short_ids.size()),
                 o_lg = in.take(4 * long_ids.size());
    const size_t o_keep = ws.take(4 * T), o_cnt = ws.take(4 * T), o_tpos = ws.take(4 * T), o_opos = ws.take(4 * T), o_tot = ws.take(16),
                 o_st = ws.take(4 * T), o_so = ws.take(8 * (T + 1)), o_sb = ws.take(4 * no), o_sv = ws.take(4 * no), o_sx = ws.take(8 * no),
                 o_tmp = ws.take(tmp_scan);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->map_in, in.off));
    HIPCHECK(grow(c->map_ws, ws.off));
    char *di = c->map_in.as<char>(), *dw = c->map_ws.as<char>();
    hipStream_t s = c->stream;
    HIPCHECK(hipMemcpyAsync(di + o_off, track_offsets, 8 * (T + 1), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_reg, registered, nv, hipMemcpyHostToDevice, s));
    if (no) {
        HIPCHECK(hipMemcpyAsync(di + o_ov, obs_view, 4 * no, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(di + o_xy, obs_xy, 8 * no, hipMemcpyHostToDevice, s));
    }
    if (!short_ids.empty()) HIPCHECK(hipMemcpyAsync(di + o_sh, short_ids.data(), 4 * short_ids.size(), hipMemcpyHostToDevice, s));
    if (!long_ids.empty()) HIPCHECK(hipMemcpyAsync(di + o_lg, long_ids.data(), 4 * long_ids.size(), hipMemcpyHostToDevice, s));
    const int32_t *sh = at<const int32_t>(di, o_sh), *lg = at<const int32_t>(di, o_lg);
    int32_t *keep = at<int32_t>(dw, o_keep), *cnt = at<int32_t>(dw, o_cnt), *tpos = at<int32_t>(dw, o_tpos), *opos = at<int32_t>(dw, o_opos);
    {
        ProfScope ps(c, "mapper_restrict", "mapper_restrict_count+scan+scatter", 0.0, 24.0 * (double)no);
        launch_mapper_restrict_count(s, sh, (int)short_ids.size(), lg, (int)long_ids.size(), at<const int64_t>(di, o_off), at<const int32_t>(di, o_ov),
                                     at<const unsigned char>(di, o_reg), keep, cnt);
        size_t tb = tmp_scan;
        HIPCHECK(rocprim::exclusive_scan(dw + o_tmp, tb, keep, tpos, 0, T, rocprim::plus<int32_t>(), s));
        tb = tmp_scan;
        HIPCHECK(rocprim::exclusive_scan(dw + o_tmp, tb, cnt, opos, 0, T, rocprim::plus<int32_t>(), s));
        launch_mapper_restrict_scatter(s, sh, (int)short_ids.size(), lg, (int)long_ids.size(), n_tracks, at<const int64_t>(di, o_off),
                                       at<const int32_t>(di, o_ov), at<const float2>(di, o_xy), at<const unsigned char>(di, o_reg), keep, cnt, tpos, opos,
                                       at<int32_t>(dw, o_st), at<int64_t>(dw, o_so), at<int32_t>(dw, o_sb), at<int32_t>(dw, o_sv), at<float2>(dw, o_sx),
                                       at<int64_t>(dw, o_tot));
    }
    HIPCHECK(hipGetLastError());
    int64_t tot[2] = {0, 0};
    HIPCHECK(hipMemcpyAsync(tot, dw + o_tot, 16, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (tot[0] < 0 || tot[0] > n_tracks || tot[1] < 0 || tot[1] > O) return fail(F + "internal: the compaction's totals are out of range");
    HIPCHECK(hipMemcpyAsync(sub_offsets, dw + o_so, 8 * ((size_t)tot[0] + 1), hipMemcpyDeviceToHost, s));
    if (tot[0]) HIPCHECK(hipMemcpyAsync(sub_track, dw + o_st, 4 * (size_t)tot[0], hipMemcpyDeviceToHost, s));
    if (tot[1]) {
        HIPCHECK(hipMemcpyAsync(sub_obs, dw + o_sb, 4 * (size_t)tot[1], hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(sub_view, dw + o_sv, 4 * (size_t)tot[1], hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(sub_xy, dw + o_sx, 8 * (size_t)tot[1], hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    *n_sub_tracks = tot[0];
    *n_sub_obs = tot[1];
    return 0;
}

extern "C" int sfd2_mapper_filter(sfd2_ctx *c, const sfd2_tri_view *views, int n_views, const double *xyz, int n_points, const int64_t *point_offsets,
                                  const int32_t *obs_view, const double *obs_xy, double max_reproj_error, double min_tri_angle_deg, uint8_t *obs_keep,
                                  uint8_t *point_live, double *point_error, double *point_angle, int flags)
{
    const std::string F("sfd2_mapper_filter: ");
    if (!c || !views || !point_offsets || (n_points > 0 && (!xyz || !point_live || !point_error || !point_angle))) return fail(F + "null argument");
    if (n_views < 1 || n_points < 0) return fail(F + "n_views must be positive and n_points non-negative");
    if (!mapping_flags_ok(flags)) return fail(F + "unknown flags (at most one of SFD2_MAPPER_FLAG_TRACK_LANE, SFD2_MAPPER_FLAG_TRACK_WAVE)");
    if (!(std::isfinite(max_reproj_error) && max_reproj_error > 0) || !(min_tri_angle_deg >= 0 && min_tri_angle_deg < 180))
        return fail(F + "max_reproj_error must be positive and finite, min_tri_angle_deg lie in [0, 180)");
    if (point_offsets[0] != 0) return fail(F + "point_offsets must start at 0");
    if (const int64_t p = first_decrease(point_offsets, n_points); p < n_points) return fail(F + "point " + std::to_string(p) + ": point_offsets decrease");
    const int64_t O = point_offsets[n_points];
    if (O > 0x7fffffffLL) return fail(F + "more than 2^31 - 1 observations");
    if (O > 0 && (!obs_view || !obs_xy || !obs_keep)) return fail(F + "null observations");
    if (const int64_t o = first_outside(obs_view, O, n_views); o < O) return fail(F + "observation " + std::to_string(o) + ": view index out of range");
    if (!all_finite(obs_xy, 2 * O)) return fail(F + "observation " + std::to_string(first_nonfinite(obs_xy, 2 * O) / 2) + ": non-finite coordinates");
    if (!all_finite(xyz, 3 * (int64_t)n_points)) return fail(F + "point " + std::to_string(first_nonfinite(xyz, 3 * (int64_t)n_points) / 3) + ": non-finite coordinates");
    if (n_points == 0) return 0;

    const size_t nv = (size_t)n_views, np = (size_t)n_points, no = (size_t)O;
    std::vector<TriViewDev> vd(nv);
    for (int i = 0; i < n_views; ++i) {                      // x_cam = R X + t, C = -R^T t
        TriViewDev &d = vd[(size_t)i];
        memset(&d, 0, sizeof(d));
        std::string w;
        if (!sfd2_pose_cam(views[i].model, views[i].params, d.cam, w)) return fail(F + "view " + std::to_string(i) + ": " + w);
        const double *q = views[i].qvec;
        const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (!all_finite(q, 4) || !all_finite(views[i].tvec, 3) || !(nq > 0))
            return fail(F + "view " + std::to_string(i) + ": the pose must be finite with a non-zero quaternion");
        quat_to_rot(q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq, d.R);
        for (int a = 0; a < 3; ++a) d.t[a] = views[i].tvec[a];
        for (int a = 0; a < 3; ++a) d.C[a] = -(d.R[a] * d.t[0] + d.R[3 + a] * d.t[1] + d.R[6 + a] * d.t[2]);
    }
    std::vector<int32_t> short_ids, long_ids, obs_pt(std::max<size_t>(no, 1));
    split_by_length(point_offsets, n_points, flags, short_ids, long_ids);
    for (int j = 0; j < n_points; ++j)
        for (int64_t o = point_offsets[j]; o < point_offsets[j + 1]; ++o) obs_pt[(size_t)o] = j;

    HIPCHECK(hipSetDevice(c->device));
    Carve in, ws;
    const size_t o_v = in.take(sizeof(TriViewDev) * nv), o_xyz = in.take(24 * np), o_off = in.take(8 * (np + 1)), o_ov = in.take(4 * no),
                 o_op = in.take(4 * no), o_xy = in.take(16 * no), o_sh = in.take(4 * short_ids.size()), o_lg = in.take(4 * long_ids.size());
    const size_t o_err = ws.take(8 * no), o_keep = ws.take(no), o_ray = ws.take(24 * no), o_live = ws.take(np), o_pe = ws.take(8 * np), o_pa = ws.take(8 * np);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->map_in, in.off));
    HIPCHECK(grow(c->map_ws, ws.off));
    char *di = c->map_in.as<char>(), *dw = c->map_ws.as<char>();
    hipStream_t s = c->stream;
    HIPCHECK(hipMemcpyAsync(di + o_v, vd.data(), sizeof(TriViewDev) * nv, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_xyz, xyz, 24 * np, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_off, point_offsets, 8 * (np + 1), hipMemcpyHostToDevice, s));
    if (no) {
        HIPCHECK(hipMemcpyAsync(di + o_ov, obs_view, 4 * no, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(di + o_op, obs_pt.data(), 4 * no, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(di + o_xy, obs_xy, 16 * no, hipMemcpyHostToDevice, s));
    }
    if (!short_ids.empty()) HIPCHECK(hipMemcpyAsync(di + o_sh, short_ids.data(), 4 * short_ids.size(), hipMemcpyHostToDevice, s));
    if (!long_ids.empty()) HIPCHECK(hipMemcpyAsync(di + o_lg, long_ids.data(), 4 * long_ids.size(), hipMemcpyHostToDevice, s));
    {
        ProfScope ps(c, "mapper_filter", "mapper_filter_obs+point", 0.0, 80.0 * (double)no);
        launch_mapper_filter_obs(s, at<const TriViewDev>(di, o_v), at<const double>(di, o_xyz), at<const int32_t>(di, o_ov), at<const int32_t>(di, o_op),
                                 at<const double2>(di, o_xy), O, max_reproj_error, at<double>(dw, o_err), at<unsigned char>(dw, o_keep), at<double>(dw, o_ray));
        launch_mapper_filter_points(s, at<const int32_t>(di, o_sh), (int)short_ids.size(), at<const int32_t>(di, o_lg), (int)long_ids.size(),
                                    at<const int64_t>(di, o_off), at<const int32_t>(di, o_ov), at<const double>(dw, o_err), at<const unsigned char>(dw, o_keep),
                                    at<const double>(dw, o_ray), min_tri_angle_deg, at<unsigned char>(dw, o_live), at<double>(dw, o_pe), at<double>(dw, o_pa));
    }
    HIPCHECK(hipGetLastError());
    if (no) HIPCHECK(hipMemcpyAsync(obs_keep, dw + o_keep, no, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(point_live, dw + o_live, np, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(point_error, dw + o_pe, 8 * np, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(point_angle, dw + o_pa, 8 * np, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int sfd2_mapper_visible(sfd2_ctx *c, const int64_t *track_offsets, int n_tracks, const int32_t *obs_view, const uint8_t *registered, int n_views,
                                   const int32_t *point_track, const uint8_t *point_live, int n_points, int64_t *counts, int flags)
{
    const std::string F("sfd2_mapper_visible: ");
    if (!c || !track_offsets || !registered || !counts || (n_points > 0 && (!point_track || !point_live))) return fail(F + "null argument");
    if (n_views < 1 || n_tracks < 0 || n_points < 0) return fail(F + "n_views must be positive, n_tracks and n_points non-negative");
    if (flags != 0) return fail(F + "unknown flags");
    std::string why;
    if (!check_tracks(track_offsets, n_tracks, obs_view, n_views, why)) return fail(F + why);
    if (!check_points(point_track, n_points, n_tracks, why)) return fail(F + why);
    const int64_t O = track_offsets[n_tracks];
    for (int v = 0; v < n_views; ++v) counts[v] = 0;
    if (O == 0 || n_points == 0) return 0;

    HIPCHECK(hipSetDevice(c->device));
    const size_t T = (size_t)n_tracks, no = (size_t)O, nv = (size_t)n_views, np = (size_t)n_points;
    Carve in, ws;
    const size_t o_off = in.take(8 * (T + 1)), o_ov = in.take(4 * no), o_reg = in.take(nv), o_pt = in.take(4 * np), o_pl = in.take(np);
    const size_t o_tl = ws.take(4 * T), o_cnt = ws.take(8 * nv);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->map_in, in.off));
    HIPCHECK(grow(c->map_ws, ws.off));
    char *di = c->map_in.as<char>(), *dw = c->map_ws.as<char>();
    hipStream_t s = c->stream;
    HIPCHECK(hipMemcpyAsync(di + o_off, track_offsets, 8 * (T + 1), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_ov, obs_view, 4 * no, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_reg, registered, nv, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_pt, point_track, 4 * np, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_pl, point_live, np, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(dw + o_tl, 0, ws.off - o_tl, s));                   // the tracks' live counts and the views' counters
    {
        ProfScope ps(c, "mapper_visible", "mapper_track_points+visible", 0.0, 4.0 * (double)no);
        launch_mapper_track_points(s, at<const int32_t>(di, o_pt), at<const unsigned char>(di, o_pl), n_points, at<int32_t>(dw, o_tl), nullptr);
        launch_mapper_visible(s, at<const int64_t>(di, o_off), n_tracks, at<const int32_t>(di, o_ov), O, at<const unsigned char>(di, o_reg),
                              at<const int32_t>(dw, o_tl), at<unsigned long long>(dw, o_cnt));
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(counts, dw + o_cnt, 8 * nv, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int sfd2_mapper_assemble(sfd2_ctx *c, const int64_t *track_offsets, int n_tracks, const int32_t *obs_view, const float *obs_xy, int n_views,
                                    const int32_t *point_track, const uint8_t *point_live, const double *xyz, int n_points, const int32_t *cand, int k,
                                    int64_t capacity, int64_t *offsets, double *points2D, double *points3D, int32_t *src_obs, int32_t *src_point, int flags)
{
    const std::string F("sfd2_mapper_assemble: ");
    if (!c || !track_offsets || !offsets || (n_points > 0 && (!point_track || !point_live || !xyz)) || (k > 0 && !cand)) return fail(F + "null argument");
    if (n_views < 1 || n_tracks < 0 || n_points < 0 || k < 0 || capacity < 0) return fail(F + "n_views must be positive, the other lengths non-negative");
    if (flags != 0) return fail(F + "unknown flags");
    if (capacity > 0 && (!points2D || !points3D || !src_obs || !src_point)) return fail(F + "null outputs");
    std::string why;
    if (!check_tracks(track_offsets, n_tracks, obs_view, n_views, why)) return fail(F + why);
    if (!check_points(point_track, n_points, n_tracks, why)) return fail(F + why);
    if (const int64_t i = first_outside(cand, k, n_views); i < k) return fail(F + "candidate " + std::to_string(i) + ": view index out of range");
    const int64_t O = track_offsets[n_tracks];
    if (O > 0 && !obs_xy) return fail(F + "null observations");
    if (!all_finite(obs_xy, 2 * O)) return fail(F + "observation " + std::to_string(first_nonfinite(obs_xy, 2 * O) / 2) + ": non-finite coordinates");
    if (!all_finite(xyz, 3 * (int64_t)n_points)) return fail(F + "point " + std::to_string(first_nonfinite(xyz, 3 * (int64_t)n_points) / 3) + ": non-finite coordinates");
    for (int i = 0; i <= k; ++i) offsets[i] = 0;
    if (k == 0 || O == 0 || n_points == 0) return 0;

    const size_t T = (size_t)n_tracks, no = (size_t)O, nv = (size_t)n_views, np = (size_t)n_points, nk = (size_t)k, cap = (size_t)capacity;
    // the by-view CSR by a stable counting sort: a view's observations in ascending index
    std::vector<int64_t> view_off(nv + 1, 0);
    std::vector<int32_t> view_obs(no);
    for (size_t o = 0; o < no; ++o) ++view_off[(size_t)obs_view[o] + 1];
    for (size_t v = 0; v < nv; ++v) view_off[v + 1] += view_off[v];
    {
        std::vector<int64_t> fill(view_off.begin(), view_off.end() - 1);
        for (size_t o = 0; o < no; ++o) view_obs[(size_t)fill[(size_t)obs_view[o]]++] = (int32_t)o;
    }

    HIPCHECK(hipSetDevice(c->device));
    size_t tmp_scan = 0;
    {
        int64_t *nil = nullptr;
        HIPCHECK(rocprim::exclusive_scan(nullptr, tmp_scan, nil, nil, (int64_t)0, nk + 1, rocprim::plus<int64_t>(), c->stream));
    }
    Carve in, ws;
    const size_t o_off = in.take(8 * (T + 1)), o_xy = in.take(8 * no), o_vo = in.take(8 * (nv + 1)), o_vb = in.take(4 * no), o_pt = in.take(4 * np),
                 o_pl = in.take(np), o_xyz = in.take(24 * np), o_cd = in.take(4 * nk);
    const size_t o_tl = ws.take(4 * T), o_tot = ws.take(8 * (nk + 1)), o_tf = ws.take(4 * T), o_offs = ws.take(8 * (nk + 1)), o_tmp = ws.take(tmp_scan),
                 o_p2 = ws.take(16 * cap), o_p3 = ws.take(24 * cap), o_so = ws.take(4 * cap), o_sp = ws.take(4 * cap);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->map_in, in.off));
    HIPCHECK(grow(c->map_ws, ws.off));
    char *di = c->map_in.as<char>(), *dw = c->map_ws.as<char>();
    hipStream_t s = c->stream;
    HIPCHECK(hipMemcpyAsync(di + o_off, track_offsets, 8 * (T + 1), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_xy, obs_xy, 8 * no, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_vo, view_off.data(), 8 * (nv + 1), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_vb, view_obs.data(), 4 * no, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_pt, point_track, 4 * np, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_pl, point_live, np, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_xyz, xyz, 24 * np, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_cd, cand, 4 * nk, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(dw + o_tl, 0, o_tf - o_tl, s));                     // the tracks' live counts and the candidates' totals
    HIPCHECK(hipMemsetAsync(dw + o_tf, 0xff, 4 * T, s));                         // no point: -1
    const int64_t *d_off = at<const int64_t>(di, o_off), *d_vo = at<const int64_t>(di, o_vo);
    const int32_t *d_vb = at<const int32_t>(di, o_vb), *d_cd = at<const int32_t>(di, o_cd);
    {
        ProfScope ps(c, "mapper_assemble", "mapper_assemble_count+scan", 0.0, 0.0);
        launch_mapper_track_points(s, at<const int32_t>(di, o_pt), at<const unsigned char>(di, o_pl), n_points, at<int32_t>(dw, o_tl), at<int32_t>(dw, o_tf));
        launch_mapper_assemble_count(s, d_cd, k, d_vo, d_vb, d_off, n_tracks, at<const int32_t>(dw, o_tl), at<int64_t>(dw, o_tot));
        size_t tb = tmp_scan;
        HIPCHECK(rocprim::exclusive_scan(dw + o_tmp, tb, at<int64_t>(dw, o_tot), at<int64_t>(dw, o_offs), (int64_t)0, nk + 1, rocprim::plus<int64_t>(), s));
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(offsets, dw + o_offs, 8 * (nk + 1), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    const int64_t total = offsets[k];
    if (total > capacity) {                                  // nothing is written beyond the offsets, which say what is needed
        return fail(F + std::to_string(total) + " correspondences for a capacity of " + std::to_string(capacity));
    }
    if (total == 0) return 0;
    {
        ProfScope ps(c, "mapper_assemble", "mapper_assemble_scatter", 0.0, 48.0 * (double)total);
        launch_mapper_assemble_scatter(s, d_cd, k, d_vo, d_vb, d_off, n_tracks, at<const float2>(di, o_xy), at<const int32_t>(dw, o_tf),
                                       at<const int32_t>(di, o_pt), at<const unsigned char>(di, o_pl), n_points, at<const double>(di, o_xyz),
                                       at<const int64_t>(dw, o_offs), at<double2>(dw, o_p2), at<double>(dw, o_p3), at<int32_t>(dw, o_so), at<int32_t>(dw, o_sp));
    }
    HIPCHECK(hipGetLastError());
    const size_t nt = (size_t)total;
    HIPCHECK(hipMemcpyAsync(points2D, dw + o_p2, 16 * nt, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(points3D, dw + o_p3, 24 * nt, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(src_obs, dw + o_so, 4 * nt, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(src_point, dw + o_sp, 4 * nt, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return 0;
}
