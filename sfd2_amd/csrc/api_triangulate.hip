// libsfd2hip: sfd2_verify_matches_batch / sfd2_build_tracks / sfd2_triangulate_tracks -- checks and packs the inputs, the launches of
// tri_kernels.hip on the context's stream, results back.  The sort and the scans of the track compaction are rocPRIM's (a stable
// radix sort and integer scans: the bytes they give depend on the input alone).
#include "sfd2_ctx.h"
#include "api_scratch.h"
#include "pose_camera.h"
#include <rocprim/rocprim.hpp>

namespace {

// views -> device form; mean focal lengths on the side
bool pack_views(const sfd2_tri_view *views, int n, std::vector<TriViewDev> &out, std::vector<double> &mean_focal, std::string &why)
{
    out.resize(std::max(n, 1));
    mean_focal.resize(std::max(n, 1));
    for (int i = 0; i < n; ++i) {
        TriViewDev &d = out[i];
        memset(&d, 0, sizeof(d));
        std::string w;
        if (!sfd2_pose_cam(views[i].model, views[i].params, d.cam, w)) { why = "view " + std::to_string(i) + ": " + w; return false; }
        const double *q = views[i].qvec;
        const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (!all_finite(q, 4) || !all_finite(views[i].tvec, 3) || !(nq > 0)) {
            why = "view " + std::to_string(i) + ": the pose must be finite with a non-zero quaternion";
            return false;
        }
        quat_to_rot(q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq, d.R);
        for (int a = 0; a < 3; ++a) d.t[a] = views[i].tvec[a];
        for (int a = 0; a < 3; ++a) d.C[a] = -(d.R[a] * d.t[0] + d.R[3 + a] * d.t[1] + d.R[6 + a] * d.t[2]);
        mean_focal[i] = 0.5 * (d.cam.f[0] + d.cam.f[1]);
    }
    return true;
}

}  // namespace

extern "C" int sfd2_verify_matches_batch(sfd2_ctx *c, const sfd2_tri_view *views, int n_views, const int64_t *kp_offsets, const float *keypoints,
                                         const int32_t *pair_views, const int64_t *match_offsets, int n_pairs, int32_t *matches,
                                         double max_error_px, int min_num_inliers, int32_t *pair_counts, int32_t *pair_status, int flags)
{
    const std::string F("sfd2_verify_matches_batch: ");
    if (!c || !views || !kp_offsets || (n_pairs > 0 && (!pair_views || !match_offsets || !pair_counts || !pair_status))) return fail(F + "null argument");
    if (n_views < 1 || n_pairs < 0) return fail(F + "n_views must be positive and n_pairs non-negative");
    if (flags != 0) return fail(F + "unknown flags");
    if (!(std::isfinite(max_error_px) && max_error_px > 0) || min_num_inliers < 0) return fail(F + "max_error_px must be positive and finite, min_num_inliers >= 0");
    if (!monotone(kp_offsets, n_views)) return fail(F + "kp_offsets must start at 0 and not decrease");
    const int64_t N = kp_offsets[n_views];
    if (N > 0 && !keypoints) return fail(F + "null keypoints");
    if (n_pairs == 0) return 0;
    if (!monotone(match_offsets, n_pairs)) return fail(F + "match_offsets must start at 0 and not decrease");
    const int64_t M = match_offsets[n_pairs];
    if (M > 0 && !matches) return fail(F + "null matches");
    if (!all_finite(keypoints, 2 * N)) return fail(F + "non-finite key points");
    std::vector<TriViewDev> vd;
    std::vector<double> mf;
    std::string why;
    if (!pack_views(views, n_views, vd, mf, why)) return fail(F + why);
    std::vector<TriPairDev> pd(n_pairs);
    std::vector<int32_t> blk_pair;
    for (int p = 0; p < n_pairs; ++p) {
        const int i = pair_views[2 * p], j = pair_views[2 * p + 1];
        const int64_t n = match_offsets[p + 1] - match_offsets[p];
        if (i < 0 || j < 0 || i >= n_views || j >= n_views) return fail(F + "pair " + std::to_string(p) + ": view index out of range");
        if (n > 0x7fffffffLL || kp_offsets[i + 1] - kp_offsets[i] > 0x7fffffffLL || kp_offsets[j + 1] - kp_offsets[j] > 0x7fffffffLL)
            return fail(F + "pair " + std::to_string(p) + ": more than 2^31 - 1 matches or key points");
        TriPairDev &d = pd[p];
        memset(&d, 0, sizeof(d));
        const TriViewDev &A = vd[i], &B = vd[j];
        double R[9], t[3];                                   // x_j = R x_i + t: R = Rj Ri^T, t = tj - R ti
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) R[3 * a + b] = B.R[3 * a] * A.R[3 * b] + B.R[3 * a + 1] * A.R[3 * b + 1] + B.R[3 * a + 2] * A.R[3 * b + 2];
        for (int a = 0; a < 3; ++a) t[a] = B.t[a] - (R[3 * a] * A.t[0] + R[3 * a + 1] * A.t[1] + R[3 * a + 2] * A.t[2]);
        for (int b = 0; b < 3; ++b) {                        // E = [t]x R
            d.E[b] = t[1] * R[6 + b] - t[2] * R[3 + b];
            d.E[3 + b] = t[2] * R[b] - t[0] * R[6 + b];
            d.E[6 + b] = t[0] * R[3 + b] - t[1] * R[b];
        }
        if (i == j) memset(d.E, 0, sizeof(d.E));             // an image with itself: E = 0 (every distance NaN, all rejected), not the
                                                             // rounding residue of R R^T - 1
        d.thr_i = max_error_px / mf[i];
        d.thr_j = max_error_px / mf[j];
        d.moff = match_offsets[p];
        d.kp_i = kp_offsets[i];
        d.kp_j = kp_offsets[j];
        d.n = (int32_t)n;
        d.n_i = (int32_t)(kp_offsets[i + 1] - kp_offsets[i]);
        d.n_j = (int32_t)(kp_offsets[j + 1] - kp_offsets[j]);
        d.blk0 = (int32_t)blk_pair.size();
        const int64_t nb = (n + SFD2_TRI_WG - 1) / SFD2_TRI_WG;
        if ((int64_t)blk_pair.size() + nb > 0x7fffffffLL) return fail(F + "too many matches for one call");
        blk_pair.insert(blk_pair.end(), (size_t)nb, p);
    }
    const int n_blocks = (int)blk_pair.size();
    HIPCHECK(hipSetDevice(c->device));
    Carve in, ws;
    const size_t o_v = in.take(sizeof(TriViewDev) * n_views), o_off = in.take(8 * (size_t)(n_views + 1)), o_kp = in.take(8 * (size_t)N),
                 o_pd = in.take(sizeof(TriPairDev) * n_pairs), o_bp = in.take(4 * (size_t)n_blocks);
    const size_t o_xn = ws.take(16 * (size_t)N), o_m = ws.take(8 * (size_t)M), o_bc = ws.take(4 * (size_t)n_blocks), o_pc = ws.take(4 * (size_t)n_pairs),
                 o_ps = ws.take(4 * (size_t)n_pairs);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->tri_in, in.off));
    HIPCHECK(grow(c->tri_ws, ws.off));
    char *di = c->tri_in.as<char>(), *dw = c->tri_ws.as<char>();
    HIPCHECK(hipMemcpyAsync(di + o_v, vd.data(), sizeof(TriViewDev) * n_views, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(di + o_off, kp_offsets, 8 * (size_t)(n_views + 1), hipMemcpyHostToDevice, c->stream));
    if (N) HIPCHECK(hipMemcpyAsync(di + o_kp, keypoints, 8 * (size_t)N, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(di + o_pd, pd.data(), sizeof(TriPairDev) * n_pairs, hipMemcpyHostToDevice, c->stream));
    if (n_blocks) HIPCHECK(hipMemcpyAsync(di + o_bp, blk_pair.data(), 4 * (size_t)n_blocks, hipMemcpyHostToDevice, c->stream));
    if (M) HIPCHECK(hipMemcpyAsync(dw + o_m, matches, 8 * (size_t)M, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemsetAsync(dw + o_ps, 0, 4 * (size_t)n_pairs, c->stream));
    {
        ProfScope ps(c, "verify_matches", "tri_normalise+verify+count+drop", 0.0, 16.0 * (double)N + 48.0 * (double)M);
        launch_tri_normalise(c->stream, at<const TriViewDev>(di, o_v), n_views, at<const int64_t>(di, o_off), at<const float>(di, o_kp), N,
                             at<double2>(dw, o_xn));
        launch_tri_verify(c->stream, at<const TriPairDev>(di, o_pd), n_pairs, at<const int32_t>(di, o_bp), n_blocks, at<const double2>(dw, o_xn),
                          at<int32_t>(dw, o_m), at<int32_t>(dw, o_bc), at<int32_t>(dw, o_pc), at<int32_t>(dw, o_ps), min_num_inliers);
    }
    HIPCHECK(hipGetLastError());
    if (M) HIPCHECK(hipMemcpyAsync(matches, dw + o_m, 8 * (size_t)M, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(pair_counts, dw + o_pc, 4 * (size_t)n_pairs, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(pair_status, dw + o_ps, 4 * (size_t)n_pairs, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int p = 0; p < n_pairs; ++p)
        if (pair_status[p]) return fail(F + "pair " + std::to_string(p) + ": a match index beyond its image's key points");
    return 0;
}

extern "C" int sfd2_build_tracks(sfd2_ctx *c, int64_t n_nodes, const int32_t *edges, int64_t n_edges, int max_rounds, int32_t *labels,
                                 int32_t *track_offsets, int32_t *track_nodes, int64_t *n_tracks, int64_t *n_track_nodes, int32_t *status, int flags)
{
    const std::string F("sfd2_build_tracks: ");
    if (!c || !n_tracks || !n_track_nodes || !status || !track_offsets || (n_nodes > 0 && (!labels || !track_nodes)) || (n_edges > 0 && !edges))
        return fail(F + "null argument");
    if (n_nodes < 0 || n_nodes > 0x7fffffffLL - 1024 || n_edges < 0) return fail(F + "n_nodes must lie in [0, 2^31 - 1025], n_edges >= 0");
    if (max_rounds < 1 || max_rounds > 100000) return fail(F + "max_rounds must lie in [1, 100000]");
    if (flags != 0) return fail(F + "unknown flags");
    status[0] = status[1] = 0;
    *n_tracks = *n_track_nodes = 0;
    track_offsets[0] = 0;
    if (n_nodes == 0) return 0;
    HIPCHECK(hipSetDevice(c->device));
    const size_t n = (size_t)n_nodes;
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < n_nodes) ++bits;
    size_t tmp_sort = 0, tmp_scan = 0;
    {
        int32_t *nil = nullptr;
        HIPCHECK(rocprim::radix_sort_pairs(nullptr, tmp_sort, nil, nil, nil, nil, n, 0, (unsigned)bits, c->stream));
        HIPCHECK(rocprim::exclusive_scan(nullptr, tmp_scan, nil, nil, 0, n, rocprim::plus<int32_t>(), c->stream));
    }
    Carve ws;
    const size_t o_e = ws.take(8 * (size_t)n_edges), o_par = ws.take(4 * n), o_w = ws.take(16), o_iota = ws.take(4 * n), o_sl = ws.take(4 * n),
                 o_sn = ws.take(4 * n), o_keep = ws.take(4 * n), o_head = ws.take(4 * n), o_pos = ws.take(4 * n), o_tid = ws.take(4 * n),
                 o_to = ws.take(4 * (n / 2 + 2)), o_tn = ws.take(4 * n), o_tmp = ws.take(std::max(tmp_sort, tmp_scan));
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->tri_ws, ws.off));
    char *d = c->tri_ws.as<char>();
    int32_t *par = at<int32_t>(d, o_par), *words = at<int32_t>(d, o_w);
    if (n_edges) HIPCHECK(hipMemcpyAsync(d + o_e, edges, 8 * (size_t)n_edges, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemsetAsync(words, 0, 16, c->stream));
    launch_tri_iota(c->stream, par, n_nodes);
    int rounds = 0;
    bool quiet = false;
    int32_t w[2] = {0, 0};
    {
        ProfScope ps(c, "build_tracks", "tri_cc_hook+jump", 0.0, 0.0);
        for (; rounds < max_rounds && !quiet;) {
            HIPCHECK(hipMemsetAsync(words, 0, 4, c->stream));
            launch_tri_cc_round(c->stream, at<const int32_t>(d, o_e), n_edges, par, n_nodes, words);
            HIPCHECK(hipMemcpyAsync(w, words, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipStreamSynchronize(c->stream));
            ++rounds;
            quiet = w[0] == 0;
            if (w[1]) break;
        }
    }
    HIPCHECK(hipGetLastError());
    status[1] = rounds;
    if (w[1]) {
        status[0] = w[1];
        return fail(F + "an edge names a node beyond n_nodes");
    }
    if (!quiet) {
        status[0] = SFD2_TRI_ST_NOT_CONVERGED;
        return fail(F + "not converged after " + std::to_string(rounds) + " rounds (max_rounds)");
    }
    int32_t *sl = at<int32_t>(d, o_sl), *sn = at<int32_t>(d, o_sn), *keep = at<int32_t>(d, o_keep), *head = at<int32_t>(d, o_head),
            *pos = at<int32_t>(d, o_pos), *tid = at<int32_t>(d, o_tid);
    {
        ProfScope ps(c, "build_tracks", "tri_cc_sort+scan+scatter", 0.0, 0.0);
        launch_tri_iota(c->stream, at<int32_t>(d, o_iota), n_nodes);
        size_t tb = tmp_sort;
        HIPCHECK(rocprim::radix_sort_pairs(d + o_tmp, tb, par, sl, at<int32_t>(d, o_iota), sn, n, 0, (unsigned)bits, c->stream));
        launch_tri_cc_flags(c->stream, sl, n_nodes, keep, head);
        tb = tmp_scan;
        HIPCHECK(rocprim::exclusive_scan(d + o_tmp, tb, keep, pos, 0, n, rocprim::plus<int32_t>(), c->stream));
        tb = tmp_scan;
        HIPCHECK(rocprim::exclusive_scan(d + o_tmp, tb, head, tid, 0, n, rocprim::plus<int32_t>(), c->stream));
        launch_tri_cc_scatter(c->stream, sl, sn, n_nodes, keep, head, pos, tid, at<int32_t>(d, o_to), at<int32_t>(d, o_tn), words + 2);
    }
    HIPCHECK(hipGetLastError());
    int32_t tot[2] = {0, 0};
    HIPCHECK(hipMemcpyAsync(labels, par, 4 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(tot, words + 2, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    *n_tracks = tot[0];
    *n_track_nodes = tot[1];
    HIPCHECK(hipMemcpyAsync(track_offsets, d + o_to, 4 * ((size_t)tot[0] + 1), hipMemcpyDeviceToHost, c->stream));
    if (tot[1]) HIPCHECK(hipMemcpyAsync(track_nodes, d + o_tn, 4 * (size_t)tot[1], hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int sfd2_triangulate_tracks(sfd2_ctx *c, const sfd2_tri_view *views, int n_views, const int64_t *track_offsets, const int64_t *track_labels,
                                       int n_tracks, const int32_t *obs_view, const float *obs_xy, const sfd2_tri_conf *conf, double *xyz, double *error,
                                       int32_t *n_obs, int8_t *obs_point, int32_t *track_status, int flags)
{
    const std::string F("sfd2_triangulate_tracks: ");
    if (!c || !views || !conf || !track_offsets || (n_tracks > 0 && (!track_labels || !xyz || !error || !n_obs || !track_status))) return fail(F + "null argument");
    if (n_views < 1 || n_tracks < 0) return fail(F + "n_views must be positive and n_tracks non-negative");
    if (flags != 0) return fail(F + "unknown flags");
    if (!(conf->min_tri_angle_deg >= 0 && conf->min_tri_angle_deg < 90) || !(conf->create_max_angle_error_deg > 0 && conf->create_max_angle_error_deg < 90) ||
        !(std::isfinite(conf->filter_max_reproj_error) && conf->filter_max_reproj_error > 0) || conf->max_refine_iterations < 1 ||
        conf->max_refine_iterations > 1000)
        return fail(F + "angles must lie in [0, 90) degrees, the reprojection bound be positive and finite, 1 <= max_refine_iterations <= 1000");
    if (n_tracks == 0) return 0;
    if (!monotone(track_offsets, n_tracks)) return fail(F + "track_offsets must start at 0 and not decrease");
    const int64_t O = track_offsets[n_tracks];
    if (O > 0 && (!obs_view || !obs_xy || !obs_point)) return fail(F + "null observations");
    if (const int64_t o = first_outside(obs_view, O, n_views); o < O) return fail(F + "observation " + std::to_string(o) + ": view index out of range");
    if (!all_finite(obs_xy, 2 * O)) return fail(F + "non-finite observations");
    {   // the one-per-image rule looks at neighbours only: a track must not come back to a view it has left
        std::vector<int32_t> run_of(n_views, -1);            // the last track that opened a run of this view
        for (int t = 0; t < n_tracks; ++t)
            for (int64_t o = track_offsets[t]; o < track_offsets[t + 1]; ++o) {
                if (o > track_offsets[t] && obs_view[o] == obs_view[o - 1]) continue;
                if (run_of[obs_view[o]] == t)
                    return fail(F + "observation " + std::to_string(o) + ": its track returns to view " + std::to_string(obs_view[o]) +
                                " after leaving it (the observations of one view must be consecutive)");
                run_of[obs_view[o]] = t;
            }
    }
    std::vector<TriViewDev> vd;
    std::vector<double> mf;
    std::string why;
    if (!pack_views(views, n_views, vd, mf, why)) return fail(F + why);
    // long tracks first: a wave per track, the launch order is the only coupling between them
    std::vector<int32_t> order(n_tracks);
    for (int t = 0; t < n_tracks; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return track_offsets[a + 1] - track_offsets[a] > track_offsets[b + 1] - track_offsets[b];
    });
    const double kDeg = 3.14159265358979323846 / 180.0;
    TriConfDev cd;
    memset(&cd, 0, sizeof(cd));
    cd.tan_create = std::tan(conf->create_max_angle_error_deg * kDeg);
    cd.cos_min_angle = std::cos(conf->min_tri_angle_deg * kDeg);
    cd.max_reproj = conf->filter_max_reproj_error;
    cd.seed = conf->seed;
    cd.lm_iters = conf->max_refine_iterations;
    HIPCHECK(hipSetDevice(c->device));
    const size_t T = (size_t)n_tracks, P = T * SFD2_TRI_MAX_POINTS;
    Carve in, ws;
    const size_t o_v = in.take(sizeof(TriViewDev) * n_views), o_off = in.take(8 * (T + 1)), o_lab = in.take(8 * T), o_ord = in.take(4 * T),
                 o_ov = in.take(4 * (size_t)O), o_xy = in.take(8 * (size_t)O);
    const size_t o_px = ws.take(16 * (size_t)O), o_xn = ws.take(16 * (size_t)O), o_pt = ws.take((size_t)O), o_tmp = ws.take((size_t)O),
                 o_xyz = ws.take(24 * P), o_err = ws.take(8 * P), o_no = ws.take(4 * P), o_st = ws.take(4 * T);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->tri_in, in.off));
    HIPCHECK(grow(c->tri_ws, ws.off));
    char *di = c->tri_in.as<char>(), *dw = c->tri_ws.as<char>();
    HIPCHECK(hipMemcpyAsync(di + o_v, vd.data(), sizeof(TriViewDev) * n_views, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(di + o_off, track_offsets, 8 * (T + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(di + o_lab, track_labels, 8 * T, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(di + o_ord, order.data(), 4 * T, hipMemcpyHostToDevice, c->stream));
    if (O) {
        HIPCHECK(hipMemcpyAsync(di + o_ov, obs_view, 4 * (size_t)O, hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(di + o_xy, obs_xy, 8 * (size_t)O, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHECK(hipMemsetAsync(dw + o_pt, 0xff, std::max<size_t>((size_t)O, 1), c->stream));
    HIPCHECK(hipMemsetAsync(dw + o_xyz, 0, ws.off - o_xyz, c->stream));     // points, errors, counts, status
    {
        ProfScope ps(c, "triangulate_tracks", "tri_obs_prep+tri_track", 0.0, 48.0 * (double)O);
        launch_tri_obs_prep(c->stream, at<const TriViewDev>(di, o_v), at<const int32_t>(di, o_ov), at<const float>(di, o_xy), O, at<double2>(dw, o_px),
                            at<double2>(dw, o_xn));
        launch_tri_tracks(c->stream, at<const TriViewDev>(di, o_v), cd, at<const int64_t>(di, o_off), at<const int64_t>(di, o_lab),
                          at<const int32_t>(di, o_ord), n_tracks, at<const int32_t>(di, o_ov), at<const double2>(dw, o_px), at<const double2>(dw, o_xn),
                          at<signed char>(dw, o_pt), at<unsigned char>(dw, o_tmp), at<double>(dw, o_xyz), at<double>(dw, o_err), at<int32_t>(dw, o_no),
                          at<int32_t>(dw, o_st));
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(xyz, dw + o_xyz, 24 * P, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(error, dw + o_err, 8 * P, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(n_obs, dw + o_no, 4 * P, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(track_status, dw + o_st, 4 * T, hipMemcpyDeviceToHost, c->stream));
    if (O) HIPCHECK(hipMemcpyAsync(obs_point, dw + o_pt, (size_t)O, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}
