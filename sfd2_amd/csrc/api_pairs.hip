// libsfd2hip: sfd2_pairs_retrieval / sfd2_pairs_covisibility / sfd2_pairs_poses -- checks the inputs (every index a kernel follows is
// bounds-checked here), uploads them, the launches of pairs_kernels.hip on the context's stream, results back.
#include "sfd2_ctx.h"
#include "api_scratch.h"

namespace {

bool k_ok(int k, int most = SFD2_PAIRS_MAX_K) { return k >= 1 && k <= most; }

}  // namespace

extern "C" int sfd2_pairs_retrieval(sfd2_ctx *c, const float *query, int nq, const float *db, int nd, int d, int k, int inputs_on_device,
                                    int32_t *idx, float *sim, int flags)
{
    const std::string F("sfd2_pairs_retrieval: ");
    if (!c || !query || !db || !idx || !sim) return fail(F + "null argument");
    if (nq < 1 || nd < 1 || d < 1) return fail(F + "nq, nd and d must be positive");
    if (!k_ok(k)) return fail(F + "k must lie in [1, " + std::to_string(SFD2_PAIRS_MAX_K) + "]");
    if (k > nd) return fail(F + "k = " + std::to_string(k) + " is larger than the " + std::to_string(nd) + " db rows");
    if (flags & ~0xff00) return fail(F + "unknown flags");
    if ((int64_t)nq * k > 0x7fffffffLL || (int64_t)nd + 128 > 0x7fffffffLL) return fail(F + "nq * k and nd must stay below 2^31");
    const int tiles = pairs_retrieval_tiles(nd), strips = pairs_retrieval_strips(nq);
    int splits = (flags >> 8) & 0xff;
    if (splits == 0) splits = (512 + strips - 1) / strips;       // about two blocks per CU when nq is small
    splits = std::max(1, std::min(splits, std::min(tiles, 64)));
    while (splits > 1 && (size_t)nq * splits * k * 8 > ((size_t)1 << 30)) --splits;
    HIPCHECK(hipSetDevice(c->device));
    const size_t na = (size_t)nq * d, nb = (size_t)nd * d;
    Carve in, ws;
    const size_t o_q = in.take(inputs_on_device ? 0 : 4 * na), o_db = in.take(inputs_on_device ? 0 : 4 * nb);
    const size_t o_ps = ws.take(4 * (size_t)nq * splits * k), o_pi = ws.take(4 * (size_t)nq * splits * k), o_idx = ws.take(4 * (size_t)nq * k),
                 o_sim = ws.take(4 * (size_t)nq * k), o_flag = ws.take(4);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->pairs_in, in.off));
    HIPCHECK(grow(c->pairs_ws, ws.off));
    char *di = c->pairs_in.as<char>(), *dw = c->pairs_ws.as<char>();
    const float *dq = query, *dd = db;
    if (!inputs_on_device) {
        HIPCHECK(hipMemcpyAsync(di + o_q, query, 4 * na, hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(di + o_db, db, 4 * nb, hipMemcpyHostToDevice, c->stream));
        dq = at<const float>(di, o_q);
        dd = at<const float>(di, o_db);
    }
    HIPCHECK(hipMemsetAsync(dw + o_flag, 0, 4, c->stream));
    {
        ProfScope ps(c, "pairs_retrieval", "pairs_finite+retrieval+merge", 2.0 * (double)nq * nd * d, 4.0 * (double)(na + nb));
        HIPCHECK(launch_pairs_finite(c->stream, dq, na, dd, nb, at<int>(dw, o_flag)));
        HIPCHECK(launch_pairs_retrieval(c->stream, dq, nq, dd, nd, d, k, splits, at<float>(dw, o_ps), at<int>(dw, o_pi), at<int32_t>(dw, o_idx),
                                        at<float>(dw, o_sim)));
    }
    int bad = 0;
    HIPCHECK(hipMemcpyAsync(&bad, dw + o_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(idx, dw + o_idx, 4 * (size_t)nq * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(sim, dw + o_sim, 4 * (size_t)nq * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    if (bad) return fail(F + "non-finite descriptor");
    return 0;
}

extern "C" int sfd2_pairs_covisibility(sfd2_ctx *c, const int64_t *obs_offsets, const int32_t *obs_point, int n_images, const int64_t *track_offsets,
                                       const int32_t *track_image, int n_points, int k, int32_t *idx, int32_t *count, int32_t *n_found, int flags)
{
    const std::string F("sfd2_pairs_covisibility: ");
    if (!c || !obs_offsets || !track_offsets || !idx || !count || !n_found) return fail(F + "null argument");
    if (n_images < 1 || n_points < 0) return fail(F + "n_images must be positive and n_points non-negative");
    if (!k_ok(k)) return fail(F + "k must lie in [1, " + std::to_string(SFD2_PAIRS_MAX_K) + "]");
    if (flags & ~SFD2_PAIRS_FLAG_GLOBAL_COUNTERS) return fail(F + "unknown flags");
    if ((int64_t)n_images * k > 0x7fffffffLL) return fail(F + "n_images * k must stay below 2^31");
    if (!monotone(obs_offsets, n_images)) return fail(F + "obs_offsets must start at 0 and not decrease");
    if (!monotone(track_offsets, n_points)) return fail(F + "track_offsets must start at 0 and not decrease");
    const int64_t O = obs_offsets[n_images], T = track_offsets[n_points];
    if ((O > 0 && !obs_point) || (T > 0 && !track_image)) return fail(F + "null argument");
    if (const int64_t o = first_outside(obs_point, O, n_points); o < O) return fail(F + "observation " + std::to_string(o) + ": point row out of range");
    if (const int64_t t = first_outside(track_image, T, n_images); t < T) return fail(F + "track element " + std::to_string(t) + ": image index out of range");
    const int global = (flags & SFD2_PAIRS_FLAG_GLOBAL_COUNTERS) || n_images > SFD2_PAIRS_COVIS_LDS_IMAGES;
    const int blocks = std::min(n_images, global ? 512 : 2048);
    HIPCHECK(hipSetDevice(c->device));
    Carve in, ws;
    const size_t o_oo = in.take(8 * (size_t)(n_images + 1)), o_op = in.take(4 * (size_t)O), o_to = in.take(8 * (size_t)(n_points + 1)),
                 o_ti = in.take(4 * (size_t)T);
    const size_t o_idx = ws.take(4 * (size_t)n_images * k), o_cnt = ws.take(4 * (size_t)n_images * k), o_n = ws.take(4 * (size_t)n_images),
                 o_scr = ws.take(global ? 4 * (size_t)blocks * n_images : 0);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->pairs_in, in.off));
    HIPCHECK(grow(c->pairs_ws, ws.off));
    char *di = c->pairs_in.as<char>(), *dw = c->pairs_ws.as<char>();
    HIPCHECK(hipMemcpyAsync(di + o_oo, obs_offsets, 8 * (size_t)(n_images + 1), hipMemcpyHostToDevice, c->stream));
    if (O) HIPCHECK(hipMemcpyAsync(di + o_op, obs_point, 4 * (size_t)O, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(di + o_to, track_offsets, 8 * (size_t)(n_points + 1), hipMemcpyHostToDevice, c->stream));
    if (T) HIPCHECK(hipMemcpyAsync(di + o_ti, track_image, 4 * (size_t)T, hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, "pairs_covisibility", global ? "pairs_covis<global>" : "pairs_covis<lds>", 0.0, 4.0 * (double)(O + T));
        HIPCHECK(launch_pairs_covis(c->stream, at<const int64_t>(di, o_oo), at<const int32_t>(di, o_op), n_images, at<const int64_t>(di, o_to),
                                    at<const int32_t>(di, o_ti), k, global, blocks, at<int>(dw, o_scr), at<int32_t>(dw, o_idx), at<int32_t>(dw, o_cnt),
                                    at<int32_t>(dw, o_n)));
    }
    HIPCHECK(hipMemcpyAsync(idx, dw + o_idx, 4 * (size_t)n_images * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(count, dw + o_cnt, 4 * (size_t)n_images * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(n_found, dw + o_n, 4 * (size_t)n_images, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int sfd2_pairs_poses(sfd2_ctx *c, const double *qvec, const double *tvec, int n, int k, double rotation_threshold_deg, int32_t *idx,
                                double *dist, int32_t *n_found, int flags)
{
    const std::string F("sfd2_pairs_poses: ");
    if (!c || !qvec || !tvec || !idx || !dist || !n_found) return fail(F + "null argument");
    if (n < 1) return fail(F + "n must be positive");
    if (!k_ok(k, SFD2_PAIRS_POSES_MAX_K)) return fail(F + "k must lie in [1, " + std::to_string(SFD2_PAIRS_POSES_MAX_K) + "]");
    if (flags & ~SFD2_PAIRS_FLAG_CENTRES) return fail(F + "unknown flags");
    if ((int64_t)n * k > 0x7fffffffLL) return fail(F + "n * k must stay below 2^31");
    if (std::isnan(rotation_threshold_deg)) return fail(F + "rotation_threshold_deg is not a number");
    if (!all_finite(qvec, 4 * (int64_t)n)) return fail(F + "non-finite qvec");
    if (!all_finite(tvec, 3 * (int64_t)n)) return fail(F + "non-finite tvec");
    HIPCHECK(hipSetDevice(c->device));
    Carve in, ws;
    const size_t o_q = in.take(32 * (size_t)n), o_t = in.take(24 * (size_t)n);
    const size_t o_rc = ws.take(96 * (size_t)n), o_idx = ws.take(4 * (size_t)n * k), o_d = ws.take(8 * (size_t)n * k), o_n = ws.take(4 * (size_t)n);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->pairs_in, in.off));
    HIPCHECK(grow(c->pairs_ws, ws.off));
    char *di = c->pairs_in.as<char>(), *dw = c->pairs_ws.as<char>();
    HIPCHECK(hipMemcpyAsync(di + o_q, qvec, 32 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(di + o_t, tvec, 24 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, "pairs_poses", "pairs_pose_prep+pairs_pose", 0.0, 96.0 * (double)n);
        HIPCHECK(launch_pairs_poses(c->stream, at<const double>(di, o_q), at<const double>(di, o_t), n, k, rotation_threshold_deg,
                                    (flags & SFD2_PAIRS_FLAG_CENTRES) ? 1 : 0, at<double>(dw, o_rc), at<int32_t>(dw, o_idx), at<double>(dw, o_d),
                                    at<int32_t>(dw, o_n)));
    }
    HIPCHECK(hipMemcpyAsync(idx, dw + o_idx, 4 * (size_t)n * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(dist, dw + o_d, 8 * (size_t)n * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(n_found, dw + o_n, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}
