// libsfd2hip: sfd2_relative_pose_batch -- checks and packs the pairs, one launch of two_view_kernels.hip.
#include "sfd2_ctx.h"
#include "api_scratch.h"

extern "C" int sfd2_relative_pose_batch(sfd2_ctx *c, const sfd2_two_view_problem *problems, int k, const sfd2_two_view_conf *conf,
                                        sfd2_two_view_result *results, uint8_t *inlier_mask_u8, double *tri_angle_deg, int flags)
{
    const std::string F("sfd2_relative_pose_batch");
    if (!c || !conf || (k > 0 && (!problems || !results))) return fail(F + ": null argument");
    if (k < 0) return fail(F + ": negative k");
    if (flags != 0) return fail(F + ": unknown flags");
    if (const char *bad = ransac_conf_error(conf->confidence, conf->min_inlier_ratio, conf->min_num_trials, conf->max_num_trials))
        return fail(F + bad);
    if (conf->min_num_inliers < 0) return fail(F + ": negative min_num_inliers");
    TvConfDev d;
    memset(&d, 0, sizeof(d));
    const double p_all = std::pow(floored_ratio(conf->min_inlier_ratio), 5);                 // sample size 5
    const TrialLimits t = trial_limits(conf->confidence, conf->min_num_trials, conf->max_num_trials, INT64_MAX, p_all);
    d.max_trials = t.max_trials;
    d.min_trials = t.min_trials;
    d.confidence = conf->confidence;
    d.seed = conf->seed;
    d.min_num_inliers = conf->min_num_inliers;
    std::vector<TvProbDev> pd(k);
    int64_t total = 0;
    for (int i = 0; i < k; ++i) {
        const sfd2_two_view_problem &p = problems[i];
        const std::string at = F + ": problem " + std::to_string(i) + ": ";
        if (p.n < 0) return fail(at + "negative n");
        if (p.n > 0 && (!p.points2D_0 || !p.points2D_1)) return fail(at + "null points");
        TvProbDev &o = pd[i];
        memset(&o, 0, sizeof(o));
        std::string why;
        if (!sfd2_pose_cam(p.model0, p.params0, o.cam0, why)) return fail(at + "camera 0: " + why);
        if (!sfd2_pose_cam(p.model1, p.params1, o.cam1, why)) return fail(at + "camera 1: " + why);
        if (!all_finite(p.points2D_0, 2 * (int64_t)p.n) || !all_finite(p.points2D_1, 2 * (int64_t)p.n)) return fail(at + "non-finite points");
        if (!(std::isfinite(p.max_error_px) && p.max_error_px > 0)) return fail(at + "max_error_px must be positive and finite");
        const double mf = 0.25 * (o.cam0.f[0] + o.cam0.f[1] + o.cam1.f[0] + o.cam1.f[1]);
        o.thresh2 = (p.max_error_px / mf) * (p.max_error_px / mf);
        o.off = total;
        o.n = p.n;
        total += p.n;
    }
    if (total > 0 && (!inlier_mask_u8 || !tri_angle_deg)) return fail(F + ": null inlier mask or angles");
    if (k == 0) return 0;
    HIPCHECK(hipSetDevice(c->device));
    const int64_t N = std::max<int64_t>(total, 1);
    Carve ci, cw, co;
    // inputs: problems | points of image 0 | of image 1;  work: normalised points 0 | 1 | the trials' matrices;  out: results | mask | angles
    const size_t o_pd = ci.take(sizeof(TvProbDev) * k), o_p0 = ci.take(16 * N), o_p1 = ci.take(16 * N);
    const size_t o_x0 = cw.take(16 * N), o_x1 = cw.take(16 * N), o_hyp = cw.take(sizeof(double) * (size_t)k * SFD2_TV_WG * SFD2_TV_CAND * 9);
    const size_t o_res = co.take(sizeof(TvResDev) * k), o_m = co.take(N), o_a = co.take(8 * N);
    HIPCHECK(hipStreamSynchronize(c->stream));              // earlier calls on this stream may still read the buffers
    HIPCHECK(grow(c->tv_in, ci.off));
    HIPCHECK(grow(c->tv_ws, cw.off));
    HIPCHECK(grow(c->tv_out, co.off));
    std::vector<double> p0(2 * (size_t)N), p1(2 * (size_t)N);
    for (int i = 0; i < k; ++i) {
        const int64_t o = pd[i].off, n = pd[i].n;
        if (n) {
            memcpy(p0.data() + 2 * o, problems[i].points2D_0, 16 * n);
            memcpy(p1.data() + 2 * o, problems[i].points2D_1, 16 * n);
        }
    }
    char *in = c->tv_in.as<char>(), *ws = c->tv_ws.as<char>(), *out = c->tv_out.as<char>();
    HIPCHECK(hipMemcpyAsync(in + o_pd, pd.data(), sizeof(TvProbDev) * k, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(in + o_p0, p0.data(), 16 * total, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(in + o_p1, p1.data(), 16 * total, hipMemcpyHostToDevice, c->stream));
    launch_two_view(c->stream, at<const TvProbDev>(in, o_pd), k, d, at<const double>(in, o_p0), at<const double>(in, o_p1), at<double2>(ws, o_x0),
                    at<double2>(ws, o_x1), at<double>(ws, o_hyp), at<unsigned char>(out, o_m), at<double>(out, o_a), at<TvResDev>(out, o_res));
    HIPCHECK(hipGetLastError());
    std::vector<TvResDev> r(k);
    HIPCHECK(hipMemcpyAsync(r.data(), out + o_res, sizeof(TvResDev) * k, hipMemcpyDeviceToHost, c->stream));
    if (total) {
        HIPCHECK(hipMemcpyAsync(inlier_mask_u8, out + o_m, total, hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(tri_angle_deg, out + o_a, 8 * total, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < k; ++i) {
        sfd2_two_view_result &o = results[i];
        o.success = r[i].success;
        o.num_inliers = r[i].num_inliers;
        o.num_trials = r[i].num_trials;
        o.reserved = 0;
        for (int j = 0; j < 4; ++j) o.qvec[j] = r[i].q[j];
        for (int j = 0; j < 3; ++j) o.tvec[j] = r[i].t[j];
        for (int j = 0; j < 9; ++j) o.E[j] = r[i].E[j];
    }
    return 0;
}
