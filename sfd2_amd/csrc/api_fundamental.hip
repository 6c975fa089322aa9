// libsfd2hip: sfd2_fundamental_batch -- checks and packs the pairs, one launch of fundamental_kernels.hip.  The checking, packing and
// scratch layer is pairs_batch below; sfd2_homography_batch (api_homography.hip) goes through it too with its own kernel and sample size.
#include "sfd2_ctx.h"
#include "api_scratch.h"

// k pairs of pixel correspondences without cameras through one launch of `launch`: the checks, the concatenation with one offset per
// pair, the context's fm_* scratch blocks, the copies.  name: the entry point in the error texts; sample_size: of the trial count.
int pairs_batch(const char *name, int sample_size, PairsLaunch launch, sfd2_ctx *c, const sfd2_fundamental_problem *problems, int k,
                const sfd2_two_view_conf *conf, sfd2_fundamental_result *results, uint8_t *inlier_mask_u8, int flags)
{
    const std::string F(name);
    if (!c || !conf || (k > 0 && (!problems || !results))) return fail(F + ": null argument");
    if (k < 0) return fail(F + ": negative k");
    if (flags != 0) return fail(F + ": unknown flags");
    if (const char *bad = ransac_conf_error(conf->confidence, conf->min_inlier_ratio, conf->min_num_trials, conf->max_num_trials))
        return fail(F + bad);
    if (conf->min_num_inliers < 0) return fail(F + ": negative min_num_inliers");
    TvConfDev d;
    memset(&d, 0, sizeof(d));
    const double p_all = std::pow(floored_ratio(conf->min_inlier_ratio), sample_size);
    const TrialLimits t = trial_limits(conf->confidence, conf->min_num_trials, conf->max_num_trials, INT64_MAX, p_all);
    d.max_trials = t.max_trials;
    d.min_trials = t.min_trials;
    d.confidence = conf->confidence;
    d.seed = conf->seed;
    d.min_num_inliers = conf->min_num_inliers;
    std::vector<FmProbDev> pd(k);
    int64_t total = 0;
    for (int i = 0; i < k; ++i) {
        const sfd2_fundamental_problem &p = problems[i];
        const std::string at = F + ": problem " + std::to_string(i) + ": ";
        if (p.n < 0) return fail(at + "negative n");
        if (p.n > 0 && (!p.points2D_0 || !p.points2D_1)) return fail(at + "null points");
        if (!all_finite(p.points2D_0, 2 * (int64_t)p.n) || !all_finite(p.points2D_1, 2 * (int64_t)p.n)) return fail(at + "non-finite points");
        if (!(std::isfinite(p.max_error_px) && p.max_error_px > 0)) return fail(at + "max_error_px must be positive and finite");
        FmProbDev &o = pd[i];
        memset(&o, 0, sizeof(o));
        o.off = total;
        o.n = p.n;
        o.max_error_px = p.max_error_px;
        total += p.n;
    }
    if (total > 0 && !inlier_mask_u8) return fail(F + ": null inlier mask");
    if (k == 0) return 0;
    HIPCHECK(hipSetDevice(c->device));
    const int64_t N = std::max<int64_t>(total, 1);
    Carve ci, cw, co;
    // inputs: problems | points of image 0 | of image 1;  work: normalised points 0 | 1;  out: results | mask
    const size_t o_pd = ci.take(sizeof(FmProbDev) * k), o_p0 = ci.take(16 * N), o_p1 = ci.take(16 * N);
    const size_t o_x0 = cw.take(16 * N), o_x1 = cw.take(16 * N);
    const size_t o_res = co.take(sizeof(FmResDev) * k), o_m = co.take(N);
    HIPCHECK(hipStreamSynchronize(c->stream));              // earlier calls on this stream may still read the buffers
    HIPCHECK(grow(c->fm_in, ci.off));
    HIPCHECK(grow(c->fm_ws, cw.off));
    HIPCHECK(grow(c->fm_out, co.off));
    std::vector<double> p0(2 * (size_t)N), p1(2 * (size_t)N);
    for (int i = 0; i < k; ++i) {
        const int64_t o = pd[i].off, n = pd[i].n;
        if (n) {
            memcpy(p0.data() + 2 * o, problems[i].points2D_0, 16 * n);
            memcpy(p1.data() + 2 * o, problems[i].points2D_1, 16 * n);
        }
    }
    char *in = c->fm_in.as<char>(), *ws = c->fm_ws.as<char>(), *out = c->fm_out.as<char>();
    HIPCHECK(hipMemcpyAsync(in + o_pd, pd.data(), sizeof(FmProbDev) * k, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(in + o_p0, p0.data(), 16 * total, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(in + o_p1, p1.data(), 16 * total, hipMemcpyHostToDevice, c->stream));
    launch(c->stream, at<const FmProbDev>(in, o_pd), k, d, at<const double>(in, o_p0), at<const double>(in, o_p1), at<double2>(ws, o_x0),
           at<double2>(ws, o_x1), at<unsigned char>(out, o_m), at<FmResDev>(out, o_res));
    HIPCHECK(hipGetLastError());
    std::vector<FmResDev> r(k);
    HIPCHECK(hipMemcpyAsync(r.data(), out + o_res, sizeof(FmResDev) * k, hipMemcpyDeviceToHost, c->stream));
    if (total) HIPCHECK(hipMemcpyAsync(inlier_mask_u8, out + o_m, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < k; ++i) {
        sfd2_fundamental_result &o = results[i];
        o.success = r[i].success;
        o.num_inliers = r[i].num_inliers;
        o.num_trials = r[i].num_trials;
        o.reserved = 0;
        for (int j = 0; j < 9; ++j) o.F[j] = r[i].F[j];
    }
    return 0;
}

extern "C" int sfd2_fundamental_batch(sfd2_ctx *c, const sfd2_fundamental_problem *problems, int k, const sfd2_two_view_conf *conf,
                                      sfd2_fundamental_result *results, uint8_t *inlier_mask_u8, int flags)
{
    return pairs_batch("sfd2_fundamental_batch", 7, launch_fundamental, c, problems, k, conf, results, inlier_mask_u8, flags);
}
