// libsfd2hip: sfd2_absolute_pose_batch / sfd2_pose_refine_batch -- checks and packs the problems, one launch of pose_kernels.hip.
#include "sfd2_ctx.h"
#include "api_scratch.h"

namespace {

const char *model_name(int m)
{
    switch (m) {
    case 0: return "SIMPLE_PINHOLE";
    case 1: return "PINHOLE";
    case 2: return "SIMPLE_RADIAL";
    case 3: return "RADIAL";
    case 4: return "OPENCV";
    case 5: return "OPENCV_FISHEYE";
    case 6: return "FULL_OPENCV";
    case 7: return "FOV";
    case 8: return "SIMPLE_RADIAL_FISHEYE";
    case 9: return "RADIAL_FISHEYE";
    case 10: return "THIN_PRISM_FISHEYE";
    default: return "unknown";
    }
}

// COLMAP's camera in the kernels' OPENCV form; false (with the reason) for a model this library does not take
bool to_cam(const sfd2_pose_problem &p, PoseCam &c, double &mean_focal, std::string &why)
{
    memset(&c, 0, sizeof(c));
    const double *q = p.params;
    int np = 0;
    switch (p.model) {
    case SFD2_CAM_SIMPLE_PINHOLE: c.f[0] = c.f[1] = q[0]; c.c[0] = q[1]; c.c[1] = q[2]; np = 3; break;
    case SFD2_CAM_PINHOLE: c.f[0] = q[0]; c.f[1] = q[1]; c.c[0] = q[2]; c.c[1] = q[3]; np = 4; break;
    case SFD2_CAM_SIMPLE_RADIAL: c.f[0] = c.f[1] = q[0]; c.c[0] = q[1]; c.c[1] = q[2]; c.k1 = q[3]; np = 4; break;
    case SFD2_CAM_OPENCV:
        c.f[0] = q[0]; c.f[1] = q[1]; c.c[0] = q[2]; c.c[1] = q[3]; c.k1 = q[4]; c.k2 = q[5]; c.p1 = q[6]; c.p2 = q[7]; np = 8;
        break;
    default:
        why = std::string("camera model ") + std::to_string(p.model) + " (" + model_name(p.model) +
              ") is not supported (SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, OPENCV)";
        return false;
    }
    if (!all_finite(q, np)) { why = "non-finite camera parameters"; return false; }
    if (!(c.f[0] > 0) || !(c.f[1] > 0)) { why = "focal lengths must be positive"; return false; }
    c.distorted = (c.k1 != 0 || c.k2 != 0 || c.p1 != 0 || c.p2 != 0) ? 1 : 0;
    mean_focal = 0.5 * (c.f[0] + c.f[1]);
    return true;
}

// checks the problems and lays them out one behind the other: pd[k], total = their correspondences; -1 with the message
int pack(const std::string &F, const sfd2_pose_problem *problems, int k, const double *qt_in, std::vector<PoseProbDev> &pd, int64_t &total)
{
    pd.resize(k);
    total = 0;
    for (int i = 0; i < k; ++i) {
        const sfd2_pose_problem &p = problems[i];
        const std::string at = F + ": problem " + std::to_string(i) + ": ";
        if (p.n < 0) return fail(at + "negative n");
        if (p.n > 0 && (!p.points2D || !p.points3D)) return fail(at + "null points");
        PoseProbDev &d = pd[i];
        memset(&d, 0, sizeof(d));
        double mf = 0;
        std::string why;
        if (!to_cam(p, d.cam, mf, why)) return fail(at + why);
        if (!all_finite(p.points2D, 2 * (int64_t)p.n) || !all_finite(p.points3D, 3 * (int64_t)p.n)) return fail(at + "non-finite points");
        if (!qt_in && !(std::isfinite(p.max_error_px) && p.max_error_px > 0)) return fail(at + "max_error_px must be positive and finite");
        if (qt_in) {
            if (!all_finite(qt_in + 7 * (int64_t)i, 7)) return fail(at + "non-finite start pose");
            const double *q = qt_in + 7 * (int64_t)i;
            const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            if (!(nq > 0)) return fail(at + "zero quaternion");
            for (int j = 0; j < 4; ++j) d.qt[j] = q[j] / nq;
            for (int j = 4; j < 7; ++j) d.qt[j] = q[j];
        }
        d.thresh2 = qt_in ? 0.0 : (p.max_error_px / mf) * (p.max_error_px / mf);
        d.off = total;
        d.n = p.n;
        total += p.n;
    }
    return 0;
}

// the problems' points, concatenated, to p2d / p3d on the device (host vectors kept by the caller until the stream is synchronised)
hipError_t upload_points(sfd2_ctx *c, const sfd2_pose_problem *problems, const std::vector<PoseProbDev> &pd, int64_t total, std::vector<double> &p2,
                         std::vector<double> &p3, double *p2d, double *p3d)
{
    const int64_t N = std::max<int64_t>(total, 1);
    p2.assign(2 * (size_t)N, 0.0);
    p3.assign(3 * (size_t)N, 0.0);
    for (size_t i = 0; i < pd.size(); ++i) {
        const int64_t o = pd[i].off, n = pd[i].n;
        if (n) {
            memcpy(p2.data() + 2 * o, problems[i].points2D, 16 * n);
            memcpy(p3.data() + 3 * o, problems[i].points3D, 24 * n);
        }
    }
    hipError_t e = hipMemcpyAsync(p2d, p2.data(), 16 * total, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(p3d, p3.data(), 24 * total, hipMemcpyHostToDevice, c->stream);
}

// the device's options: the trial limits of sample size 3 (api_scratch.h), both at most cap
PoseConfDev trial_conf(const sfd2_pose_conf &conf, int64_t cap)
{
    PoseConfDev d;
    memset(&d, 0, sizeof(d));
    const double r = floored_ratio(conf.min_inlier_ratio);
    const TrialLimits t = trial_limits(conf.confidence, conf.min_num_trials, conf.max_num_trials, cap, r * r * r);
    d.max_trials = t.max_trials;
    d.min_trials = t.min_trials;
    d.confidence = conf.confidence;
    d.seed = conf.seed;
    d.refine_only = 0;
    return d;
}

int run(sfd2_ctx *c, const char *fn, const sfd2_pose_problem *problems, int k, const PoseConfDev &conf, const double *qt_in,
        const uint8_t *mask_in, sfd2_pose_result *results, uint8_t *mask_out)
{
    std::vector<PoseProbDev> pd;
    int64_t total = 0;
    if (pack(fn, problems, k, qt_in, pd, total) != 0) return -1;
    if (k == 0) return 0;
    HIPCHECK(hipSetDevice(c->device));
    const int64_t N = std::max<int64_t>(total, 1);
    Carve ci, cw, co;
    // inputs: problems | points2D | points3D | mask
    const size_t o_pd = ci.take(sizeof(PoseProbDev) * k), o_p2 = ci.take(16 * N), o_p3 = ci.take(24 * N), o_m = ci.take(N);
    // work: float4 X | float2 x | double2 x | hypotheses;  out: results | mask
    const size_t o_X = cw.take(16 * N), o_x2 = cw.take(8 * N), o_xn = cw.take(16 * N), o_hyp = cw.take(sizeof(double) * (size_t)k * SFD2_POSE_WG * 4 * 12);
    const size_t o_res = co.take(sizeof(PoseResDev) * k), o_mo = co.take(N);
    HIPCHECK(hipStreamSynchronize(c->stream));              // earlier pose calls on this stream may still read the buffers
    HIPCHECK(grow(c->pose_in, ci.off));
    HIPCHECK(grow(c->pose_ws, cw.off));
    HIPCHECK(grow(c->pose_out, co.off));
    std::vector<double> p2, p3;
    std::vector<uint8_t> m(mask_in ? (size_t)N : 0);
    if (mask_in)
        for (int64_t j = 0; j < total; ++j) m[j] = mask_in[j] ? 1 : 0;
    char *in = c->pose_in.as<char>(), *ws = c->pose_ws.as<char>(), *out = c->pose_out.as<char>();
    HIPCHECK(hipMemcpyAsync(in + o_pd, pd.data(), sizeof(PoseProbDev) * k, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(upload_points(c, problems, pd, total, p2, p3, at<double>(in, o_p2), at<double>(in, o_p3)));
    if (mask_in) HIPCHECK(hipMemcpyAsync(in + o_m, m.data(), total, hipMemcpyHostToDevice, c->stream));
    launch_pose(c->stream, at<const PoseProbDev>(in, o_pd), k, conf, at<const double>(in, o_p2), at<const double>(in, o_p3), at<float4>(ws, o_X),
                at<float2>(ws, o_x2), at<double2>(ws, o_xn), at<double>(ws, o_hyp), at<const unsigned char>(in, o_m), at<unsigned char>(out, o_mo),
                at<PoseResDev>(out, o_res));
    HIPCHECK(hipGetLastError());
    std::vector<PoseResDev> r(k);
    HIPCHECK(hipMemcpyAsync(r.data(), out + o_res, sizeof(PoseResDev) * k, hipMemcpyDeviceToHost, c->stream));
    if (mask_out && total) HIPCHECK(hipMemcpyAsync(mask_out, out + o_mo, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < k; ++i) {
        sfd2_pose_result &o = results[i];
        o.success = r[i].success;
        o.num_inliers = r[i].num_inliers;
        o.num_trials = r[i].num_trials;
        o.reserved = 0;
        for (int j = 0; j < 4; ++j) o.qvec[j] = r[i].q[j];
        for (int j = 0; j < 3; ++j) o.tvec[j] = r[i].t[j];
    }
    return 0;
}

}  // namespace

// the same camera conversion for sfd2_assemble_2d3d's gate (api_assemble.hip)
bool sfd2_pose_cam(int model, const double *params, PoseCam &c, std::string &why)
{
    sfd2_pose_problem p;
    memset(&p, 0, sizeof(p));
    p.model = model;
    memcpy(p.params, params, sizeof(p.params));
    double mf = 0;
    return to_cam(p, c, mf, why);
}

extern "C" int sfd2_absolute_pose_batch(sfd2_ctx *c, const sfd2_pose_problem *problems, int k, const sfd2_pose_conf *conf,
                                        sfd2_pose_result *results, uint8_t *inlier_mask_u8, int flags)
{
    if (!c || !conf || (k > 0 && (!problems || !results))) return fail("sfd2_absolute_pose_batch: null argument");
    if (k < 0) return fail("sfd2_absolute_pose_batch: negative k");
    if (flags != 0) return fail("sfd2_absolute_pose_batch: unknown flags");
    if (const char *bad = ransac_conf_error(conf->confidence, conf->min_inlier_ratio, conf->min_num_trials, conf->max_num_trials))
        return fail(std::string("sfd2_absolute_pose_batch") + bad);
    int64_t total = 0;
    for (int i = 0; i < k; ++i) total += std::max(problems[i].n, 0);
    if (total > 0 && !inlier_mask_u8) return fail("sfd2_absolute_pose_batch: null inlier mask");
    return run(c, "sfd2_absolute_pose_batch", problems, k, trial_conf(*conf, INT64_MAX), nullptr, nullptr, results, inlier_mask_u8);
}

extern "C" int sfd2_pose_refine_batch(sfd2_ctx *c, const sfd2_pose_problem *problems, int k, const double *qvec_tvec_in,
                                      const uint8_t *inlier_mask_u8, sfd2_pose_result *results, int flags)
{
    if (!c || (k > 0 && (!problems || !results || !qvec_tvec_in))) return fail("sfd2_pose_refine_batch: null argument");
    if (k < 0) return fail("sfd2_pose_refine_batch: negative k");
    if (flags != 0) return fail("sfd2_pose_refine_batch: unknown flags");
    int64_t total = 0;
    for (int i = 0; i < k; ++i) total += std::max(problems[i].n, 0);
    if (total > 0 && !inlier_mask_u8) return fail("sfd2_pose_refine_batch: null inlier mask");
    PoseConfDev d;
    memset(&d, 0, sizeof(d));
    d.refine_only = 1;
    return run(c, "sfd2_pose_refine_batch", problems, k, d, qvec_tvec_in, inlier_mask_u8, results, nullptr);
}

// ------------------------------------------------------------------------------------------------ absolute pose, unknown focal
namespace {

int check_focal_conf(const std::string &F, const sfd2_pose_focal_conf *fc)
{
    if (fc->reserved[0] != 0 || fc->reserved[1] != 0) return fail(F + ": reserved words of sfd2_pose_focal_conf must be zero");
    if (fc->num_focal_length_samples < 1 || fc->num_focal_length_samples > SFD2_POSE_FOCAL_MAX_SAMPLES)
        return fail(F + ": num_focal_length_samples must lie in [1, 64]");
    const double lo = fc->min_focal_length_ratio, hi = fc->max_focal_length_ratio;
    if (!(std::isfinite(lo) && std::isfinite(hi) && lo > 0 && lo <= hi))
        return fail(F + ": focal length ratios must be finite with 0 < min_focal_length_ratio <= max_focal_length_ratio");
    if (fc->sweep_max_num_trials < 1) return fail(F + ": sweep_max_num_trials must be at least 1");
    return 0;
}

// the refinement's record of a problem: the focal range, the re-scoring threshold and the parameters its model and the flags select
PoseFocalProbDev focal_prob(const sfd2_pose_problem &p, const PoseCam &given, const sfd2_pose_focal_conf &fc)
{
    PoseFocalProbDev f;
    memset(&f, 0, sizeof(f));
    for (int i = 0; i < 2; ++i) {
        f.f_lo[i] = fc.min_focal_length_ratio * given.f[i];
        f.f_hi[i] = fc.max_focal_length_ratio * given.f[i];
    }
    f.max_err2 = p.max_error_px * p.max_error_px;
    f.single_f = (p.model == SFD2_CAM_SIMPLE_PINHOLE || p.model == SFD2_CAM_SIMPLE_RADIAL) ? 1 : 0;
    f.active = 0x3f;
    if (fc.refine_focal_length) f.active |= f.single_f ? 0x40 : 0xc0;
    if (fc.refine_extra_params) {
        if (p.model == SFD2_CAM_SIMPLE_RADIAL) f.active |= 0x100;
        if (p.model == SFD2_CAM_OPENCV) f.active |= 0xf00;
    }
    return f;
}

void focal_result(const sfd2_pose_problem &p, const PoseFocalResDev &r, sfd2_pose_focal_result &o)
{
    o.success = r.success;
    o.num_inliers = r.num_inliers;
    o.num_trials = r.num_trials;
    o.reserved = 0;
    for (int j = 0; j < 4; ++j) o.qvec[j] = r.q[j];
    for (int j = 0; j < 3; ++j) o.tvec[j] = r.t[j];
    memcpy(o.params, p.params, sizeof(o.params));          // the principal point (and an unused tail) as given
    switch (p.model) {
    case SFD2_CAM_SIMPLE_PINHOLE: o.params[0] = r.f[0]; break;
    case SFD2_CAM_PINHOLE: o.params[0] = r.f[0]; o.params[1] = r.f[1]; break;
    case SFD2_CAM_SIMPLE_RADIAL: o.params[0] = r.f[0]; o.params[3] = r.k[0]; break;
    default: o.params[0] = r.f[0]; o.params[1] = r.f[1]; for (int j = 0; j < 4; ++j) o.params[4 + j] = r.k[j]; break;
    }
    o.focal_sample = -1;
    o.ransac_num_inliers = r.ransac_num_inliers;
    o.focal_factor = 1.0;
}

}  // namespace

extern "C" int sfd2_absolute_pose_focal_batch(sfd2_ctx *c, const sfd2_pose_problem *problems, int k, const sfd2_pose_conf *conf,
                                              const sfd2_pose_focal_conf *fc, sfd2_pose_focal_result *results, uint8_t *inlier_mask_u8,
                                              sfd2_pose_sweep_record *sweep_out, int flags)
{
    const std::string F("sfd2_absolute_pose_focal_batch");
    if (!c || !conf || !fc || (k > 0 && (!problems || !results))) return fail(F + ": null argument");
    if (k < 0) return fail(F + ": negative k");
    if (flags != 0) return fail(F + ": unknown flags");
    if (const char *bad = ransac_conf_error(conf->confidence, conf->min_inlier_ratio, conf->min_num_trials, conf->max_num_trials))
        return fail(F + bad);
    if (check_focal_conf(F, fc) != 0) return -1;
    std::vector<PoseProbDev> pd;
    int64_t total = 0;
    if (pack(F, problems, k, nullptr, pd, total) != 0) return -1;
    if (total > 0 && !inlier_mask_u8) return fail(F + ": null inlier mask");
    if (k == 0) return 0;
    const bool est = fc->estimate_focal_length != 0;
    const int S = fc->num_focal_length_samples, ns = est ? S + 1 : 0, nsw = std::max(ns, 1);
    // the factors from the integer index, and per (problem, sample) the focal lengths and the threshold: one rounding each, the words a
    // caller gets who multiplies the camera's focal parameters by the factor and hands it to sfd2_absolute_pose_batch
    std::vector<double> factor(ns);
    for (int i = 0; i < ns; ++i) {
        const double t = (double)i / (double)S;
        const double tt = t * t;
        const double span = fc->max_focal_length_ratio - fc->min_focal_length_ratio;
        const double st = span * tt;
        factor[i] = fc->min_focal_length_ratio + st;
    }
    std::vector<PoseFocalTabDev> tab((size_t)k * ns);
    std::vector<PoseFocalProbDev> fp(k);
    for (int i = 0; i < k; ++i) {
        fp[i] = focal_prob(problems[i], pd[i].cam, *fc);
        for (int s = 0; s < ns; ++s) {
            PoseFocalTabDev &t = tab[(size_t)i * ns + s];
            memset(&t, 0, sizeof(t));
            t.f[0] = pd[i].cam.f[0] * factor[s];
            t.f[1] = pd[i].cam.f[1] * factor[s];
            const double sum = t.f[0] + t.f[1];
            const double mf = 0.5 * sum;
            if (!(std::isfinite(mf) && t.f[0] > 0 && t.f[1] > 0))
                return fail(F + ": problem " + std::to_string(i) + ": focal sample " + std::to_string(s) + " is not a positive finite focal length");
            const double e = problems[i].max_error_px / mf;
            t.thresh2 = e * e;
            t.fm = (float)mf;
        }
    }
    HIPCHECK(hipSetDevice(c->device));
    const int64_t N = std::max<int64_t>(total, 1);
    Carve ci, cw, co;
    const size_t o_pd = ci.take(sizeof(PoseProbDev) * k), o_p2 = ci.take(16 * N), o_p3 = ci.take(24 * N),
                 o_tab = ci.take(sizeof(PoseFocalTabDev) * tab.size()), o_fp = ci.take(sizeof(PoseFocalProbDev) * k);
    // the hypotheses are 96 KiB per workgroup: the sweep runs in launches of `chunk` problems that share one block of at most 256 MiB
    const size_t hyp_wg = sizeof(double) * SFD2_POSE_WG * 4 * 12;
    const int chunk = est ? (int)std::max<size_t>(1, std::min<size_t>((size_t)k, ((size_t)256 << 20) / (hyp_wg * nsw))) : k;
    const size_t o_X = cw.take(16 * N * nsw), o_x2 = cw.take(8 * N * nsw), o_xn = cw.take(16 * N * nsw),
                 o_hyp = cw.take(hyp_wg * std::max<size_t>((size_t)chunk * nsw, (size_t)k)), o_mp = cw.take(sizeof(PoseProbDev) * k),
                 o_mn = cw.take(N), o_un = cw.take(sizeof(PoseResDev) * (size_t)chunk * nsw);
    const size_t o_res = co.take(sizeof(PoseResDev) * k), o_mo = co.take(N), o_sw = co.take(sizeof(PoseSweepDev) * tab.size()),
                 o_sel = co.take(sizeof(int32_t) * k), o_fr = co.take(sizeof(PoseFocalResDev) * k);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->pose_in, ci.off));
    HIPCHECK(grow(c->pose_ws, cw.off));
    HIPCHECK(grow(c->pose_out, co.off));
    char *in = c->pose_in.as<char>(), *ws = c->pose_ws.as<char>(), *out = c->pose_out.as<char>();
    std::vector<double> p2, p3;
    HIPCHECK(hipMemcpyAsync(in + o_pd, pd.data(), sizeof(PoseProbDev) * k, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(upload_points(c, problems, pd, total, p2, p3, at<double>(in, o_p2), at<double>(in, o_p3)));
    HIPCHECK(hipMemcpyAsync(in + o_fp, fp.data(), sizeof(PoseFocalProbDev) * k, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemsetAsync(out + o_mo, 0, N, c->stream));
    const PoseProbDev *main_probs = at<const PoseProbDev>(in, o_pd);
    if (est) {
        HIPCHECK(hipMemcpyAsync(in + o_tab, tab.data(), sizeof(PoseFocalTabDev) * tab.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemsetAsync(out + o_sw, 0, sizeof(PoseSweepDev) * tab.size(), c->stream));
        const PoseConfDev sweep_conf = trial_conf(*conf, fc->sweep_max_num_trials);
        for (int p0 = 0; p0 < k; p0 += chunk)                   // (a problem's result does not depend on its batch: DESIGN.md 9)
            launch_pose_sweep(c->stream, at<const PoseProbDev>(in, o_pd) + p0, std::min(chunk, k - p0), at<const PoseFocalTabDev>(in, o_tab) + (size_t)p0 * ns,
                              ns, sweep_conf, at<const double>(in, o_p2), at<const double>(in, o_p3), at<float4>(ws, o_X), at<float2>(ws, o_x2),
                              at<double2>(ws, o_xn), at<double>(ws, o_hyp), N, at<PoseResDev>(ws, o_un), at<PoseSweepDev>(out, o_sw) + (size_t)p0 * ns);
        HIPCHECK(hipGetLastError());
        launch_pose_focal_select(c->stream, at<const PoseProbDev>(in, o_pd), k, at<const PoseFocalTabDev>(in, o_tab), ns,
                                 at<const PoseSweepDev>(out, o_sw), at<PoseProbDev>(ws, o_mp), at<int32_t>(out, o_sel));
        HIPCHECK(hipGetLastError());
        main_probs = at<const PoseProbDev>(ws, o_mp);
    }
    launch_pose(c->stream, main_probs, k, trial_conf(*conf, INT64_MAX), at<const double>(in, o_p2), at<const double>(in, o_p3), at<float4>(ws, o_X),
                at<float2>(ws, o_x2), at<double2>(ws, o_xn), at<double>(ws, o_hyp), nullptr, at<unsigned char>(out, o_mo), at<PoseResDev>(out, o_res));
    HIPCHECK(hipGetLastError());
    PoseFocalConfDev rc;
    rc.rounds = (fc->refine_focal_length || fc->refine_extra_params) ? 3 : 0;
    rc.start_from_res = 1;
    launch_pose_cam_refine(c->stream, main_probs, at<const PoseFocalProbDev>(in, o_fp), k, rc, at<const double>(in, o_p2), at<const double>(in, o_p3),
                           at<const PoseResDev>(out, o_res), at<unsigned char>(out, o_mo), at<unsigned char>(ws, o_mn), at<PoseFocalResDev>(out, o_fr));
    HIPCHECK(hipGetLastError());
    std::vector<PoseFocalResDev> r(k);
    std::vector<int32_t> sel(k, -1);
    HIPCHECK(hipMemcpyAsync(r.data(), out + o_fr, sizeof(PoseFocalResDev) * k, hipMemcpyDeviceToHost, c->stream));
    if (est) HIPCHECK(hipMemcpyAsync(sel.data(), out + o_sel, sizeof(int32_t) * k, hipMemcpyDeviceToHost, c->stream));
    if (est && sweep_out) {
        static_assert(sizeof(sfd2_pose_sweep_record) == sizeof(PoseSweepDev), "the sweep record is copied as it is");
        HIPCHECK(hipMemcpyAsync(sweep_out, out + o_sw, sizeof(PoseSweepDev) * tab.size(), hipMemcpyDeviceToHost, c->stream));
    }
    if (total) HIPCHECK(hipMemcpyAsync(inlier_mask_u8, out + o_mo, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < k; ++i) {
        focal_result(problems[i], r[i], results[i]);
        if (est) {
            results[i].focal_sample = sel[i];
            if (sel[i] >= 0 && sel[i] < ns) results[i].focal_factor = factor[sel[i]];
        }
    }
    return 0;
}

extern "C" int sfd2_pose_refine_camera_batch(sfd2_ctx *c, const sfd2_pose_problem *problems, int k, const double *qvec_tvec_in,
                                             const uint8_t *inlier_mask_u8, const sfd2_pose_focal_conf *fc, sfd2_pose_focal_result *results,
                                             int flags)
{
    const std::string F("sfd2_pose_refine_camera_batch");
    if (!c || !fc || (k > 0 && (!problems || !results || !qvec_tvec_in))) return fail(F + ": null argument");
    if (k < 0) return fail(F + ": negative k");
    if (flags != 0) return fail(F + ": unknown flags");
    if (check_focal_conf(F, fc) != 0) return -1;
    std::vector<PoseProbDev> pd;
    int64_t total = 0;
    if (pack(F, problems, k, qvec_tvec_in, pd, total) != 0) return -1;
    if (total > 0 && !inlier_mask_u8) return fail(F + ": null inlier mask");
    if (k == 0) return 0;
    std::vector<PoseFocalProbDev> fp(k);
    for (int i = 0; i < k; ++i) fp[i] = focal_prob(problems[i], pd[i].cam, *fc);
    HIPCHECK(hipSetDevice(c->device));
    const int64_t N = std::max<int64_t>(total, 1);
    Carve ci, cw, co;
    const size_t o_pd = ci.take(sizeof(PoseProbDev) * k), o_p2 = ci.take(16 * N), o_p3 = ci.take(24 * N), o_fp = ci.take(sizeof(PoseFocalProbDev) * k);
    const size_t o_m = cw.take(N), o_mn = cw.take(N);
    const size_t o_fr = co.take(sizeof(PoseFocalResDev) * k);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->pose_in, ci.off));
    HIPCHECK(grow(c->pose_ws, cw.off));
    HIPCHECK(grow(c->pose_out, co.off));
    char *in = c->pose_in.as<char>(), *ws = c->pose_ws.as<char>(), *out = c->pose_out.as<char>();
    std::vector<double> p2, p3;
    std::vector<uint8_t> m((size_t)N, 0);
    for (int64_t j = 0; j < total; ++j) m[j] = inlier_mask_u8[j] ? 1 : 0;
    HIPCHECK(hipMemcpyAsync(in + o_pd, pd.data(), sizeof(PoseProbDev) * k, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(upload_points(c, problems, pd, total, p2, p3, at<double>(in, o_p2), at<double>(in, o_p3)));
    HIPCHECK(hipMemcpyAsync(in + o_fp, fp.data(), sizeof(PoseFocalProbDev) * k, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(ws + o_m, m.data(), N, hipMemcpyHostToDevice, c->stream));
    PoseFocalConfDev rc;
    rc.rounds = 1;
    rc.start_from_res = 0;
    launch_pose_cam_refine(c->stream, at<const PoseProbDev>(in, o_pd), at<const PoseFocalProbDev>(in, o_fp), k, rc, at<const double>(in, o_p2),
                           at<const double>(in, o_p3), nullptr, at<unsigned char>(ws, o_m), at<unsigned char>(ws, o_mn), at<PoseFocalResDev>(out, o_fr));
    HIPCHECK(hipGetLastError());
    std::vector<PoseFocalResDev> r(k);
    HIPCHECK(hipMemcpyAsync(r.data(), out + o_fr, sizeof(PoseFocalResDev) * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < k; ++i) focal_result(problems[i], r[i], results[i]);
    return 0;
}
