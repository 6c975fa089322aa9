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

// COLMAP ComputeNumTrials (sample size 3, dyn_num_trials_multiplier 3)
double num_trials(double inlier_ratio, double confidence)
{
    const double nom = 1.0 - confidence;
    if (nom <= 0) return 1e300;
    const double den = 1.0 - inlier_ratio * inlier_ratio * inlier_ratio;
    if (den <= 0) return 1.0;
    if (den == 1.0 || std::fabs(std::log(den)) < 1e-16) return 1e300;
    return std::ceil(std::log(nom) / std::log(den) * 3.0);
}

int run(sfd2_ctx *c, const char *fn, const sfd2_pose_problem *problems, int k, const PoseConfDev &conf, const double *qt_in,
        const uint8_t *mask_in, sfd2_pose_result *results, uint8_t *mask_out)
{
    const std::string F(fn);
    std::vector<PoseProbDev> pd(k);
    int64_t total = 0;
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
    std::vector<double> p2(2 * (size_t)N), p3(3 * (size_t)N);
    std::vector<uint8_t> m(mask_in ? (size_t)N : 0);
    for (int i = 0; i < k; ++i) {
        const int64_t o = pd[i].off, n = pd[i].n;
        if (n) {
            memcpy(p2.data() + 2 * o, problems[i].points2D, 16 * n);
            memcpy(p3.data() + 3 * o, problems[i].points3D, 24 * n);
        }
        if (mask_in)
            for (int64_t j = 0; j < n; ++j) m[o + j] = mask_in[o + j] ? 1 : 0;
    }
    char *in = c->pose_in.as<char>(), *ws = c->pose_ws.as<char>(), *out = c->pose_out.as<char>();
    HIPCHECK(hipMemcpyAsync(in + o_pd, pd.data(), sizeof(PoseProbDev) * k, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(in + o_p2, p2.data(), 16 * total, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(in + o_p3, p3.data(), 24 * total, hipMemcpyHostToDevice, c->stream));
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
    if (!(conf->confidence >= 0 && conf->confidence <= 1) || !(conf->min_inlier_ratio >= 0 && conf->min_inlier_ratio <= 1))
        return fail("sfd2_absolute_pose_batch: confidence and min_inlier_ratio must lie in [0, 1]");
    if (conf->max_num_trials < 1 || conf->max_num_trials > 1000000000 || conf->min_num_trials < 0)
        return fail("sfd2_absolute_pose_batch: trial limits out of range (1 <= max_num_trials <= 1e9, min_num_trials >= 0)");
    int64_t total = 0;
    for (int i = 0; i < k; ++i) total += std::max(problems[i].n, 0);
    if (total > 0 && !inlier_mask_u8) return fail("sfd2_absolute_pose_batch: null inlier mask");
    PoseConfDev d;
    memset(&d, 0, sizeof(d));
    // COLMAP's RANSAC: max_num_trials limited by the trial count of an assumed min_inlier_ratio (kNumSamples = 100000)
    const double dyn = num_trials(std::floor(conf->min_inlier_ratio * 100000) / 100000.0, conf->confidence);
    d.max_trials = std::max<int64_t>(1, std::min<double>((double)conf->max_num_trials, dyn));
    d.min_trials = std::min(conf->min_num_trials, d.max_trials);
    d.confidence = conf->confidence;
    d.seed = conf->seed;
    d.refine_only = 0;
    return run(c, "sfd2_absolute_pose_batch", problems, k, d, nullptr, nullptr, results, inlier_mask_u8);
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
