// libsfd2hip: sfd2_bundle_adjust -- checks and packs the inputs, builds the by-view CSR, and drives the Levenberg-Marquardt loop of
// bundle_kernels.hip on the context's stream.  The accept / reject decision is taken on the device, so the host
// reads the state block once per LM iteration and once per batch of PCG iterations.
#include "sfd2_ctx.h"
#include "api_scratch.h"
#include "pose_camera.h"
#include "bundle.h"

namespace {

template <typename T> int64_t first_nonfinite(const T *p, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return i;
    return n;
}

}  // namespace

extern "C" int sfd2_bundle_adjust(sfd2_ctx *c, sfd2_tri_view *views, int n_views, const uint8_t *view_constant, double *xyz, int n_points,
                                  const uint8_t *point_constant, const int64_t *point_offsets, const int32_t *obs_view, const double *obs_xy,
                                  const sfd2_ba_conf *conf, sfd2_ba_result *result, double *obs_error, int flags)
{
    const std::string F("sfd2_bundle_adjust: ");
    if (!c || !views || !view_constant || !point_offsets || !conf || !result || (n_points > 0 && (!xyz || !point_constant))) return fail(F + "null argument");
    if (n_views < 1 || n_points < 0) return fail(F + "n_views must be positive and n_points non-negative");
    if (flags & ~(SFD2_BA_FLAG_POINT_LANE | SFD2_BA_FLAG_POINT_WAVE) || flags == (SFD2_BA_FLAG_POINT_LANE | SFD2_BA_FLAG_POINT_WAVE))
        return fail(F + "unknown flags (at most one of SFD2_BA_FLAG_POINT_LANE, SFD2_BA_FLAG_POINT_WAVE)");
    if (conf->max_iterations < 0 || conf->max_iterations > 100000 || conf->pcg_max_iterations < 1 || conf->pcg_max_iterations > 1000000 || conf->pcg_batch < 0 ||
        conf->pcg_batch > 4096)
        return fail(F + "0 <= max_iterations <= 100000, 1 <= pcg_max_iterations <= 1000000, 0 <= pcg_batch <= 4096");
    if (!(conf->gradient_tolerance >= 0) || !(conf->function_tolerance >= 0) || !(conf->pcg_tolerance >= 0) || !std::isfinite(conf->gradient_tolerance) ||
        !std::isfinite(conf->function_tolerance) || !std::isfinite(conf->pcg_tolerance))
        return fail(F + "the tolerances must be finite and non-negative");
    if (!(conf->initial_lambda > 0) || !std::isfinite(conf->initial_lambda)) return fail(F + "initial_lambda must be positive and finite");
    if (conf->loss != SFD2_BA_LOSS_TRIVIAL && conf->loss != SFD2_BA_LOSS_CAUCHY) return fail(F + "loss must be SFD2_BA_LOSS_TRIVIAL or SFD2_BA_LOSS_CAUCHY");
    if (conf->loss == SFD2_BA_LOSS_CAUCHY && (!(conf->loss_scale > 0) || !std::isfinite(conf->loss_scale))) return fail(F + "loss_scale must be positive and finite");
    if (conf->reserved[0] || conf->reserved[1] || conf->reserved[2] || conf->reserved[3]) return fail(F + "reserved words must be zero");
    if (!monotone(point_offsets, n_points)) return fail(F + "point_offsets must start at 0 and not decrease");
    const int64_t O = point_offsets[n_points];
    if (O > 0x7fffffffLL) return fail(F + "more than 2^31 - 1 observations");
    if (O > 0 && (!obs_view || !obs_xy || !obs_error)) return fail(F + "null observations");
    if (const int64_t o = first_outside(obs_view, O, n_views); o < O) return fail(F + "observation " + std::to_string(o) + ": view index out of range");
    if (!all_finite(obs_xy, 2 * O)) return fail(F + "observation " + std::to_string(first_nonfinite(obs_xy, 2 * O) / 2) + ": non-finite coordinates");
    if (!all_finite(xyz, 3 * (int64_t)n_points)) return fail(F + "point " + std::to_string(first_nonfinite(xyz, 3 * (int64_t)n_points) / 3) + ": non-finite coordinates");

    const size_t nv = (size_t)n_views, np = (size_t)n_points, no = (size_t)O;
    std::vector<PoseCam> cams(nv);
    std::vector<double> pose(12 * nv);
    for (int i = 0; i < n_views; ++i) {
        std::string w;
        memset(&cams[i], 0, sizeof(PoseCam));
        if (!sfd2_pose_cam(views[i].model, views[i].params, cams[i], w)) return fail(F + "view " + std::to_string(i) + ": " + w);
        const double *q = views[i].qvec;
        const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (!all_finite(q, 4) || !all_finite(views[i].tvec, 3) || !(nq > 0))
            return fail(F + "view " + std::to_string(i) + ": the pose must be finite with a non-zero quaternion");
        quat_to_rot(q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq, &pose[12 * (size_t)i]);
        for (int a = 0; a < 3; ++a) pose[12 * (size_t)i + 9 + a] = views[i].tvec[a];
    }
    // the by-view CSR by a stable counting sort: a view's observations in ascending index; the point of every observation
    std::vector<int64_t> view_off(nv + 1, 0);
    std::vector<int32_t> view_obs(std::max<size_t>(no, 1)), obs_pt(std::max<size_t>(no, 1));
    for (size_t o = 0; o < no; ++o) ++view_off[(size_t)obs_view[o] + 1];
    for (size_t v = 0; v < nv; ++v) view_off[v + 1] += view_off[v];
    {
        std::vector<int64_t> fill(view_off.begin(), view_off.end() - 1);
        for (size_t o = 0; o < no; ++o) view_obs[(size_t)fill[(size_t)obs_view[o]]++] = (int32_t)o;
    }
    // points by mapping: a lane each up to SFD2_BA_LONG_TRACK observations, beyond that a wave each (the flags force either side)
    std::vector<int32_t> short_ids, long_ids;
    for (int j = 0; j < n_points; ++j) {
        const int64_t len = point_offsets[j + 1] - point_offsets[j];
        for (int64_t o = point_offsets[j]; o < point_offsets[j + 1]; ++o) obs_pt[(size_t)o] = j;
        const bool wave = (flags & SFD2_BA_FLAG_POINT_WAVE) || (!(flags & SFD2_BA_FLAG_POINT_LANE) && len > SFD2_BA_LONG_TRACK);
        (wave ? long_ids : short_ids).push_back(j);
    }

    HIPCHECK(hipSetDevice(c->device));
    Carve in, ws;
    const size_t o_cam = in.take(sizeof(PoseCam) * nv), o_vc = in.take(nv), o_pc = in.take(np), o_po = in.take(8 * (np + 1)), o_ov = in.take(4 * no),
                 o_op = in.take(4 * no), o_xy = in.take(16 * no), o_vo = in.take(8 * (nv + 1)), o_vb = in.take(4 * no), o_sh = in.take(4 * short_ids.size()),
                 o_lg = in.take(4 * long_ids.size());
    const size_t nred = (std::max(std::max(no, 3 * np), 6 * nv) + SFD2_BA_RED_CHUNK - 1) / SFD2_BA_RED_CHUNK + 1;
    const size_t o_st = ws.take(sizeof(BaState)), o_pose = ws.take(96 * nv), o_poset = ws.take(96 * nv), o_xyz = ws.take(24 * np), o_xyzt = ws.take(24 * np),
                 o_rec = ws.take(8 * SFD2_BA_REC * no), o_err = ws.take(8 * no), o_oc = ws.take(8 * no), o_V = ws.take(48 * np), o_gp = ws.take(24 * np),
                 o_Vi = ws.take(48 * np), o_zg = ws.take(24 * np), o_z = ws.take(24 * np), o_B = ws.take(288 * nv), o_gc = ws.take(48 * nv),
                 o_Mi = ws.take(288 * nv), o_Dd = ws.take(48 * nv), o_b = ws.take(48 * nv), o_x = ws.take(48 * nv), o_r = ws.take(48 * nv),
                 o_zz = ws.take(48 * nv), o_p = ws.take(48 * nv), o_q = ws.take(48 * nv), o_part = ws.take(8 * nred);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->ba_in, in.off));
    HIPCHECK(grow(c->ba_ws, ws.off));
    char *di = c->ba_in.as<char>(), *dw = c->ba_ws.as<char>();
    hipStream_t s = c->stream;
    HIPCHECK(hipMemcpyAsync(di + o_cam, cams.data(), sizeof(PoseCam) * nv, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_vc, view_constant, nv, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_po, point_offsets, 8 * (np + 1), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(di + o_vo, view_off.data(), 8 * (nv + 1), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(dw + o_pose, pose.data(), 96 * nv, hipMemcpyHostToDevice, s));
    if (np) {
        HIPCHECK(hipMemcpyAsync(di + o_pc, point_constant, np, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(dw + o_xyz, xyz, 24 * np, hipMemcpyHostToDevice, s));
    }
    if (no) {
        HIPCHECK(hipMemcpyAsync(di + o_ov, obs_view, 4 * no, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(di + o_op, obs_pt.data(), 4 * no, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(di + o_xy, obs_xy, 16 * no, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(di + o_vb, view_obs.data(), 4 * no, hipMemcpyHostToDevice, s));
    }
    if (!short_ids.empty()) HIPCHECK(hipMemcpyAsync(di + o_sh, short_ids.data(), 4 * short_ids.size(), hipMemcpyHostToDevice, s));
    if (!long_ids.empty()) HIPCHECK(hipMemcpyAsync(di + o_lg, long_ids.data(), 4 * long_ids.size(), hipMemcpyHostToDevice, s));
    BaState hs;
    memset(&hs, 0, sizeof(hs));
    hs.lambda = conf->initial_lambda;
    hs.accepted = 1;
    HIPCHECK(hipMemcpyAsync(dw + o_st, &hs, sizeof(hs), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(dw + o_oc, 0, std::max<size_t>(8 * no, 1), s));

    BaPtrs P;
    memset(&P, 0, sizeof(P));
    P.st = at<BaState>(dw, o_st);
    P.cams = at<const PoseCam>(di, o_cam);
    P.vconst = at<const unsigned char>(di, o_vc);
    P.pconst = at<const unsigned char>(di, o_pc);
    P.pt_off = at<const int64_t>(di, o_po);
    P.obs_view = at<const int32_t>(di, o_ov);
    P.obs_pt = at<const int32_t>(di, o_op);
    P.obs_xy = at<const double2>(di, o_xy);
    P.view_off = at<const int64_t>(di, o_vo);
    P.view_obs = at<const int32_t>(di, o_vb);
    P.short_ids = at<const int32_t>(di, o_sh);
    P.long_ids = at<const int32_t>(di, o_lg);
    P.pose = at<double>(dw, o_pose); P.pose_trial = at<double>(dw, o_poset);
    P.xyz = at<double>(dw, o_xyz); P.xyz_trial = at<double>(dw, o_xyzt);
    P.rec = at<double>(dw, o_rec); P.err = at<double>(dw, o_err); P.obs_cost = at<double>(dw, o_oc);
    P.V = at<double>(dw, o_V); P.gp = at<double>(dw, o_gp); P.Vinv = at<double>(dw, o_Vi); P.zg = at<double>(dw, o_zg); P.z = at<double>(dw, o_z);
    P.B = at<double>(dw, o_B); P.gc = at<double>(dw, o_gc); P.Minv = at<double>(dw, o_Mi); P.Dd = at<double>(dw, o_Dd);
    P.b = at<double>(dw, o_b); P.x = at<double>(dw, o_x); P.r = at<double>(dw, o_r); P.zz = at<double>(dw, o_zz); P.p = at<double>(dw, o_p);
    P.q = at<double>(dw, o_q);
    P.partial = at<double>(dw, o_part);
    P.nv = n_views; P.np = n_points; P.n_short = (int)short_ids.size(); P.n_long = (int)long_ids.size();
    P.no = O;

    const double c2 = conf->loss == SFD2_BA_LOSS_CAUCHY ? conf->loss_scale * conf->loss_scale : 1.0;
    // the state's Jacobians, blocks, gradients and max |g|: behind the start (gate none) or behind an accepted step
    auto relinearise = [&](int gate) {
        launch_ba_linearise(s, P, gate, true, false, conf->loss, c2);
        launch_ba_point_build(s, P, gate);
        launch_ba_view_build(s, P, gate);
        launch_ba_reduce(s, P, gate, P.gc, 6 * (int64_t)nv, SFD2_BA_OP_ABSMAX, &P.st->gmax, false);
        if (np) launch_ba_reduce(s, P, gate, P.gp, 3 * (int64_t)np, SFD2_BA_OP_ABSMAX, &P.st->gmax, true);
    };
    auto read_state = [&]() -> hipError_t {
        hipError_t e = hipMemcpyAsync(&hs, P.st, sizeof(hs), hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipStreamSynchronize(s);
    };

    memset(result, 0, sizeof(*result));
    {
        ProfScope ps(c, "bundle_adjust", "ba_linearise+build", 0.0, 8.0 * SFD2_BA_REC * (double)no);
        launch_ba_linearise(s, P, SFD2_BA_GATE_NONE, false, false, conf->loss, c2);
        launch_ba_reduce(s, P, SFD2_BA_GATE_NONE, P.obs_cost, O, SFD2_BA_OP_SUM, &P.st->cost, false);
        relinearise(SFD2_BA_GATE_NONE);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(read_state());
    result->initial_cost = result->final_cost = hs.cost;
    result->gradient_max = hs.gmax;
    result->lambda = hs.lambda;
    if (!std::isfinite(hs.cost)) {                           // nothing is written
        result->status = SFD2_BA_ST_NONFINITE;
        return 0;
    }
    const int batch = conf->pcg_batch ? conf->pcg_batch : 16;
    const double tol2 = conf->pcg_tolerance * conf->pcg_tolerance;
    int status = SFD2_BA_ST_MAX_ITERATIONS, iters = 0;
    int64_t pcg_total = 0;
    while (true) {
        if (hs.gmax <= conf->gradient_tolerance) { status = SFD2_BA_ST_GRADIENT; break; }
        if (hs.lambda > 1e12) { status = SFD2_BA_ST_LAMBDA; break; }
        if (iters >= conf->max_iterations) break;
        launch_ba_point_invert(s, P);
        launch_ba_view_precond(s, P);
        launch_ba_view_apply(s, P, SFD2_BA_GATE_NONE, true);
        launch_ba_pcg_init(s, P);
        for (int k = 0; k < conf->pcg_max_iterations;) {
            for (int e = std::min(conf->pcg_max_iterations, k + batch); k < e; ++k) {
                launch_ba_point_apply(s, P, SFD2_BA_GATE_PCG, P.p);
                launch_ba_view_apply(s, P, SFD2_BA_GATE_PCG, false);
                launch_ba_pcg_step(s, P, tol2, conf->pcg_max_iterations);
            }
            HIPCHECK(read_state());
            if (hs.pcg_done) break;
        }
        pcg_total += hs.pcg_iters;
        launch_ba_point_apply(s, P, SFD2_BA_GATE_NONE, P.x);
        launch_ba_update(s, P);
        launch_ba_linearise(s, P, SFD2_BA_GATE_NONE, false, true, conf->loss, c2);
        launch_ba_reduce(s, P, SFD2_BA_GATE_NONE, P.obs_cost, O, SFD2_BA_OP_SUM, &P.st->trial_cost, false);
        launch_ba_decide_commit(s, P);
        relinearise(SFD2_BA_GATE_ACCEPTED);
        HIPCHECK(hipGetLastError());
        HIPCHECK(read_state());
        ++iters;
        if (hs.accepted && std::fabs(hs.prev_cost - hs.cost) <= conf->function_tolerance * hs.prev_cost) { status = SFD2_BA_ST_FUNCTION; break; }
    }
    result->status = status;
    result->iterations = iters;
    result->accepted_steps = hs.n_accepted;
    result->pcg_iterations = (int32_t)std::min<int64_t>(pcg_total, 0x7fffffff);
    result->final_cost = hs.cost;
    result->gradient_max = hs.gmax;
    result->lambda = hs.lambda;
    HIPCHECK(hipMemcpyAsync(pose.data(), P.pose, 96 * nv, hipMemcpyDeviceToHost, s));
    if (np) HIPCHECK(hipMemcpyAsync(xyz, P.xyz, 24 * np, hipMemcpyDeviceToHost, s));
    if (no) HIPCHECK(hipMemcpyAsync(obs_error, P.err, 8 * no, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    for (int i = 0; i < n_views; ++i) {                      // a constant or unobserved view keeps its words as they came
        if (view_constant[i] || view_off[(size_t)i + 1] == view_off[(size_t)i] || hs.n_accepted == 0) continue;
        rot_to_quat(&pose[12 * (size_t)i], views[i].qvec);
        for (int a = 0; a < 3; ++a) views[i].tvec[a] = pose[12 * (size_t)i + 9 + a];
    }
    return 0;
}
