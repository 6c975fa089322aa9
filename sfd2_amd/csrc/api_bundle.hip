// libsfd2hip: sfd2_bundle_adjust and sfd2_bundle_adjust_cameras -- check and pack the inputs, build the by-view CSR, and drive the
// Levenberg-Marquardt loop of bundle_kernels.hip on the context's stream.  The accept / reject decision is taken on
// the device, so the host reads the state block once per LM iteration and once per batch of PCG iterations.  With cameras among the
// unknowns (section 20) the same loop queues the passes of bundle_cam_kernels.hip where a pass has to know about them.  With
// conf->solver = SFD2_BA_SOLVER_DENSE (section 21) the conjugate gradients give way to bundle_dense_kernels.hip: the pair list is built
// once per call (integer kernels and rocPRIM's stable radix sort), S is formed, factored and solved per step; sfd2_spd_solve runs the same
// factor and solve kernels on a caller's matrix.
#include "sfd2_ctx.h"
#include "api_scratch.h"
#include "pose_camera.h"
#include "bundle_cam.h"
#include <rocprim/rocprim.hpp>

namespace {

template <typename T> int64_t first_nonfinite(const T *p, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return i;
    return n;
}

// the active parameters of a camera: (SFD2_BA_SLOT_*, index into the model's COLMAP parameters) each, in COLMAP order
int cam_slots(int model, int refine, int32_t slot[SFD2_BA_CAM_K], int param[SFD2_BA_CAM_K])
{
    int k = 0;
    auto add = [&](int s, int p) { slot[k] = s; param[k] = p; ++k; };
    const bool simple = model == SFD2_CAM_SIMPLE_PINHOLE || model == SFD2_CAM_SIMPLE_RADIAL;
    const int pp = simple ? 1 : 2;                           // where cx stands
    if (refine & SFD2_BA_REFINE_FOCAL) {
        if (simple) add(SFD2_BA_SLOT_F, 0);
        else { add(SFD2_BA_SLOT_FX, 0); add(SFD2_BA_SLOT_FY, 1); }
    }
    if (refine & SFD2_BA_REFINE_PRINCIPAL) { add(SFD2_BA_SLOT_CX, pp); add(SFD2_BA_SLOT_CY, pp + 1); }
    if (refine & SFD2_BA_REFINE_EXTRA) {
        if (model == SFD2_CAM_SIMPLE_RADIAL) add(SFD2_BA_SLOT_K1, 3);
        if (model == SFD2_CAM_OPENCV) { add(SFD2_BA_SLOT_K1, 4); add(SFD2_BA_SLOT_K2, 5); add(SFD2_BA_SLOT_P1, 6); add(SFD2_BA_SLOT_P2, 7); }
    }
    const int n = k;
    for (; k < SFD2_BA_CAM_K; ++k) { slot[k] = SFD2_BA_SLOT_NONE; param[k] = -1; }
    return n;
}

double cam_word(const PoseCam &c, int slot)
{
    switch (slot) {
    case SFD2_BA_SLOT_F: case SFD2_BA_SLOT_FX: return c.f[0];
    case SFD2_BA_SLOT_FY: return c.f[1];
    case SFD2_BA_SLOT_CX: return c.c[0];
    case SFD2_BA_SLOT_CY: return c.c[1];
    case SFD2_BA_SLOT_K1: return c.k1;
    case SFD2_BA_SLOT_K2: return c.k2;
    case SFD2_BA_SLOT_P1: return c.p1;
    default: return c.p2;
    }
}

// cameras == nullptr: sfd2_bundle_adjust, every view with the constant camera of its own words
int ba_run(sfd2_ctx *c, const std::string &F, sfd2_ba_camera *cameras, int n_cameras, const int32_t *view_camera, sfd2_tri_view *views, int n_views,
           const uint8_t *view_constant, double *xyz, int n_points, const uint8_t *point_constant, const int64_t *point_offsets, const int32_t *obs_view,
           const double *obs_xy, const sfd2_ba_conf *conf, sfd2_ba_result *result, double *obs_error, int flags)
{
    const bool CAM = cameras != nullptr;
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
    if (conf->solver != SFD2_BA_SOLVER_PCG && conf->solver != SFD2_BA_SOLVER_DENSE) return fail(F + "solver must be SFD2_BA_SOLVER_PCG or SFD2_BA_SOLVER_DENSE");
    if (conf->reserved[0] || conf->reserved[1] || conf->reserved[2]) return fail(F + "reserved words must be zero");
    const bool DENSE = conf->solver == SFD2_BA_SOLVER_DENSE;
    if (DENSE && CAM) return fail(F + "the dense solver does not take camera intrinsics among the unknowns: solver must be SFD2_BA_SOLVER_PCG");
    if (DENSE && n_views > SFD2_BA_DENSE_MAX_VIEWS)
        return fail(F + "the dense solver takes at most SFD2_BA_DENSE_MAX_VIEWS = " + std::to_string(SFD2_BA_DENSE_MAX_VIEWS) + " views, got " + std::to_string(n_views));
    if (!monotone(point_offsets, n_points)) return fail(F + "point_offsets must start at 0 and not decrease");
    const int64_t O = point_offsets[n_points];
    if (O > 0x7fffffffLL) return fail(F + "more than 2^31 - 1 observations");
    if (O > 0 && (!obs_view || !obs_xy || !obs_error)) return fail(F + "null observations");
    if (const int64_t o = first_outside(obs_view, O, n_views); o < O) return fail(F + "observation " + std::to_string(o) + ": view index out of range");
    if (!all_finite(obs_xy, 2 * O)) return fail(F + "observation " + std::to_string(first_nonfinite(obs_xy, 2 * O) / 2) + ": non-finite coordinates");
    if (!all_finite(xyz, 3 * (int64_t)n_points)) return fail(F + "point " + std::to_string(first_nonfinite(xyz, 3 * (int64_t)n_points) / 3) + ": non-finite coordinates");

    const size_t nv = (size_t)n_views, np = (size_t)n_points, no = (size_t)O, nc = CAM ? (size_t)n_cameras : 0;
    std::vector<PoseCam> cams(CAM ? nc : nv);
    std::vector<int32_t> slots(SFD2_BA_CAM_K * nc), slot_param(SFD2_BA_CAM_K * nc);
    int kmax = 0;
    for (size_t i = 0; i < nc; ++i) {
        std::string w;
        if (cameras[i].refine & ~(SFD2_BA_REFINE_FOCAL | SFD2_BA_REFINE_PRINCIPAL | SFD2_BA_REFINE_EXTRA))
            return fail(F + "camera " + std::to_string(i) + ": unknown refine bits");
        if (!sfd2_pose_cam(cameras[i].model, cameras[i].params, cams[i], w)) return fail(F + "camera " + std::to_string(i) + ": " + w);
        kmax = std::max(kmax, cam_slots(cameras[i].model, cameras[i].refine, &slots[SFD2_BA_CAM_K * i], &slot_param[SFD2_BA_CAM_K * i]));
    }
    if (CAM)
        if (const int64_t v = first_outside(view_camera, n_views, n_cameras); v < n_views)
            return fail(F + "view " + std::to_string(v) + ": camera index out of range");
    std::vector<double> pose(12 * nv);
    for (int i = 0; i < n_views; ++i) {
        std::string w;
        if (!CAM) {
            memset(&cams[i], 0, sizeof(PoseCam));
            if (!sfd2_pose_cam(views[i].model, views[i].params, cams[i], w)) return fail(F + "view " + std::to_string(i) + ": " + w);
        }
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
    // the by-camera list the same way: a camera's views in ascending index
    std::vector<int64_t> cam_off(nc + 1, 0);
    std::vector<int32_t> cam_views(nv);
    if (CAM) {
        for (size_t v = 0; v < nv; ++v) ++cam_off[(size_t)view_camera[v] + 1];
        for (size_t i = 0; i < nc; ++i) cam_off[i + 1] += cam_off[i];
        std::vector<int64_t> fill(cam_off.begin(), cam_off.end() - 1);
        for (size_t v = 0; v < nv; ++v) cam_views[(size_t)fill[(size_t)view_camera[v]]++] = (int32_t)v;
    }
    // points by mapping: a lane each up to SFD2_BA_LONG_TRACK observations, beyond that a wave each (the flags force either side)
    std::vector<int32_t> short_ids, long_ids;
    for (int j = 0; j < n_points; ++j) {
        const int64_t len = point_offsets[j + 1] - point_offsets[j];
        for (int64_t o = point_offsets[j]; o < point_offsets[j + 1]; ++o) obs_pt[(size_t)o] = j;
        const bool wave = (flags & SFD2_BA_FLAG_POINT_WAVE) || (!(flags & SFD2_BA_FLAG_POINT_LANE) && len > SFD2_BA_LONG_TRACK);
        (wave ? long_ids : short_ids).push_back(j);
    }
    // the dense solver's pair list: observation a pairs with every observation b of its point whose view is not beyond a's own
    std::vector<int64_t> pair_off;
    if (DENSE) {
        pair_off.assign(no + 1, 0);
        std::vector<int32_t> sorted;
        for (int j = 0; j < n_points; ++j) {
            sorted.assign(obs_view + point_offsets[j], obs_view + point_offsets[j + 1]);
            std::sort(sorted.begin(), sorted.end());
            for (int64_t o = point_offsets[j]; o < point_offsets[j + 1]; ++o)
                pair_off[(size_t)o + 1] = pair_off[(size_t)o] + (std::upper_bound(sorted.begin(), sorted.end(), obs_view[o]) - sorted.begin());
        }
        if (pair_off[no] > 0x7fffffffLL) return fail(F + "the dense solver's pair list would hold more than 2^31 - 1 entries (" + std::to_string(pair_off[no]) + ")");
    }
    const size_t n_pairs = DENSE ? (size_t)pair_off[no] : 0, n_keys = nv * nv, ld = (6 * nv + SFD2_BA_DENSE_TILE - 1) / SFD2_BA_DENSE_TILE * SFD2_BA_DENSE_TILE;
    unsigned key_bits = 1;
    while (key_bits < 32 && ((size_t)1 << key_bits) < n_keys) ++key_bits;

    HIPCHECK(hipSetDevice(c->device));
    Carve in, ws;
    const size_t o_cam = in.take(sizeof(PoseCam) * cams.size()), o_vc = in.take(nv), o_pc = in.take(np), o_po = in.take(8 * (np + 1)), o_ov = in.take(4 * no),
                 o_op = in.take(4 * no), o_xy = in.take(16 * no), o_vo = in.take(8 * (nv + 1)), o_vb = in.take(4 * no), o_sh = in.take(4 * short_ids.size()),
                 o_lg = in.take(4 * long_ids.size());
    const size_t nx = 48 * nv + 8 * SFD2_BA_CAM_K * nc;      // bytes of a vector of the reduced system
    const size_t nred = (std::max(std::max(std::max(no, 3 * np), 6 * nv), SFD2_BA_CAM_K * nc) + SFD2_BA_RED_CHUNK - 1) / SFD2_BA_RED_CHUNK + 1;
    const size_t o_st = ws.take(sizeof(BaState)), o_pose = ws.take(96 * nv), o_poset = ws.take(96 * nv), o_xyz = ws.take(24 * np), o_xyzt = ws.take(24 * np),
                 o_rec = ws.take(8 * SFD2_BA_REC * no), o_err = ws.take(8 * no), o_oc = ws.take(8 * no), o_V = ws.take(48 * np), o_gp = ws.take(24 * np),
                 o_Vi = ws.take(48 * np), o_zg = ws.take(24 * np), o_z = ws.take(24 * np), o_B = ws.take(288 * nv), o_gc = ws.take(48 * nv),
                 o_Mi = ws.take(288 * nv), o_Dd = ws.take(48 * nv), o_b = ws.take(nx), o_x = ws.take(nx), o_r = ws.take(nx), o_zz = ws.take(nx),
                 o_p = ws.take(nx), o_q = ws.take(nx), o_part = ws.take(8 * nred);
    size_t o_vcam = 0, o_slot = 0, o_co = 0, o_cv = 0, o_camc = 0, o_camt = 0, o_bad = 0, o_reck = 0, o_W = 0, o_Cp = 0, o_gkp = 0, o_qkp = 0, o_C = 0, o_gk = 0,
           o_Ci = 0, o_Dk = 0;
    if (CAM) {
        o_vcam = in.take(4 * nv); o_slot = in.take(4 * SFD2_BA_CAM_K * nc); o_co = in.take(8 * (nc + 1)); o_cv = in.take(4 * nv);
        o_camc = ws.take(sizeof(PoseCam) * nc); o_camt = ws.take(sizeof(PoseCam) * nc); o_bad = ws.take(4); o_reck = ws.take(16 * (size_t)kmax * no);
        o_W = ws.take(8 * 48 * nv); o_Cp = ws.take(8 * 36 * nv); o_gkp = ws.take(8 * SFD2_BA_CAM_K * nv); o_qkp = ws.take(8 * SFD2_BA_CAM_K * nv);
        o_C = ws.take(8 * 64 * nc); o_gk = ws.take(8 * SFD2_BA_CAM_K * nc); o_Ci = ws.take(8 * 64 * nc); o_Dk = ws.take(8 * SFD2_BA_CAM_K * nc);
    }
    size_t o_pf = 0, o_S = 0, o_G = 0, o_k0 = 0, o_k1 = 0, o_v0 = 0, o_v1 = 0, o_tmp = 0, o_bs = 0, o_dw = 0, o_dy = 0, o_fail = 0, tmp_sort = 0;
    if (DENSE) {
        if (n_pairs) {
            uint32_t *nk = nullptr;
            uint64_t *nl = nullptr;
            HIPCHECK(rocprim::radix_sort_pairs(nullptr, tmp_sort, nk, nk, nl, nl, n_pairs, 0, key_bits, c->stream));
        }
        o_pf = in.take(8 * (no + 1));
        o_S = ws.take(8 * ld * ld); o_G = ws.take(144 * no); o_k0 = ws.take(4 * n_pairs); o_k1 = ws.take(4 * n_pairs); o_v0 = ws.take(8 * n_pairs);
        o_v1 = ws.take(8 * n_pairs); o_tmp = ws.take(tmp_sort); o_bs = ws.take(4 * (n_keys + 1)); o_dw = ws.take(8 * ld); o_dy = ws.take(8 * ld);
        o_fail = ws.take(4);
    }
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->ba_in, in.off));
    HIPCHECK(grow(c->ba_ws, ws.off));
    char *di = c->ba_in.as<char>(), *dw = c->ba_ws.as<char>();
    hipStream_t s = c->stream;
    HIPCHECK(hipMemcpyAsync(di + o_cam, cams.data(), sizeof(PoseCam) * cams.size(), hipMemcpyHostToDevice, s));
    if (CAM) {
        HIPCHECK(hipMemcpyAsync(dw + o_camc, cams.data(), sizeof(PoseCam) * nc, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(di + o_vcam, view_camera, 4 * nv, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(di + o_slot, slots.data(), 4 * SFD2_BA_CAM_K * nc, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(di + o_co, cam_off.data(), 8 * (nc + 1), hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(di + o_cv, cam_views.data(), 4 * nv, hipMemcpyHostToDevice, s));
    }
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

    BaCamPtrs Q;
    memset(&Q, 0, sizeof(Q));
    BaPtrs &P = Q.P;
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
    if (CAM) {
        Q.view_cam = at<const int32_t>(di, o_vcam); Q.slots = at<const int32_t>(di, o_slot);
        Q.cam_off = at<const int64_t>(di, o_co); Q.cam_views = at<const int32_t>(di, o_cv);
        Q.cams = at<PoseCam>(dw, o_camc); Q.cams_trial = at<PoseCam>(dw, o_camt); Q.bad = at<int32_t>(dw, o_bad);
        Q.reck = at<double>(dw, o_reck);
        Q.W = at<double>(dw, o_W); Q.Cp = at<double>(dw, o_Cp); Q.gkp = at<double>(dw, o_gkp); Q.qkp = at<double>(dw, o_qkp);
        Q.C = at<double>(dw, o_C); Q.gk = at<double>(dw, o_gk); Q.Cinv = at<double>(dw, o_Ci); Q.Dk = at<double>(dw, o_Dk);
        Q.nc = n_cameras; Q.kmax = kmax;
    }

    BaDense D;
    memset(&D, 0, sizeof(D));
    if (DENSE) {                                             // once per call: the pair list by block, every block's start, the padding of S
        HIPCHECK(hipMemcpyAsync(di + o_pf, pair_off.data(), 8 * (no + 1), hipMemcpyHostToDevice, s));
        D.S = at<double>(dw, o_S); D.ld = (int64_t)ld; D.G = at<double>(dw, o_G); D.pairs = at<const uint64_t>(dw, o_v1);
        D.blk_start = at<const int32_t>(dw, o_bs); D.w = at<double>(dw, o_dw); D.y = at<double>(dw, o_dy); D.fail = at<int32_t>(dw, o_fail);
        ProfScope ps(c, "bundle_adjust", "ba_dense_pairs+sort", 0.0, 24.0 * (double)n_pairs);
        launch_ba_dense_pairs(s, P, at<const int64_t>(di, o_pf), at<uint32_t>(dw, o_k0), at<uint64_t>(dw, o_v0));
        if (n_pairs) {
            size_t tb = tmp_sort;
            HIPCHECK(rocprim::radix_sort_pairs(dw + o_tmp, tb, at<uint32_t>(dw, o_k0), at<uint32_t>(dw, o_k1), at<uint64_t>(dw, o_v0), at<uint64_t>(dw, o_v1),
                                               n_pairs, 0, key_bits, s));
        }
        launch_ba_dense_block_start(s, at<const uint32_t>(dw, o_k1), (int64_t)n_pairs, (int64_t)n_keys, at<int32_t>(dw, o_bs));
        launch_dense_pad(s, D.S, D.ld, 6 * n_views);
    }

    const double c2 = conf->loss == SFD2_BA_LOSS_CAUCHY ? conf->loss_scale * conf->loss_scale : 1.0;
    // the state's Jacobians, blocks, gradients and max |g|: behind the start (gate none) or behind an accepted step
    auto linearise = [&](int gate, bool full, bool trial) {
        if (CAM) launch_bac_linearise(s, Q, gate, full, trial, conf->loss, c2);
        else launch_ba_linearise(s, P, gate, full, trial, conf->loss, c2);
    };
    auto relinearise = [&](int gate) {
        linearise(gate, true, false);
        launch_ba_point_build(s, P, gate);
        launch_ba_view_build(s, P, gate);
        if (CAM) launch_bac_cam_build(s, Q, gate);
        launch_ba_reduce(s, P, gate, P.gc, 6 * (int64_t)nv, SFD2_BA_OP_ABSMAX, &P.st->gmax, false);
        if (np) launch_ba_reduce(s, P, gate, P.gp, 3 * (int64_t)np, SFD2_BA_OP_ABSMAX, &P.st->gmax, true);
        if (CAM) launch_ba_reduce(s, P, gate, Q.gk, SFD2_BA_CAM_K * (int64_t)nc, SFD2_BA_OP_ABSMAX, &P.st->gmax, true);
    };
    auto read_state = [&]() -> hipError_t {
        hipError_t e = hipMemcpyAsync(&hs, P.st, sizeof(hs), hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipStreamSynchronize(s);
    };

    memset(result, 0, sizeof(*result));
    {
        ProfScope ps(c, "bundle_adjust", "ba_linearise+build", 0.0, 8.0 * SFD2_BA_REC * (double)no);
        linearise(SFD2_BA_GATE_NONE, false, false);
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
        if (DENSE) {                                         // S dc = b by a factorisation: no read of the state inside the step
            launch_ba_view_apply(s, P, SFD2_BA_GATE_NONE, true);
            HIPCHECK(hipMemsetAsync(D.fail, 0, 4, s));
            launch_ba_dense_form(s, P, D);
            launch_dense_cholesky(s, D.S, D.ld, D.fail);
            launch_dense_solve(s, D.S, D.ld, 6 * n_views, P.b, D.w, D.y, P.x, D.fail);
        } else if (CAM) {
            launch_bac_cam_precond(s, Q);
            launch_bac_apply(s, Q, SFD2_BA_GATE_NONE, true);
            launch_bac_pcg_init(s, Q);
        } else {
            launch_ba_view_apply(s, P, SFD2_BA_GATE_NONE, true);
            launch_ba_pcg_init(s, P);
        }
        for (int k = 0; k < conf->pcg_max_iterations && !DENSE;) {
            for (int e = std::min(conf->pcg_max_iterations, k + batch); k < e; ++k) {
                if (CAM) {
                    launch_bac_point_apply(s, Q, SFD2_BA_GATE_PCG, P.p);
                    launch_bac_apply(s, Q, SFD2_BA_GATE_PCG, false);
                    launch_bac_pcg_step(s, Q, tol2, conf->pcg_max_iterations);
                } else {
                    launch_ba_point_apply(s, P, SFD2_BA_GATE_PCG, P.p);
                    launch_ba_view_apply(s, P, SFD2_BA_GATE_PCG, false);
                    launch_ba_pcg_step(s, P, tol2, conf->pcg_max_iterations);
                }
            }
            HIPCHECK(read_state());
            if (hs.pcg_done) break;
        }
        if (!DENSE) pcg_total += hs.pcg_iters;
        if (CAM) {
            launch_bac_point_apply(s, Q, SFD2_BA_GATE_NONE, P.x);
            launch_bac_update_cams(s, Q);
        } else {
            launch_ba_point_apply(s, P, SFD2_BA_GATE_NONE, P.x);
        }
        launch_ba_update(s, P);
        linearise(SFD2_BA_GATE_NONE, false, true);
        launch_ba_reduce(s, P, SFD2_BA_GATE_NONE, P.obs_cost, O, SFD2_BA_OP_SUM, &P.st->trial_cost, false);
        if (CAM) launch_bac_veto(s, Q);
        if (DENSE) launch_ba_dense_veto(s, P, D);            // a failed pivot: a rejected step
        launch_ba_decide_commit(s, P);
        if (CAM) launch_bac_commit_cams(s, Q);
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
    if (CAM) HIPCHECK(hipMemcpyAsync(cams.data(), Q.cams, sizeof(PoseCam) * nc, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    for (int i = 0; i < n_views; ++i) {                      // a constant or unobserved view keeps its words as they came
        if (view_constant[i] || view_off[(size_t)i + 1] == view_off[(size_t)i] || hs.n_accepted == 0) continue;
        rot_to_quat(&pose[12 * (size_t)i], views[i].qvec);
        for (int a = 0; a < 3; ++a) views[i].tvec[a] = pose[12 * (size_t)i + 9 + a];
    }
    for (size_t i = 0; i < nc; ++i) {                        // a constant or unobserved camera keeps its words as they came
        bool observed = false;
        for (int64_t k = cam_off[i]; k < cam_off[i + 1] && !observed; ++k)
            observed = view_off[(size_t)cam_views[(size_t)k] + 1] > view_off[(size_t)cam_views[(size_t)k]];
        if (!observed || hs.n_accepted == 0) continue;
        for (int k = 0; k < SFD2_BA_CAM_K && slots[SFD2_BA_CAM_K * i + k] != SFD2_BA_SLOT_NONE; ++k)
            cameras[i].params[slot_param[SFD2_BA_CAM_K * i + k]] = cam_word(cams[i], slots[SFD2_BA_CAM_K * i + k]);
    }
    for (size_t v = 0; v < nv && CAM; ++v) {                 // every view leaves with its camera's words
        views[v].model = cameras[view_camera[v]].model;
        memcpy(views[v].params, cameras[view_camera[v]].params, sizeof(views[v].params));
    }
    return 0;
}

}  // namespace

extern "C" int sfd2_bundle_adjust(sfd2_ctx *c, sfd2_tri_view *views, int n_views, const uint8_t *view_constant, double *xyz, int n_points,
                                  const uint8_t *point_constant, const int64_t *point_offsets, const int32_t *obs_view, const double *obs_xy,
                                  const sfd2_ba_conf *conf, sfd2_ba_result *result, double *obs_error, int flags)
{
    return ba_run(c, "sfd2_bundle_adjust: ", nullptr, 0, nullptr, views, n_views, view_constant, xyz, n_points, point_constant, point_offsets, obs_view, obs_xy,
                  conf, result, obs_error, flags);
}

extern "C" int sfd2_bundle_adjust_cameras(sfd2_ctx *c, sfd2_ba_camera *cameras, int n_cameras, const int32_t *view_camera, sfd2_tri_view *views, int n_views,
                                          const uint8_t *view_constant, double *xyz, int n_points, const uint8_t *point_constant,
                                          const int64_t *point_offsets, const int32_t *obs_view, const double *obs_xy, const sfd2_ba_conf *conf,
                                          sfd2_ba_result *result, double *obs_error, int flags)
{
    const std::string F("sfd2_bundle_adjust_cameras: ");
    if (!cameras || !view_camera) return fail(F + "null argument");
    if (n_cameras < 1) return fail(F + "n_cameras must be positive");
    return ba_run(c, F, cameras, n_cameras, view_camera, views, n_views, view_constant, xyz, n_points, point_constant, point_offsets, obs_view, obs_xy, conf,
                  result, obs_error, flags);
}

// A x = b for a symmetric positive definite A by the dense solver's factor and solve kernels (bundle_dense_kernels.hip)
extern "C" int sfd2_spd_solve(sfd2_ctx *c, const double *A, int n, const double *b, double *x, int32_t *info)
{
    const std::string F("sfd2_spd_solve: ");
    if (!c || !A || !b || !x || !info) return fail(F + "null argument");
    if (n < 1 || n > 6 * SFD2_BA_DENSE_MAX_VIEWS) return fail(F + "1 <= n <= " + std::to_string(6 * SFD2_BA_DENSE_MAX_VIEWS));
    const size_t N = (size_t)n, ld = (N + SFD2_BA_DENSE_TILE - 1) / SFD2_BA_DENSE_TILE * SFD2_BA_DENSE_TILE;
    for (size_t r = 0; r < N; ++r)                           // only the lower triangle is read
        if (!all_finite(A + r * N, (int64_t)r + 1)) return fail(F + "row " + std::to_string(r) + ": non-finite entry in the lower triangle");
    if (!all_finite(b, n)) return fail(F + "non-finite right-hand side");
    HIPCHECK(hipSetDevice(c->device));
    Carve ws;
    const size_t o_A = ws.take(8 * ld * ld), o_b = ws.take(8 * N), o_w = ws.take(8 * ld), o_y = ws.take(8 * ld), o_x = ws.take(8 * N), o_fail = ws.take(4);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->ba_ws, ws.off));
    char *dw = c->ba_ws.as<char>();
    hipStream_t s = c->stream;
    double *dA = at<double>(dw, o_A);
    int32_t *dfail = at<int32_t>(dw, o_fail);
    HIPCHECK(hipMemcpy2DAsync(dA, 8 * ld, A, 8 * N, 8 * N, N, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(dw + o_b, b, 8 * N, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(dfail, 0, 4, s));
    {
        ProfScope ps(c, "spd_solve", "dense_cholesky+solve", (double)N * N * N / 3.0, 8.0 * (double)ld * ld);
        launch_dense_pad(s, dA, (int64_t)ld, n);
        launch_dense_cholesky(s, dA, (int64_t)ld, dfail);
        launch_dense_solve(s, dA, (int64_t)ld, n, at<const double>(dw, o_b), at<double>(dw, o_w), at<double>(dw, o_y), at<double>(dw, o_x), dfail);
    }
    HIPCHECK(hipGetLastError());
    std::vector<double> hx(N);
    int32_t hf = 0;
    HIPCHECK(hipMemcpyAsync(&hf, dfail, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(hx.data(), dw + o_x, 8 * N, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    *info = hf;
    if (hf == 0) memcpy(x, hx.data(), 8 * N);                // behind a failed pivot x stays as it came
    return 0;
}
