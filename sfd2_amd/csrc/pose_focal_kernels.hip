// libsfd2hip: absolute pose with an unknown focal length, the device side of sfd2_absolute_pose_focal_batch /
// sfd2_pose_refine_camera_batch (api_pose.hip).  Modelled on COLMAP's EstimateAbsolutePose with estimate_focal_length /
// refine_focal_length / refine_extra_params.
//
//   pose_sweep_kernel        one workgroup of SFD2_POSE_WG per (problem, focal sample): steps 1-4 of pose_kernels.hip (preparation, rounds,
//                            local optimisation, stopping) at the given camera with its focal lengths scaled, no step 5.  It is the
//                            text of pose_kernel (pose_kernels.hip is included below for it, not copied), so a sample's count and trial
//                            number are those of sfd2_absolute_pose_batch at that camera.  The points are shared by the samples; Xf / xf / xn and the
//                            hypotheses are per workgroup.
//   pose_focal_select_kernel per problem the best sample (more inliers, then the smaller sum in squared pixels, then the smaller index) and
//                            the main run's problem record: the given one at the winner's focal lengths.  The main run is pose_kernel.
//   pose_cam_refine_kernel   one workgroup per problem: Levenberg-Marquardt as step 5 (Cauchy at 1 px, fp64, <= 100 iterations) over the 6
//                            pose parameters (apply_update's perturbation) and, additively, the focal group and the extra group; the
//                            Jacobian rows of DESIGN.md 20 item 3.  Up to three refinements with an fp64 re-scoring in pixels between
//                            them, repeated while the mask grows.
// The host makes the scaled focal lengths and thresholds (one rounding each, so that they are the words a caller who scales the camera
// gets); the kernels only copy them.  Reductions run in a fixed order (wg_sum), nothing waits on another workgroup, every loop is bounded.
// ---------------------------------------------------------------------------------------------------------------- sweep
// pose_kernels.hip's text with another head and an exit after step 4: the workgroup is (problem, sample) b = blockIdx.x, its camera the
// problem's with the sample's focal lengths, its scratch the sample's copy; `pi` is b for the body, which indexes its hypotheses (and the
// result of a problem of fewer than 4 points, which goes to the unused res[b]) by it.  The sweep records are zeroed before the launch.
#define SFD2_POSE_KERNEL_HEAD                                                                                                                       \
__global__ __launch_bounds__(kWG) void pose_sweep_kernel(const PoseProbDev *__restrict__ probs, const PoseFocalTabDev *__restrict__ tab, int ns,   \
                                                         PoseConfDev conf, const double *__restrict__ p2, const double *__restrict__ p3,            \
                                                         float4 *__restrict__ xf4g, float2 *__restrict__ xf2g, double2 *__restrict__ xng,           \
                                                         double *__restrict__ hypg, int64_t N, PoseResDev *__restrict__ res,                        \
                                                         PoseSweepDev *__restrict__ sw)                                                             \
{                                                                                                                                                   \
    __shared__ double red[kWaves * kNS];                                                                                                            \
    __shared__ PoseSupport sred[kWaves];                                                                                                            \
    const int pi = blockIdx.x, tid = threadIdx.x;                                                                                                   \
    const PoseFocalTabDev tb = tab[pi];                                                                                                             \
    PoseProbDev pb = probs[pi / ns];                                                                                                                \
    pb.cam.f[0] = tb.f[0];                                                                                                                          \
    pb.cam.f[1] = tb.f[1];                                                                                                                          \
    pb.thresh2 = tb.thresh2;                                                                                                                        \
    const int64_t off = pb.off, so = (int64_t)(pi % ns) * N + off;                                                                                  \
    const int n = pb.n;                                                                                                                             \
    const PoseCam cam = pb.cam;                                                                                                                     \
    const double *P2 = p2 + 2 * off;                                                                                                                \
    const double *P3 = p3 + 3 * off;                                                                                                                \
    const unsigned char *mask_in = nullptr;                                                                                                         \
    unsigned char *mask_out = nullptr;                                                                                                              \
    float4 *Xf = xf4g + so;                                                                                                                         \
    float2 *xf = xf2g + so;                                                                                                                         \
    double2 *xn = xng + so;
#define SFD2_POSE_AFTER_RANSAC                                                                                                                      \
    if (tid == 0) {                                                                                                                                 \
        PoseSweepDev r;                                                                                                                             \
        r.cnt = found ? best.cnt : 0;                                                                                                               \
        r.num_trials = (int)trials;                                                                                                                 \
        r.sum_px = found ? (best.sum * tb.fm) * tb.fm : 0.f;                                                                                        \
        r.pad = 0;                                                                                                                                  \
        sw[pi] = r;                                                                                                                                 \
    }                                                                                                                                               \
    return;
#include "pose_kernels.hip"           // the solver's own text: everything in front of its kernel, and the kernel's body under the head above

namespace {

// ---------------------------------------------------------------------------------------------------------------- select
__global__ void pose_focal_select_kernel(const PoseProbDev *__restrict__ probs, int k, const PoseFocalTabDev *__restrict__ tab, int ns,
                                         const PoseSweepDev *__restrict__ sw, PoseProbDev *__restrict__ main_probs, int32_t *__restrict__ sel)
{
    const int pi = blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= k) return;
    int best = -1, bc = 2;
    float bs = 0.f;
    for (int i = 0; i < ns; ++i) {
        const PoseSweepDev s = sw[(size_t)pi * ns + i];
        if (s.cnt > bc || (best >= 0 && s.cnt == bc && s.sum_px < bs)) { best = i; bc = s.cnt; bs = s.sum_px; }
    }
    PoseProbDev p = probs[pi];
    if (best >= 0) {
        const PoseFocalTabDev tb = tab[(size_t)pi * ns + best];
        p.cam.f[0] = tb.f[0];
        p.cam.f[1] = tb.f[1];
        p.thresh2 = tb.thresh2;
    } else {
        p.n = 0;                                              // no sample with 3 inliers: the main run reports no pose
    }
    main_probs[pi] = p;
    sel[pi] = best;
}

// ---------------------------------------------------------------------------------------------------------------- refinement
constexpr int kFP = 12;                       // 6 pose | fx fy | k1 k2 p1 p2
constexpr int kFT = kFP * (kFP + 1) / 2;      // 78: the upper triangle
constexpr int kFS = kFT + kFP + 1;            // 91: triangle, gradient, robust cost
constexpr int kParts = 4;                     // the 91 sums are accumulated in four passes over the points: 23 accumulators live, not 91
constexpr int kPartN = 23;
static_assert(kParts * kPartN >= kFS && kPartN <= kNS, "parts cover the sums and fit wg_sum's LDS");

struct CamPose {
    double R[9], t[3];                        // centred coordinates, as in pose_run
    double f[2], k[4];
};

// sums [PART * kPartN, (PART + 1) * kPartN) of the normal equations over the masked points, every thread gets the totals
template <int PART>
__device__ __forceinline__ void refine_part(const CamPose &s, const PoseCam &cam0, int active, int single_f, int n, const double *__restrict__ P2,
                                            const double *__restrict__ P3, const double (&c)[3], const unsigned char *msk, double *red,
                                            double *S)
{
    constexpr int LO = PART * kPartN, HI = LO + kPartN;
    const int tid = threadIdx.x;
    PoseCam cam = cam0;
    cam.f[0] = s.f[0]; cam.f[1] = s.f[1];
    cam.k1 = s.k[0]; cam.k2 = s.k[1]; cam.p1 = s.k[2]; cam.p2 = s.k[3];
    double a[kPartN];
#pragma unroll
    for (int i = 0; i < kPartN; ++i) a[i] = 0.0;
    for (int j = tid; j < n; j += kWG) {
        if (!msk[j]) continue;
        double Xc[3], Pc[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) Xc[i] = P3[3 * j + i] - c[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) Pc[i] = s.R[i * 3] * Xc[0] + s.R[i * 3 + 1] * Xc[1] + s.R[i * 3 + 2] * Xc[2] + s.t[i];
        if (!(Pc[2] > 0)) continue;
        const double iz = 1.0 / Pc[2], u = Pc[0] * iz, v = Pc[1] * iz;
        double ud, vd, Jd[4];
        distort(cam, u, v, ud, vd, Jd);
        const double r0 = cam.f[0] * ud + cam.c[0] - P2[2 * j], r1 = cam.f[1] * vd + cam.c[1] - P2[2 * j + 1];
        const double sq = r0 * r0 + r1 * r1;
        const double w = 1.0 / (1.0 + sq);
        const double g0[3] = {cam.f[0] * Jd[0] * iz, cam.f[0] * Jd[1] * iz, -cam.f[0] * (Jd[0] * u + Jd[1] * v) * iz};
        const double g1[3] = {cam.f[1] * Jd[2] * iz, cam.f[1] * Jd[3] * iz, -cam.f[1] * (Jd[2] * u + Jd[3] * v) * iz};
        double j0[kFP], j1[kFP];
        {
            double c0[3], c1[3];
            cross3(Pc, g0, c0);
            cross3(Pc, g1, c1);
#pragma unroll
            for (int i = 0; i < 3; ++i) { j0[i] = c0[i]; j1[i] = c1[i]; j0[3 + i] = g0[i]; j1[3 + i] = g1[i]; }
        }
        const double r2 = u * u + v * v;
        j0[6] = ud;                         j1[6] = single_f ? vd : 0.0;
        j0[7] = 0.0;                        j1[7] = single_f ? 0.0 : vd;
        j0[8] = cam.f[0] * u * r2;          j1[8] = cam.f[1] * v * r2;
        j0[9] = cam.f[0] * u * r2 * r2;     j1[9] = cam.f[1] * v * r2 * r2;
        j0[10] = 2.0 * cam.f[0] * u * v;    j1[10] = cam.f[1] * (r2 + 2.0 * v * v);
        j0[11] = cam.f[0] * (r2 + 2.0 * u * u); j1[11] = 2.0 * cam.f[1] * u * v;
#pragma unroll
        for (int i = 6; i < kFP; ++i)
            if (!((active >> i) & 1)) { j0[i] = 0.0; j1[i] = 0.0; }
        int q = 0;
#pragma unroll
        for (int x = 0; x < kFP; ++x)
#pragma unroll
            for (int y = x; y < kFP; ++y, ++q)
                if (q >= LO && q < HI) a[q - LO] += w * (j0[x] * j0[y] + j1[x] * j1[y]);
#pragma unroll
        for (int x = 0; x < kFP; ++x)
            if (kFT + x >= LO && kFT + x < HI) a[kFT + x - LO] += w * (j0[x] * r0 + j1[x] * r1);
        if (kFS - 1 >= LO && kFS - 1 < HI) a[kFS - 1 - LO] += log1p(sq);
    }
    wg_sum(a, red);
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < kPartN; ++i)
            if (LO + i < kFS) S[LO + i] = a[i];
    }
}

// the 91 sums of state s into S (LDS); returns the robust cost
__device__ __forceinline__ double refine_sums(const CamPose &s, const PoseCam &cam0, int active, int single_f, int n, const double *P2, const double *P3,
                                              const double (&c)[3], const unsigned char *msk, double *red, double *S)
{
    refine_part<0>(s, cam0, active, single_f, n, P2, P3, c, msk, red, S);
    refine_part<1>(s, cam0, active, single_f, n, P2, P3, c, msk, red, S);
    refine_part<2>(s, cam0, active, single_f, n, P2, P3, c, msk, red, S);
    refine_part<3>(s, cam0, active, single_f, n, P2, P3, c, msk, red, S);
    __syncthreads();
    return S[kFS - 1];
}

// chol_solve's system (H + lambda diag(H) + 1e-15 max diag(H) I) d = -g for the 12 slots, in LDS by one thread: twelve parameters in
// registers are 144 doubles of matrix per lane.  A slot that is not refined has a zero row and column; its pivot is set to 1 and its step
// is exactly 0.  A: 144 doubles, D: 12, ok: 1 word.
__device__ __forceinline__ bool solve_lds(const double *S, double lambda, int active, double *A, double *D, int *ok, double (&d)[kFP])
{
    if (threadIdx.x == 0) {
        int q = 0;
        for (int x = 0; x < kFP; ++x)
            for (int y = x; y < kFP; ++y, ++q) { A[x * kFP + y] = S[q]; A[y * kFP + x] = S[q]; }
        double mx = 0;
        for (int x = 0; x < kFP; ++x)
            if ((active >> x) & 1) mx = fmax(mx, A[x * (kFP + 1)]);
        bool good = mx > 0 && finite_d(mx);
        if (good) {
            for (int x = 0; x < kFP; ++x) {
                if ((active >> x) & 1) A[x * (kFP + 1)] += lambda * A[x * (kFP + 1)] + 1e-15 * mx;
                else A[x * (kFP + 1)] = 1.0;
            }
            for (int j = 0; j < kFP && good; ++j) {
                double dj = A[j * (kFP + 1)];
                for (int p = 0; p < j; ++p) dj -= A[j * kFP + p] * A[j * kFP + p];
                if (!(dj > 0)) { good = false; break; }
                const double l = sqrt(dj);
                A[j * (kFP + 1)] = l;
                for (int i = j + 1; i < kFP; ++i) {
                    double v = A[i * kFP + j];
                    for (int p = 0; p < j; ++p) v -= A[i * kFP + p] * A[j * kFP + p];
                    A[i * kFP + j] = v / l;
                }
            }
        }
        if (good) {
            for (int i = 0; i < kFP; ++i) {                  // D holds y, then d
                double v = -S[kFT + i];
                for (int p = 0; p < i; ++p) v -= A[i * kFP + p] * D[p];
                D[i] = v / A[i * (kFP + 1)];
            }
            for (int i = kFP - 1; i >= 0; --i) {
                double v = D[i];
                for (int p = i + 1; p < kFP; ++p) v -= A[p * kFP + i] * D[p];
                D[i] = v / A[i * (kFP + 1)];
            }
            for (int i = 0; i < kFP; ++i) good = good && finite_d(D[i]);
        }
        *ok = good ? 1 : 0;
    }
    __syncthreads();
    const bool good = *ok != 0;
#pragma unroll
    for (int i = 0; i < kFP; ++i) d[i] = D[i];
    __syncthreads();
    return good;
}

__global__ __launch_bounds__(kWG) void pose_cam_refine_kernel(const PoseProbDev *__restrict__ probs, const PoseFocalProbDev *__restrict__ fprobs,
                                                              PoseFocalConfDev conf, const double *__restrict__ p2, const double *__restrict__ p3,
                                                              const PoseResDev *__restrict__ main_res, unsigned char *__restrict__ maskg,
                                                              unsigned char *__restrict__ mask_newg, PoseFocalResDev *__restrict__ res)
{
    __shared__ double red[kWaves * kNS];
    __shared__ double Sc[kParts * kPartN], Sn[kParts * kPartN], A[kFP * kFP], D[kFP];
    __shared__ int okw;
    const int pi = blockIdx.x, tid = threadIdx.x;
    const PoseProbDev &pb = probs[pi];
    const PoseFocalProbDev fp = fprobs[pi];
    const PoseCam cam0 = pb.cam;
    const int64_t off = pb.off;
    const int n = pb.n;
    const double *P2 = p2 + 2 * off, *P3 = p3 + 3 * off;
    unsigned char *msk = maskg + off, *mnew = mask_newg + off;
    PoseFocalResDev out;
    out.q[0] = 1.0; out.q[1] = out.q[2] = out.q[3] = 0.0;
    out.t[0] = out.t[1] = out.t[2] = 0.0;
    out.f[0] = cam0.f[0]; out.f[1] = cam0.f[1];
    out.k[0] = cam0.k1; out.k[1] = cam0.k2; out.k[2] = cam0.p1; out.k[3] = cam0.p2;
    out.success = 0; out.num_inliers = 0; out.ransac_num_inliers = 0; out.num_trials = 0;
    double q0[4], t0[3];
    if (conf.start_from_res) {
        const PoseResDev mr = main_res[pi];
#pragma unroll
        for (int i = 0; i < 4; ++i) q0[i] = mr.q[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t0[i] = mr.t[i];
        out.success = mr.success;
        out.num_inliers = out.ransac_num_inliers = mr.num_inliers;
        out.num_trials = mr.num_trials;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) q0[i] = pb.qt[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t0[i] = pb.qt[4 + i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) out.q[i] = q0[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) out.t[i] = t0[i];
    int cnt = 0;
    if (n >= 4) {
        double v[1] = {0};
        for (int j = tid; j < n; j += kWG) v[0] += msk[j] ? 1.0 : 0.0;
        wg_sum(v, red);
        cnt = (int)v[0];
    }
    if (!conf.start_from_res) {
        out.success = cnt >= 3 ? 1 : 0;
        out.num_inliers = out.ransac_num_inliers = cnt;
    }
    if (!out.success || conf.rounds <= 0 || n < 4) {
        if (tid == 0) res[pi] = out;
        return;
    }
    double c[3];
    {
        double v[3] = {0, 0, 0};
        for (int j = tid; j < n; j += kWG) { v[0] += P3[3 * j]; v[1] += P3[3 * j + 1]; v[2] += P3[3 * j + 2]; }
        wg_sum(v, red);
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = v[i] / n;
    }
    CamPose s;
    quat_to_rot(q0[0], q0[1], q0[2], q0[3], s.R);
#pragma unroll
    for (int i = 0; i < 3; ++i) s.t[i] = t0[i] + s.R[i * 3] * c[0] + s.R[i * 3 + 1] * c[1] + s.R[i * 3 + 2] * c[2];
    s.f[0] = cam0.f[0]; s.f[1] = cam0.f[1];
    s.k[0] = cam0.k1; s.k[1] = cam0.k2; s.k[2] = cam0.p1; s.k[3] = cam0.p2;
    const int active = fp.active, single_f = fp.single_f;
    for (int round = 0; round < conf.rounds && round < 3; ++round) {
        // ---- Levenberg-Marquardt over the current mask
        double cost = refine_sums(s, cam0, active, single_f, n, P2, P3, c, msk, red, Sc);
        double lambda = 1e-4;
        for (int it = 0; it < kRefIters; ++it) {
            double d[kFP];
            if (!solve_lds(Sc, lambda, active, A, D, &okw, d)) break;
            CamPose sn = s;
            const double dp[kNP] = {d[0], d[1], d[2], d[3], d[4], d[5]};
            apply_update(sn.R, sn.t, dp);
            sn.f[0] += d[6];
            sn.f[1] += single_f ? d[6] : d[7];
#pragma unroll
            for (int i = 0; i < 4; ++i) sn.k[i] += d[8 + i];
            bool valid = true;
#pragma unroll
            for (int i = 0; i < 9; ++i) valid = valid && finite_d(sn.R[i]);
#pragma unroll
            for (int i = 0; i < 3; ++i) valid = valid && finite_d(sn.t[i]);
#pragma unroll
            for (int i = 0; i < 4; ++i) valid = valid && finite_d(sn.k[i]);
#pragma unroll
            for (int i = 0; i < 2; ++i) valid = valid && finite_d(sn.f[i]) && sn.f[i] > 0 && sn.f[i] >= fp.f_lo[i] && sn.f[i] <= fp.f_hi[i];
            double costn = cost;
            if (valid) costn = refine_sums(sn, cam0, active, single_f, n, P2, P3, c, msk, red, Sn);   // (valid is uniform: the same words in every lane)
            const double step = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] +
                                (d[3] * d[3] + d[4] * d[4] + d[5] * d[5]) / (1.0 + s.t[0] * s.t[0] + s.t[1] * s.t[1] + s.t[2] * s.t[2]) +
                                (d[6] / s.f[0]) * (d[6] / s.f[0]) + (d[7] / s.f[1]) * (d[7] / s.f[1]) +
                                d[8] * d[8] + d[9] * d[9] + d[10] * d[10] + d[11] * d[11];
            if (valid && finite_d(costn) && costn <= cost) {
                s = sn;
                cost = costn;
                if (tid < kFS) Sc[tid] = Sn[tid];
                __syncthreads();
                lambda = fmax(lambda * 0.1, 1e-12);
                if (step < 1e-26) break;
            } else {
                lambda *= 10.0;
                if (lambda > 1e12 || step < 1e-26) break;
            }
        }
        if (round + 1 >= conf.rounds || round + 1 >= 3) break;
        // ---- re-scoring in pixels, fp64
        PoseCam cam = cam0;
        cam.f[0] = s.f[0]; cam.f[1] = s.f[1];
        cam.k1 = s.k[0]; cam.k2 = s.k[1]; cam.p1 = s.k[2]; cam.p2 = s.k[3];
        double v[1] = {0};
        for (int j = tid; j < n; j += kWG) {
            double Xc[3], Pc[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) Xc[i] = P3[3 * j + i] - c[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) Pc[i] = s.R[i * 3] * Xc[0] + s.R[i * 3 + 1] * Xc[1] + s.R[i * 3 + 2] * Xc[2] + s.t[i];
            bool in = false;
            if (Pc[2] > 0) {
                double px, py;
                project_px(cam, Pc, px, py);
                const double ex = px - P2[2 * j], ey = py - P2[2 * j + 1];
                in = ex * ex + ey * ey <= fp.max_err2;
            }
            mnew[j] = in ? 1 : 0;
            v[0] += in ? 1.0 : 0.0;
        }
        wg_sum(v, red);
        if (!((int)v[0] > cnt)) break;
        cnt = (int)v[0];
        for (int j = tid; j < n; j += kWG) msk[j] = mnew[j];   // (each lane copies the points it scored)
    }
    if (tid == 0) {
        rot_to_quat(s.R, out.q);
        double Rq[9];
        quat_to_rot(out.q[0], out.q[1], out.q[2], out.q[3], Rq);
#pragma unroll
        for (int i = 0; i < 3; ++i) out.t[i] = s.t[i] - (Rq[i * 3] * c[0] + Rq[i * 3 + 1] * c[1] + Rq[i * 3 + 2] * c[2]);
        out.f[0] = s.f[0]; out.f[1] = s.f[1];
#pragma unroll
        for (int i = 0; i < 4; ++i) out.k[i] = s.k[i];
        out.num_inliers = cnt;
        res[pi] = out;
    }
}

}  // namespace

void launch_pose_sweep(hipStream_t st, const PoseProbDev *probs, int k, const PoseFocalTabDev *tab, int ns, const PoseConfDev &conf, const double *p2,
                       const double *p3, float4 *xf4, float2 *xf2, double2 *xn, double *hyp, int64_t N, PoseResDev *unused, PoseSweepDev *sweep)
{
    hipLaunchKernelGGL(pose_sweep_kernel, dim3((unsigned)k * ns), dim3(kWG), 0, st, probs, tab, ns, conf, p2, p3, xf4, xf2, xn, hyp, N, unused, sweep);
}

void launch_pose_focal_select(hipStream_t st, const PoseProbDev *probs, int k, const PoseFocalTabDev *tab, int ns, const PoseSweepDev *sweep,
                              PoseProbDev *main_probs, int32_t *sel)
{
    hipLaunchKernelGGL(pose_focal_select_kernel, dim3((k + 63) / 64), dim3(64), 0, st, probs, k, tab, ns, sweep, main_probs, sel);
}

void launch_pose_cam_refine(hipStream_t st, const PoseProbDev *probs, const PoseFocalProbDev *fprobs, int k, const PoseFocalConfDev &conf,
                            const double *p2, const double *p3, const PoseResDev *main_res, unsigned char *mask, unsigned char *mask_new,
                            PoseFocalResDev *res)
{
    hipLaunchKernelGGL(pose_cam_refine_kernel, dim3(k), dim3(kWG), 0, st, probs, fprobs, conf, p2, p3, main_res, mask, mask_new, res);
}
