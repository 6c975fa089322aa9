// libsfd2hip: calibrated relative pose of a matched image pair (LO-RANSAC over the five-point solver, then a refinement on the
// Sampson error and the cheirality choice), the device side of sfd2_relative_pose_batch (api_two_view.hip).  The estimator COLMAP
// runs inside matches_importer for calibrated pairs (hloc/triangulation.py:114, hloc/reconstruction.py:145), essential matrix only.
//
// One workgroup of SFD2_TV_WG threads owns one pair from start to end; a batch of pairs of any sizes is one launch.
//   1. preparation: both point sets go to normalised coordinates through their own camera model (img_to_norm, pose_camera.h).
//   2. RANSAC rounds of SFD2_TV_WG trials, one per lane: the sample of trial i is drawn by sample_k<5> from (seed, i) only.  The
//      five-point solver (five_point.h: action matrix, QR iteration) keeps its matrices in LDS: kSlots workspaces, four lanes of each wave solve at a time.  Its
//      <= 10 matrices go to a per-pair scratch; then every lane takes its trial's matrices one at a time, polishes each by kPolish
//      Gauss-Newton steps on the sample's five Sampson residuals (so that the matrix no longer depends on the solver's route) and
//      scores it in fp64 over all correspondences in point order.  Support order: more inliers, then the smaller sum of the inliers'
//      squared Sampson errors, then the smaller trial index; no cheirality test.
//   3. local optimisation whenever a round improves the best support: E -> (R, t), kLoGN Gauss-Newton steps on 5 parameters (so(3),
//      the tangent plane of the unit t) over the best matrix's inliers, re-scored, repeated while the support grows (<= kLoSteps).
//   4. stopping: COLMAP's trial count (sample size 5, multiplier 3) after every round, clamped to [min_trials, max_trials].
//   5. final: Levenberg-Marquardt on the same 5 parameters and cost over the RANSAC inliers, then among (R, t), (R, -t), (R', t),
//      (R', -t), R' = (2 t t^T - I) R, the first with the most inliers in front of both cameras (midpoint triangulation); the
//      triangulation angle of every such inlier.
// Shared with the other RANSAC kernels (ransac_common.h, ransac_math.h): the sampler, reductions, scoring loops, winner
// broadcast, Cholesky solve and stopping rule.  Here: the solver call and polish, the Sampson error, E <-> (R, t), the frame with its
// residual and update, the LO loop, the Levenberg-Marquardt loop and the cheirality choice.
// Every reduction runs in a fixed order (wave butterflies, then the waves in index order) and nothing depends on another workgroup,
// so a pair's result depends on the pair and the seed only.  All loops are bounded.  No private segment, no spills.
#include "sfd2_internal.h"
#include "pose_camera.h"
#include "five_point.h"
#include "ransac_common.h"

namespace {

constexpr int kWG = SFD2_TV_WG;
constexpr int kWaves = kWG / 64;
constexpr int kSlotsPerWave = 4;
constexpr int kSlots = kWaves * kSlotsPerWave;   // five-point workspaces in LDS
constexpr int kPolish = 3;
constexpr int kLoSteps = 8;
constexpr int kLoGN = 3;
constexpr int kRefIters = 50;
constexpr int kNP = 5;               // so(3) and the tangent plane of the unit t
constexpr int kNS = 21;              // normal equations: 15 (upper triangle) + 5 (gradient) + 1 (cost)

SFD2_PD void cross3(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
SFD2_PD double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// ---------------------------------------------------------------------------------------------------------------- geometry
// squared Sampson error of x1^T E x0 (COLMAP's ComputeSquaredSampsonError)
SFD2_PD double sampson(const double E[9], double2 a, double2 b)
{
    const double e0 = E[0] * a.x + E[1] * a.y + E[2], e1 = E[3] * a.x + E[4] * a.y + E[5], e2 = E[6] * a.x + E[7] * a.y + E[8];
    const double f0 = E[0] * b.x + E[3] * b.y + E[6], f1 = E[1] * b.x + E[4] * b.y + E[7];
    const double C = b.x * e0 + b.y * e1 + e2;
    return C * C / (e0 * e0 + e1 * e1 + f0 * f0 + f1 * f1);
}

SFD2_PD void essential(const double R[9], const double t[3], double E[9])   // [t]x R
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
    }
}

// E -> (R, t), |t| = 1, with [t]x R = +-E: E is scaled to |E|_F^2 = 2, C is its cofactor matrix (= t t^T R), t the longest column of
// C normalised (the first on a tie), R = C - [t]x E (Horn 1990), made orthonormal through its quaternion.
SFD2_PD bool decompose(const double Ein[9], double R[9], double t[3])
{
    double nn = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) nn += Ein[i] * Ein[i];
    const double s = sqrt(2.0 / nn);
    double E[9], C[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = Ein[i] * s;
    cross3(E + 3, E + 6, C);
    cross3(E + 6, E, C + 3);
    cross3(E, E + 3, C + 6);
    int bj = 0;
    double bn = -1;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double cn = C[j] * C[j] + C[3 + j] * C[3 + j] + C[6 + j] * C[6 + j];
        if (cn > bn) { bn = cn; bj = j; }
    }
    const double inv = 1.0 / sqrt(bn);
    t[0] = (bj == 0 ? C[0] : bj == 1 ? C[1] : C[2]) * inv;
    t[1] = (bj == 0 ? C[3] : bj == 1 ? C[4] : C[5]) * inv;
    t[2] = (bj == 0 ? C[6] : bj == 1 ? C[7] : C[8]) * inv;
    double TE[9];
    essential(E, t, TE);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = C[i] - TE[i];
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) fin = fin && finite_d(R[i]);
    if (!fin) return false;
    double q[4];
    rot_to_quat(R, q);
    quat_to_rot(q[0], q[1], q[2], q[3], R);
#pragma unroll
    for (int i = 0; i < 9; ++i) fin = fin && finite_d(R[i]);
    return fin && finite_d(t[0]) && finite_d(t[1]) && finite_d(t[2]);
}

// the five derivative matrices of E = [t]x R: d/dw_k (R <- Exp(w) R) = [t]x [e_k]x R, d/da = [b1]x R, d/db = [b2]x R, where
// b1 = normalise(t x e_i), i the first smallest |t_i|, b2 = t x b1 (t <- normalise(t + a b1 + b b2))
struct Frame { double D[5][9]; };
SFD2_PD void tangent(const double t[3], double b1[3], double b2[3])
{
    int ai = 0;
    if (fabs(t[1]) < fabs(t[ai])) ai = 1;
    if (fabs(t[2]) < fabs(ai == 0 ? t[0] : t[1])) ai = 2;
    const double e[3] = {ai == 0 ? 1.0 : 0.0, ai == 1 ? 1.0 : 0.0, ai == 2 ? 1.0 : 0.0};
    cross3(t, e, b1);
    const double inv = 1.0 / sqrt(dot3(b1, b1));
#pragma unroll
    for (int i = 0; i < 3; ++i) b1[i] *= inv;
    cross3(t, b1, b2);
}
SFD2_PD void make_frame(const double R[9], const double t[3], Frame &f)
{
    double b1[3], b2[3];
    tangent(t, b1, b2);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double ek[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        double G[9];
        essential(R, ek, G);
        essential(G, t, f.D[k]);
    }
    essential(R, b1, f.D[3]);
    essential(R, b2, f.D[4]);
}
// residual C / sqrt(den) of one correspondence and its derivative by the five parameters
SFD2_PD void residual(const double E[9], const Frame &f, double2 a, double2 b, double &r, double (&J)[5])
{
    const double e0 = E[0] * a.x + E[1] * a.y + E[2], e1 = E[3] * a.x + E[4] * a.y + E[5], e2 = E[6] * a.x + E[7] * a.y + E[8];
    const double f0 = E[0] * b.x + E[3] * b.y + E[6], f1 = E[1] * b.x + E[4] * b.y + E[7];
    const double C = b.x * e0 + b.y * e1 + e2;
    const double den = e0 * e0 + e1 * e1 + f0 * f0 + f1 * f1;
    const double is = 1.0 / sqrt(den), c3 = C * is * is * is;
    r = C * is;
    const double x0[3] = {a.x, a.y, 1.0}, x1[3] = {b.x, b.y, 1.0}, ex[3] = {e0, e1, 0.0}, fx[3] = {f0, f1, 0.0};
    double g[9];                                        // d r / d E
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) g[i * 3 + j] = x1[i] * x0[j] * is - c3 * (ex[i] * x0[j] + fx[j] * x1[i]);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double s = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) s += g[i] * f.D[k][i];
        J[k] = s;
    }
}
// R <- Exp(d[0..2]) R, t <- normalise(t + d[3] b1 + d[4] b2)
SFD2_PD void apply_update(double R[9], double t[3], const double (&d)[5])
{
    double b1[3], b2[3];
    tangent(t, b1, b2);
    const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const double th = sqrt(th2);
    double a, b;                                      // Exp(w) = I + a [w]x + b [w]x^2
    if (th < 1e-8) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; }
    else { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
    const double wx = d[0], wy = d[1], wz = d[2];
    double X[9];
    X[0] = 1 - b * (wy * wy + wz * wz); X[1] = -a * wz + b * wx * wy;    X[2] = a * wy + b * wx * wz;
    X[3] = a * wz + b * wx * wy;        X[4] = 1 - b * (wx * wx + wz * wz); X[5] = -a * wx + b * wy * wz;
    X[6] = -a * wy + b * wx * wz;       X[7] = a * wx + b * wy * wz;     X[8] = 1 - b * (wx * wx + wy * wy);
    double Rn[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = X[i * 3] * R[j] + X[i * 3 + 1] * R[3 + j] + X[i * 3 + 2] * R[6 + j];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    double tn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) tn[i] = t[i] + d[3] * b1[i] + d[4] * b2[i];
    const double inv = 1.0 / sqrt(dot3(tn, tn));
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tn[i] * inv;
}

// midpoint triangulation of one correspondence under x1 = R x0 + t: the ray parameters l0 (camera 0) and l1 (camera 1) of the two
// closest points, and the angle in degrees at their midpoint between the rays to the two centres
SFD2_PD void triangulate(const double R[9], const double t[3], double2 a, double2 b, double &l0, double &l1, double &deg)
{
    const double d0[3] = {a.x, a.y, 1.0};
    double d1[3], w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d1[i] = R[i] * b.x + R[3 + i] * b.y + R[6 + i];
        w[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
    }
    const double aa = dot3(d0, d0), bb = dot3(d0, d1), cc = dot3(d1, d1), p = dot3(d0, w), q = dot3(d1, w);
    const double den = aa * cc - bb * bb;
    l0 = (cc * p - bb * q) / den;
    l1 = (bb * p - aa * q) / den;
    double u[3], v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double X = 0.5 * (l0 * d0[i] + w[i] + l1 * d1[i]);
        u[i] = -X;
        v[i] = w[i] - X;
    }
    const double cs = dot3(u, v) / sqrt(dot3(u, u) * dot3(v, v));
    deg = acos(fmin(1.0, fmax(-1.0, cs))) * (180.0 / 3.14159265358979323846);
}

// ---------------------------------------------------------------------------------------------------------------- kernel
__global__ __launch_bounds__(kWG) void two_view_kernel(const TvProbDev *__restrict__ probs, TvConfDev conf, const double *__restrict__ p0,
                                                       const double *__restrict__ p1, double2 *__restrict__ x0g, double2 *__restrict__ x1g,
                                                       double *__restrict__ hypg, unsigned char *__restrict__ mask_out,
                                                       double *__restrict__ angle_out, TvResDev *__restrict__ res)
{
    __shared__ double ws[kSlots * kFpWs];
    __shared__ double red[kWaves * kNS];
    __shared__ double shE[9];
    __shared__ Support sred[kWaves];
    const int pi = blockIdx.x, tid = threadIdx.x;
    const TvProbDev &pb = probs[pi];
    const int64_t off = pb.off;
    const int n = pb.n;
    double2 *x0 = x0g + off, *x1 = x1g + off;
    unsigned char *mask = mask_out + off;
    double *ang = angle_out + off;
    const double qnan = __builtin_nan("");
    TvResDev out;
    out.q[0] = 1.0; out.q[1] = out.q[2] = out.q[3] = 0.0;
    out.t[0] = out.t[1] = out.t[2] = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) out.E[i] = 0.0;
    out.success = 0; out.num_inliers = 0; out.num_trials = 0; out.pad = 0;
    if (n < 5) {
        for (int j = tid; j < n; j += kWG) { mask[j] = 0; ang[j] = qnan; }
        if (tid == 0) res[pi] = out;
        return;
    }
    // ---- 1. preparation
    {
        const PoseCam c0 = pb.cam0, c1 = pb.cam1;
        for (int j = tid; j < n; j += kWG) {
            double u, v;
            img_to_norm(c0, p0[2 * (off + j)], p0[2 * (off + j) + 1], u, v);
            x0[j] = make_double2(u, v);
            img_to_norm(c1, p1[2 * (off + j)], p1[2 * (off + j) + 1], u, v);
            x1[j] = make_double2(u, v);
        }
    }
    __syncthreads();
    const double th2 = pb.thresh2;
    double *hyp = hypg + (size_t)pi * kWG * SFD2_TV_CAND * 9 + tid;     // element (c, e) of this lane at hyp[(c * 9 + e) * kWG]
    double bE[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) bE[i] = 0.0;
    Support best;
    best.cnt = -1; best.sum = 0.0; best.trial = 0x7fffffffffffffffll;
    int64_t trials = 0;
    const int lane = tid & 63;
    double *wsl = ws + (tid >> 6) * kSlotsPerWave + (lane & (kSlotsPerWave - 1));

    // the normal equations of (R, t) over the correspondences `use` selects
    auto accumulate = [&](const double (&R)[9], const double (&t)[3], double (&s)[kNS], auto use) {
        Frame f;
        make_frame(R, t, f);
        double E[9];
        essential(R, t, E);
#pragma unroll
        for (int i = 0; i < kNS; ++i) s[i] = 0.0;
        for (int j = tid; j < n; j += kWG) {
            const double2 a = x0[j], b = x1[j];
            if (!use(j, a, b)) continue;
            double r, J[5];
            residual(E, f, a, b, r, J);
            normal_acc(s, J, r);
        }
        wg_sum(s, red);
    };

    for (int64_t round = 0;; ++round) {
        const int64_t trial = round * kWG + tid;
        const bool live = trial < conf.max_trials;
        int id[5] = {0, 1, 2, 3, 4};
        if (live) sample_k<5>(conf.seed, trial, n, id);
        // ---- 2a. the five-point solver, kSlotsPerWave lanes of every wave at a time (their workspaces are the wave's own)
        int ncand = 0;
        for (int sub = 0; sub < 64 / kSlotsPerWave; ++sub) {
            if (live && (lane / kSlotsPerWave) == sub) {
#pragma unroll
                for (int s = 0; s < 5; ++s) {
                    const double2 a = x0[id[s]], b = x1[id[s]];
                    const double r0[3] = {a.x, a.y, 1.0}, r1[3] = {b.x, b.y, 1.0};
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) wsl[(s * 9 + i * 3 + j) * kSlots] = r1[i] * r0[j];
                }
                five_point<kSlots>(wsl, [&](const double (&E)[9]) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) hyp[(size_t)(ncand * 9 + i) * kWG] = E[i];
                    ++ncand;
                });
            }
            __builtin_amdgcn_wave_barrier();              // the next four lanes take the same workspaces
        }
        // ---- 2b. polish and score, one matrix at a time
        Support mine;
        mine.cnt = -1; mine.sum = 0.0; mine.trial = trial;
        double mE[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) mE[i] = 0.0;
        double2 sa[5], sb[5];
#pragma unroll
        for (int s = 0; s < 5; ++s) { sa[s] = x0[id[s]]; sb[s] = x1[id[s]]; }
        for (int c = 0; c < SFD2_TV_CAND; ++c) {
            if (c >= ncand) break;
            double E[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) E[i] = hyp[(size_t)(c * 9 + i) * kWG];
            {
                double R[9], t[3];
                bool good = decompose(E, R, t);
                for (int it = 0; it < kPolish && good; ++it) {
                    Frame f;
                    make_frame(R, t, f);
                    double Ec[9], s[kNS];
                    essential(R, t, Ec);
#pragma unroll
                    for (int i = 0; i < kNS; ++i) s[i] = 0.0;
#pragma unroll
                    for (int k = 0; k < 5; ++k) {
                        double r, J[5];
                        residual(Ec, f, sa[k], sb[k], r, J);
                        normal_acc(s, J, r);
                    }
                    double d[5];
                    good = chol_solve<kNP>(s, 0.0, d);
                    if (good) apply_update(R, t, d);
                }
                if (good) {
                    double Ep[9];
                    essential(R, t, Ep);
                    bool fin = true;
#pragma unroll
                    for (int i = 0; i < 9; ++i) fin = fin && finite_d(Ep[i]);
                    if (fin) {
#pragma unroll
                        for (int i = 0; i < 9; ++i) E[i] = Ep[i];
                    }
                }
            }
            int cnt;
            double sum;
            score_lane(sampson, E, x0, x1, n, th2, cnt, sum);
            if (cnt > mine.cnt || (cnt == mine.cnt && sum < mine.sum)) {
                mine.cnt = cnt;
                mine.sum = sum;
#pragma unroll
                for (int i = 0; i < 9; ++i) mE[i] = E[i];
            }
        }
        const Support win = wg_best(mine, sred);
        if (win.cnt >= 0 && better(win, best)) {
            publish_winner(win.trial == trial, mE, shE, bE);
            best = win;
            // ---- 3. local optimisation over the best matrix's inliers
            double R[9], t[3];
            bool good = decompose(bE, R, t);
            for (int lo = 0; lo < kLoSteps && good; ++lo) {
                for (int gn = 0; gn < kLoGN && good; ++gn) {
                    double s[kNS];
                    accumulate(R, t, s, [&](int, double2 a, double2 b) { return sampson(bE, a, b) <= th2; });
                    double d[5];
                    good = chol_solve<kNP>(s, 0.0, d);
                    if (good) apply_update(R, t, d);
                }
                if (!good) break;
                double En[9];
                essential(R, t, En);
                int cnt;
                double sum;
                score_wg(sampson, En, x0, x1, n, th2, red, cnt, sum);
                if (!(cnt > best.cnt || (cnt == best.cnt && sum < best.sum))) break;
                best.cnt = cnt;
                best.sum = sum;
#pragma unroll
                for (int i = 0; i < 9; ++i) bE[i] = En[i];
            }
        }
        // ---- 4. stopping (COLMAP ComputeNumTrials on the best inlier ratio, sample size 5, multiplier 3)
        trials = min((round + 1) * kWG, conf.max_trials);
        // (the power is spelt out, not pow(): its last bit reaches num_trials)
        if (ransac_enough(trials, conf, n, best.cnt, [](double r) { return r * r * r * r * r; })) break;
        __syncthreads();                                      // shE and the reductions' LDS are reused by the next round
    }
    out.num_trials = (int)trials;
    // ---- 5. the RANSAC inliers, the refinement over them, the cheirality choice
    const bool found = best.cnt >= 5;
    for (int j = tid; j < n; j += kWG) {
        mask[j] = (found && sampson(bE, x0[j], x1[j]) <= th2) ? 1 : 0;
        ang[j] = qnan;
    }
    double R[9], t[3];
    if (!found || !decompose(bE, R, t)) {
        if (tid == 0) res[pi] = out;
        return;
    }
    out.num_inliers = best.cnt;
    auto in_mask = [&](int j, double2, double2) { return mask[j] != 0; };   // a lane reads the entries it wrote
    {
        double s[kNS];
        accumulate(R, t, s, in_mask);
        double lambda = 1e-4;
        for (int it = 0; it < kRefIters; ++it) {
            double d[5];
            if (!chol_solve<kNP>(s, lambda, d)) break;
            double Rn[9], tn[3];
#pragma unroll
            for (int i = 0; i < 9; ++i) Rn[i] = R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) tn[i] = t[i];
            apply_update(Rn, tn, d);
            double sn[kNS];
            accumulate(Rn, tn, sn, in_mask);
            const double step = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4];
            if (finite_d(sn[20]) && sn[20] <= s[20]) {
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) t[i] = tn[i];
#pragma unroll
                for (int i = 0; i < kNS; ++i) s[i] = sn[i];
                lambda = fmax(lambda * 0.1, 1e-12);
                if (step < 1e-26) break;
            } else {
                lambda *= 10.0;
                if (lambda > 1e12 || step < 1e-26) break;
            }
        }
    }
    {
        double q[4];
        rot_to_quat(R, q);
        quat_to_rot(q[0], q[1], q[2], q[3], R);
    }
    // slots 0: (R, t), 1: (R, -t), 2: (R', t), 3: (R', -t), R' = (2 t t^T - I) R
    double Rt[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rt[i * 3 + j] = 2.0 * t[i] * (t[0] * R[j] + t[1] * R[3 + j] + t[2] * R[6 + j]) - R[i * 3 + j];
    const double tm[3] = {-t[0], -t[1], -t[2]};
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < n; j += kWG) {
        if (!mask[j]) continue;
        const double2 a = x0[j], b = x1[j];
        double l0, l1, deg;
        triangulate(R, t, a, b, l0, l1, deg);
        v[0] += (l0 > 0 && l1 > 0) ? 1.0 : 0.0;
        triangulate(R, tm, a, b, l0, l1, deg);
        v[1] += (l0 > 0 && l1 > 0) ? 1.0 : 0.0;
        triangulate(Rt, t, a, b, l0, l1, deg);
        v[2] += (l0 > 0 && l1 > 0) ? 1.0 : 0.0;
        triangulate(Rt, tm, a, b, l0, l1, deg);
        v[3] += (l0 > 0 && l1 > 0) ? 1.0 : 0.0;
    }
    wg_sum(v, red);
    int slot = 0;
    double front = v[0];
#pragma unroll
    for (int s = 1; s < 4; ++s)
        if (v[s] > front) { front = v[s]; slot = s; }
    const bool chosen = front > 0;
    double Rc[9], tc[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rc[i] = slot >= 2 ? Rt[i] : R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tc[i] = (slot & 1) ? tm[i] : t[i];
    {
        double q[4];
        rot_to_quat(Rc, q);
        quat_to_rot(q[0], q[1], q[2], q[3], Rc);
#pragma unroll
        for (int i = 0; i < 4; ++i) out.q[i] = q[i];
    }
    if (chosen) {
        for (int j = tid; j < n; j += kWG) {
            if (!mask[j]) continue;
            double l0, l1, deg;
            triangulate(Rc, tc, x0[j], x1[j], l0, l1, deg);
            if (l0 > 0 && l1 > 0) ang[j] = deg;
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) out.t[i] = tc[i];
        essential(Rc, tc, out.E);
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 9; ++i) fin = fin && finite_d(out.E[i]);
        out.success = (fin && chosen && best.cnt >= conf.min_num_inliers) ? 1 : 0;
        if (!fin) {
            out.q[0] = 1.0; out.q[1] = out.q[2] = out.q[3] = 0.0;
            out.t[0] = out.t[1] = out.t[2] = 0.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) out.E[i] = 0.0;
        }
        res[pi] = out;
    }
}

}  // namespace

void launch_two_view(hipStream_t st, const TvProbDev *probs, int k, const TvConfDev &conf, const double *p0, const double *p1, double2 *x0,
                     double2 *x1, double *hyp, unsigned char *mask_out, double *angle_out, TvResDev *res)
{
    hipLaunchKernelGGL(two_view_kernel, dim3(k), dim3(kWG), 0, st, probs, conf, p0, p1, x0, x1, hyp, mask_out, angle_out, res);
}
