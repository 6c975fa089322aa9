// libsfd2hip: absolute pose from 2D-3D correspondences (LO-RANSAC over P3P, then a robust refinement), the device side of
// sfd2_absolute_pose_batch / sfd2_pose_refine_batch (api_pose.hip).  Replaces pycolmap.absolute_pose_estimation and
// pycolmap.pose_refinement (it_loc/localize_cv2.py:731, :390, :451).
//
// One workgroup of SFD2_POSE_WG threads owns one problem from start to end; a batch of problems of any sizes is one launch.
//   1. preparation: the 3D centroid (fp64, fixed-order reduction) is subtracted so that scoring can run in fp32; every 2D point is
//      mapped to normalised coordinates through the camera model (COLMAP's ImageToWorld: Newton iterations for the distortion).
//   2. RANSAC rounds of SFD2_POSE_WG trials, one per lane: the sample of trial i is drawn from a counter-based generator keyed by
//      (seed, i) only, P3P (Lambda Twist, Persson & Nordberg, ECCV 2018) is solved in fp64 and each of its <= 4 poses is scored
//      by its lane over every point in fp32 (the lanes are the hypotheses, the loop runs over the points, whose loads are
//      uniform across the wave).  Support order: more inliers, then a smaller fp32 residual sum over the inliers (accumulated
//      in point order), then a smaller hypothesis key (4 * trial + solution slot).
//   3. local optimisation whenever a round improves the best support: fp64 Gauss-Newton on the 6 pose parameters over the
//      best pose's inliers, re-scored, repeated while the support grows (bounded).
//   4. stopping: COLMAP's trial count (confidence, best inlier ratio, sample size 3, its default multiplier 3) evaluated after
//      every round, clamped to [min_num_trials, max_num_trials]; the round structure makes the stopping point deterministic.
//   5. refinement (pycolmap's RefineAbsolutePose with the intrinsics fixed): Levenberg-Marquardt on sum rho(|pi(R X + t) - x|^2)
//      in pixels through the camera model over the RANSAC inliers, rho = Cauchy with a 1 px scale, fp64.
// Shared with the two-view RANSAC kernels (ransac_common.h, ransac_math.h): the sampler (sample_k<3>), reductions,
// Cholesky solve and stopping rule.  Here: P3P, the fp32 support and scoring, the weighted two-row normal equations, the LO loop and
// the Levenberg-Marquardt loop on the robust cost.
// Every reduction runs in a fixed order (wave butterflies, then the waves in index order) and nothing depends on another
// workgroup, so results are bit-identical whatever the batch, its order and the scheduling.  All loops are bounded.
#include "sfd2_internal.h"
#include "pose_camera.h"              // SFD2_PD, distort, img_to_norm: the camera model, shared with assemble_kernels.hip and tri_kernels.hip
#include "ransac_common.h"            // wg_sum, wg_best, sample_k, chol_solve, ransac_enough: shared with the two-view kernels

namespace {

constexpr int kWG = SFD2_POSE_WG;
constexpr int kWaves = kWG / 64;
constexpr int kLoSteps = 8;          // local optimisation: re-estimations per improvement
constexpr int kLoGN = 3;             // Gauss-Newton iterations per re-estimation
constexpr int kRefIters = 100;       // refinement iterations (pycolmap's max_num_iterations)
constexpr int kHypD = 12;            // doubles per stored hypothesis (R row-major, t)
constexpr int kNP = 6;               // so(3), translation
constexpr int kNS = 28;              // normal equations: 21 (upper triangle) + 6 (gradient) + 1 (robust cost, the refinement's only)

// ---------------------------------------------------------------------------------------------------------------- camera model
// (distort: pose_camera.h)
// (img_to_norm: pose_camera.h)

// ---------------------------------------------------------------------------------------------------------------- small algebra
SFD2_PD void cross3(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
SFD2_PD double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// det of the matrix with columns a, b, c
SFD2_PD double det_cols(const double a[3], const double b[3], const double c[3])
{
    double x[3];
    cross3(b, c, x);
    return dot3(a, x);
}

// (quat_to_rot, rot_to_quat: pose_camera.h)
SFD2_PD void orthonormalise(double R[9])
{
    double q[4];
    rot_to_quat(R, q);
    quat_to_rot(q[0], q[1], q[2], q[3], R);
}

// R <- Exp(w) R, t <- Exp(w) t + d  (left perturbation: x_cam' = Exp(w) x_cam + d)
SFD2_PD void apply_update(double R[9], double t[3], const double (&d)[kNP])
{
    const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const double th = sqrt(th2);
    double a, b;                                      // Exp(w) = I + a [w]x + b [w]x^2
    if (th < 1e-8) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; }
    else { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
    const double wx = d[0], wy = d[1], wz = d[2];
    double E[9];
    E[0] = 1 - b * (wy * wy + wz * wz); E[1] = -a * wz + b * wx * wy;    E[2] = a * wy + b * wx * wz;
    E[3] = a * wz + b * wx * wy;        E[4] = 1 - b * (wx * wx + wz * wz); E[5] = -a * wx + b * wy * wz;
    E[6] = -a * wy + b * wx * wz;       E[7] = a * wx + b * wy * wz;     E[8] = 1 - b * (wx * wx + wy * wy);
    double Rn[9], tn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = E[i * 3] * R[j] + E[i * 3 + 1] * R[3 + j] + E[i * 3 + 2] * R[6 + j];
        tn[i] = E[i * 3] * t[0] + E[i * 3 + 1] * t[1] + E[i * 3 + 2] * t[2] + d[3 + i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tn[i];
}

// One point's two residual rows under the weight w into the normal equations (ransac_math.h's layout).  Not normal_acc twice:
// w (j0a j0b + j1a j1b) rounds differently from two separate accumulations, and the results are pinned.
template <int N>
SFD2_PD void acc_normal(double (&s)[N], const double j0[6], const double j1[6], double r0, double r1, double w)
{
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b, ++k) s[k] += w * (j0[a] * j0[b] + j1[a] * j1[b]);
#pragma unroll
    for (int a = 0; a < 6; ++a) s[21 + a] += w * (j0[a] * r0 + j1[a] * r1);
}

// ---------------------------------------------------------------------------------------------------------------- support
// fp32 by design: the sum is the scoring loop's own fp32 accumulator
struct PoseSupport {
    int cnt;        // -1: no hypothesis
    float sum;
    long long key;  // 4 * trial + slot
};
__device__ __forceinline__ bool better(const PoseSupport &a, const PoseSupport &b)
{
    if (a.cnt != b.cnt) return a.cnt > b.cnt;
    if (a.sum != b.sum) return a.sum < b.sum;
    return a.key < b.key;
}
__device__ __forceinline__ PoseSupport shfl_support(const PoseSupport &s, int m)
{
    PoseSupport o;
    o.cnt = __shfl_xor(s.cnt, m, 64);
    o.sum = __shfl_xor(s.sum, m, 64);
    o.key = __shfl_xor(s.key, m, 64);
    return o;
}

// ---------------------------------------------------------------------------------------------------------------- P3P
// one real root of x^3 + b x^2 + c x + d (Cardano / trigonometric form, two Newton steps)
SFD2_PD double cubic_root(double b, double c, double d)
{
    const double p = c - b * b / 3.0;
    const double q = 2.0 * b * b * b / 27.0 - b * c / 3.0 + d;
    const double disc = q * q / 4.0 + p * p * p / 27.0;
    double x;
    if (disc >= 0) {
        const double s = sqrt(disc);
        x = cbrt(-q / 2.0 + s) + cbrt(-q / 2.0 - s) - b / 3.0;
    } else {
        const double r = sqrt(-p / 3.0);
        const double cs = fmin(1.0, fmax(-1.0, -q / (2.0 * r * r * r)));
        x = 2.0 * r * cos(acos(cs) / 3.0) - b / 3.0;
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double f = ((x + b) * x + c) * x + d, fp = (3.0 * x + 2.0 * b) * x + c;
        if (fp != 0.0) x -= f / fp;
    }
    return x;
}

// unit eigenvector of the symmetric S for eigenvalue sig: the longest cross product of two rows of S - sig I
SFD2_PD void eigvec(const double S[9], double sig, double e[3])
{
    const double r0[3] = {S[0] - sig, S[1], S[2]}, r1[3] = {S[3], S[4] - sig, S[5]}, r2[3] = {S[6], S[7], S[8] - sig};
    double a[3], b[3], c[3];
    cross3(r0, r1, a);
    cross3(r0, r2, b);
    cross3(r1, r2, c);
    const double na = dot3(a, a), nb = dot3(b, b), nc = dot3(c, c);
    double m[3] = {a[0], a[1], a[2]}, nm = na;
    if (nb > nm) { m[0] = b[0]; m[1] = b[1]; m[2] = b[2]; nm = nb; }
    if (nc > nm) { m[0] = c[0]; m[1] = c[1]; m[2] = c[2]; nm = nc; }
    const double s = nm > 0 ? 1.0 / sqrt(nm) : 0.0;
    e[0] = m[0] * s; e[1] = m[1] * s; e[2] = m[2] * s;
}

// Lambda Twist P3P (Persson & Nordberg, "Lambda Twist: An Accurate Fast Robust Perspective Three Point (P3P) Solver", ECCV 2018):
// the depths L solve L^T M_ij L = a_ij; D1 = a23 M12 - a12 M23 and D2 = a23 M13 - a13 M23 span the homogeneous conics through the
// solutions, a real root of det(D1 + g D2) = 0 gives a degenerate member (a pair of planes through the origin), and each plane
// meets a13 M12 - a12 M13 = 0 in a quadratic.  The depths are polished by Gauss-Newton; R = Y X^-1 from the difference vectors.
// y: unit bearings, X: 3D points (fp64).  Writes up to 4 poses into fixed slots (R row-major, t) and their validity.
SFD2_PD void p3p(const double y[3][3], const double X[3][3], double (&P)[4][kHypD], bool (&ok)[4])
{
#pragma unroll
    for (int s = 0; s < 4; ++s) ok[s] = false;
    double d12[3], d13[3], d23[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { d12[i] = X[0][i] - X[1][i]; d13[i] = X[0][i] - X[2][i]; d23[i] = X[1][i] - X[2][i]; }
    const double a12 = dot3(d12, d12), a13 = dot3(d13, d13), a23 = dot3(d23, d23);
    double n13[3];
    cross3(d12, d13, n13);
    const double nn = dot3(n13, n13);
    if (!(nn > 1e-10 * a12 * a13) || !finite_d(nn)) return;        // collinear or coincident 3D points
    const double b12 = dot3(y[0], y[1]), b13 = dot3(y[0], y[2]), b23 = dot3(y[1], y[2]);
    double yc[3];
    cross3(y[0], y[1], yc);
    if (!(fabs(dot3(yc, y[2])) > 1e-12)) return;                   // coplanar bearings: no finite solution set worth scoring
    // M12 = [[1,-b12,0],[-b12,1,0],[0,0,0]], M13 = [[1,0,-b13],[0,0,0],[-b13,0,1]], M23 = [[0,0,0],[0,1,-b23],[0,-b23,1]]
    const double M12[9] = {1, -b12, 0, -b12, 1, 0, 0, 0, 0};
    const double M13[9] = {1, 0, -b13, 0, 0, 0, -b13, 0, 1};
    const double M23[9] = {0, 0, 0, 0, 1, -b23, 0, -b23, 1};
    double D1[9], D2[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { D1[i] = a23 * M12[i] - a12 * M23[i]; D2[i] = a23 * M13[i] - a13 * M23[i]; }
    // columns (symmetric: rows)
    const double A1[3] = {D1[0], D1[3], D1[6]}, A2[3] = {D1[1], D1[4], D1[7]}, A3[3] = {D1[2], D1[5], D1[8]};
    const double B1[3] = {D2[0], D2[3], D2[6]}, B2[3] = {D2[1], D2[4], D2[7]}, B3[3] = {D2[2], D2[5], D2[8]};
    const double c0 = det_cols(A1, A2, A3), c3 = det_cols(B1, B2, B3);
    const double c1 = det_cols(B1, A2, A3) + det_cols(A1, B2, A3) + det_cols(A1, A2, B3);
    const double c2 = det_cols(A1, B2, B3) + det_cols(B1, A2, B3) + det_cols(B1, B2, A3);
    double D0[9];
    if (fabs(c3) >= fabs(c0)) {
        if (c3 == 0.0) return;
        const double g = cubic_root(c2 / c3, c1 / c3, c0 / c3);
#pragma unroll
        for (int i = 0; i < 9; ++i) D0[i] = D1[i] + g * D2[i];
    } else {                                                        // det(mu D1 + D2) = c0 mu^3 + c1 mu^2 + c2 mu + c3
        const double mu = cubic_root(c1 / c0, c2 / c0, c3 / c0);
#pragma unroll
        for (int i = 0; i < 9; ++i) D0[i] = mu * D1[i] + D2[i];
    }
    // the two non-zero eigenvalues of the rank-2 D0 and their eigenvectors
    const double tr = D0[0] + D0[4] + D0[8];
    const double m2 = D0[0] * D0[4] - D0[1] * D0[1] + D0[0] * D0[8] - D0[2] * D0[2] + D0[4] * D0[8] - D0[5] * D0[5];
    if (!(m2 < 0)) return;                                          // the planes must be real: eigenvalues of opposite sign
    const double sq = sqrt(fmax(0.0, tr * tr - 4.0 * m2));
    const double sa = 0.5 * (tr + sq), sb = 0.5 * (tr - sq);        // sa > 0 > sb
    double ea[3], eb[3];
    eigvec(D0, sa, ea);
    eigvec(D0, sb, eb);
    const double sv = sqrt(-sb / sa);
    double Q[9];                                                    // a13 M12 - a12 M13: homogeneous, through every solution
#pragma unroll
    for (int i = 0; i < 9; ++i) Q[i] = a13 * M12[i] - a12 * M13[i];
    const double Xinvn = 1.0 / nn;
    // X^-1 of [d12 d13 n13] (columns): rows are (d13 x n13, n13 x d12, d12 x d13) / det, det = |n13|^2
    double Xi0[3], Xi1[3];
    cross3(d13, n13, Xi0);
    cross3(n13, d12, Xi1);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        const double sg = pl ? -sv : sv;
        const double nrm[3] = {ea[0] - sg * eb[0], ea[1] - sg * eb[1], ea[2] - sg * eb[2]};
        if (!(fabs(nrm[0]) > 1e-12 * (fabs(nrm[1]) + fabs(nrm[2])))) continue;
        const double w0 = -nrm[1] / nrm[0], w1 = -nrm[2] / nrm[0];  // l1 = w0 l2 + w1 l3
        // f(tau) = v^T Q v, v = p + tau q, p = (w0, 1, 0), q = (w1, 0, 1)
        const double p[3] = {w0, 1, 0}, qv[3] = {w1, 0, 1};
        double Qp[3], Qq[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { Qp[i] = Q[i * 3] * p[0] + Q[i * 3 + 1] * p[1] + Q[i * 3 + 2] * p[2]; Qq[i] = Q[i * 3] * qv[0] + Q[i * 3 + 1] * qv[1] + Q[i * 3 + 2] * qv[2]; }
        const double qa = dot3(qv, Qq), qb = 2.0 * dot3(p, Qq), qc = dot3(p, Qp);
        double tau[2];
        bool tv[2] = {false, false};
        if (fabs(qa) > 1e-14 * (fabs(qb) + fabs(qc))) {
            const double disc = qb * qb - 4.0 * qa * qc;
            if (disc >= 0) {
                const double h = -0.5 * (qb + (qb >= 0 ? sqrt(disc) : -sqrt(disc)));
                tau[0] = h / qa; tv[0] = true;
                if (h != 0.0) { tau[1] = qc / h; tv[1] = true; }
            }
        } else if (qb != 0.0) {
            tau[0] = -qc / qb; tv[0] = true;
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int slot = pl * 2 + r;
            if (!tv[r] || !(tau[r] > 0)) continue;
            const double den = 1.0 + tau[r] * tau[r] - 2.0 * b23 * tau[r];
            if (!(den > 0)) continue;
            double L[3];
            L[1] = sqrt(a23 / den);
            L[2] = tau[r] * L[1];
            L[0] = w0 * L[1] + w1 * L[2];
            if (!(L[0] > 0)) continue;
#pragma unroll
            for (int it = 0; it < 3; ++it) {                        // Gauss-Newton on the three distance equations
                const double r12 = L[0] * L[0] + L[1] * L[1] - 2.0 * b12 * L[0] * L[1] - a12;
                const double r13 = L[0] * L[0] + L[2] * L[2] - 2.0 * b13 * L[0] * L[2] - a13;
                const double r23 = L[1] * L[1] + L[2] * L[2] - 2.0 * b23 * L[1] * L[2] - a23;
                const double J0[3] = {2 * L[0] - 2 * b12 * L[1], 2 * L[1] - 2 * b12 * L[0], 0};
                const double J1[3] = {2 * L[0] - 2 * b13 * L[2], 0, 2 * L[2] - 2 * b13 * L[0]};
                const double J2[3] = {0, 2 * L[1] - 2 * b23 * L[2], 2 * L[2] - 2 * b23 * L[1]};
                double c12[3], c20[3], c01[3];                      // rows J0, J1, J2: J^-1 columns are cross products / det
                cross3(J1, J2, c12);
                cross3(J2, J0, c20);
                cross3(J0, J1, c01);
                const double dt = dot3(J0, c12);
                if (!(fabs(dt) > 1e-300)) break;
#pragma unroll
                for (int i = 0; i < 3; ++i) L[i] -= (c12[i] * r12 + c20[i] * r13 + c01[i] * r23) / dt;
            }
            double P1[3], e12[3], e13[3], ec[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                P1[i] = L[0] * y[0][i];
                e12[i] = P1[i] - L[1] * y[1][i];
                e13[i] = P1[i] - L[2] * y[2][i];
            }
            cross3(e12, e13, ec);
            // R = Y X^-1, Y = [e12 e13 ec] (columns), X^-1 rows Xi0 / nn, Xi1 / nn, n13 / nn
            double R[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) R[i * 3 + j] = (e12[i] * Xi0[j] + e13[i] * Xi1[j] + ec[i] * n13[j]) * Xinvn;
            double t[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = P1[i] - (R[i * 3] * X[0][0] + R[i * 3 + 1] * X[0][1] + R[i * 3 + 2] * X[0][2]);
            bool fin = true;
#pragma unroll
            for (int i = 0; i < 9; ++i) fin = fin && finite_d(R[i]);
#pragma unroll
            for (int i = 0; i < 3; ++i) fin = fin && finite_d(t[i]);
            if (!fin) continue;
#pragma unroll
            for (int i = 0; i < 9; ++i) P[slot][i] = R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) P[slot][9 + i] = t[i];
            ok[slot] = true;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- scoring
struct PoseF { float r[9], t[3]; };
__device__ __forceinline__ PoseF to_f32(const double R[9], const double t[3])
{
    PoseF p;
#pragma unroll
    for (int i = 0; i < 9; ++i) p.r[i] = (float)R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) p.t[i] = (float)t[i];
    return p;
}
// squared normalised reprojection error of one point, and whether it is an inlier (depth > 0, error <= th2)
__device__ __forceinline__ bool eval_f32(const PoseF &p, float4 X, float2 x, float th2, float &e)
{
    const float z = p.r[6] * X.x + p.r[7] * X.y + p.r[8] * X.z + p.t[2];
    const float px = p.r[0] * X.x + p.r[1] * X.y + p.r[2] * X.z + p.t[0];
    const float py = p.r[3] * X.x + p.r[4] * X.y + p.r[5] * X.z + p.t[1];
    const float iz = __builtin_amdgcn_rcpf(z);
    const float ex = px * iz - x.x, ey = py * iz - x.y;
    e = ex * ex + ey * ey;
    return (z > 0.f) & (e <= th2);
}

// one pose scored over every point by the whole workgroup (strided), totals in a fixed order
__device__ __forceinline__ PoseSupport score_wg(const PoseF &p, const float4 *Xf, const float2 *xf, int n, float th2, double *red, long long key)
{
    int cnt = 0;
    float sum = 0.f;
    for (int j = threadIdx.x; j < n; j += kWG) {
        float e;
        if (eval_f32(p, Xf[j], xf[j], th2, e)) { ++cnt; sum += e; }
    }
    double v[2] = {(double)cnt, (double)sum};
    wg_sum(v, red);
    PoseSupport s;
    s.cnt = (int)v[0];
    s.sum = (float)v[1];
    s.key = key;
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- kernel
// pose_focal_kernels.hip builds its sweep kernel from this text (one definition of P3P, the scoring and the round / LO / stop logic): it
// defines the two macros before it includes this file -- its own signature and problem set-up in front of the body, and its exit after step
// 4.  Here they spell pose_kernel out as it always was, so its code object does not change.
// What the body takes from a head, by name: red[kWaves * kNS] and sred[kWaves] (LDS); pi (the workgroup's index into hypg and res), tid; pb
// (PoseProbDev, for thresh2 and qt); off (added to mask_in / mask_out indices), n, cam; P2, P3, Xf, xf, xn (the problem's own); conf; hypg;
// mask_in, mask_out (may be null where conf.refine_only is 0 and the head returns in SFD2_POSE_AFTER_RANSAC); res (res[pi] is written for
// n < 4 before any exit of the head's: a second head gives it a record nobody reads).  SFD2_POSE_AFTER_RANSAC stands where found, best
// (cnt, sum) and trials are final and uniform over the workgroup.  An edit of the body that renames one of these breaks the second head.
#ifndef SFD2_POSE_KERNEL_HEAD
#define SFD2_POSE_KERNEL_IS_SOLVER
#define SFD2_POSE_AFTER_RANSAC
#define SFD2_POSE_KERNEL_HEAD \
__global__ __launch_bounds__(kWG) void pose_kernel(const PoseProbDev *__restrict__ probs, PoseConfDev conf, const double *__restrict__ p2,          \
                                                   const double *__restrict__ p3, float4 *__restrict__ xf4g, float2 *__restrict__ xf2g,             \
                                                   double2 *__restrict__ xng, double *__restrict__ hypg, const unsigned char *__restrict__ mask_in, \
                                                   unsigned char *__restrict__ mask_out, PoseResDev *__restrict__ res)                              \
{                                                                                                                                                   \
    __shared__ double red[kWaves * kNS];                                                                                                            \
    __shared__ PoseSupport sred[kWaves];                                                                                                            \
    const int pi = blockIdx.x, tid = threadIdx.x;                                                                                                   \
    const PoseProbDev &pb = probs[pi];                                                                                                              \
    const int64_t off = pb.off;                                                                                                                     \
    const int n = pb.n;                                                                                                                             \
    const PoseCam cam = pb.cam;                                                                                                                     \
    const double *P2 = p2 + 2 * off;                                                                                                                \
    const double *P3 = p3 + 3 * off;                                                                                                                \
    float4 *Xf = xf4g + off;                                                                                                                        \
    float2 *xf = xf2g + off;                                                                                                                        \
    double2 *xn = xng + off;
#endif
SFD2_POSE_KERNEL_HEAD
    PoseResDev out;
    out.q[0] = 1.0; out.q[1] = out.q[2] = out.q[3] = 0.0;
    out.t[0] = out.t[1] = out.t[2] = 0.0;
    out.success = 0; out.num_inliers = 0; out.num_trials = 0; out.pad = 0;
    if (n < 4) {
        if (mask_out)
            for (int j = tid; j < n; j += kWG) mask_out[off + j] = 0;
        if (tid == 0) res[pi] = out;
        return;
    }
    // ---- 1. preparation
    double c[3];
    {
        double v[3] = {0, 0, 0};
        for (int j = tid; j < n; j += kWG) { v[0] += P3[3 * j]; v[1] += P3[3 * j + 1]; v[2] += P3[3 * j + 2]; }
        wg_sum(v, red);
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = v[i] / n;
    }
    for (int j = tid; j < n; j += kWG) {
        double u, v;
        img_to_norm(cam, P2[2 * j], P2[2 * j + 1], u, v);
        xn[j] = make_double2(u, v);
        xf[j] = make_float2((float)u, (float)v);
        Xf[j] = make_float4((float)(P3[3 * j] - c[0]), (float)(P3[3 * j + 1] - c[1]), (float)(P3[3 * j + 2] - c[2]), 0.f);
    }
    __syncthreads();
    const float th2 = (float)pb.thresh2;
    double bR[9], bt[3];
    PoseSupport best;
    best.cnt = -1; best.sum = 0.f; best.key = 0x7fffffffffffffffll;
    int64_t trials = 0;
    if (conf.refine_only) {
        quat_to_rot(pb.qt[0], pb.qt[1], pb.qt[2], pb.qt[3], bR);
        // centred coordinates: x_cam = R (X - c) + (t + R c)
#pragma unroll
        for (int i = 0; i < 3; ++i) bt[i] = pb.qt[4 + i] + bR[i * 3] * c[0] + bR[i * 3 + 1] * c[1] + bR[i * 3 + 2] * c[2];
        double v[1] = {0};
        for (int j = tid; j < n; j += kWG) v[0] += mask_in[off + j] ? 1.0 : 0.0;
        wg_sum(v, red);
        best.cnt = (int)v[0];
    } else {
        // ---- 2-4. LO-RANSAC
        double *hyp = hypg + (size_t)pi * kWG * 4 * kHypD;
        for (int64_t round = 0;; ++round) {
            const int64_t trial = round * kWG + tid;
            PoseSupport mine;
            mine.cnt = -1; mine.sum = 0.f; mine.key = 0x7fffffffffffffffll;
            if (trial < conf.max_trials) {
                int id[3];
                sample_k<3>(conf.seed, trial, n, id);
                double y[3][3], X[3][3];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const double2 u = xn[id[s]];
                    const double inv = 1.0 / sqrt(u.x * u.x + u.y * u.y + 1.0);
                    y[s][0] = u.x * inv; y[s][1] = u.y * inv; y[s][2] = inv;
#pragma unroll
                    for (int i = 0; i < 3; ++i) X[s][i] = P3[3 * id[s] + i] - c[i];
                }
                double P[4][kHypD];
                bool ok[4];
                p3p(y, X, P, ok);
                PoseF pf[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if (!ok[s]) {                                   // no pose: every depth -1, never an inlier
#pragma unroll
                        for (int i = 0; i < 9; ++i) P[s][i] = 0.0;
                        P[s][9] = P[s][10] = 0.0; P[s][11] = -1.0;
                    }
                    pf[s] = to_f32(P[s], P[s] + 9);
#pragma unroll
                    for (int i = 0; i < kHypD; ++i) hyp[((size_t)tid * 4 + s) * kHypD + i] = P[s][i];
                }
                int cnt[4] = {0, 0, 0, 0};
                float sum[4] = {0.f, 0.f, 0.f, 0.f};
                if (ok[0] | ok[1] | ok[2] | ok[3]) {
                    for (int j = 0; j < n; ++j) {                   // j is wave-uniform: one load per wave and point
                        const float4 Xj = Xf[j];
                        const float2 xj = xf[j];
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            float e;
                            const bool in = eval_f32(pf[s], Xj, xj, th2, e);
                            cnt[s] += in ? 1 : 0;
                            sum[s] += in ? e : 0.f;
                        }
                    }
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    PoseSupport h;
                    h.cnt = ok[s] ? cnt[s] : -1;
                    h.sum = sum[s];
                    h.key = trial * 4 + s;
                    if (ok[s] && better(h, mine)) mine = h;
                }
            }
            const PoseSupport win = wg_best(mine, sred);       // (its barriers also publish the stored hypotheses)
            if (win.cnt >= 0 && better(win, best)) {
                const int wt = (int)((win.key >> 2) - round * kWG), ws = (int)(win.key & 3);
                const double *h = hyp + ((size_t)wt * 4 + ws) * kHypD;
#pragma unroll
                for (int i = 0; i < 9; ++i) bR[i] = h[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) bt[i] = h[9 + i];
                best = win;
                // ---- local optimisation over the best pose's inliers
                orthonormalise(bR);
                for (int lo = 0; lo < kLoSteps; ++lo) {
                    const PoseF bf = to_f32(bR, bt);
                    double R[9], t[3];
#pragma unroll
                    for (int i = 0; i < 9; ++i) R[i] = bR[i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) t[i] = bt[i];
                    bool good = true;
                    for (int gn = 0; gn < kLoGN && good; ++gn) {
                        double s[27];
#pragma unroll
                        for (int i = 0; i < 27; ++i) s[i] = 0.0;
                        for (int j = tid; j < n; j += kWG) {
                            float e;
                            if (!eval_f32(bf, Xf[j], xf[j], th2, e)) continue;
                            double Xc[3];
#pragma unroll
                            for (int i = 0; i < 3; ++i) Xc[i] = P3[3 * j + i] - c[i];
                            double Pc[3];
#pragma unroll
                            for (int i = 0; i < 3; ++i) Pc[i] = R[i * 3] * Xc[0] + R[i * 3 + 1] * Xc[1] + R[i * 3 + 2] * Xc[2] + t[i];
                            if (!(Pc[2] > 0)) continue;
                            const double iz = 1.0 / Pc[2], u = Pc[0] * iz, v = Pc[1] * iz;
                            const double2 x = xn[j];
                            const double g0[3] = {iz, 0.0, -u * iz}, g1[3] = {0.0, iz, -v * iz};
                            double j0[6], j1[6];
                            cross3(Pc, g0, j0);
                            cross3(Pc, g1, j1);
#pragma unroll
                            for (int i = 0; i < 3; ++i) { j0[3 + i] = g0[i]; j1[3 + i] = g1[i]; }
                            acc_normal(s, j0, j1, u - x.x, v - x.y, 1.0);
                        }
                        wg_sum(s, red);
                        double d[6];
                        good = chol_solve<kNP>(s, 0.0, d);
                        if (good) apply_update(R, t, d);
                    }
                    if (!good) break;
                    const PoseSupport ls = score_wg(to_f32(R, t), Xf, xf, n, th2, red, best.key);
                    if (!(ls.cnt > best.cnt || (ls.cnt == best.cnt && ls.sum < best.sum))) break;
                    best.cnt = ls.cnt;
                    best.sum = ls.sum;
#pragma unroll
                    for (int i = 0; i < 9; ++i) bR[i] = R[i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) bt[i] = t[i];
                }
            }
            // ---- stopping (COLMAP ComputeNumTrials on the best inlier ratio, multiplier 3)
            trials = min((round + 1) * kWG, conf.max_trials);
            // (the power is spelt out, not pow(): its last bit reaches num_trials)
            if (ransac_enough(trials, conf, n, best.cnt, [](double r) { return r * r * r; })) break;
            __syncthreads();                                  // the next round overwrites the stored hypotheses
        }
        out.num_trials = (int)trials;
    }
    const bool found = best.cnt >= 3;
    SFD2_POSE_AFTER_RANSAC
    // ---- RANSAC inliers (the reported mask and count), or the given mask
    const PoseF bf = to_f32(bR, bt);
    if (!conf.refine_only) {
        for (int j = tid; j < n; j += kWG) {
            float e;
            mask_out[off + j] = (found && eval_f32(bf, Xf[j], xf[j], th2, e)) ? 1 : 0;
        }
    }
    if (!found) {
        if (tid == 0) res[pi] = out;
        return;
    }
    // ---- 5. refinement: Levenberg-Marquardt on the Cauchy loss (scale 1 px) in pixels, fp64
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = bR[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = bt[i];
    orthonormalise(R);
    const unsigned char *msk = conf.refine_only ? mask_in : mask_out;
    auto accumulate = [&](const double (&Rc)[9], const double (&tc)[3], double (&s)[28]) {
#pragma unroll
        for (int i = 0; i < 28; ++i) s[i] = 0.0;
        for (int j = tid; j < n; j += kWG) {
            if (!msk[off + j]) continue;
            double Xc[3], Pc[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) Xc[i] = P3[3 * j + i] - c[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) Pc[i] = Rc[i * 3] * Xc[0] + Rc[i * 3 + 1] * Xc[1] + Rc[i * 3 + 2] * Xc[2] + tc[i];
            if (!(Pc[2] > 0)) continue;
            const double iz = 1.0 / Pc[2], u = Pc[0] * iz, v = Pc[1] * iz;
            double ud, vd, Jd[4];
            distort(cam, u, v, ud, vd, Jd);
            const double r0 = cam.f[0] * ud + cam.c[0] - P2[2 * j], r1 = cam.f[1] * vd + cam.c[1] - P2[2 * j + 1];
            const double sq = r0 * r0 + r1 * r1;
            const double w = 1.0 / (1.0 + sq);
            // d pixel / d P = diag(f) Jd [[iz, 0, -u iz], [0, iz, -v iz]]
            const double g0[3] = {cam.f[0] * Jd[0] * iz, cam.f[0] * Jd[1] * iz, -cam.f[0] * (Jd[0] * u + Jd[1] * v) * iz};
            const double g1[3] = {cam.f[1] * Jd[2] * iz, cam.f[1] * Jd[3] * iz, -cam.f[1] * (Jd[2] * u + Jd[3] * v) * iz};
            double j0[6], j1[6];
            cross3(Pc, g0, j0);
            cross3(Pc, g1, j1);
#pragma unroll
            for (int i = 0; i < 3; ++i) { j0[3 + i] = g0[i]; j1[3 + i] = g1[i]; }
            acc_normal(s, j0, j1, r0, r1, w);
            s[27] += log1p(sq);
        }
        wg_sum(s, red);
    };
    double s[28];
    accumulate(R, t, s);
    double lambda = 1e-4;
    for (int it = 0; it < kRefIters; ++it) {
        double d[6];
        if (!chol_solve<kNP>(s, lambda, d)) break;
        double Rn[9], tn[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) Rn[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) tn[i] = t[i];
        apply_update(Rn, tn, d);
        double sn[28];
        accumulate(Rn, tn, sn);
        const double step = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] +
                            (d[3] * d[3] + d[4] * d[4] + d[5] * d[5]) / (1.0 + t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        if (finite_d(sn[27]) && sn[27] <= s[27]) {
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = tn[i];
#pragma unroll
            for (int i = 0; i < 28; ++i) s[i] = sn[i];
            lambda = fmax(lambda * 0.1, 1e-12);
            if (step < 1e-26) break;
        } else {
            lambda *= 10.0;
            if (lambda > 1e12 || step < 1e-26) break;
        }
    }
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) fin = fin && finite_d(R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) fin = fin && finite_d(t[i]);
    if (!fin) {                                               // keep the unrefined pose
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = bR[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = bt[i];
        orthonormalise(R);
    }
    if (tid == 0) {
        rot_to_quat(R, out.q);
        double Rq[9];
        quat_to_rot(out.q[0], out.q[1], out.q[2], out.q[3], Rq);
#pragma unroll
        for (int i = 0; i < 3; ++i) out.t[i] = t[i] - (Rq[i * 3] * c[0] + Rq[i * 3 + 1] * c[1] + Rq[i * 3 + 2] * c[2]);
        out.success = 1;
        out.num_inliers = best.cnt;
        res[pi] = out;
    }
}

}  // namespace

#ifdef SFD2_POSE_KERNEL_IS_SOLVER
void launch_pose(hipStream_t st, const PoseProbDev *probs, int k, const PoseConfDev &conf, const double *p2, const double *p3, float4 *xf4,
                 float2 *xf2, double2 *xn, double *hyp, const unsigned char *mask_in, unsigned char *mask_out, PoseResDev *res)
{
    hipLaunchKernelGGL(pose_kernel, dim3(k), dim3(kWG), 0, st, probs, conf, p2, p3, xf4, xf2, xn, hyp, mask_in, mask_out, res);
}
#endif
