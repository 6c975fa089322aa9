// libsfd2hip: fundamental matrix of a matched image pair without any camera (LO-RANSAC over the seven-point solver, then a refinement
// on the Sampson error), the device side of sfd2_fundamental_batch (api_fundamental.hip).  The estimator COLMAP runs for a pair without
// a trusted focal length (EstimateUncalibrated).  Built like two_view_kernels.hip:
//
// One workgroup of SFD2_TV_WG threads owns one pair from start to end; a batch of pairs of any sizes is one launch.
//   1. preparation: the centroids of both point sets and one common isotropic scale s = sqrt(2) / mean of the two mean distances to the
//      centroid; x' = s (x - c_i).  With a common scale the squared Sampson error obeys e' = s^2 e, so everything runs in normalised
//      coordinates against th2 = (s max_error_px)^2.
//   2. RANSAC rounds of SFD2_TV_WG trials, one per lane: the sample of trial i is drawn by sample_k<7> from (seed, i) only.  The
//      seven-point solver (seven_point.h) keeps its 7 x 9 system in LDS (element e of lane l at ws[e * SFD2_TV_WG + l], 126 KiB), the
//      null space and the cubic in registers.  Each of its <= 3 matrices is scored in fp64 over all correspondences in point order.
//      Support order: more inliers, then the smaller sum of the inliers' squared Sampson errors, then the smaller trial index.
//   3. local optimisation whenever a round improves the best support: kLoGN Gauss-Newton steps on the 7 parameters of a rank-2 chart
//      (two rows, one entry held constant, the third row a r_i + b r_j) over the best matrix's inliers, re-scored, repeated while
//      the support grows (<= kLoSteps).
//   4. stopping: COLMAP's trial count (sample size 7, multiplier 3) after every round, clamped to [min_trials, max_trials].
//   5. final: Levenberg-Marquardt on the same chart and cost over the RANSAC inliers; F_px = T1^T F T0 at unit Frobenius norm, the first
//      entry of largest magnitude positive.  No cheirality test, no pose.
// Shared with the other RANSAC kernels (ransac_common.h, ransac_math.h): the sampler, reductions, winner broadcast,
// Cholesky solve, stopping rule and output convention (finish_matrix).  Here: the solver call, the Sampson error and the scoring loops,
// the preparation, the chart with its residual and update, the LO loop and the Levenberg-Marquardt loop.
// Every reduction runs in a fixed order (wave butterflies, then the waves in index order) and nothing depends on another workgroup,
// so a pair's result depends on the pair and the seed only.  All loops are bounded.  No private segment, no spills.
#include "sfd2_internal.h"
#include "ransac_common.h"
#include "seven_point.h"

namespace {

constexpr int kWG = SFD2_TV_WG;
constexpr int kWaves = kWG / 64;
constexpr int kLoSteps = 8;
constexpr int kLoGN = 3;
constexpr int kRefIters = 50;
constexpr int kNP = 7;               // parameters of the chart
constexpr int kNS = 36;              // normal equations: 28 (upper triangle) + 7 (gradient) + 1 (cost)

// squared Sampson error of x1^T F x0 (COLMAP's ComputeSquaredSampsonError)
SFD2_PD double sampson(const double F[9], double2 a, double2 b)
{
    const double e0 = F[0] * a.x + F[1] * a.y + F[2], e1 = F[3] * a.x + F[4] * a.y + F[5], e2 = F[6] * a.x + F[7] * a.y + F[8];
    const double f0 = F[0] * b.x + F[3] * b.y + F[6], f1 = F[1] * b.x + F[4] * b.y + F[7];
    const double C = b.x * e0 + b.y * e1 + e2;
    return C * C / (e0 * e0 + e1 * e1 + f0 * f0 + f1 * f1);
}

// ---------------------------------------------------------------------------------------------------------------- the rank-2 chart
// Row k = a r_i + b r_j, i < j the other two rows; of the six entries f[] = (r_i, r_j) entry `fix` is held constant.
struct Chart {
    int k, fix;
    double f[6], a, b;
};
SFD2_PD void get_row(const double M[9], int r, double o[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {                       // values, not places: a choice between places becomes an indexed load
        const double m0 = M[c], m1 = M[3 + c], m2 = M[6 + c];
        o[c] = r == 0 ? m0 : r == 1 ? m1 : m2;
    }
}
SFD2_PD double cross_n2(const double a[3], const double b[3])
{
    const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
    return x * x + y * y + z * z;
}
// k: the row whose two others have the largest |r_i x r_j| (the first on a tie); (a, b) by least squares; fix: the first largest |f|
SFD2_PD bool make_chart(const double F[9], Chart &c)
{
    const double n0 = cross_n2(F + 3, F + 6), n1 = cross_n2(F, F + 6), n2 = cross_n2(F, F + 3);
    c.k = 0;
    double bn = n0;
    if (n1 > bn) { bn = n1; c.k = 1; }
    if (n2 > bn) { bn = n2; c.k = 2; }
    const int i = c.k == 0 ? 1 : 0, j = c.k == 2 ? 1 : 2;
    double rk[3];
    get_row(F, i, c.f);
    get_row(F, j, c.f + 3);
    get_row(F, c.k, rk);
    const double m11 = c.f[0] * c.f[0] + c.f[1] * c.f[1] + c.f[2] * c.f[2], m12 = c.f[0] * c.f[3] + c.f[1] * c.f[4] + c.f[2] * c.f[5],
                 m22 = c.f[3] * c.f[3] + c.f[4] * c.f[4] + c.f[5] * c.f[5];
    const double b1 = c.f[0] * rk[0] + c.f[1] * rk[1] + c.f[2] * rk[2], b2 = c.f[3] * rk[0] + c.f[4] * rk[1] + c.f[5] * rk[2];
    const double det = m11 * m22 - m12 * m12;
    c.a = (b1 * m22 - b2 * m12) / det;
    c.b = (m11 * b2 - m12 * b1) / det;
    c.fix = 0;
    double bf = fabs(c.f[0]);
#pragma unroll
    for (int q = 1; q < 6; ++q)
        if (fabs(c.f[q]) > bf) { bf = fabs(c.f[q]); c.fix = q; }
    return finite_d(c.a) && finite_d(c.b) && bf > 0;
}
SFD2_PD void chart_matrix(const Chart &c, double F[9])
{
    const int i = c.k == 0 ? 1 : 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double vi = c.f[q], vj = c.f[3 + q], vk = c.a * vi + c.b * vj;
            F[r * 3 + q] = r == c.k ? vk : r == i ? vi : vj;
        }
}
// residual C / sqrt(den) of one correspondence and its derivative by the seven parameters (the five free entries of f in order, a, b)
SFD2_PD void residual(const double F[9], const Chart &c, double2 a, double2 b, double &r, double (&J)[kNP])
{
    const double e0 = F[0] * a.x + F[1] * a.y + F[2], e1 = F[3] * a.x + F[4] * a.y + F[5], e2 = F[6] * a.x + F[7] * a.y + F[8];
    const double f0 = F[0] * b.x + F[3] * b.y + F[6], f1 = F[1] * b.x + F[4] * b.y + F[7];
    const double C = b.x * e0 + b.y * e1 + e2;
    const double den = e0 * e0 + e1 * e1 + f0 * f0 + f1 * f1;
    const double is = 1.0 / sqrt(den), c3 = C * is * is * is;
    r = C * is;
    const double x0[3] = {a.x, a.y, 1.0}, x1[3] = {b.x, b.y, 1.0}, ex[3] = {e0, e1, 0.0}, fx[3] = {f0, f1, 0.0};
    double g[9];                                        // d r / d F
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) g[i * 3 + j] = x1[i] * x0[j] * is - c3 * (ex[i] * x0[j] + fx[j] * x1[i]);
    const int i = c.k == 0 ? 1 : 0, j = c.k == 2 ? 1 : 2;
    double gi[3], gj[3], gk[3], J6[6];
    get_row(g, i, gi);
    get_row(g, j, gj);
    get_row(g, c.k, gk);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        J6[q] = gi[q] + c.a * gk[q];
        J6[3 + q] = gj[q] + c.b * gk[q];
    }
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        const double lo = J6[m], hi = J6[m + 1];
        J[m] = m < c.fix ? lo : hi;
    }
    J[5] = gk[0] * c.f[0] + gk[1] * c.f[1] + gk[2] * c.f[2];
    J[6] = gk[0] * c.f[3] + gk[1] * c.f[4] + gk[2] * c.f[5];
}
SFD2_PD void apply_update(Chart &c, const double (&d)[kNP])
{
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double lo = d[q < 5 ? q : 4], hi = d[q > 0 ? q - 1 : 0];
        const double dq = q < c.fix ? lo : hi;
        if (q != c.fix) c.f[q] += dq;
    }
    c.a += d[5];
    c.b += d[6];
}

// ---------------------------------------------------------------------------------------------------------------- kernel
__global__ __launch_bounds__(kWG) void fundamental_kernel(const FmProbDev *__restrict__ probs, TvConfDev conf, const double *__restrict__ p0,
                                                          const double *__restrict__ p1, double2 *__restrict__ x0g, double2 *__restrict__ x1g,
                                                          unsigned char *__restrict__ mask_out, FmResDev *__restrict__ res)
{
    __shared__ double ws[63 * kWG];
    __shared__ double red[kWaves * kNS];
    __shared__ double shF[9];
    __shared__ Support sred[kWaves];
    const int pi = blockIdx.x, tid = threadIdx.x;
    const FmProbDev &pb = probs[pi];
    const int64_t off = pb.off;
    const int n = pb.n;
    double2 *x0 = x0g + off, *x1 = x1g + off;
    unsigned char *mask = mask_out + off;
    FmResDev out;
#pragma unroll
    for (int i = 0; i < 9; ++i) out.F[i] = 0.0;
    out.success = 0; out.num_inliers = 0; out.num_trials = 0; out.pad = 0;
    // ---- 1. preparation
    double cen[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < n; j += kWG) {
        cen[0] += p0[2 * (off + j)]; cen[1] += p0[2 * (off + j) + 1];
        cen[2] += p1[2 * (off + j)]; cen[3] += p1[2 * (off + j) + 1];
    }
    wg_sum(cen, red);
#pragma unroll
    for (int i = 0; i < 4; ++i) cen[i] /= n;
    double dist[2] = {0.0, 0.0};
    for (int j = tid; j < n; j += kWG) {
        const double ax = p0[2 * (off + j)] - cen[0], ay = p0[2 * (off + j) + 1] - cen[1];
        const double bx = p1[2 * (off + j)] - cen[2], by = p1[2 * (off + j) + 1] - cen[3];
        dist[0] += sqrt(ax * ax + ay * ay);
        dist[1] += sqrt(bx * bx + by * by);
    }
    wg_sum(dist, red);
    dist[0] /= n;
    dist[1] /= n;
    if (n < 7 || !(dist[0] > 0) || !(dist[1] > 0) || !finite_d(dist[0]) || !finite_d(dist[1])) {
        for (int j = tid; j < n; j += kWG) mask[j] = 0;
        if (tid == 0) res[pi] = out;
        return;
    }
    const double sc = sqrt(2.0) / (0.5 * (dist[0] + dist[1]));
    for (int j = tid; j < n; j += kWG) {
        x0[j] = make_double2(sc * (p0[2 * (off + j)] - cen[0]), sc * (p0[2 * (off + j) + 1] - cen[1]));
        x1[j] = make_double2(sc * (p1[2 * (off + j)] - cen[2]), sc * (p1[2 * (off + j) + 1] - cen[3]));
    }
    __syncthreads();
    const double th2 = (sc * pb.max_error_px) * (sc * pb.max_error_px);
    double bF[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) bF[i] = 0.0;
    Support best;
    best.cnt = -1; best.sum = 0.0; best.trial = 0x7fffffffffffffffll;
    int64_t trials = 0;
    double *wsl = ws + tid;

    // one matrix scored by the whole workgroup (strided), totals in a fixed order
    auto score_wg = [&](const double (&F)[9], int &cnt, double &sum) {
        double v[2] = {0.0, 0.0};
        for (int j = tid; j < n; j += kWG) {
            const double e = sampson(F, x0[j], x1[j]);
            if (e <= th2) { v[0] += 1.0; v[1] += e; }
        }
        wg_sum(v, red);
        cnt = (int)v[0];
        sum = v[1];
    };
    // the normal equations of the chart over the correspondences `use` selects
    auto accumulate = [&](const Chart &c, double (&s)[kNS], auto use) {
        double F[9];
        chart_matrix(c, F);
#pragma unroll
        for (int i = 0; i < kNS; ++i) s[i] = 0.0;
        for (int j = tid; j < n; j += kWG) {
            const double2 a = x0[j], b = x1[j];
            if (!use(j, a, b)) continue;
            double r, J[kNP];
            residual(F, c, a, b, r, J);
            normal_acc(s, J, r);
        }
        wg_sum(s, red);
    };

    for (int64_t round = 0;; ++round) {
        const int64_t trial = round * kWG + tid;
        const bool live = trial < conf.max_trials;
        // ---- 2a. the seven-point solver, every lane on its own columns of the LDS workspace
        int ncand = 0;
        double Fs[3][9];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 9; ++i) Fs[c][i] = 0.0;
        if (live) {
            int id[7];
            sample_k<7>(conf.seed, trial, n, id);
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                const double2 a = x0[id[s]], b = x1[id[s]];
                seven_point_row<kWG>(wsl, s, a.x, a.y, b.x, b.y);
            }
            ncand = seven_point<kWG>(wsl, Fs);
        }
        // ---- 2b. score, one matrix at a time
        Support mine;
        mine.cnt = -1; mine.sum = 0.0; mine.trial = trial;
        double mF[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) mF[i] = 0.0;
        for (int c = 0; c < 3; ++c) {
            if (c >= ncand) break;
            double F[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const double f0 = Fs[0][i], f1 = Fs[1][i], f2 = Fs[2][i];
                F[i] = c == 0 ? f0 : c == 1 ? f1 : f2;
            }
            int cnt = 0;
            double sum = 0.0;
            for (int j = 0; j < n; ++j) {                   // j is wave-uniform: one load per wave and point
                const double e = sampson(F, x0[j], x1[j]);
                const bool in = e <= th2;
                cnt += in ? 1 : 0;
                sum += in ? e : 0.0;
            }
            if (cnt > mine.cnt || (cnt == mine.cnt && sum < mine.sum)) {
                mine.cnt = cnt;
                mine.sum = sum;
#pragma unroll
                for (int i = 0; i < 9; ++i) mF[i] = F[i];
            }
        }
        const Support win = wg_best(mine, sred);
        if (win.cnt >= 0 && better(win, best)) {
            publish_winner(win.trial == trial, mF, shF, bF);
            best = win;
            // ---- 3. local optimisation over the best matrix's inliers
            for (int lo = 0; lo < kLoSteps; ++lo) {
                Chart ch;
                bool good = make_chart(bF, ch);
                for (int gn = 0; gn < kLoGN && good; ++gn) {
                    double s[kNS];
                    accumulate(ch, s, [&](int, double2 a, double2 b) { return sampson(bF, a, b) <= th2; });
                    double d[kNP];
                    good = chol_solve<kNP>(s, 0.0, d);
                    if (good) apply_update(ch, d);
                }
                if (!good) break;
                double Fn[9];
                chart_matrix(ch, Fn);
                int cnt;
                double sum;
                score_wg(Fn, cnt, sum);
                if (!(cnt > best.cnt || (cnt == best.cnt && sum < best.sum))) break;
                best.cnt = cnt;
                best.sum = sum;
#pragma unroll
                for (int i = 0; i < 9; ++i) bF[i] = Fn[i];
            }
        }
        // ---- 4. stopping (COLMAP ComputeNumTrials on the best inlier ratio, sample size 7, multiplier 3)
        trials = min((round + 1) * kWG, conf.max_trials);
        // (the power is spelt out, not pow(): its last bit reaches num_trials)
        if (ransac_enough(trials, conf, n, best.cnt, [](double r) { const double r2 = r * r, r4 = r2 * r2; return r4 * r2 * r; })) break;
        __syncthreads();                                      // shF and the reductions' LDS are reused by the next round
    }
    out.num_trials = (int)trials;
    // ---- 5. the RANSAC inliers and the refinement over them
    const bool found = best.cnt >= 7;
    for (int j = tid; j < n; j += kWG) mask[j] = (found && sampson(bF, x0[j], x1[j]) <= th2) ? 1 : 0;
    Chart ch;
    if (!found || !make_chart(bF, ch)) {
        if (tid == 0) res[pi] = out;
        return;
    }
    out.num_inliers = best.cnt;
    auto in_mask = [&](int j, double2, double2) { return mask[j] != 0; };   // a lane reads the entries it wrote
    {
        double s[kNS];
        accumulate(ch, s, in_mask);
        double lambda = 1e-4;
        for (int it = 0; it < kRefIters; ++it) {
            double d[kNP];
            if (!chol_solve<kNP>(s, lambda, d)) break;
            Chart cn = ch;
            apply_update(cn, d);
            double sn[kNS];
            accumulate(cn, sn, in_mask);
            double step = 0;
#pragma unroll
            for (int i = 0; i < kNP; ++i) step += d[i] * d[i];
            if (finite_d(sn[35]) && sn[35] <= s[35]) {
                ch = cn;
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
    if (tid == 0) {
        // ---- 6. F_px = T1^T F T0, T_i = [s 0 -s cx; 0 s -s cy; 0 0 1]
        double F[9], G[9], P[9];
        chart_matrix(ch, F);
#pragma unroll
        for (int r = 0; r < 3; ++r) {                        // G = F T0
            G[r * 3] = sc * F[r * 3];
            G[r * 3 + 1] = sc * F[r * 3 + 1];
            G[r * 3 + 2] = F[r * 3 + 2] - sc * (cen[0] * F[r * 3] + cen[1] * F[r * 3 + 1]);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {                        // P = T1^T G
            P[q] = sc * G[q];
            P[3 + q] = sc * G[3 + q];
            P[6 + q] = G[6 + q] - sc * (cen[2] * G[q] + cen[3] * G[3 + q]);
        }
        finish_matrix(P, best.cnt, conf, out);
        res[pi] = out;
    }
}

}  // namespace

void launch_fundamental(hipStream_t st, const FmProbDev *probs, int k, const TvConfDev &conf, const double *p0, const double *p1, double2 *x0,
                        double2 *x1, unsigned char *mask_out, FmResDev *res)
{
    hipLaunchKernelGGL(fundamental_kernel, dim3(k), dim3(kWG), 0, st, probs, conf, p0, p1, x0, x1, mask_out, res);
}
