// libsfd2hip: homography of a matched image pair (LO-RANSAC over the four-point solver, then a refinement on the one-sided transfer
// error), the device side of sfd2_homography_batch (api_homography.hip).  The estimator COLMAP runs next to E and F for every pair to
// tell a plane or a panorama from a general scene.  Built like fundamental_kernels.hip:
//
// One workgroup of SFD2_TV_WG threads owns one pair from start to end; a batch of pairs of any sizes is one launch.
//   1. preparation: each image's own Hartley normalisation, centroid c_i and scale s_i = sqrt(2) / mean distance to it; x' = s_i (x - c_i).
//      The error e = |x1 - pi(H x0)|^2 lives in image 1 alone, so it obeys e' = s1^2 e: th2 = (s1 max_error_px)^2.  NaN / inf: no inlier.
//   2. RANSAC rounds of SFD2_TV_WG trials, one per lane: the sample of trial i is drawn by sample_k<4> from (seed, i) only.  The
//      four-point solver (four_point.h) is closed form and lives in registers: no LDS workspace.  Its matrix is scored in fp64 over all
//      correspondences in point order.  Support order: more inliers, then the smaller sum of the inliers' errors, then the smaller
//      trial index.
//   3. local optimisation whenever a round improves the best support: kLoGN Gauss-Newton steps on the 8 parameters of a chart (the first
//      entry of largest magnitude held constant) over the best matrix's inliers, re-scored, repeated while the support grows (<= kLoSteps).
//   4. stopping: COLMAP's trial count (sample size 4, multiplier 3) after every round, clamped to [min_trials, max_trials].
//   5. final: Levenberg-Marquardt on the same chart and cost over the RANSAC inliers; H_px = T1^-1 H T0 at unit Frobenius norm, the
//      first entry of largest magnitude positive.  No decomposition, no pose.
// Shared with the other RANSAC kernels (ransac_common.h, ransac_math.h): the sampler, reductions, scoring loops, winner
// broadcast, Cholesky solve, stopping rule and output convention (finish_matrix).  Here: the solver call, the transfer error, the
// preparation, the chart with its residual and update, the LO loop and the Levenberg-Marquardt loop.
// Every reduction runs in a fixed order (wave butterflies, then the waves in index order) and nothing depends on another workgroup,
// so a pair's result depends on the pair and the seed only.  All loops are bounded.  No private segment, no spills.
#include "sfd2_internal.h"
#include "ransac_common.h"
#include "four_point.h"

namespace {

constexpr int kWG = SFD2_TV_WG;
constexpr int kWaves = kWG / 64;
constexpr int kLoSteps = 8;
constexpr int kLoGN = 3;
constexpr int kRefIters = 50;
constexpr int kNP = 8;               // parameters of the chart
constexpr int kNS = 45;              // 36 (upper triangle) + 8 (gradient) + 1 (cost)

// squared one-sided transfer error in image 1 (COLMAP's HomographyMatrixEstimator::Residuals); NaN or inf when the denominator is 0
SFD2_PD double transfer(const double H[9], double2 a, double2 b)
{
    const double w = H[6] * a.x + H[7] * a.y + H[8];
    const double dx = b.x - (H[0] * a.x + H[1] * a.y + H[2]) / w, dy = b.y - (H[3] * a.x + H[4] * a.y + H[5]) / w;
    return dx * dx + dy * dy;
}

// ---------------------------------------------------------------------------------------------------------------- the chart
// Entry `fix` of H (the first of largest magnitude, row-major) is held constant, the other eight in order are the parameters.
SFD2_PD bool make_chart(const double H[9], int &fix)
{
    fix = 0;
    double bf = fabs(H[0]);
#pragma unroll
    for (int q = 1; q < 9; ++q)
        if (fabs(H[q]) > bf) { bf = fabs(H[q]); fix = q; }
    return bf > 0 && finite_d(bf);
}
// residuals (x and y transfer differences) of one correspondence and their derivatives by the eight parameters
SFD2_PD void residual(const double H[9], int fix, double2 a, double2 b, double (&r)[2], double (&Jx)[kNP], double (&Jy)[kNP])
{
    const double iw = 1.0 / (H[6] * a.x + H[7] * a.y + H[8]);
    const double u = (H[0] * a.x + H[1] * a.y + H[2]) * iw, v = (H[3] * a.x + H[4] * a.y + H[5]) * iw;
    r[0] = u - b.x;
    r[1] = v - b.y;
    const double x[3] = {a.x * iw, a.y * iw, iw};
    const double gx[9] = {x[0], x[1], x[2], 0.0, 0.0, 0.0, -u * x[0], -u * x[1], -u * x[2]};
    const double gy[9] = {0.0, 0.0, 0.0, x[0], x[1], x[2], -v * x[0], -v * x[1], -v * x[2]};
#pragma unroll
    for (int m = 0; m < kNP; ++m) {                      // values, not places: a choice between places becomes an indexed load
        Jx[m] = m < fix ? gx[m] : gx[m + 1];
        Jy[m] = m < fix ? gy[m] : gy[m + 1];
    }
}
SFD2_PD void apply_update(double (&H)[9], int fix, const double (&d)[kNP])
{
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const double lo = d[q < kNP ? q : kNP - 1], hi = d[q > 0 ? q - 1 : 0];
        const double dq = q < fix ? lo : hi;
        if (q != fix) H[q] += dq;
    }
}

// ---------------------------------------------------------------------------------------------------------------- kernel
__global__ __launch_bounds__(kWG) void homography_kernel(const FmProbDev *__restrict__ probs, TvConfDev conf, const double *__restrict__ p0,
                                                         const double *__restrict__ p1, double2 *__restrict__ x0g, double2 *__restrict__ x1g,
                                                         unsigned char *__restrict__ mask_out, FmResDev *__restrict__ res)
{
    __shared__ double red[kWaves * kNS];
    __shared__ double shH[9];
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
    if (n < 4 || !(dist[0] > 0) || !(dist[1] > 0) || !finite_d(dist[0]) || !finite_d(dist[1])) {
        for (int j = tid; j < n; j += kWG) mask[j] = 0;
        if (tid == 0) res[pi] = out;
        return;
    }
    const double s0 = sqrt(2.0) / dist[0], s1 = sqrt(2.0) / dist[1];
    for (int j = tid; j < n; j += kWG) {
        x0[j] = make_double2(s0 * (p0[2 * (off + j)] - cen[0]), s0 * (p0[2 * (off + j) + 1] - cen[1]));
        x1[j] = make_double2(s1 * (p1[2 * (off + j)] - cen[2]), s1 * (p1[2 * (off + j) + 1] - cen[3]));
    }
    __syncthreads();
    const double th2 = (s1 * pb.max_error_px) * (s1 * pb.max_error_px);
    double bH[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) bH[i] = 0.0;
    Support best;
    best.cnt = -1; best.sum = 0.0; best.trial = 0x7fffffffffffffffll;
    int64_t trials = 0;

    // the normal equations of the chart over the correspondences `use` selects
    auto accumulate = [&](const double (&H)[9], int fix, double (&s)[kNS], auto use) {
#pragma unroll
        for (int i = 0; i < kNS; ++i) s[i] = 0.0;
        for (int j = tid; j < n; j += kWG) {
            const double2 a = x0[j], b = x1[j];
            if (!use(j, a, b)) continue;
            double r[2], Jx[kNP], Jy[kNP];
            residual(H, fix, a, b, r, Jx, Jy);
            normal_acc(s, Jx, r[0]);
            normal_acc(s, Jy, r[1]);
        }
        wg_sum(s, red);
    };

    for (int64_t round = 0;; ++round) {
        const int64_t trial = round * kWG + tid;
        const bool live = trial < conf.max_trials;
        // ---- 2. the four-point solver in registers, then the score of its matrix
        Support mine;
        mine.cnt = -1; mine.sum = 0.0; mine.trial = trial;
        double mH[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) mH[i] = 0.0;
        bool have = false;
        if (live) {
            int id[4];
            sample_k<4>(conf.seed, trial, n, id);
            double2 a[4], b[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) { a[s] = x0[id[s]]; b[s] = x1[id[s]]; }
            have = four_point(a, b, mH);
        }
        if (have) {
            score_lane(transfer, mH, x0, x1, n, th2, mine.cnt, mine.sum);
        }
        const Support win = wg_best(mine, sred);
        if (win.cnt >= 0 && better(win, best)) {
            publish_winner(win.trial == trial, mH, shH, bH);
            best = win;
            // ---- 3. local optimisation over the best matrix's inliers
            for (int lo = 0; lo < kLoSteps; ++lo) {
                int fix;
                bool good = make_chart(bH, fix);
                double Hn[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) Hn[i] = bH[i];
                for (int gn = 0; gn < kLoGN && good; ++gn) {
                    double s[kNS];
                    accumulate(Hn, fix, s, [&](int, double2 a, double2 b) { return transfer(bH, a, b) <= th2; });
                    double d[kNP];
                    good = chol_solve<kNP>(s, 0.0, d);
                    if (good) apply_update(Hn, fix, d);
                }
                if (!good) break;
                int cnt;
                double sum;
                score_wg(transfer, Hn, x0, x1, n, th2, red, cnt, sum);
                if (!(cnt > best.cnt || (cnt == best.cnt && sum < best.sum))) break;
                best.cnt = cnt;
                best.sum = sum;
#pragma unroll
                for (int i = 0; i < 9; ++i) bH[i] = Hn[i];
            }
        }
        // ---- 4. stopping (COLMAP ComputeNumTrials on the best inlier ratio, sample size 4, multiplier 3)
        trials = min((round + 1) * kWG, conf.max_trials);
        // (the power is spelt out, not pow(): its last bit reaches num_trials)
        if (ransac_enough(trials, conf, n, best.cnt, [](double r) { const double r2 = r * r; return r2 * r2; })) break;
        __syncthreads();                                      // shH and the reductions' LDS are reused by the next round
    }
    out.num_trials = (int)trials;
    // ---- 5. the RANSAC inliers and the refinement over them
    const bool found = best.cnt >= 4;
    for (int j = tid; j < n; j += kWG) mask[j] = (found && transfer(bH, x0[j], x1[j]) <= th2) ? 1 : 0;
    int fix;
    if (!found || !make_chart(bH, fix)) {
        if (tid == 0) res[pi] = out;
        return;
    }
    out.num_inliers = best.cnt;
    auto in_mask = [&](int j, double2, double2) { return mask[j] != 0; };   // a lane reads the entries it wrote
    double H[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = bH[i];
    {
        double s[kNS];
        accumulate(H, fix, s, in_mask);
        double lambda = 1e-4;
        for (int it = 0; it < kRefIters; ++it) {
            double d[kNP];
            if (!chol_solve<kNP>(s, lambda, d)) break;
            double Hc[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) Hc[i] = H[i];
            apply_update(Hc, fix, d);
            double sn[kNS];
            accumulate(Hc, fix, sn, in_mask);
            double step = 0;
#pragma unroll
            for (int i = 0; i < kNP; ++i) step += d[i] * d[i];
            if (finite_d(sn[kNS - 1]) && sn[kNS - 1] <= s[kNS - 1]) {
#pragma unroll
                for (int i = 0; i < 9; ++i) H[i] = Hc[i];
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
        // ---- 6. H_px = T1^-1 H T0, T_i = [s_i 0 -s_i cx; 0 s_i -s_i cy; 0 0 1]
        double G[9], P[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {                        // G = H T0
            G[r * 3] = s0 * H[r * 3];
            G[r * 3 + 1] = s0 * H[r * 3 + 1];
            G[r * 3 + 2] = H[r * 3 + 2] - s0 * (cen[0] * H[r * 3] + cen[1] * H[r * 3 + 1]);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {                        // P = T1^-1 G
            P[q] = G[q] / s1 + cen[2] * G[6 + q];
            P[3 + q] = G[3 + q] / s1 + cen[3] * G[6 + q];
            P[6 + q] = G[6 + q];
        }
        finish_matrix(P, best.cnt, conf, out);
        res[pi] = out;
    }
}

}  // namespace

void launch_homography(hipStream_t st, const FmProbDev *probs, int k, const TvConfDev &conf, const double *p0, const double *p1, double2 *x0,
                       double2 *x1, unsigned char *mask_out, FmResDev *res)
{
    hipLaunchKernelGGL(homography_kernel, dim3(k), dim3(kWG), 0, st, probs, conf, p0, p1, x0, x1, mask_out, res);
}
