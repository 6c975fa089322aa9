// libsfd2hip: the five-point relative pose solver of two_view_kernels.hip (Nister, "An efficient solution to the five-point relative
// pose problem", PAMI 2004, in the action-matrix form of Stewenius, Engels and Nister, ISPRS 2006), fp64, pure arithmetic, also compiled
// for the host.
//
// One caller (a lane) owns one workspace of kFpWs doubles, element i at ws[i * S]: on the device the workspace lives in LDS with the
// lanes interleaved (S = slots), so that every runtime-indexed access is an LDS access and nothing needs the private segment.
//   in : ws[0 .. 44] the 5 x 9 epipolar system, row s = x1_s (x) x0_s, so that row . vec(E, row-major) = x1^T E x0
//   out: emit(E[9]) once per real solution, E row-major with unit Frobenius norm; the return value counts them (<= 10)
// Steps, each with a bounded trip count:
//   1. null space: Gauss-Jordan with full pivoting; a pivot <= 1e-12 * max|A| is a rank-deficient sample (no hypothesis).  The four
//      null vectors of the reduced system (free columns in ascending order) are orthonormalised by modified Gram-Schmidt; the one
//      least like an essential matrix becomes W (see there), the others X, Y, Z: E = x X + y Y + z Z + W.
//   2. the ten cubic constraints (2 E E^T - tr(E E^T) I) E = 0 and det E = 0 as a 10 x 20 matrix over the monomials
//      x^3 x^2y x^2z xy^2 xyz xz^2 y^3 y^2z yz^2 z^3 | x^2 xy xz y^2 yz z^2 x y z 1.
//   3. Gauss-Jordan on the first ten columns with partial pivoting; a pivot <= 1e-12 * max|M| gives no hypothesis.
//   4. the 10 x 10 action matrix of multiplication by x on the ten lower monomials (six rows of the reduced system, four unit rows),
//      reduced to Hessenberg form by elimination with pivoting.
//   5. its real eigenvalues by Francis' double-shift QR iteration (EISPACK hqr): at most kFpQrIts steps per eigenvalue with an
//      exceptional shift every tenth; complex pairs are dropped; if an eigenvalue does not converge the ones found so far stand.
//   6. per real eigenvalue the eigenvector by two steps of inverse iteration; its entries are the monomials at the solution, so
//      (x, y, z) = v[6 .. 8] / v[9]; a non-finite E is dropped.
// The elimination to a degree-10 polynomial in one unknown (Nister's own route) was built first and is not used: near a pure rotation
// it lost real roots that the eigenvalues keep.
#pragma once
#include <math.h>

#ifndef SFD2_PD
#define SFD2_PD __host__ __device__ __forceinline__
#endif

constexpr int kFpWs = 400;        // doubles of workspace per trial
constexpr int kFpN = 200;         // the null space basis, 4 x 9
constexpr int kFpT = 236;         // 64 doubles: Lambda (6 x 10), then the cross products (3 x 10), then the eigenvalues and one vector
constexpr int kFpA = 300;         // 100 doubles: the 10 x 10 action matrix (steps 4 to 6)
constexpr int kFpQrIts = 60;      // QR steps per eigenvalue at the most (an exceptional shift every tenth)
constexpr int kFpQrSteps = 610;   // QR steps and deflations in all
constexpr double kFpRankTol = 1e-12, kFpPivotTol = 1e-12;

template <int S, class Emit>
SFD2_PD int five_point(double *wp, Emit emit)
{
#define FPW(i) wp[(i) * S]
    // products of monomials: linear terms (x y z 1), quadratic ones (x^2 xy xz y^2 yz z^2 x y z 1), the order of step 2
    static constexpr unsigned char L2[16] = {0, 1, 2, 6, 1, 3, 4, 7, 2, 4, 5, 8, 6, 7, 8, 9};
    static constexpr unsigned char D3[40] = {0, 1, 2, 10, 1, 3, 4, 11, 2, 4, 5, 12, 3, 6, 7, 13, 4, 7, 8, 14, 5, 8, 9, 15, 10, 11, 12, 16, 11, 13, 14, 17, 12, 14, 15, 18, 16, 17, 18, 19};
    // ---- 1. null space
    double amax = 0;
    for (int i = 0; i < 45; ++i) amax = fmax(amax, fabs(FPW(i)));
    if (!(amax > 0) || !__builtin_isfinite(amax)) return 0;
    unsigned used = 0, pc = 0;
    for (int k = 0; k < 5; ++k) {
        double best = -1;
        int br = k, bc = 0;
        for (int r = k; r < 5; ++r)
            for (int c = 0; c < 9; ++c) {
                const double v = fabs(FPW(r * 9 + c));
                if (!((used >> c) & 1) && v > best) { best = v; br = r; bc = c; }
            }
        if (!(best > kFpRankTol * amax)) return 0;
        for (int c = 0; c < 9; ++c) { const double a = FPW(k * 9 + c); FPW(k * 9 + c) = FPW(br * 9 + c); FPW(br * 9 + c) = a; }
        const double inv = 1.0 / FPW(k * 9 + bc);
        for (int c = 0; c < 9; ++c) FPW(k * 9 + c) *= inv;
        for (int r = 0; r < 5; ++r) {
            if (r == k) continue;
            const double f = FPW(r * 9 + bc);
            for (int c = 0; c < 9; ++c) FPW(r * 9 + c) -= f * FPW(k * 9 + c);
            FPW(r * 9 + bc) = 0.0;
        }
        used |= 1u << bc;
        pc |= (unsigned)bc << (4 * k);
    }
    {
        int m = 0;
        for (int fc = 0; fc < 9; ++fc) {
            if ((used >> fc) & 1) continue;
            for (int c = 0; c < 9; ++c) FPW(kFpN + m * 9 + c) = 0.0;
            FPW(kFpN + m * 9 + fc) = 1.0;
            for (int k = 0; k < 5; ++k) FPW(kFpN + m * 9 + ((pc >> (4 * k)) & 15)) = -FPW(k * 9 + fc);
            ++m;
        }
        for (m = 0; m < 4; ++m) {
            for (int p = 0; p < m; ++p) {
                double d = 0;
                for (int c = 0; c < 9; ++c) d += FPW(kFpN + m * 9 + c) * FPW(kFpN + p * 9 + c);
                for (int c = 0; c < 9; ++c) FPW(kFpN + m * 9 + c) -= d * FPW(kFpN + p * 9 + c);
            }
            double nn = 0;
            for (int c = 0; c < 9; ++c) nn += FPW(kFpN + m * 9 + c) * FPW(kFpN + m * 9 + c);
            const double s = 1.0 / sqrt(nn);
            for (int c = 0; c < 9; ++c) FPW(kFpN + m * 9 + c) *= s;
        }
    }
    // The chart: W is the basis vector that is least like an essential matrix (largest |2 E E^T E - tr(E E^T) E|^2, the first on a
    // tie).  Near a pure rotation the matrices [t]x R0 of every t fill a 3-dimensional part of the null space with near-solutions;
    // with W outside it they lie at infinity of the chart W = 1 and the solutions proper stay isolated.
    {
        int worst = 3;
        double rmax = -1;
        for (int m = 0; m < 4; ++m) {
            double e[9], g[9], tr = 0, r = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i) e[i] = FPW(kFpN + m * 9 + i);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) g[i * 3 + j] = e[i * 3] * e[j * 3] + e[i * 3 + 1] * e[j * 3 + 1] + e[i * 3 + 2] * e[j * 3 + 2];
            tr = g[0] + g[4] + g[8];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double v = 2.0 * (g[i * 3] * e[j] + g[i * 3 + 1] * e[3 + j] + g[i * 3 + 2] * e[6 + j]) - tr * e[i * 3 + j];
                    r += v * v;
                }
            if (r > rmax) { rmax = r; worst = m; }
        }
        for (int c = 0; c < 9; ++c) { const double a = FPW(kFpN + worst * 9 + c); FPW(kFpN + worst * 9 + c) = FPW(kFpN + 27 + c); FPW(kFpN + 27 + c) = a; }
    }
    // ---- 2. constraints.  Lambda = E E^T - tr(E E^T) / 2 I (symmetric: 6 quadratic polynomials), rows 0 .. 8 = Lambda E, row 9 = det E
    for (int i = 0; i < 60; ++i) FPW(kFpT + i) = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            const int sy = i * 3 - (i * (i - 1)) / 2 + (j - i);
            for (int k = 0; k < 3; ++k)
                for (int la = 0; la < 4; ++la)
                    for (int lb = 0; lb < 4; ++lb)
                        FPW(kFpT + sy * 10 + L2[la * 4 + lb]) += FPW(kFpN + la * 9 + i * 3 + k) * FPW(kFpN + lb * 9 + j * 3 + k);
        }
    for (int m = 0; m < 10; ++m) {
        const double h = 0.5 * (FPW(kFpT + m) + FPW(kFpT + 30 + m) + FPW(kFpT + 50 + m));
        FPW(kFpT + m) -= h;
        FPW(kFpT + 30 + m) -= h;
        FPW(kFpT + 50 + m) -= h;
    }
    for (int i = 0; i < 200; ++i) FPW(i) = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) {
                const int a = i < k ? i : k, b = i < k ? k : i;
                const int sy = a * 3 - (a * (a - 1)) / 2 + (b - a);
                for (int m = 0; m < 10; ++m)
                    for (int l = 0; l < 4; ++l)
                        FPW((i * 3 + j) * 20 + D3[m * 4 + l]) += FPW(kFpT + sy * 10 + m) * FPW(kFpN + l * 9 + k * 3 + j);
            }
    for (int i = 0; i < 30; ++i) FPW(kFpT + i) = 0.0;
    for (int a = 0; a < 3; ++a) {
        const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
        for (int la = 0; la < 4; ++la)
            for (int lb = 0; lb < 4; ++lb)
                FPW(kFpT + a * 10 + L2[la * 4 + lb]) += FPW(kFpN + la * 9 + 3 + a1) * FPW(kFpN + lb * 9 + 6 + a2) -
                                                        FPW(kFpN + la * 9 + 3 + a2) * FPW(kFpN + lb * 9 + 6 + a1);
        for (int m = 0; m < 10; ++m)
            for (int l = 0; l < 4; ++l) FPW(180 + D3[m * 4 + l]) += FPW(kFpT + a * 10 + m) * FPW(kFpN + l * 9 + a);
    }
    // ---- 3. Gauss-Jordan on the first ten columns
    double mmax = 0;
    for (int i = 0; i < 200; ++i) mmax = fmax(mmax, fabs(FPW(i)));
    if (!(mmax > 0) || !__builtin_isfinite(mmax)) return 0;
    for (int k = 0; k < 10; ++k) {
        double best = -1;
        int br = k;
        for (int r = k; r < 10; ++r) {
            const double v = fabs(FPW(r * 20 + k));
            if (v > best) { best = v; br = r; }
        }
        if (!(best > kFpPivotTol * mmax)) return 0;
        for (int c = k; c < 20; ++c) { const double a = FPW(k * 20 + c); FPW(k * 20 + c) = FPW(br * 20 + c); FPW(br * 20 + c) = a; }
        const double inv = 1.0 / FPW(k * 20 + k);
        for (int c = k; c < 20; ++c) FPW(k * 20 + c) *= inv;
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = FPW(r * 20 + k);
            for (int c = k; c < 20; ++c) FPW(r * 20 + c) -= f * FPW(k * 20 + c);
        }
    }
    // ---- 4. the action matrix of multiplication by x on the basis (x^2 xy xz y^2 yz z^2 x y z 1), reduced to Hessenberg form
#define FPA(i, j) FPW(kFpA + ((i) - 1) * 10 + ((j) - 1))      // 1-based, as the QR iteration below is usually written
    for (int i = 1; i <= 10; ++i)
        for (int j = 1; j <= 10; ++j) FPA(i, j) = i <= 6 ? -FPW((i - 1) * 20 + 9 + j) : 0.0;
    FPA(7, 1) = 1.0; FPA(8, 2) = 1.0; FPA(9, 3) = 1.0; FPA(10, 7) = 1.0;
    for (int m = 2; m < 10; ++m) {
        double x = 0.0;
        int i = m;
        for (int j = m; j <= 10; ++j)
            if (fabs(FPA(j, m - 1)) > fabs(x)) { x = FPA(j, m - 1); i = j; }
        if (i != m) {
            for (int j = m - 1; j <= 10; ++j) { const double a = FPA(i, j); FPA(i, j) = FPA(m, j); FPA(m, j) = a; }
            for (int j = 1; j <= 10; ++j) { const double a = FPA(j, i); FPA(j, i) = FPA(j, m); FPA(j, m) = a; }
        }
        if (x != 0.0)
            for (i = m + 1; i <= 10; ++i) {
                double y = FPA(i, m - 1);
                if (y != 0.0) {
                    y /= x;
                    for (int j = m; j <= 10; ++j) FPA(i, j) -= y * FPA(m, j);
                    for (int j = 1; j <= 10; ++j) FPA(j, m) += y * FPA(j, i);
                }
                FPA(i, m - 1) = 0.0;
            }
    }
    // ---- 5. its real eigenvalues: Francis' double-shift QR iteration (EISPACK hqr), at most kFpQrSteps steps in all
    constexpr int kWr = kFpT;                                 // the real eigenvalues found
    int nr = 0, nn = 10, its = 0;
    double t = 0.0, anorm = 0.0;
    for (int i = 1; i <= 10; ++i)
        for (int j = (i > 1 ? i - 1 : 1); j <= 10; ++j) anorm += fabs(FPA(i, j));
    if (!(anorm > 0) || !__builtin_isfinite(anorm)) return 0;
    for (int step = 0; step < kFpQrSteps && nn >= 1; ++step) {
        int l;
        for (l = nn; l >= 2; --l) {
            double s = fabs(FPA(l - 1, l - 1)) + fabs(FPA(l, l));
            if (s == 0.0) s = anorm;
            if (fabs(FPA(l, l - 1)) + s == s) { FPA(l, l - 1) = 0.0; break; }
        }
        double x = FPA(nn, nn);
        if (l == nn) {                                        // one root
            FPW(kWr + nr) = x + t; ++nr;
            --nn; its = 0;
            continue;
        }
        double y = FPA(nn - 1, nn - 1), w = FPA(nn, nn - 1) * FPA(nn - 1, nn);
        if (l == nn - 1) {                                    // two roots, real or a complex pair (dropped)
            const double p = 0.5 * (y - x), q = p * p + w;
            double z = sqrt(fabs(q));
            x += t;
            if (q >= 0.0) {
                z = p + (p >= 0.0 ? z : -z);
                FPW(kWr + nr) = x + z; ++nr;
                FPW(kWr + nr) = z != 0.0 ? x - w / z : x + z; ++nr;
            }
            nn -= 2; its = 0;
            continue;
        }
        if (its == kFpQrIts) break;                           // no convergence: the eigenvalues found so far stand
        if (its > 0 && its % 10 == 0) {                       // exceptional shift
            t += x;
            for (int i = 1; i <= nn; ++i) FPA(i, i) -= x;
            const double s = fabs(FPA(nn, nn - 1)) + fabs(FPA(nn - 1, nn - 2));
            y = x = 0.75 * s;
            w = -0.4375 * s * s;
        }
        ++its;
        int m;
        double p = 0, q = 0, r = 0, z;
        for (m = nn - 2; m >= l; --m) {
            z = FPA(m, m);
            r = x - z;
            double s = y - z;
            p = (r * s - w) / FPA(m + 1, m) + FPA(m, m + 1);
            q = FPA(m + 1, m + 1) - z - r - s;
            r = FPA(m + 2, m + 1);
            s = fabs(p) + fabs(q) + fabs(r);
            p /= s; q /= s; r /= s;
            if (m == l) break;
            const double u = fabs(FPA(m, m - 1)) * (fabs(q) + fabs(r));
            const double v = fabs(p) * (fabs(FPA(m - 1, m - 1)) + fabs(z) + fabs(FPA(m + 1, m + 1)));
            if (u + v == v) break;
        }
        for (int i = m + 2; i <= nn; ++i) {
            FPA(i, i - 2) = 0.0;
            if (i != m + 2) FPA(i, i - 3) = 0.0;
        }
        for (int k = m; k <= nn - 1; ++k) {
            if (k != m) {
                p = FPA(k, k - 1);
                q = FPA(k + 1, k - 1);
                r = k != nn - 1 ? FPA(k + 2, k - 1) : 0.0;
                x = fabs(p) + fabs(q) + fabs(r);
                if (x != 0.0) { p /= x; q /= x; r /= x; }
            }
            const double sq = sqrt(p * p + q * q + r * r), s = p >= 0.0 ? sq : -sq;
            if (s != 0.0) {
                if (k == m) {
                    if (l != m) FPA(k, k - 1) = -FPA(k, k - 1);
                } else
                    FPA(k, k - 1) = -s * x;
                p += s;
                x = p / s; y = q / s; z = r / s;
                q /= p; r /= p;
                for (int j = k; j <= nn; ++j) {
                    p = FPA(k, j) + q * FPA(k + 1, j);
                    if (k != nn - 1) { p += r * FPA(k + 2, j); FPA(k + 2, j) -= p * z; }
                    FPA(k + 1, j) -= p * y;
                    FPA(k, j) -= p * x;
                }
                const int mmin = nn < k + 3 ? nn : k + 3;
                for (int i = l; i <= mmin; ++i) {
                    p = x * FPA(i, k) + y * FPA(i, k + 1);
                    if (k != nn - 1) { p += z * FPA(i, k + 2); FPA(i, k + 2) -= p * r; }
                    FPA(i, k + 1) -= p * q;
                    FPA(i, k) -= p;
                }
            }
        }
    }
    // ---- 6. per real eigenvalue: the eigenvector by two steps of inverse iteration on the action matrix (Gaussian elimination with
    // partial pivoting, a vanishing pivot replaced by 1e-16 * its norm), (x, y, z) = v[6 .. 8] / v[9]
    constexpr int kV = kFpT + 10;                             // right-hand side / eigenvector
    int ne = 0;
    for (int ri = 0; ri < 10; ++ri) {
        if (ri >= nr) break;
        const double lam = FPW(kWr + ri);
        for (int i = 1; i <= 10; ++i) FPW(kV + i - 1) = 1.0;
        for (int it = 0; it < 2; ++it) {
            for (int i = 1; i <= 10; ++i)
                for (int j = 1; j <= 10; ++j) FPA(i, j) = (i <= 6 ? -FPW((i - 1) * 20 + 9 + j) : 0.0) - (i == j ? lam : 0.0);
            FPA(7, 1) += 1.0; FPA(8, 2) += 1.0; FPA(9, 3) += 1.0; FPA(10, 7) += 1.0;
            for (int k = 1; k <= 10; ++k) {
                int br = k;
                double best = -1;
                for (int i = k; i <= 10; ++i)
                    if (fabs(FPA(i, k)) > best) { best = fabs(FPA(i, k)); br = i; }
                if (br != k) {
                    for (int j = k; j <= 10; ++j) { const double a = FPA(k, j); FPA(k, j) = FPA(br, j); FPA(br, j) = a; }
                    const double a = FPW(kV + k - 1); FPW(kV + k - 1) = FPW(kV + br - 1); FPW(kV + br - 1) = a;
                }
                if (!(best > 1e-16 * anorm)) FPA(k, k) = 1e-16 * anorm;
                for (int i = k + 1; i <= 10; ++i) {
                    const double f = FPA(i, k) / FPA(k, k);
                    for (int j = k + 1; j <= 10; ++j) FPA(i, j) -= f * FPA(k, j);
                    FPW(kV + i - 1) -= f * FPW(kV + k - 1);
                }
            }
            double big = 0;
            for (int i = 10; i >= 1; --i) {
                double v = FPW(kV + i - 1);
                for (int j = i + 1; j <= 10; ++j) v -= FPA(i, j) * FPW(kV + j - 1);
                v /= FPA(i, i);
                FPW(kV + i - 1) = v;
                big = fmax(big, fabs(v));
            }
            for (int i = 0; i < 10; ++i) FPW(kV + i) /= big;
        }
        const double w = FPW(kV + 9), x = FPW(kV + 6) / w, y = FPW(kV + 7) / w, z = FPW(kV + 8) / w;
        double E[9], nn2 = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            E[i] = x * FPW(kFpN + i) + y * FPW(kFpN + 9 + i) + z * FPW(kFpN + 18 + i) + FPW(kFpN + 27 + i);
            nn2 += E[i] * E[i];
        }
        const double sc = 1.0 / sqrt(nn2);
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 9; ++i) { E[i] *= sc; fin = fin && __builtin_isfinite(E[i]); }
        if (!fin) continue;
        emit(E);
        ++ne;
    }
    return ne;
#undef FPA
#undef FPW
}
