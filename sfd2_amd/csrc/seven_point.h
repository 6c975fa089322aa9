// libsfd2hip: the seven-point fundamental matrix solver of fundamental_kernels.hip (Hartley & Zisserman, Multiple View Geometry,
// 11.1.2), pure arithmetic, also compiled for the host.
//   1. the 7 x 9 system of x1^T F x0 = 0 lies in the caller's workspace: element (r, c) at ws[(r * 9 + c) * STRIDE], so that the
//      lanes of a wave read consecutive doubles.  Only the system is indexed dynamically (by the pivoting); all else is registers.
//   2. Gauss-Jordan with full pivoting (the first largest entry in row-major order); a pivot <= kSpPivot max|A| ends the sample.
//      The two columns left over give the null space, made orthonormal by modified Gram-Schmidt.
//   3. chart F = x Y + W with Y the basis vector of the larger |det|; the cubic det(x Y + W) from the rows' mixed determinants;
//      a leading coefficient <= kSpLead of the largest coefficient ends the sample.
//   4. the real roots without complex arithmetic: the derivative's critical points cut [-B, B] (B: Cauchy's bound) into monotone
//      pieces; on each piece whose end values differ in sign a Newton iteration safeguarded by bisection (kSpIters steps at the
//      most), then kSpPolish plain Newton steps.  Roots come in ascending order of x, each matrix at unit Frobenius norm.
#pragma once

#ifndef SFD2_PD
#define SFD2_PD __host__ __device__ __forceinline__
#endif

constexpr double kSpPivot = 1e-12;
constexpr double kSpLead = 1e-12;
constexpr int kSpIters = 100;
constexpr int kSpPolish = 3;

SFD2_PD double sp_det3(const double a[3], const double b[3], const double c[3])
{
    return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// the row of the system for one correspondence a (image 0) -> b (image 1): vec(F) row-major
template <int STRIDE>
SFD2_PD void seven_point_row(double *ws, int r, double ax, double ay, double bx, double by)
{
    double *w = ws + (size_t)r * 9 * STRIDE;
    w[0 * STRIDE] = bx * ax; w[1 * STRIDE] = bx * ay; w[2 * STRIDE] = bx;
    w[3 * STRIDE] = by * ax; w[4 * STRIDE] = by * ay; w[5 * STRIDE] = by;
    w[6 * STRIDE] = ax;      w[7 * STRIDE] = ay;      w[8 * STRIDE] = 1.0;
}

// Solves the system in ws (destroyed).  Returns the number of matrices (0, 1 or 3 bar rounding) written to Fs[c][9].
template <int STRIDE>
SFD2_PD int seven_point(double *ws, double (&Fs)[3][9])
{
    double amax = 0;
    for (int e = 0; e < 63; ++e) amax = fmax(amax, fabs(ws[(size_t)e * STRIDE]));
    if (!(amax > 0) || !__builtin_isfinite(amax)) return 0;
    const double tiny = kSpPivot * amax;
    unsigned rows = 0, cols = 0;                        // bit sets of the rows and columns that have had a pivot
    unsigned long long pc_of_row = 0;                   // 4 bits per row: its pivot's column
    for (int k = 0; k < 7; ++k) {
        double best = -1.0;
        int pr = 0, pc = 0;
        for (int r = 0; r < 7; ++r) {
            if (rows >> r & 1) continue;
            for (int c = 0; c < 9; ++c) {
                if (cols >> c & 1) continue;
                const double v = fabs(ws[(size_t)(r * 9 + c) * STRIDE]);
                if (v > best) { best = v; pr = r; pc = c; }
            }
        }
        if (!(best > tiny)) return 0;
        rows |= 1u << pr;
        cols |= 1u << pc;
        pc_of_row |= (unsigned long long)pc << (4 * pr);
        const double inv = 1.0 / ws[(size_t)(pr * 9 + pc) * STRIDE];
        for (int c = 0; c < 9; ++c) ws[(size_t)(pr * 9 + c) * STRIDE] *= inv;
        ws[(size_t)(pr * 9 + pc) * STRIDE] = 1.0;
        for (int r = 0; r < 7; ++r) {
            if (r == pr) continue;
            const double f = ws[(size_t)(r * 9 + pc) * STRIDE];
            for (int c = 0; c < 9; ++c) ws[(size_t)(r * 9 + c) * STRIDE] -= f * ws[(size_t)(pr * 9 + c) * STRIDE];
            ws[(size_t)(r * 9 + pc) * STRIDE] = 0.0;
        }
    }
    // the two free columns f0 < f1: null vector of f has 1 at f, -A[r][f] at the pivot column of row r
    int f0 = -1, f1 = -1;
#pragma unroll
    for (int c = 0; c < 9; ++c)
        if (!(cols >> c & 1)) { if (f0 < 0) f0 = c; else f1 = c; }
    double u[9], v[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) { u[e] = e == f0 ? 1.0 : 0.0; v[e] = e == f1 ? 1.0 : 0.0; }
    for (int r = 0; r < 7; ++r) {
        const int pc = (int)(pc_of_row >> (4 * r) & 15);
        const double a = -ws[(size_t)(r * 9 + f0) * STRIDE], b = -ws[(size_t)(r * 9 + f1) * STRIDE];
#pragma unroll
        for (int e = 0; e < 9; ++e) { u[e] = e == pc ? a : u[e]; v[e] = e == pc ? b : v[e]; }
    }
    {   // modified Gram-Schmidt
        double s = 0;
#pragma unroll
        for (int e = 0; e < 9; ++e) s += u[e] * u[e];
        s = 1.0 / sqrt(s);
#pragma unroll
        for (int e = 0; e < 9; ++e) u[e] *= s;
        double d = 0;
#pragma unroll
        for (int e = 0; e < 9; ++e) d += u[e] * v[e];
#pragma unroll
        for (int e = 0; e < 9; ++e) v[e] -= d * u[e];
        s = 0;
#pragma unroll
        for (int e = 0; e < 9; ++e) s += v[e] * v[e];
        if (!(s > 0)) return 0;
        s = 1.0 / sqrt(s);
#pragma unroll
        for (int e = 0; e < 9; ++e) v[e] *= s;
    }
    const bool swap = fabs(sp_det3(v, v + 3, v + 6)) > fabs(sp_det3(u, u + 3, u + 6));
    double Y[9], W[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) { Y[e] = swap ? v[e] : u[e]; W[e] = swap ? u[e] : v[e]; }
    const double c3 = sp_det3(Y, Y + 3, Y + 6);
    const double c2 = sp_det3(W, Y + 3, Y + 6) + sp_det3(Y, W + 3, Y + 6) + sp_det3(Y, Y + 3, W + 6);
    const double c1 = sp_det3(Y, W + 3, W + 6) + sp_det3(W, Y + 3, W + 6) + sp_det3(W, W + 3, Y + 6);
    const double c0 = sp_det3(W, W + 3, W + 6);
    const double cmax = fmax(fmax(fabs(c3), fabs(c2)), fmax(fabs(c1), fabs(c0)));
    if (!__builtin_isfinite(cmax) || !(fabs(c3) > kSpLead * cmax)) return 0;
    const double B = 1.0 + fmax(fmax(fabs(c2), fabs(c1)), fabs(c0)) / fabs(c3);
    const double disc = c2 * c2 - 3.0 * c3 * c1;
    int npiece = 1;
    double xa = 0, xb = 0;                               // the critical points, ascending
    if (disc > 0) {
        const double q = -(c2 + (c2 < 0 ? -1.0 : 1.0) * sqrt(disc));
        const double r0 = q / (3.0 * c3), r1 = q != 0 ? c1 / q : r0;
        xa = fmin(r0, r1);
        xb = fmax(r0, r1);
        if (__builtin_isfinite(xa) && __builtin_isfinite(xb) && xa > -B && xb < B) npiece = 3;
    }
    auto poly = [&](double x) { return ((c3 * x + c2) * x + c1) * x + c0; };
    auto dpoly = [&](double x) { return (3.0 * c3 * x + 2.0 * c2) * x + c1; };
    int nroot = 0;
    for (int piece = 0; piece < 3; ++piece) {
        if (piece >= npiece) break;
        double lo = npiece == 1 ? -B : piece == 0 ? -B : piece == 1 ? xa : xb;
        double hi = npiece == 1 ? B : piece == 0 ? xa : piece == 1 ? xb : B;
        double flo = poly(lo);
        const double fhi = poly(hi);
        if ((flo < 0) == (fhi < 0)) continue;           // no sign change on this monotone piece
        double x = 0.5 * (lo + hi);
        for (int it = 0; it < kSpIters; ++it) {
            const double fx = poly(x);
            if (fx == 0) break;
            if ((fx < 0) == (flo < 0)) { lo = x; flo = fx; } else hi = x;
            double xn = x - fx / dpoly(x);
            if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
            const double step = fabs(xn - x);
            x = xn;
            if (step <= 4e-16 * fabs(x) || !(hi > lo)) break;
        }
#pragma unroll
        for (int it = 0; it < kSpPolish; ++it) {
            const double xn = x - poly(x) / dpoly(x);
            if (__builtin_isfinite(xn)) x = xn;
        }
        double F[9], s = 0;
#pragma unroll
        for (int e = 0; e < 9; ++e) { F[e] = x * Y[e] + W[e]; s += F[e] * F[e]; }
        s = 1.0 / sqrt(s);
        bool fin = __builtin_isfinite(s);
#pragma unroll
        for (int e = 0; e < 9; ++e) { F[e] *= s; fin = fin && __builtin_isfinite(F[e]); }
        if (!fin) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c == nroot)
#pragma unroll
                for (int e = 0; e < 9; ++e) Fs[c][e] = F[e];
        ++nroot;
    }
    return nroot;
}
