// libsfd2hip: the four-point homography solver of homography_kernels.hip, closed form and in registers: for each
// image the projective basis that maps the canonical frame e1, e2, e3, (1 1 1) to the four sampled points -- lambda of
// [p1 p2 p3] lambda = p4 through cross and triple products, A = [lambda1 p1, lambda2 p2, lambda3 p3] -- and H = B adj(A) at unit
// Frobenius norm.  No pivoting and no dynamic indexing, so no workspace.
#pragma once
#include "sfd2_internal.h"

#ifndef SFD2_PD
#define SFD2_PD __host__ __device__ __forceinline__
#endif

namespace {

constexpr double kFourPointCollinear = 1e-12;   // a triple product at or below this times the three norms: three collinear points

SFD2_PD void fp_cross(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
SFD2_PD double fp_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The columns lambda_i p_i of the basis of four points (x, y, 1); false when three of them are collinear.
SFD2_PD bool four_point_basis(const double2 (&p)[4], double (&A)[3][3])
{
    const double p1[3] = {p[0].x, p[0].y, 1.0}, p2[3] = {p[1].x, p[1].y, 1.0}, p3[3] = {p[2].x, p[2].y, 1.0}, p4[3] = {p[3].x, p[3].y, 1.0};
    const double n1 = sqrt(fp_dot(p1, p1)), n2 = sqrt(fp_dot(p2, p2)), n3 = sqrt(fp_dot(p3, p3)), n4 = sqrt(fp_dot(p4, p4));
    double c23[3], c31[3], c12[3];
    fp_cross(p2, p3, c23);
    fp_cross(p3, p1, c31);
    fp_cross(p1, p2, c12);
    const double d = fp_dot(p1, c23);                     // [p1 p2 p3]
    const double t1 = fp_dot(p4, c23), t2 = fp_dot(p4, c31), t3 = fp_dot(p4, c12);       // [p4 p2 p3], [p1 p4 p3], [p1 p2 p4]
    const bool ok = fabs(d) > kFourPointCollinear * (n1 * n2 * n3) && fabs(t1) > kFourPointCollinear * (n4 * n2 * n3) &&
                    fabs(t2) > kFourPointCollinear * (n1 * n4 * n3) && fabs(t3) > kFourPointCollinear * (n1 * n2 * n4);
    const double l1 = t1 / d, l2 = t2 / d, l3 = t3 / d;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        A[r][0] = l1 * p1[r];
        A[r][1] = l2 * p2[r];
        A[r][2] = l3 * p3[r];
    }
    return ok;
}

// H (row-major, unit Frobenius norm) with b_i ~ H a_i for the four correspondences; false: no hypothesis.
SFD2_PD bool four_point(const double2 (&a)[4], const double2 (&b)[4], double (&H)[9])
{
    double A[3][3], B[3][3];
    const bool oka = four_point_basis(a, A);
    const bool okb = four_point_basis(b, B);
    const double a1[3] = {A[0][0], A[1][0], A[2][0]}, a2[3] = {A[0][1], A[1][1], A[2][1]}, a3[3] = {A[0][2], A[1][2], A[2][2]};
    double r1[3], r2[3], r3[3];                           // the rows of adj(A)
    fp_cross(a2, a3, r1);
    fp_cross(a3, a1, r2);
    fp_cross(a1, a2, r3);
    double nn = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            H[r * 3 + c] = B[r][0] * r1[c] + B[r][1] * r2[c] + B[r][2] * r3[c];
            nn += H[r * 3 + c] * H[r * 3 + c];
        }
    const double inv = 1.0 / sqrt(nn);
    bool fin = __builtin_isfinite(inv);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        H[i] *= inv;
        fin = fin && __builtin_isfinite(H[i]);
    }
    return oka && okb && fin;
}

}  // namespace
