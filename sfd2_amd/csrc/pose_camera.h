// libsfd2hip: the camera model shared by the pose kernels (pose_kernels.hip, two_view_kernels.hip), the 2D-3D assembly's reprojection gate
// (assemble_kernels.hip) and the SfM map kernels (tri_kernels.hip): COLMAP's cameras in OPENCV form (PoseCam, sfd2_internal.h), and the
// rotation <-> quaternion pair of the two pose kernels; fp64, pure arithmetic.
#pragma once
#include "sfd2_internal.h"

#define SFD2_PD __host__ __device__ __forceinline__   // pure arithmetic, also compiled for the host

// distortion of normalised (u, v) and its 2x2 Jacobian (OPENCV form; zero coefficients for the simpler models)
SFD2_PD void distort(const PoseCam &c, double u, double v, double &ud, double &vd, double J[4])
{
    const double u2 = u * u, v2 = v * v, uv = u * v, r2 = u2 + v2;
    const double rad = c.k1 * r2 + c.k2 * r2 * r2;
    const double drad = c.k1 + 2.0 * c.k2 * r2;            // d rad / d r2
    ud = u + u * rad + 2.0 * c.p1 * uv + c.p2 * (r2 + 2.0 * u2);
    vd = v + v * rad + 2.0 * c.p2 * uv + c.p1 * (r2 + 2.0 * v2);
    J[0] = 1.0 + rad + 2.0 * u2 * drad + 2.0 * c.p1 * v + 6.0 * c.p2 * u;
    J[1] = 2.0 * uv * drad + 2.0 * c.p1 * u + 2.0 * c.p2 * v;
    J[2] = 2.0 * uv * drad + 2.0 * c.p2 * v + 2.0 * c.p1 * u;
    J[3] = 1.0 + rad + 2.0 * v2 * drad + 2.0 * c.p2 * u + 6.0 * c.p1 * v;
}

constexpr int kPoseUndistIters = 100;   // COLMAP's IterativeUndistortion bound

// pixel -> normalised image coordinates (COLMAP CamFromImg / ImageToWorld)
SFD2_PD void img_to_norm(const PoseCam &c, double px, double py, double &u, double &v)
{
    const double xd = (px - c.c[0]) / c.f[0], yd = (py - c.c[1]) / c.f[1];
    u = xd;
    v = yd;
    if (!c.distorted) return;
    for (int it = 0; it < kPoseUndistIters; ++it) {
        double ud, vd, J[4];
        distort(c, u, v, ud, vd, J);
        const double fx = ud - xd, fy = vd - yd;
        const double det = J[0] * J[3] - J[1] * J[2];
        if (!(fabs(det) > 1e-300)) break;
        const double du = (J[3] * fx - J[1] * fy) / det, dv = (J[0] * fy - J[2] * fx) / det;
        u -= du;
        v -= dv;
        if (du * du + dv * dv < 1e-30) break;
    }
}

// camera-frame point -> pixel, no depth test (a point on or behind the image plane gives what the division gives)
SFD2_PD void project_px(const PoseCam &c, const double Pc[3], double &px, double &py)
{
    const double u = Pc[0] / Pc[2], v = Pc[1] / Pc[2];
    double ud, vd, J[4];
    distort(c, u, v, ud, vd, J);
    px = c.f[0] * ud + c.c[0];
    py = c.f[1] * vd + c.c[1];
}

// R (row-major) from a unit quaternion (w, x, y, z)
SFD2_PD void quat_to_rot(double w, double x, double y, double z, double R[9])
{
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}

// unit quaternion (w >= 0) of a (nearly) orthonormal R
SFD2_PD void rot_to_quat(const double R[9], double q[4])
{
    const double tr = R[0] + R[4] + R[8];
    double w, x, y, z;
    if (tr > 0) {
        const double s = 0.5 / sqrt(tr + 1.0);
        w = 0.25 / s; x = (R[7] - R[5]) * s; y = (R[2] - R[6]) * s; z = (R[3] - R[1]) * s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
        w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
        w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
        w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s;
    }
    const double nq = sqrt(w * w + x * x + y * y + z * z);
    const double sg = (w < 0 ? -1.0 : 1.0) / nq;
    q[0] = w * sg; q[1] = x * sg; q[2] = y * sg; q[3] = z * sg;
}
