// libsfd2hip: bundle adjustment -- Levenberg-Marquardt over camera poses and 3D points with the points
// eliminated, the reduced camera system solved by matrix-free preconditioned conjugate gradients.  fp64 throughout.
//
// Every phase is a launch of its own; none waits on another workgroup, none uses a floating-point atomic.  Every sum has a fixed
// order: a point's sums run over its observations in the given order (one lane), or, beyond SFD2_BA_LONG_TRACK observations, as 64
// strided partial sums joined by a fixed tree (one wave); a view's sums run over its observations in ascending index as 256 strided
// partial sums joined by a fixed tree (one workgroup); the dot products over the 6 x n_views vectors are 1024 strided partial sums
// joined by a fixed tree (one workgroup).  The Jacobians are stored per observation by the linearisation (SFD2_BA_REC doubles) and read
// back by the products: the passes are bound by those bytes, not by the arithmetic.  Kernels queued behind a rejected step or a
// stopped PCG read one word of BaState and return.
#include "pose_camera.h"
#include "bundle.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- linearise
// residual, IRLS weight, the 2x6 and 2x3 Jacobians and the cost term of one observation per lane; FULL = false: the cost term only
template <bool FULL>
__global__ void __launch_bounds__(256) ba_linearise_kernel(const BaState *st, int gate, const double *__restrict__ pose, const PoseCam *__restrict__ cams,
                                                           const unsigned char *__restrict__ vconst, const unsigned char *__restrict__ pconst,
                                                           const double *__restrict__ xyz, const int32_t *__restrict__ obs_view,
                                                           const int32_t *__restrict__ obs_pt, const double2 *__restrict__ obs_xy, int64_t n, int loss,
                                                           double c2, double *__restrict__ rec, double *__restrict__ err, double *__restrict__ obs_cost)
{
    if (ba_gated(st, gate)) return;
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n) return;
    const int v = obs_view[o], j = obs_pt[o];
    const double *P = pose + 12 * (int64_t)v;
    const double R0 = P[0], R1 = P[1], R2 = P[2], R3 = P[3], R4 = P[4], R5 = P[5], R6 = P[6], R7 = P[7], R8 = P[8];
    const double X0 = xyz[3 * (int64_t)j], X1 = xyz[3 * (int64_t)j + 1], X2 = xyz[3 * (int64_t)j + 2];
    const double q0 = R0 * X0 + R1 * X1 + R2 * X2, q1 = R3 * X0 + R4 * X1 + R5 * X2, q2 = R6 * X0 + R7 * X1 + R8 * X2;   // R X
    const double pc0 = q0 + P[9], pc1 = q1 + P[10], pc2 = q2 + P[11];
    const PoseCam cam = cams[v];
    const double iz = 1.0 / pc2, u = pc0 * iz, w = pc1 * iz;
    double ud, vd, Jd[4];
    distort(cam, u, w, ud, vd, Jd);
    const double2 xy = obs_xy[o];
    const double rx = cam.f[0] * ud + cam.c[0] - xy.x, ry = cam.f[1] * vd + cam.c[1] - xy.y;
    const double s = rx * rx + ry * ry;
    double w2 = 1.0, rho = s;
    if (loss == 1) {                                         // Cauchy
        w2 = 1.0 / (1.0 + s / c2);
        rho = c2 * log1p(s / c2);
    }
    obs_cost[o] = 0.5 * rho;
    if (!FULL) return;
    err[o] = sqrt(s);
    const double sw = sqrt(w2);
    // A = sw diag(f) Jd [[iz, 0, -u iz], [0, iz, -w iz]]
    const double a0 = sw * cam.f[0], a1 = sw * cam.f[1];
    const double p02 = -u * iz, p12 = -w * iz;
    const double A00 = a0 * Jd[0] * iz, A01 = a0 * Jd[1] * iz, A02 = a0 * (Jd[0] * p02 + Jd[1] * p12);
    const double A10 = a1 * Jd[2] * iz, A11 = a1 * Jd[3] * iz, A12 = a1 * (Jd[2] * p02 + Jd[3] * p12);
    double *rc = rec + SFD2_BA_REC * o;
    const double vz = vconst[v] ? 0.0 : 1.0, pz = pconst[j] ? 0.0 : 1.0;
    // d(Exp(w) q) / dw = -[q]x
    rc[0] = vz * (A02 * q1 - A01 * q2);
    rc[1] = vz * (A00 * q2 - A02 * q0);
    rc[2] = vz * (A01 * q0 - A00 * q1);
    rc[3] = vz * A00; rc[4] = vz * A01; rc[5] = vz * A02;
    rc[6] = vz * (A12 * q1 - A11 * q2);
    rc[7] = vz * (A10 * q2 - A12 * q0);
    rc[8] = vz * (A11 * q0 - A10 * q1);
    rc[9] = vz * A10; rc[10] = vz * A11; rc[11] = vz * A12;
    rc[12] = pz * (A00 * R0 + A01 * R3 + A02 * R6);
    rc[13] = pz * (A00 * R1 + A01 * R4 + A02 * R7);
    rc[14] = pz * (A00 * R2 + A01 * R5 + A02 * R8);
    rc[15] = pz * (A10 * R0 + A11 * R3 + A12 * R6);
    rc[16] = pz * (A10 * R1 + A11 * R4 + A12 * R7);
    rc[17] = pz * (A10 * R2 + A11 * R5 + A12 * R8);
    rc[18] = sw * rx;
    rc[19] = sw * ry;
}

// ---------------------------------------------------------------------------------------------------------------- reductions
// blocks of SFD2_BA_RED_CHUNK elements -> one partial each; then one block over the partials.  The decomposition depends on n only.
__device__ __forceinline__ double ba_op(int op, double a, double x) { return op == SFD2_BA_OP_SUM ? a + x : fmax(a, fabs(x)); }

__global__ void __launch_bounds__(SFD2_BA_RED_WG) ba_reduce_partial_kernel(const BaState *st, int gate, const double *__restrict__ src, int64_t n, int op,
                                                                          double *__restrict__ partial)
{
    if (ba_gated(st, gate)) return;
    __shared__ double sh[SFD2_BA_RED_WG];
    const int t = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * SFD2_BA_RED_CHUNK;
    double a = 0.0;
    for (int i = t; i < SFD2_BA_RED_CHUNK; i += SFD2_BA_RED_WG)
        if (lo + i < n) a = ba_op(op, a, src[lo + i]);
    sh[t] = a;
    __syncthreads();
    for (int s = SFD2_BA_RED_WG / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = op == SFD2_BA_OP_SUM ? sh[t] + sh[t + s] : fmax(sh[t], sh[t + s]);
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = sh[0];
}

__global__ void __launch_bounds__(SFD2_BA_RED_WG) ba_reduce_final_kernel(const BaState *st, int gate, const double *__restrict__ partial, int64_t nb, int op,
                                                                        double *dst, int combine)
{
    if (ba_gated(st, gate)) return;
    __shared__ double sh[SFD2_BA_RED_WG];
    const int t = threadIdx.x;
    double a = 0.0;
    for (int64_t i = t; i < nb; i += SFD2_BA_RED_WG) a = op == SFD2_BA_OP_SUM ? a + partial[i] : fmax(a, partial[i]);
    sh[t] = a;
    __syncthreads();
    for (int s = SFD2_BA_RED_WG / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = op == SFD2_BA_OP_SUM ? sh[t] + sh[t + s] : fmax(sh[t], sh[t + s]);
        __syncthreads();
    }
    if (t == 0) *dst = combine ? fmax(*dst, sh[0]) : sh[0];
}

// ---------------------------------------------------------------------------------------------------------------- point-major
// a += (Jp^T Jp upper triangle, Jp^T r) of one record
__device__ __forceinline__ void ba_point_acc(const double *__restrict__ rc, double a[9])
{
    const double j0 = rc[12], j1 = rc[13], j2 = rc[14], k0 = rc[15], k1 = rc[16], k2 = rc[17], r0 = rc[18], r1 = rc[19];
    a[0] += j0 * j0 + k0 * k0; a[1] += j0 * j1 + k0 * k1; a[2] += j0 * j2 + k0 * k2;
    a[3] += j1 * j1 + k1 * k1; a[4] += j1 * j2 + k1 * k2; a[5] += j2 * j2 + k2 * k2;
    a[6] += j0 * r0 + k0 * r1; a[7] += j1 * r0 + k1 * r1; a[8] += j2 * r0 + k2 * r1;
}

// a += Jp^T (Jc x_view) of one record
__device__ __forceinline__ void ba_point_prod(const double *__restrict__ rc, const double *__restrict__ xv, double a[3])
{
    const double x0 = xv[0], x1 = xv[1], x2 = xv[2], x3 = xv[3], x4 = xv[4], x5 = xv[5];
    const double e0 = rc[0] * x0 + rc[1] * x1 + rc[2] * x2 + rc[3] * x3 + rc[4] * x4 + rc[5] * x5;
    const double e1 = rc[6] * x0 + rc[7] * x1 + rc[8] * x2 + rc[9] * x3 + rc[10] * x4 + rc[11] * x5;
    a[0] += rc[12] * e0 + rc[15] * e1;
    a[1] += rc[13] * e0 + rc[16] * e1;
    a[2] += rc[14] * e0 + rc[17] * e1;
}

__device__ __forceinline__ void ba_point_store_build(int64_t j, const double a[9], double *__restrict__ V, double *__restrict__ gp)
{
#pragma unroll
    for (int k = 0; k < 6; ++k) V[6 * j + k] = a[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) gp[3 * j + k] = a[6 + k];
}

__device__ __forceinline__ void ba_point_store_prod(int64_t j, const double a[3], const double *__restrict__ Vinv, double *__restrict__ z)
{
    const double *I = Vinv + 6 * j;                          // (00 01 02 11 12 22)
    z[3 * j] = I[0] * a[0] + I[1] * a[1] + I[2] * a[2];
    z[3 * j + 1] = I[1] * a[0] + I[3] * a[1] + I[4] * a[2];
    z[3 * j + 2] = I[2] * a[0] + I[4] * a[1] + I[5] * a[2];
}

// one lane per point of ids[n]
__global__ void __launch_bounds__(256) ba_point_build_lane_kernel(const BaState *st, int gate, const int32_t *__restrict__ ids, int n,
                                                                  const int64_t *__restrict__ off, const double *__restrict__ rec, double *__restrict__ V,
                                                                  double *__restrict__ gp)
{
    if (ba_gated(st, gate)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = ids[i];
    double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t o = off[j]; o < off[j + 1]; ++o) ba_point_acc(rec + SFD2_BA_REC * o, a);
    ba_point_store_build(j, a, V, gp);
}

// one wave per point of ids[]: lane l takes observations l, l + 64, ...
__global__ void __launch_bounds__(64) ba_point_build_wave_kernel(const BaState *st, int gate, const int32_t *__restrict__ ids,
                                                                 const int64_t *__restrict__ off, const double *__restrict__ rec, double *__restrict__ V,
                                                                 double *__restrict__ gp)
{
    if (ba_gated(st, gate)) return;
    __shared__ double sh[9 * 64];
    const int64_t j = ids[blockIdx.x];
    double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t o = off[j] + threadIdx.x; o < off[j + 1]; o += 64) ba_point_acc(rec + SFD2_BA_REC * o, a);
    ba_tree_sum<9, 64>(a, sh);
    if (threadIdx.x == 0) ba_point_store_build(j, a, V, gp);
}

__global__ void __launch_bounds__(256) ba_point_apply_lane_kernel(const BaState *st, int gate, const int32_t *__restrict__ ids, int n,
                                                                  const int64_t *__restrict__ off, const int32_t *__restrict__ obs_view,
                                                                  const double *__restrict__ rec, const double *__restrict__ x,
                                                                  const double *__restrict__ Vinv, double *__restrict__ z)
{
    if (ba_gated(st, gate)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = ids[i];
    double a[3] = {0, 0, 0};
    for (int64_t o = off[j]; o < off[j + 1]; ++o) ba_point_prod(rec + SFD2_BA_REC * o, x + 6 * (int64_t)obs_view[o], a);
    ba_point_store_prod(j, a, Vinv, z);
}

__global__ void __launch_bounds__(64) ba_point_apply_wave_kernel(const BaState *st, int gate, const int32_t *__restrict__ ids,
                                                                 const int64_t *__restrict__ off, const int32_t *__restrict__ obs_view,
                                                                 const double *__restrict__ rec, const double *__restrict__ x,
                                                                 const double *__restrict__ Vinv, double *__restrict__ z)
{
    if (ba_gated(st, gate)) return;
    __shared__ double sh[3 * 64];
    const int64_t j = ids[blockIdx.x];
    double a[3] = {0, 0, 0};
    for (int64_t o = off[j] + threadIdx.x; o < off[j + 1]; o += 64) ba_point_prod(rec + SFD2_BA_REC * o, x + 6 * (int64_t)obs_view[o], a);
    ba_tree_sum<3, 64>(a, sh);
    if (threadIdx.x == 0) ba_point_store_prod(j, a, Vinv, z);
}

// (V + lambda D)^-1 by a closed-form Cholesky, D = clamp(diag V, 1e-6, 1e32), and zg = that inverse times gp; one lane per point
__global__ void __launch_bounds__(256) ba_point_invert_kernel(const BaState *st, int n, const double *__restrict__ V, const double *__restrict__ gp,
                                                              double *__restrict__ Vinv, double *__restrict__ zg)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double lam = st->lambda;
    const double *v = V + 6 * j;
    const double a00 = v[0] + lam * fmin(fmax(v[0], 1e-6), 1e32), a10 = v[1], a20 = v[2];
    const double a11 = v[3] + lam * fmin(fmax(v[3], 1e-6), 1e32), a21 = v[4];
    const double a22 = v[5] + lam * fmin(fmax(v[5], 1e-6), 1e32);
    const double l00 = sqrt(a00), l10 = a10 / l00, l20 = a20 / l00;
    const double l11 = sqrt(a11 - l10 * l10), l21 = (a21 - l20 * l10) / l11;
    const double l22 = sqrt(a22 - l20 * l20 - l21 * l21);
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;     // L^-1: diagonal, then below it
    const double i10 = -l10 * m00 * m11, i21 = -l21 * m11 * m22, i20 = -(l20 * m00 + l21 * i10) * m22;
    const double I0 = m00 * m00 + i10 * i10 + i20 * i20, I1 = i10 * m11 + i20 * i21, I2 = i20 * m22;
    const double I3 = m11 * m11 + i21 * i21, I4 = i21 * m22, I5 = m22 * m22;
    double *I = Vinv + 6 * j;
    I[0] = I0; I[1] = I1; I[2] = I2; I[3] = I3; I[4] = I4; I[5] = I5;
    const double g0 = gp[3 * j], g1 = gp[3 * j + 1], g2 = gp[3 * j + 2];
    zg[3 * j] = I0 * g0 + I1 * g1 + I2 * g2;
    zg[3 * j + 1] = I1 * g0 + I3 * g1 + I4 * g2;
    zg[3 * j + 2] = I2 * g0 + I4 * g1 + I5 * g2;
}

// ---------------------------------------------------------------------------------------------------------------- view-major
// one workgroup per view: B = sum Jc^T Jc (stored full, 36) and gc = sum Jc^T r
__global__ void __launch_bounds__(SFD2_BA_VIEW_WG) ba_view_build_kernel(const BaState *st, int gate, const int64_t *__restrict__ voff,
                                                                       const int32_t *__restrict__ vobs, const double *__restrict__ rec,
                                                                       double *__restrict__ B, double *__restrict__ gc)
{
    if (ba_gated(st, gate)) return;
    __shared__ double sh[9 * SFD2_BA_VIEW_WG];
    const int v = blockIdx.x;
    double a[27];                                            // the upper triangle row by row (21), then Jc^T r (6)
#pragma unroll
    for (int k = 0; k < 27; ++k) a[k] = 0.0;
    for (int64_t i = voff[v] + threadIdx.x; i < voff[v + 1]; i += SFD2_BA_VIEW_WG) {
        const double *rc = rec + SFD2_BA_REC * (int64_t)vobs[i];
        double j0[6], j1[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { j0[k] = rc[k]; j1[k] = rc[6 + k]; }
        const double r0 = rc[18], r1 = rc[19];
        int s = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) a[s++] += j0[r] * j0[c] + j1[r] * j1[c];
#pragma unroll
        for (int k = 0; k < 6; ++k) a[21 + k] += j0[k] * r0 + j1[k] * r1;
    }
    ba_tree_sum<9, SFD2_BA_VIEW_WG>(a, sh);
    ba_tree_sum<9, SFD2_BA_VIEW_WG>(a + 9, sh);
    ba_tree_sum<9, SFD2_BA_VIEW_WG>(a + 18, sh);
    if (threadIdx.x == 0) {
        double *Bv = B + 36 * (int64_t)v;
        int s = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) { Bv[6 * r + c] = a[s]; Bv[6 * c + r] = a[s]; ++s; }
#pragma unroll
        for (int k = 0; k < 6; ++k) gc[6 * (int64_t)v + k] = a[21 + k];
    }
}

// the block-Jacobi preconditioner (B + lambda D)^-1 of a view by a 6x6 Cholesky, and the damping lambda D itself; one lane per view
__global__ void __launch_bounds__(64) ba_view_precond_kernel(const BaState *st, int n, const double *__restrict__ B, double *__restrict__ Minv,
                                                             double *__restrict__ Dd)
{
    const int64_t v = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (v >= n) return;
    const double lam = st->lambda;
    double L[6][6], Y[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) L[r][c] = B[36 * v + 6 * r + c];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double d = lam * fmin(fmax(L[k][k], 1e-6), 1e32);
        Dd[6 * v + k] = d;
        L[k][k] += d;
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {                            // Cholesky in place, lower triangle
        double d = L[c][c];
#pragma unroll
        for (int k = 0; k < c; ++k) d -= L[c][k] * L[c][k];
        d = sqrt(d);
        L[c][c] = d;
        const double id = 1.0 / d;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            double s = L[r][c];
#pragma unroll
            for (int k = 0; k < c; ++k) s -= L[r][k] * L[c][k];
            L[r][c] = s * id;
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {                            // Y = L^-1, column by column
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (r < c) { Y[r][c] = 0.0; continue; }
            double s = r == c ? 1.0 : 0.0;
#pragma unroll
            for (int k = c; k < r; ++k) s -= L[r][k] * Y[k][c];
            Y[r][c] = s / L[r][r];
        }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) {                        // (L L^T)^-1 = Y^T Y
            double s = 0.0;
#pragma unroll
            for (int k = c; k < 6; ++k) s += Y[k][r] * Y[k][c];
            Minv[36 * v + 6 * r + c] = s;
            Minv[36 * v + 6 * c + r] = s;
        }
}

// one workgroup per view: acc = sum Jc^T (Jp z_point).  rhs: y = -gc + acc (z = zg); else y = (B + lambda D) x - acc
__global__ void __launch_bounds__(SFD2_BA_VIEW_WG) ba_view_apply_kernel(const BaState *st, int gate, int rhs, const int64_t *__restrict__ voff,
                                                                       const int32_t *__restrict__ vobs, const int32_t *__restrict__ obs_pt,
                                                                       const double *__restrict__ rec, const double *__restrict__ z,
                                                                       const double *__restrict__ B, const double *__restrict__ Dd,
                                                                       const double *__restrict__ gc, const double *__restrict__ x, double *__restrict__ y)
{
    if (ba_gated(st, gate)) return;
    __shared__ double sh[6 * SFD2_BA_VIEW_WG];
    const int64_t v = blockIdx.x;
    double a[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t i = voff[v] + threadIdx.x; i < voff[v + 1]; i += SFD2_BA_VIEW_WG) {
        const int64_t o = vobs[i];
        const double *rc = rec + SFD2_BA_REC * o;
        const double *zp = z + 3 * (int64_t)obs_pt[o];
        const double z0 = zp[0], z1 = zp[1], z2 = zp[2];
        const double e0 = rc[12] * z0 + rc[13] * z1 + rc[14] * z2, e1 = rc[15] * z0 + rc[16] * z1 + rc[17] * z2;
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] += rc[k] * e0 + rc[6 + k] * e1;
    }
    ba_tree_sum<6, SFD2_BA_VIEW_WG>(a, sh);
    if (threadIdx.x == 0) {
        if (rhs) {
#pragma unroll
            for (int k = 0; k < 6; ++k) y[6 * v + k] = a[k] - gc[6 * v + k];
        } else {
            double xv[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) xv[k] = x[6 * v + k];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                double s = Dd[6 * v + r] * xv[r];
#pragma unroll
                for (int c = 0; c < 6; ++c) s += B[36 * v + 6 * r + c] * xv[c];
                y[6 * v + r] = s - a[r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- PCG vectors
// out = Minv_v in
__device__ __forceinline__ void ba_precond(const double *__restrict__ M, const double in[6], double out[6])
{
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s += M[6 * r + c] * in[c];
        out[r] = s;
    }
}

// x = 0, r = b, z = Minv r, p = z; one workgroup
__global__ void __launch_bounds__(SFD2_BA_VEC_WG) ba_pcg_init_kernel(BaState *st, int nv, const double *__restrict__ b, const double *__restrict__ Minv,
                                                                    double *__restrict__ x, double *__restrict__ r, double *__restrict__ zz,
                                                                    double *__restrict__ p)
{
    __shared__ double sh[2 * SFD2_BA_VEC_WG];
    double a[2] = {0, 0};                                    // r.z, r.r
    for (int64_t v = threadIdx.x; v < nv; v += SFD2_BA_VEC_WG) {
        double rv[6], zv[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) rv[k] = b[6 * v + k];
        ba_precond(Minv + 36 * v, rv, zv);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            x[6 * v + k] = 0.0;
            r[6 * v + k] = rv[k];
            zz[6 * v + k] = zv[k];
            p[6 * v + k] = zv[k];
            a[0] += rv[k] * zv[k];
            a[1] += rv[k] * rv[k];
        }
    }
    ba_tree_sum<2, SFD2_BA_VEC_WG>(a, sh);
    if (threadIdx.x == 0) {
        st->rz = a[0];
        st->r0sq = a[1];
        st->rsq = a[1];
        st->pcg_iters = 0;
        st->pcg_done = !(a[1] > 0.0) || !(a[0] > 0.0);       // a zero (or non-finite) right-hand side: the step stays zero
    }
}

// one PCG iteration behind q = S p: alpha, x, r, z, beta, p and the stopping test; one workgroup
__global__ void __launch_bounds__(SFD2_BA_VEC_WG) ba_pcg_step_kernel(BaState *st, int nv, double tol2, int max_iters, const double *__restrict__ Minv,
                                                                    const double *__restrict__ q, double *__restrict__ x, double *__restrict__ r,
                                                                    double *__restrict__ zz, double *__restrict__ p)
{
    if (st->pcg_done) return;
    __shared__ double sh[2 * SFD2_BA_VEC_WG];
    const double rz = st->rz, r0sq = st->r0sq;
    const int iters = st->pcg_iters;
    double a[2] = {0, 0};
    for (int64_t i = threadIdx.x; i < 6 * (int64_t)nv; i += SFD2_BA_VEC_WG) a[0] += p[i] * q[i];
    ba_tree_sum<1, SFD2_BA_VEC_WG>(a, sh);
    const double pq = a[0];
    if (!(pq > 0.0) || !isfinite(pq)) {                      // breakdown: keep x as it is
        if (threadIdx.x == 0) st->pcg_done = 1;
        return;
    }
    const double alpha = rz / pq;
    a[0] = a[1] = 0.0;                                       // r.z, r.r of the new residual
    for (int64_t v = threadIdx.x; v < nv; v += SFD2_BA_VEC_WG) {
        double rv[6], zv[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            x[6 * v + k] += alpha * p[6 * v + k];
            rv[k] = r[6 * v + k] - alpha * q[6 * v + k];
            r[6 * v + k] = rv[k];
        }
        ba_precond(Minv + 36 * v, rv, zv);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            zz[6 * v + k] = zv[k];
            a[0] += rv[k] * zv[k];
            a[1] += rv[k] * rv[k];
        }
    }
    ba_tree_sum<2, SFD2_BA_VEC_WG>(a, sh);
    const double beta = a[0] / rz;
    for (int64_t i = threadIdx.x; i < 6 * (int64_t)nv; i += SFD2_BA_VEC_WG) p[i] = zz[i] + beta * p[i];
    if (threadIdx.x == 0) {
        st->rz = a[0];
        st->rsq = a[1];
        st->pcg_iters = iters + 1;
        st->pcg_done = !(a[1] > tol2 * r0sq) || iters + 1 >= max_iters || !(a[0] > 0.0);
    }
}

// ---------------------------------------------------------------------------------------------------------------- update
// the trial state: R <- Exp(w) R, t <- t + v per view; X <- X - (zg + z) per point (z = Vinv E^T dc); constants are copied
__global__ void __launch_bounds__(256) ba_update_views_kernel(int nv, const unsigned char *__restrict__ vconst, const double *__restrict__ x,
                                                              const double *__restrict__ pose, double *__restrict__ out)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const double *P = pose + 12 * v;
    double *O = out + 12 * v;
    if (vconst[v]) {
#pragma unroll
        for (int k = 0; k < 12; ++k) O[k] = P[k];
        return;
    }
    const double w0 = x[6 * v], w1 = x[6 * v + 1], w2 = x[6 * v + 2];
    const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
    double ca, cb;                                           // Exp(w) = 1 + ca [w]x + cb [w]x^2
    if (th2 < 1e-12) {
        ca = 1.0 - th2 / 6.0;
        cb = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2);
        ca = sin(th) / th;
        cb = (1.0 - cos(th)) / th2;
    }
    double E[9];
    E[0] = 1.0 - cb * (w1 * w1 + w2 * w2); E[1] = cb * w0 * w1 - ca * w2;         E[2] = cb * w0 * w2 + ca * w1;
    E[3] = cb * w0 * w1 + ca * w2;         E[4] = 1.0 - cb * (w0 * w0 + w2 * w2); E[5] = cb * w1 * w2 - ca * w0;
    E[6] = cb * w0 * w2 - ca * w1;         E[7] = cb * w1 * w2 + ca * w0;         E[8] = 1.0 - cb * (w0 * w0 + w1 * w1);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) O[3 * r + c] = E[3 * r] * P[c] + E[3 * r + 1] * P[3 + c] + E[3 * r + 2] * P[6 + c];
#pragma unroll
    for (int k = 0; k < 3; ++k) O[9 + k] = P[9 + k] + x[6 * v + 3 + k];
}

__global__ void __launch_bounds__(256) ba_update_points_kernel(int64_t n3, const unsigned char *__restrict__ pconst, const double *__restrict__ zg,
                                                               const double *__restrict__ z, const double *__restrict__ xyz, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    out[i] = pconst[i / 3] ? xyz[i] : xyz[i] - (zg[i] + z[i]);
}

// accept when the trial cost is finite and lower: lambda x 0.1, else lambda x 10
__global__ void ba_decide_kernel(BaState *st)
{
    const double c = st->trial_cost;
    const int acc = isfinite(c) && c < st->cost;
    st->accepted = acc;
    if (acc) {
        st->prev_cost = st->cost;
        st->cost = c;
        st->lambda *= 0.1;
        st->n_accepted += 1;
    } else {
        st->lambda *= 10.0;
    }
}

__global__ void __launch_bounds__(256) ba_commit_kernel(const BaState *st, int64_t n, const double *__restrict__ src, double *__restrict__ dst)
{
    if (!st->accepted) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)std::max<int64_t>((n + per - 1) / per, 1); }

}  // namespace

void launch_ba_linearise(hipStream_t s, const BaPtrs &P, int gate, bool full, bool trial, int loss, double c2)
{
    if (P.no == 0) return;
    const double *pose = trial ? P.pose_trial : P.pose, *xyz = trial ? P.xyz_trial : P.xyz;
    if (full)
        ba_linearise_kernel<true><<<blocks_of(P.no, 256), 256, 0, s>>>(P.st, gate, pose, P.cams, P.vconst, P.pconst, xyz, P.obs_view, P.obs_pt, P.obs_xy,
                                                                     P.no, loss, c2, P.rec, P.err, P.obs_cost);
    else
        ba_linearise_kernel<false><<<blocks_of(P.no, 256), 256, 0, s>>>(P.st, gate, pose, P.cams, P.vconst, P.pconst, xyz, P.obs_view, P.obs_pt, P.obs_xy,
                                                                      P.no, loss, c2, P.rec, P.err, P.obs_cost);
}

void launch_ba_reduce(hipStream_t s, const BaPtrs &P, int gate, const double *src, int64_t n, int op, double *dst, bool combine)
{
    const unsigned nb = blocks_of(n, SFD2_BA_RED_CHUNK);
    ba_reduce_partial_kernel<<<nb, SFD2_BA_RED_WG, 0, s>>>(P.st, gate, src, n, op, P.partial);
    ba_reduce_final_kernel<<<1, SFD2_BA_RED_WG, 0, s>>>(P.st, gate, P.partial, (int64_t)nb, op, dst, combine ? 1 : 0);
}

void launch_ba_point_build(hipStream_t s, const BaPtrs &P, int gate)
{
    if (P.n_short) ba_point_build_lane_kernel<<<blocks_of(P.n_short, 256), 256, 0, s>>>(P.st, gate, P.short_ids, P.n_short, P.pt_off, P.rec, P.V, P.gp);
    if (P.n_long) ba_point_build_wave_kernel<<<(unsigned)P.n_long, 64, 0, s>>>(P.st, gate, P.long_ids, P.pt_off, P.rec, P.V, P.gp);
}

void launch_ba_point_invert(hipStream_t s, const BaPtrs &P)
{
    if (P.np) ba_point_invert_kernel<<<blocks_of(P.np, 256), 256, 0, s>>>(P.st, P.np, P.V, P.gp, P.Vinv, P.zg);
}

void launch_ba_point_apply(hipStream_t s, const BaPtrs &P, int gate, const double *x)
{
    if (P.n_short)
        ba_point_apply_lane_kernel<<<blocks_of(P.n_short, 256), 256, 0, s>>>(P.st, gate, P.short_ids, P.n_short, P.pt_off, P.obs_view, P.rec, x, P.Vinv, P.z);
    if (P.n_long) ba_point_apply_wave_kernel<<<(unsigned)P.n_long, 64, 0, s>>>(P.st, gate, P.long_ids, P.pt_off, P.obs_view, P.rec, x, P.Vinv, P.z);
}

void launch_ba_view_build(hipStream_t s, const BaPtrs &P, int gate)
{
    ba_view_build_kernel<<<(unsigned)P.nv, SFD2_BA_VIEW_WG, 0, s>>>(P.st, gate, P.view_off, P.view_obs, P.rec, P.B, P.gc);
}

void launch_ba_view_precond(hipStream_t s, const BaPtrs &P)
{
    ba_view_precond_kernel<<<blocks_of(P.nv, 64), 64, 0, s>>>(P.st, P.nv, P.B, P.Minv, P.Dd);
}

void launch_ba_view_apply(hipStream_t s, const BaPtrs &P, int gate, bool rhs)
{
    ba_view_apply_kernel<<<(unsigned)P.nv, SFD2_BA_VIEW_WG, 0, s>>>(P.st, gate, rhs ? 1 : 0, P.view_off, P.view_obs, P.obs_pt, P.rec, rhs ? P.zg : P.z, P.B,
                                                                   P.Dd, P.gc, P.p, rhs ? P.b : P.q);
}

void launch_ba_pcg_init(hipStream_t s, const BaPtrs &P)
{
    ba_pcg_init_kernel<<<1, SFD2_BA_VEC_WG, 0, s>>>(P.st, P.nv, P.b, P.Minv, P.x, P.r, P.zz, P.p);
}

void launch_ba_pcg_step(hipStream_t s, const BaPtrs &P, double tol2, int max_iters)
{
    ba_pcg_step_kernel<<<1, SFD2_BA_VEC_WG, 0, s>>>(P.st, P.nv, tol2, max_iters, P.Minv, P.q, P.x, P.r, P.zz, P.p);
}

void launch_ba_update(hipStream_t s, const BaPtrs &P)
{
    ba_update_views_kernel<<<blocks_of(P.nv, 256), 256, 0, s>>>(P.nv, P.vconst, P.x, P.pose, P.pose_trial);
    if (P.np) ba_update_points_kernel<<<blocks_of(3 * (int64_t)P.np, 256), 256, 0, s>>>(3 * (int64_t)P.np, P.pconst, P.zg, P.z, P.xyz, P.xyz_trial);
}

void launch_ba_decide_commit(hipStream_t s, const BaPtrs &P)
{
    ba_decide_kernel<<<1, 1, 0, s>>>(P.st);
    ba_commit_kernel<<<blocks_of(12 * (int64_t)P.nv, 256), 256, 0, s>>>(P.st, 12 * (int64_t)P.nv, P.pose_trial, P.pose);
    if (P.np) ba_commit_kernel<<<blocks_of(3 * (int64_t)P.np, 256), 256, 0, s>>>(P.st, 3 * (int64_t)P.np, P.xyz_trial, P.xyz);
}
