// libsfd2hip: bundle adjustment with camera intrinsics among the unknowns -- the passes sfd2_bundle_adjust_cameras
// adds to those of bundle_kernels.hip.  The view and point blocks B, gc, V, gp and their inverses are built by the kernels of that file from
// the first SFD2_BA_REC doubles of a record, unchanged; here are the linearisation that also writes the camera block Jk, the camera
// blocks W_v (view x camera), C_c and g_c, the widened products and the PCG vector kernels over [6 nv ; 8 nc].
//
// The rules of bundle_kernels.hip hold: every phase is a launch of its own, no floating-point atomic, no workgroup waits on another.  A
// camera's sums are taken in two fixed stages: one partial per view by the view's workgroup (ascending observation index, 256 strided
// sums, ba_tree_sum), then per camera over its views in ascending view index (256 strided sums, the same tree).
#include "pose_camera.h"
#include "bundle_cam.h"

namespace {

constexpr int KC = SFD2_BA_CAM_K;

// ---------------------------------------------------------------------------------------------------------------- linearise
// ba_linearise_kernel with the view's camera looked up and the 2 x kmax block d r / d camera written beside the record
template <bool FULL>
__global__ void __launch_bounds__(256) bac_linearise_kernel(const BaState *st, int gate, const double *__restrict__ pose, const PoseCam *__restrict__ cams,
                                                            const int32_t *__restrict__ view_cam, const int32_t *__restrict__ slots, int kmax,
                                                            const unsigned char *__restrict__ vconst, const unsigned char *__restrict__ pconst,
                                                            const double *__restrict__ xyz, const int32_t *__restrict__ obs_view,
                                                            const int32_t *__restrict__ obs_pt, const double2 *__restrict__ obs_xy, int64_t n, int loss,
                                                            double c2, double *__restrict__ rec, double *__restrict__ reck, double *__restrict__ err,
                                                            double *__restrict__ obs_cost)
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
    const int ci = view_cam[v];
    const PoseCam cam = cams[ci];
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
    // d r / d (the camera's active parameters): r = diag(f) (ud, vd) + c
    const double r2 = u * u + w * w, uw2 = 2.0 * u * w;
    const double fu = a0 * u, fw = a1 * w;                   // sw f u, sw f w
    double *rk = reck + 2 * (int64_t)kmax * o;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        if (k >= kmax) break;
        double d0 = 0.0, d1 = 0.0;
        switch (slots[KC * ci + k]) {
        case SFD2_BA_SLOT_F: d0 = sw * ud; d1 = sw * vd; break;
        case SFD2_BA_SLOT_FX: d0 = sw * ud; break;
        case SFD2_BA_SLOT_FY: d1 = sw * vd; break;
        case SFD2_BA_SLOT_CX: d0 = sw; break;
        case SFD2_BA_SLOT_CY: d1 = sw; break;
        case SFD2_BA_SLOT_K1: d0 = fu * r2; d1 = fw * r2; break;
        case SFD2_BA_SLOT_K2: d0 = fu * r2 * r2; d1 = fw * r2 * r2; break;
        case SFD2_BA_SLOT_P1: d0 = a0 * uw2; d1 = a1 * (r2 + 2.0 * w * w); break;
        case SFD2_BA_SLOT_P2: d0 = a0 * (r2 + 2.0 * u * u); d1 = a1 * uw2; break;
        default: break;
        }
        rk[k] = d0;
        rk[kmax + k] = d1;
    }
}

// the two rows of an observation's camera block, zero beyond kmax
__device__ __forceinline__ void bac_load_jk(const double *__restrict__ rk, int kmax, double k0[KC], double k1[KC])
{
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        k0[k] = k < kmax ? rk[k] : 0.0;
        k1[k] = k < kmax ? rk[kmax + k] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- camera blocks
// One workgroup per (view, part): the view's sums over its observations of W = Jc^T Jk (6 x 8; parts 0 and 1: rows 0-2 and 3-5), of the
// upper triangle of Jk^T Jk (36, row by row; part 2: rows 0-2, part 3: rows 3-7) and of Jk^T r (8, part 3).  At most 24 sums per thread
// and pass: all 92 at once would not fit the registers in fp64.
template <int PART>
__device__ __forceinline__ void bac_view_cam_part(int64_t v, const int64_t *__restrict__ voff, const int32_t *__restrict__ vobs, const double *__restrict__ rec,
                                                  const double *__restrict__ reck, int kmax, double *__restrict__ W, double *__restrict__ Cp,
                                                  double *__restrict__ gkp, double *sh)
{
    double a[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) a[k] = 0.0;
    for (int64_t i = voff[v] + threadIdx.x; i < voff[v + 1]; i += SFD2_BA_VIEW_WG) {
        const int64_t o = vobs[i];
        const double *rc = rec + SFD2_BA_REC * o;
        double k0[KC], k1[KC];
        bac_load_jk(reck + 2 * (int64_t)kmax * o, kmax, k0, k1);
        if (PART < 2) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double j0 = rc[3 * PART + r], j1 = rc[6 + 3 * PART + r];
#pragma unroll
                for (int k = 0; k < KC; ++k) a[KC * r + k] += j0 * k0[k] + j1 * k1[k];
            }
        } else {
            int s = 0;
#pragma unroll
            for (int r = PART == 2 ? 0 : 3; r < (PART == 2 ? 3 : KC); ++r)
#pragma unroll
                for (int c = r; c < KC; ++c) a[s++] += k0[r] * k0[c] + k1[r] * k1[c];
            if (PART == 3) {
                const double r0 = rc[18], r1 = rc[19];
#pragma unroll
                for (int k = 0; k < KC; ++k) a[15 + k] += k0[k] * r0 + k1[k] * r1;
            }
        }
    }
    ba_tree_sum<8, SFD2_BA_VIEW_WG>(a, sh);
    ba_tree_sum<8, SFD2_BA_VIEW_WG>(a + 8, sh);
    ba_tree_sum<8, SFD2_BA_VIEW_WG>(a + 16, sh);
    if (threadIdx.x) return;
    if (PART < 2) {
#pragma unroll
        for (int k = 0; k < 24; ++k) W[48 * v + 24 * PART + k] = a[k];
    } else if (PART == 2) {
#pragma unroll
        for (int k = 0; k < 21; ++k) Cp[36 * v + k] = a[k];
    } else {
#pragma unroll
        for (int k = 0; k < 15; ++k) Cp[36 * v + 21 + k] = a[k];
#pragma unroll
        for (int k = 0; k < KC; ++k) gkp[KC * v + k] = a[15 + k];
    }
}

__global__ void __launch_bounds__(SFD2_BA_VIEW_WG) bac_view_cam_kernel(const BaState *st, int gate, const int64_t *__restrict__ voff,
                                                                      const int32_t *__restrict__ vobs, const double *__restrict__ rec,
                                                                      const double *__restrict__ reck, int kmax, double *__restrict__ W,
                                                                      double *__restrict__ Cp, double *__restrict__ gkp)
{
    if (ba_gated(st, gate)) return;
    __shared__ double sh[8 * SFD2_BA_VIEW_WG];
    const int64_t v = blockIdx.x;
    switch (blockIdx.y) {
    case 0: bac_view_cam_part<0>(v, voff, vobs, rec, reck, kmax, W, Cp, gkp, sh); break;
    case 1: bac_view_cam_part<1>(v, voff, vobs, rec, reck, kmax, W, Cp, gkp, sh); break;
    case 2: bac_view_cam_part<2>(v, voff, vobs, rec, reck, kmax, W, Cp, gkp, sh); break;
    default: bac_view_cam_part<3>(v, voff, vobs, rec, reck, kmax, W, Cp, gkp, sh); break;
    }
}

// one workgroup per camera: C = sum over its views of Cp (stored full, 64) and gk = sum of gkp
__global__ void __launch_bounds__(SFD2_BA_CAM_WG) bac_cam_sum_kernel(const BaState *st, int gate, const int64_t *__restrict__ coff,
                                                                    const int32_t *__restrict__ cviews, const double *__restrict__ Cp,
                                                                    const double *__restrict__ gkp, double *__restrict__ C, double *__restrict__ gk)
{
    if (ba_gated(st, gate)) return;
    __shared__ double sh[8 * SFD2_BA_CAM_WG];
    const int64_t c = blockIdx.x;
    double a[48];                                            // the upper triangle (36), Jk^T r (8), 4 unused
#pragma unroll
    for (int k = 0; k < 48; ++k) a[k] = 0.0;
    for (int64_t i = coff[c] + threadIdx.x; i < coff[c + 1]; i += SFD2_BA_CAM_WG) {
        const int64_t v = cviews[i];
#pragma unroll
        for (int k = 0; k < 36; ++k) a[k] += Cp[36 * v + k];
#pragma unroll
        for (int k = 0; k < KC; ++k) a[36 + k] += gkp[KC * v + k];
    }
#pragma unroll
    for (int k = 0; k < 48; k += 8) ba_tree_sum<8, SFD2_BA_CAM_WG>(a + k, sh);
    if (threadIdx.x) return;
    int s = 0;
#pragma unroll
    for (int r = 0; r < KC; ++r)
#pragma unroll
        for (int cc = r; cc < KC; ++cc) { C[64 * c + KC * r + cc] = a[s]; C[64 * c + KC * cc + r] = a[s]; ++s; }
#pragma unroll
    for (int k = 0; k < KC; ++k) gk[KC * c + k] = a[36 + k];
}

// (C + lambda D)^-1 of a camera by an 8 x 8 Cholesky, D = clamp(diag C, 1e-6, 1e32), and the damping lambda D itself; one lane per camera.
// A slot without a parameter has a zero row: the clamp makes its pivot lambda 1e-6, and its step stays zero with its gradient.
__global__ void __launch_bounds__(64) bac_cam_precond_kernel(const BaState *st, int n, const double *__restrict__ C, double *__restrict__ Cinv,
                                                             double *__restrict__ Dk)
{
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= n) return;
    const double lam = st->lambda;
    double L[KC][KC], Y[KC][KC];
#pragma unroll
    for (int r = 0; r < KC; ++r)
#pragma unroll
        for (int cc = 0; cc <= r; ++cc) L[r][cc] = C[64 * c + KC * r + cc];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const double d = lam * fmin(fmax(L[k][k], 1e-6), 1e32);
        Dk[KC * c + k] = d;
        L[k][k] += d;
    }
#pragma unroll
    for (int cc = 0; cc < KC; ++cc) {                        // Cholesky in place, lower triangle
        double d = L[cc][cc];
#pragma unroll
        for (int k = 0; k < cc; ++k) d -= L[cc][k] * L[cc][k];
        d = sqrt(d);
        L[cc][cc] = d;
        const double id = 1.0 / d;
#pragma unroll
        for (int r = cc + 1; r < KC; ++r) {
            double s = L[r][cc];
#pragma unroll
            for (int k = 0; k < cc; ++k) s -= L[r][k] * L[cc][k];
            L[r][cc] = s * id;
        }
    }
#pragma unroll
    for (int cc = 0; cc < KC; ++cc) {                        // Y = L^-1, column by column (lower triangle)
#pragma unroll
        for (int r = cc; r < KC; ++r) {
            double s = r == cc ? 1.0 : 0.0;
#pragma unroll
            for (int k = cc; k < r; ++k) s -= L[r][k] * Y[k][cc];
            Y[r][cc] = s / L[r][r];
        }
    }
#pragma unroll
    for (int r = 0; r < KC; ++r)
#pragma unroll
        for (int cc = r; cc < KC; ++cc) {                    // (L L^T)^-1 = Y^T Y
            double s = 0.0;
#pragma unroll
            for (int k = cc; k < KC; ++k) s += Y[k][r] * Y[k][cc];
            Cinv[64 * c + KC * r + cc] = s;
            Cinv[64 * c + KC * cc + r] = s;
        }
}

// ---------------------------------------------------------------------------------------------------------------- products
// a += Jp^T (Jc x_view + Jk x_camera) of one record
__device__ __forceinline__ void bac_point_prod(const double *__restrict__ rc, const double *__restrict__ rk, int kmax, const double *__restrict__ xv,
                                               const double *__restrict__ xc, double a[3])
{
    const double x0 = xv[0], x1 = xv[1], x2 = xv[2], x3 = xv[3], x4 = xv[4], x5 = xv[5];
    double e0 = rc[0] * x0 + rc[1] * x1 + rc[2] * x2 + rc[3] * x3 + rc[4] * x4 + rc[5] * x5;
    double e1 = rc[6] * x0 + rc[7] * x1 + rc[8] * x2 + rc[9] * x3 + rc[10] * x4 + rc[11] * x5;
#pragma unroll
    for (int k = 0; k < KC; ++k)
        if (k < kmax) {
            e0 += rk[k] * xc[k];
            e1 += rk[kmax + k] * xc[k];
        }
    a[0] += rc[12] * e0 + rc[15] * e1;
    a[1] += rc[13] * e0 + rc[16] * e1;
    a[2] += rc[14] * e0 + rc[17] * e1;
}

__device__ __forceinline__ void bac_point_store(int64_t j, const double a[3], const double *__restrict__ Vinv, double *__restrict__ z)
{
    const double *I = Vinv + 6 * j;                          // (00 01 02 11 12 22)
    z[3 * j] = I[0] * a[0] + I[1] * a[1] + I[2] * a[2];
    z[3 * j + 1] = I[1] * a[0] + I[3] * a[1] + I[4] * a[2];
    z[3 * j + 2] = I[2] * a[0] + I[4] * a[1] + I[5] * a[2];
}

// z_j = V'_j^-1 sum Jp^T (Jc x_view + Jk x_camera); x = [6 nv ; 8 nc], xk its camera part.  One lane per point of ids[n] ...
__global__ void __launch_bounds__(256) bac_point_apply_lane_kernel(const BaState *st, int gate, const int32_t *__restrict__ ids, int n,
                                                                   const int64_t *__restrict__ off, const int32_t *__restrict__ obs_view,
                                                                   const int32_t *__restrict__ view_cam, const double *__restrict__ rec,
                                                                   const double *__restrict__ reck, int kmax, const double *__restrict__ x,
                                                                   const double *__restrict__ xk, const double *__restrict__ Vinv, double *__restrict__ z)
{
    if (ba_gated(st, gate)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = ids[i];
    double a[3] = {0, 0, 0};
    for (int64_t o = off[j]; o < off[j + 1]; ++o) {
        const int64_t v = obs_view[o];
        bac_point_prod(rec + SFD2_BA_REC * o, reck + 2 * (int64_t)kmax * o, kmax, x + 6 * v, xk + KC * (int64_t)view_cam[v], a);
    }
    bac_point_store(j, a, Vinv, z);
}

// ... or one wave per point of ids[]: lane l takes observations l, l + 64, ...
__global__ void __launch_bounds__(64) bac_point_apply_wave_kernel(const BaState *st, int gate, const int32_t *__restrict__ ids,
                                                                  const int64_t *__restrict__ off, const int32_t *__restrict__ obs_view,
                                                                  const int32_t *__restrict__ view_cam, const double *__restrict__ rec,
                                                                  const double *__restrict__ reck, int kmax, const double *__restrict__ x,
                                                                  const double *__restrict__ xk, const double *__restrict__ Vinv, double *__restrict__ z)
{
    if (ba_gated(st, gate)) return;
    __shared__ double sh[3 * 64];
    const int64_t j = ids[blockIdx.x];
    double a[3] = {0, 0, 0};
    for (int64_t o = off[j] + threadIdx.x; o < off[j + 1]; o += 64) {
        const int64_t v = obs_view[o];
        bac_point_prod(rec + SFD2_BA_REC * o, reck + 2 * (int64_t)kmax * o, kmax, x + 6 * v, xk + KC * (int64_t)view_cam[v], a);
    }
    ba_tree_sum<3, 64>(a, sh);
    if (threadIdx.x == 0) bac_point_store(j, a, Vinv, z);
}

// one workgroup per view: acc = sum Jc^T (Jp z_point) and the view's partial qkp = sum Jk^T (Jp z_point) for its camera.
// rhs: y_v = -gc + acc (z = zg); else y_v = (B + lambda D) x_v + W_v x_camera - acc
__global__ void __launch_bounds__(SFD2_BA_VIEW_WG) bac_view_apply_kernel(const BaState *st, int gate, int rhs, const int64_t *__restrict__ voff,
                                                                        const int32_t *__restrict__ vobs, const int32_t *__restrict__ obs_pt,
                                                                        const int32_t *__restrict__ view_cam, const double *__restrict__ rec,
                                                                        const double *__restrict__ reck, int kmax, const double *__restrict__ z,
                                                                        const double *__restrict__ B, const double *__restrict__ Dd,
                                                                        const double *__restrict__ W, const double *__restrict__ gc,
                                                                        const double *__restrict__ x, const double *__restrict__ xk,
                                                                        double *__restrict__ y, double *__restrict__ qkp)
{
    if (ba_gated(st, gate)) return;
    __shared__ double sh[8 * SFD2_BA_VIEW_WG];
    const int64_t v = blockIdx.x;
    double a[6] = {0, 0, 0, 0, 0, 0}, ak[KC] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = voff[v] + threadIdx.x; i < voff[v + 1]; i += SFD2_BA_VIEW_WG) {
        const int64_t o = vobs[i];
        const double *rc = rec + SFD2_BA_REC * o;
        const double *zp = z + 3 * (int64_t)obs_pt[o];
        const double z0 = zp[0], z1 = zp[1], z2 = zp[2];
        const double e0 = rc[12] * z0 + rc[13] * z1 + rc[14] * z2, e1 = rc[15] * z0 + rc[16] * z1 + rc[17] * z2;
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] += rc[k] * e0 + rc[6 + k] * e1;
        double k0[KC], k1[KC];
        bac_load_jk(reck + 2 * (int64_t)kmax * o, kmax, k0, k1);
#pragma unroll
        for (int k = 0; k < KC; ++k) ak[k] += k0[k] * e0 + k1[k] * e1;
    }
    ba_tree_sum<6, SFD2_BA_VIEW_WG>(a, sh);
    ba_tree_sum<8, SFD2_BA_VIEW_WG>(ak, sh);
    if (threadIdx.x) return;
#pragma unroll
    for (int k = 0; k < KC; ++k) qkp[KC * v + k] = ak[k];
    if (rhs) {
#pragma unroll
        for (int k = 0; k < 6; ++k) y[6 * v + k] = a[k] - gc[6 * v + k];
        return;
    }
    double xv[6], xc[KC];
#pragma unroll
    for (int k = 0; k < 6; ++k) xv[k] = x[6 * v + k];
#pragma unroll
    for (int k = 0; k < KC; ++k) xc[k] = xk[KC * (int64_t)view_cam[v] + k];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double s = Dd[6 * v + r] * xv[r];
#pragma unroll
        for (int c = 0; c < 6; ++c) s += B[36 * v + 6 * r + c] * xv[c];
#pragma unroll
        for (int k = 0; k < KC; ++k)
            if (k < kmax) s += W[48 * v + KC * r + k] * xc[k];
        y[6 * v + r] = s - a[r];
    }
}

// one workgroup per camera, over its views in ascending order.  rhs: y_c = -gk + sum qkp; else
// y_c = (C + lambda D) x_c + sum (W_v^T x_v - qkp_v)
__global__ void __launch_bounds__(SFD2_BA_CAM_WG) bac_cam_apply_kernel(const BaState *st, int gate, int rhs, const int64_t *__restrict__ coff,
                                                                      const int32_t *__restrict__ cviews, const double *__restrict__ W,
                                                                      const double *__restrict__ qkp, const double *__restrict__ C,
                                                                      const double *__restrict__ Dk, const double *__restrict__ gk,
                                                                      const double *__restrict__ x, const double *__restrict__ xk, double *__restrict__ yk)
{
    if (ba_gated(st, gate)) return;
    __shared__ double sh[8 * SFD2_BA_CAM_WG];
    const int64_t c = blockIdx.x;
    double a[KC] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = coff[c] + threadIdx.x; i < coff[c + 1]; i += SFD2_BA_CAM_WG) {
        const int64_t v = cviews[i];
        if (rhs) {
#pragma unroll
            for (int k = 0; k < KC; ++k) a[k] += qkp[KC * v + k];
        } else {
            double t[KC];
#pragma unroll
            for (int k = 0; k < KC; ++k) t[k] = -qkp[KC * v + k];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const double xr = x[6 * v + r];
#pragma unroll
                for (int k = 0; k < KC; ++k) t[k] += W[48 * v + KC * r + k] * xr;
            }
#pragma unroll
            for (int k = 0; k < KC; ++k) a[k] += t[k];
        }
    }
    ba_tree_sum<8, SFD2_BA_CAM_WG>(a, sh);
    if (threadIdx.x) return;
    if (rhs) {
#pragma unroll
        for (int k = 0; k < KC; ++k) yk[KC * c + k] = a[k] - gk[KC * c + k];
        return;
    }
    double xc[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) xc[k] = xk[KC * c + k];
#pragma unroll
    for (int r = 0; r < KC; ++r) {
        double s = Dk[KC * c + r] * xc[r];
#pragma unroll
        for (int k = 0; k < KC; ++k) s += C[64 * c + KC * r + k] * xc[k];
        yk[KC * c + r] = s + a[r];
    }
}

// ---------------------------------------------------------------------------------------------------------------- PCG vectors
// out = M in, M an N x N block
template <int N> __device__ __forceinline__ void bac_precond(const double *__restrict__ M, const double in[N], double out[N])
{
#pragma unroll
    for (int r = 0; r < N; ++r) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < N; ++c) s += M[N * r + c] * in[c];
        out[r] = s;
    }
}

// r = b, z = M^-1 r of the blocks [lo, hi) of size N (INIT: and x = 0, p = z); a += (r.z, r.r)
template <int N, bool INIT>
__device__ __forceinline__ void bac_pcg_blocks(int64_t n, double alpha, const double *__restrict__ Minv, const double *__restrict__ bq, double *__restrict__ x,
                                               double *__restrict__ r, double *__restrict__ zz, double *__restrict__ p, double a[2])
{
    for (int64_t v = threadIdx.x; v < n; v += SFD2_BA_VEC_WG) {
        double rv[N], zv[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            if (INIT) {
                rv[k] = bq[N * v + k];
                x[N * v + k] = 0.0;
            } else {
                x[N * v + k] += alpha * p[N * v + k];
                rv[k] = r[N * v + k] - alpha * bq[N * v + k];
            }
            r[N * v + k] = rv[k];
        }
        bac_precond<N>(Minv + N * N * v, rv, zv);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            zz[N * v + k] = zv[k];
            if (INIT) p[N * v + k] = zv[k];
            a[0] += rv[k] * zv[k];
            a[1] += rv[k] * rv[k];
        }
    }
}

// x = 0, r = b, z = M^-1 r, p = z over [6 nv ; 8 nc]; one workgroup
__global__ void __launch_bounds__(SFD2_BA_VEC_WG) bac_pcg_init_kernel(BaState *st, int nv, int nc, const double *__restrict__ b, const double *__restrict__ Minv,
                                                                     const double *__restrict__ Cinv, double *__restrict__ x, double *__restrict__ r,
                                                                     double *__restrict__ zz, double *__restrict__ p)
{
    __shared__ double sh[2 * SFD2_BA_VEC_WG];
    const int64_t nk = 6 * (int64_t)nv;
    double a[2] = {0, 0};                                    // r.z, r.r
    bac_pcg_blocks<6, true>(nv, 0.0, Minv, b, x, r, zz, p, a);
    bac_pcg_blocks<KC, true>(nc, 0.0, Cinv, b + nk, x + nk, r + nk, zz + nk, p + nk, a);
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
__global__ void __launch_bounds__(SFD2_BA_VEC_WG) bac_pcg_step_kernel(BaState *st, int nv, int nc, double tol2, int max_iters, const double *__restrict__ Minv,
                                                                     const double *__restrict__ Cinv, const double *__restrict__ q, double *__restrict__ x,
                                                                     double *__restrict__ r, double *__restrict__ zz, double *__restrict__ p)
{
    if (st->pcg_done) return;
    __shared__ double sh[2 * SFD2_BA_VEC_WG];
    const double rz = st->rz, r0sq = st->r0sq;
    const int iters = st->pcg_iters;
    const int64_t nk = 6 * (int64_t)nv, n = nk + KC * (int64_t)nc;
    double a[2] = {0, 0};
    for (int64_t i = threadIdx.x; i < n; i += SFD2_BA_VEC_WG) a[0] += p[i] * q[i];
    ba_tree_sum<1, SFD2_BA_VEC_WG>(a, sh);
    const double pq = a[0];
    if (!(pq > 0.0) || !isfinite(pq)) {                      // breakdown: keep x as it is
        if (threadIdx.x == 0) st->pcg_done = 1;
        return;
    }
    const double alpha = rz / pq;
    a[0] = a[1] = 0.0;                                       // r.z, r.r of the new residual
    bac_pcg_blocks<6, false>(nv, alpha, Minv, q, x, r, zz, p, a);
    bac_pcg_blocks<KC, false>(nc, alpha, Cinv, q + nk, x + nk, r + nk, zz + nk, p + nk, a);
    ba_tree_sum<2, SFD2_BA_VEC_WG>(a, sh);
    const double beta = a[0] / rz;
    for (int64_t i = threadIdx.x; i < n; i += SFD2_BA_VEC_WG) p[i] = zz[i] + beta * p[i];
    if (threadIdx.x == 0) {
        st->rz = a[0];
        st->rsq = a[1];
        st->pcg_iters = iters + 1;
        st->pcg_done = !(a[1] > tol2 * r0sq) || iters + 1 >= max_iters || !(a[0] > 0.0);
    }
}

// ---------------------------------------------------------------------------------------------------------------- update
// the trial cameras: every active parameter plus its step; *bad = some parameter left the finite numbers or a focal length is <= 0.
// One workgroup.
__global__ void __launch_bounds__(SFD2_BA_CAM_WG) bac_update_cams_kernel(int nc, const int32_t *__restrict__ slots, const double *__restrict__ xk,
                                                                        const PoseCam *__restrict__ cams, PoseCam *__restrict__ out, int32_t *bad)
{
    int mine = 0;
    for (int64_t c = threadIdx.x; c < nc; c += SFD2_BA_CAM_WG) {
        PoseCam cam = cams[c];
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const double d = xk[KC * c + k];
            switch (slots[KC * c + k]) {
            case SFD2_BA_SLOT_F: cam.f[0] += d; cam.f[1] += d; break;
            case SFD2_BA_SLOT_FX: cam.f[0] += d; break;
            case SFD2_BA_SLOT_FY: cam.f[1] += d; break;
            case SFD2_BA_SLOT_CX: cam.c[0] += d; break;
            case SFD2_BA_SLOT_CY: cam.c[1] += d; break;
            case SFD2_BA_SLOT_K1: cam.k1 += d; break;
            case SFD2_BA_SLOT_K2: cam.k2 += d; break;
            case SFD2_BA_SLOT_P1: cam.p1 += d; break;
            case SFD2_BA_SLOT_P2: cam.p2 += d; break;
            default: break;
            }
        }
        cam.distorted = (cam.k1 != 0 || cam.k2 != 0 || cam.p1 != 0 || cam.p2 != 0) ? 1 : 0;
        out[c] = cam;
        const double sum = cam.f[0] + cam.f[1] + cam.c[0] + cam.c[1] + cam.k1 + cam.k2 + cam.p1 + cam.p2;
        mine |= !isfinite(sum) || !(cam.f[0] > 0.0) || !(cam.f[1] > 0.0);
    }
    const int any = __syncthreads_or(mine);
    if (threadIdx.x == 0) *bad = any;
}

// a trial state with a bad camera is rejected as a non-finite cost is
__global__ void bac_veto_kernel(BaState *st, const int32_t *bad)
{
    if (*bad) st->trial_cost = INFINITY;
}

__global__ void __launch_bounds__(256) bac_commit_kernel(const BaState *st, int64_t n, const double *__restrict__ src, double *__restrict__ dst)
{
    if (!st->accepted) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)std::max<int64_t>((n + per - 1) / per, 1); }

}  // namespace

void launch_bac_linearise(hipStream_t s, const BaCamPtrs &Q, int gate, bool full, bool trial, int loss, double c2)
{
    const BaPtrs &P = Q.P;
    if (P.no == 0) return;
    const double *pose = trial ? P.pose_trial : P.pose, *xyz = trial ? P.xyz_trial : P.xyz;
    const PoseCam *cams = trial ? Q.cams_trial : Q.cams;
    if (full)
        bac_linearise_kernel<true><<<blocks_of(P.no, 256), 256, 0, s>>>(P.st, gate, pose, cams, Q.view_cam, Q.slots, Q.kmax, P.vconst, P.pconst, xyz, P.obs_view,
                                                                      P.obs_pt, P.obs_xy, P.no, loss, c2, P.rec, Q.reck, P.err, P.obs_cost);
    else
        bac_linearise_kernel<false><<<blocks_of(P.no, 256), 256, 0, s>>>(P.st, gate, pose, cams, Q.view_cam, Q.slots, Q.kmax, P.vconst, P.pconst, xyz, P.obs_view,
                                                                       P.obs_pt, P.obs_xy, P.no, loss, c2, P.rec, Q.reck, P.err, P.obs_cost);
}

void launch_bac_cam_build(hipStream_t s, const BaCamPtrs &Q, int gate)
{
    const BaPtrs &P = Q.P;
    bac_view_cam_kernel<<<dim3((unsigned)P.nv, 4), SFD2_BA_VIEW_WG, 0, s>>>(P.st, gate, P.view_off, P.view_obs, P.rec, Q.reck, Q.kmax, Q.W, Q.Cp, Q.gkp);
    bac_cam_sum_kernel<<<(unsigned)Q.nc, SFD2_BA_CAM_WG, 0, s>>>(P.st, gate, Q.cam_off, Q.cam_views, Q.Cp, Q.gkp, Q.C, Q.gk);
}

void launch_bac_cam_precond(hipStream_t s, const BaCamPtrs &Q)
{
    bac_cam_precond_kernel<<<blocks_of(Q.nc, 64), 64, 0, s>>>(Q.P.st, Q.nc, Q.C, Q.Cinv, Q.Dk);
}

void launch_bac_point_apply(hipStream_t s, const BaCamPtrs &Q, int gate, const double *x)
{
    const BaPtrs &P = Q.P;
    const double *xk = x + 6 * (int64_t)P.nv;
    if (P.n_short)
        bac_point_apply_lane_kernel<<<blocks_of(P.n_short, 256), 256, 0, s>>>(P.st, gate, P.short_ids, P.n_short, P.pt_off, P.obs_view, Q.view_cam, P.rec,
                                                                             Q.reck, Q.kmax, x, xk, P.Vinv, P.z);
    if (P.n_long)
        bac_point_apply_wave_kernel<<<(unsigned)P.n_long, 64, 0, s>>>(P.st, gate, P.long_ids, P.pt_off, P.obs_view, Q.view_cam, P.rec, Q.reck, Q.kmax, x, xk,
                                                                     P.Vinv, P.z);
}

void launch_bac_apply(hipStream_t s, const BaCamPtrs &Q, int gate, bool rhs)
{
    const BaPtrs &P = Q.P;
    const int64_t nk = 6 * (int64_t)P.nv;
    double *y = rhs ? P.b : P.q;
    bac_view_apply_kernel<<<(unsigned)P.nv, SFD2_BA_VIEW_WG, 0, s>>>(P.st, gate, rhs ? 1 : 0, P.view_off, P.view_obs, P.obs_pt, Q.view_cam, P.rec, Q.reck, Q.kmax,
                                                                    rhs ? P.zg : P.z, P.B, P.Dd, Q.W, P.gc, P.p, P.p + nk, y, Q.qkp);
    bac_cam_apply_kernel<<<(unsigned)Q.nc, SFD2_BA_CAM_WG, 0, s>>>(P.st, gate, rhs ? 1 : 0, Q.cam_off, Q.cam_views, Q.W, Q.qkp, Q.C, Q.Dk, Q.gk, P.p, P.p + nk,
                                                                  y + nk);
}

void launch_bac_pcg_init(hipStream_t s, const BaCamPtrs &Q)
{
    const BaPtrs &P = Q.P;
    bac_pcg_init_kernel<<<1, SFD2_BA_VEC_WG, 0, s>>>(P.st, P.nv, Q.nc, P.b, P.Minv, Q.Cinv, P.x, P.r, P.zz, P.p);
}

void launch_bac_pcg_step(hipStream_t s, const BaCamPtrs &Q, double tol2, int max_iters)
{
    const BaPtrs &P = Q.P;
    bac_pcg_step_kernel<<<1, SFD2_BA_VEC_WG, 0, s>>>(P.st, P.nv, Q.nc, tol2, max_iters, P.Minv, Q.Cinv, P.q, P.x, P.r, P.zz, P.p);
}

void launch_bac_update_cams(hipStream_t s, const BaCamPtrs &Q)
{
    bac_update_cams_kernel<<<1, SFD2_BA_CAM_WG, 0, s>>>(Q.nc, Q.slots, Q.P.x + 6 * (int64_t)Q.P.nv, Q.cams, Q.cams_trial, Q.bad);
}

void launch_bac_veto(hipStream_t s, const BaCamPtrs &Q) { bac_veto_kernel<<<1, 1, 0, s>>>(Q.P.st, Q.bad); }

void launch_bac_commit_cams(hipStream_t s, const BaCamPtrs &Q)
{
    const int64_t n = (int64_t)(sizeof(PoseCam) / 8) * Q.nc;
    bac_commit_kernel<<<blocks_of(n, 256), 256, 0, s>>>(Q.P.st, n, reinterpret_cast<const double *>(Q.cams_trial), reinterpret_cast<double *>(Q.cams));
}
