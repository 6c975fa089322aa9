// libsfd2hip: the dense solver of the reduced camera system -- S = B' - sum E V'^-1 E^T formed as a matrix, its
// Cholesky factorisation S = L L^T by 64 x 64 tiles and the two triangular solves with the one right-hand side.  fp64 throughout; the
// factor and solve kernels know nothing of bundle adjustment and also serve sfd2_spd_solve.
//
// Section 14's rules hold: every phase is a launch of its own, none waits on another workgroup, none uses a floating-point atomic, and
// every sum has a fixed order.  A block S_ij (i >= j) is the sum over its segment of the pair list -- the (a, b) observation pairs of a
// common point, sorted by (view(a), view(b)) and inside a block by (point, a, b) -- as 64 strided partial sums joined by ba_tree_sum (one
// wave).  The factorisation is right-looking: per tile step one workgroup factors the diagonal tile in LDS, one workgroup per tile below
// it solves the panel, and one workgroup per tile of the trailing lower triangle subtracts the panel's product on
// v_mfma_f64_16x16x4_f64; a tile's updates come in the order of the steps and each runs over its 64 columns in ascending order, so the
// bytes depend on n alone.  Only the lower triangle is read or written.  The matrix is padded to whole tiles with an identity diagonal.
// A pivot that is <= 0 or not finite raises one device word; every kernel queued behind it reads the word and returns.
#include "bundle.h"

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int TS = SFD2_BA_DENSE_TILE;                       // 64
constexpr int TP = TS + 1;                                   // LDS row pitch of a whole tile
constexpr int KH = 32, KP = KH + 2;                          // the trailing update takes the 64 columns of the panel in two halves

// ---------------------------------------------------------------------------------------------------------------- the pair list
// one lane per observation a: its pairs (a, b), b over the point's observations in order with view(b) <= view(a), from pair_off[a] on
__global__ void __launch_bounds__(256) ba_dense_pairs_kernel(int64_t no, int nv, const int64_t *__restrict__ pt_off, const int32_t *__restrict__ obs_pt,
                                                             const int32_t *__restrict__ obs_view, const int64_t *__restrict__ pair_off,
                                                             uint32_t *__restrict__ keys, uint64_t *__restrict__ vals)
{
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= no) return;
    const int64_t p = obs_pt[a];
    const int va = obs_view[a];
    int64_t k = pair_off[a];
    const int64_t end = pair_off[a + 1];
    for (int64_t b = pt_off[p]; b < pt_off[p + 1] && k < end; ++b) {
        const int vb = obs_view[b];
        if (vb > va) continue;
        keys[k] = (uint32_t)va * (uint32_t)nv + (uint32_t)vb;
        vals[k] = ((uint64_t)a << 32) | (uint64_t)b;
        ++k;
    }
}

// start[k] = the first position of the sorted keys that holds a key >= k, for k = 0 .. nkeys
__global__ void __launch_bounds__(256) ba_dense_block_start_kernel(const uint32_t *__restrict__ keys, int64_t n, int64_t nkeys, int32_t *__restrict__ start)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > nkeys) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    start[k] = (int32_t)lo;
}

// ---------------------------------------------------------------------------------------------------------------- forming S
// G_o = E_o L_p^-T (6 x 3) with E_o = Jc_o^T Jp_o and V_p + lambda D_p = L_p L_p^T (ba_point_invert_kernel's damping); one lane per observation
__global__ void __launch_bounds__(256) ba_dense_g_kernel(const BaState *st, int64_t no, const double *__restrict__ rec, const int32_t *__restrict__ obs_pt,
                                                         const double *__restrict__ V, double *__restrict__ G)
{
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= no) return;
    const double lam = st->lambda;
    const double *v = V + 6 * (int64_t)obs_pt[o];
    const double a00 = v[0] + lam * fmin(fmax(v[0], 1e-6), 1e32), a10 = v[1], a20 = v[2];
    const double a11 = v[3] + lam * fmin(fmax(v[3], 1e-6), 1e32), a21 = v[4];
    const double a22 = v[5] + lam * fmin(fmax(v[5], 1e-6), 1e32);
    const double l00 = sqrt(a00), l10 = a10 / l00, l20 = a20 / l00;
    const double l11 = sqrt(a11 - l10 * l10), l21 = (a21 - l20 * l10) / l11;
    const double l22 = sqrt(a22 - l20 * l20 - l21 * l21);
    const double *rc = rec + SFD2_BA_REC * o;
    const double j0 = rc[12], j1 = rc[13], j2 = rc[14], k0 = rc[15], k1 = rc[16], k2 = rc[17];
    double *g = G + 18 * o;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const double c0 = rc[r], c1 = rc[6 + r];
        const double e0 = c0 * j0 + c1 * k0, e1 = c0 * j1 + c1 * k1, e2 = c0 * j2 + c1 * k2;
        const double g0 = e0 / l00, g1 = (e1 - l10 * g0) / l11, g2 = (e2 - l20 * g0 - l21 * g1) / l22;
        g[3 * r] = g0; g[3 * r + 1] = g1; g[3 * r + 2] = g2;
    }
}

// one wave per block (i, j), i >= j: S_ij = [i = j] (B_i + lambda D_i) - sum over the block's pairs of G_a G_b^T
__global__ void __launch_bounds__(64) ba_dense_form_kernel(int nv, int64_t ld, const double *__restrict__ B, const double *__restrict__ Dd,
                                                           const double *__restrict__ G, const uint64_t *__restrict__ pairs,
                                                           const int32_t *__restrict__ start, double *__restrict__ S)
{
    const int i = blockIdx.y, j = blockIdx.x, t = threadIdx.x;
    if (j > i) return;
    __shared__ double sh[9 * 64];
    const int64_t key = (int64_t)i * nv + j;
    const int32_t lo = start[key], hi = start[key + 1];
    if (lo < hi) {
        double a[36];
#pragma unroll
        for (int k = 0; k < 36; ++k) a[k] = 0.0;
        for (int32_t idx = lo + t; idx < hi; idx += 64) {
            const uint64_t pr = pairs[idx];
            const double *ga = G + 18 * (int64_t)(pr >> 32), *gb = G + 18 * (int64_t)(pr & 0xffffffffu);
            double x[18], y[18];
#pragma unroll
            for (int k = 0; k < 18; ++k) { x[k] = ga[k]; y[k] = gb[k]; }
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) a[6 * r + c] += x[3 * r] * y[3 * c] + x[3 * r + 1] * y[3 * c + 1] + x[3 * r + 2] * y[3 * c + 2];
        }
        ba_tree_sum<9, 64>(a, sh);
        ba_tree_sum<9, 64>(a + 9, sh);
        ba_tree_sum<9, 64>(a + 18, sh);
        ba_tree_sum<9, 64>(a + 27, sh);
        if (t == 0) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const double d = i == j ? B[36 * (int64_t)i + 6 * r + c] + (r == c ? Dd[6 * (int64_t)i + r] : 0.0) : 0.0;
                    S[(6 * (int64_t)i + r) * ld + 6 * (int64_t)j + c] = d - a[6 * r + c];
                }
        }
    } else if (t < 36) {
        const int r = t / 6, c = t % 6;
        S[(6 * (int64_t)i + r) * ld + 6 * (int64_t)j + c] = i == j ? B[36 * (int64_t)i + t] + (r == c ? Dd[6 * (int64_t)i + r] : 0.0) : 0.0;
    }
}

// rows n .. ld of the lower triangle: zero with a unit diagonal
__global__ void __launch_bounds__(256) dense_pad_kernel(double *__restrict__ A, int64_t ld, int n)
{
    const int64_t r = n + blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < ld && c <= r) A[r * ld + c] = r == c ? 1.0 : 0.0;
}

// w = b padded with zeros to ld entries, x = 0
__global__ void __launch_bounds__(256) dense_rhs_kernel(const double *__restrict__ b, int n, int64_t ld, double *__restrict__ w, double *__restrict__ x)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ld) return;
    w[i] = i < n ? b[i] : 0.0;
    if (i < n) x[i] = 0.0;
}

__global__ void ba_dense_veto_kernel(BaState *st, const int32_t *fail)
{
    if (*fail) st->trial_cost = INFINITY;
}

// ---------------------------------------------------------------------------------------------------------------- factorisation
// tile (k, k) -> its Cholesky factor, in LDS; the first pivot that is <= 0 or not finite raises *fail = its index + 1
__global__ void __launch_bounds__(256) dense_potrf_tile_kernel(double *__restrict__ A, int64_t ld, int k, int32_t *fail)
{
    if (*fail) return;
    __shared__ double T[TS * TP];
    const int t = threadIdx.x, r = t & 63, g = t >> 6;
    double *Ak = A + ((int64_t)k * TS) * ld + (int64_t)k * TS;
    for (int e = t; e < TS * TS; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        T[rr * TP + cc] = cc <= rr ? Ak[rr * ld + cc] : 0.0;
    }
    __syncthreads();
    // thread (r, g) keeps T[r][g + 4 q], q < 16, in registers; only the pivot column goes through LDS, unscaled and then scaled
    __shared__ double col[2][TS], scol[2][TS];
    double a[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = T[r * TP + g + 4 * q];
#pragma unroll
    for (int j = 0; j < TS; ++j) {
        if (g == (j & 3)) col[j & 1][r] = a[j >> 2];
        __syncthreads();
        const double d = col[j & 1][j];
        if (!(d > 0.0) || !isfinite(d)) {                    // the same word for every thread
            if (t == 0) *fail = k * TS + j + 1;
            return;
        }
        const double s = sqrt(d);
        if (t < TS) scol[j & 1][t] = t == j ? s : col[j & 1][t] / s;
        __syncthreads();
        const double lr = scol[j & 1][r];
        if (g == (j & 3) && r >= j) a[j >> 2] = lr;
#pragma unroll
        for (int q = j >> 2; q < 16; ++q) {
            const int c = g + 4 * q;
            if (c > j && r >= c) a[q] -= lr * scol[j & 1][c];
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) T[r * TP + g + 4 * q] = a[q];
    __syncthreads();
    for (int e = t; e < TS * TS; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        if (cc <= rr) Ak[rr * ld + cc] = T[rr * TP + cc];
    }
}

// tile (k + 1 + blockIdx.x, k) <- X with X L_kk^T = that tile, by substitution in LDS
__global__ void __launch_bounds__(256) dense_trsm_tile_kernel(double *__restrict__ A, int64_t ld, int k, const int32_t *fail)
{
    if (*fail) return;
    __shared__ double L[TS * (TS + 1) / 2], X[TS * TP];           // L_kk packed by rows: a wave reads one word of it at a time
    const int t = threadIdx.x, r = t & 63, g = t >> 6;
    const double *Ak = A + ((int64_t)k * TS) * ld + (int64_t)k * TS;
    double *Ai = A + ((int64_t)(k + 1 + blockIdx.x) * TS) * ld + (int64_t)k * TS;
    for (int e = t; e < TS * TS; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        if (cc <= rr) L[rr * (rr + 1) / 2 + cc] = Ak[rr * ld + cc];
        X[rr * TP + cc] = Ai[rr * ld + cc];
    }
    __syncthreads();
    // thread (r, g) keeps X[r][g + 4 q], q < 16, in registers; column j of X goes through LDS once it is final
    __shared__ double xcol[2][TS];
    double a[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = X[r * TP + g + 4 * q];
#pragma unroll
    for (int j = 0; j < TS; ++j) {
        if (g == (j & 3)) {
            a[j >> 2] /= L[j * (j + 1) / 2 + j];
            xcol[j & 1][r] = a[j >> 2];
        }
        __syncthreads();
        const double xj = xcol[j & 1][r];
#pragma unroll
        for (int q = j >> 2; q < 16; ++q) {
            const int c = g + 4 * q;
            if (c > j) a[q] -= xj * L[c * (c + 1) / 2 + j];
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) X[r * TP + g + 4 * q] = a[q];
    __syncthreads();
    for (int e = t; e < TS * TS; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        Ai[rr * ld + cc] = X[rr * TP + cc];
    }
}

// tile (bi, bj), k < bj <= bi: -= L_bi,k L_bj,k^T on the fp64 matrix instruction.  Four waves, 16 rows of the tile each; lane l
// holds A[l & 15][l >> 4] and B[l >> 4][l & 15] of a 16 x 16 x 4 product and the results of column l & 15, rows (l >> 4) + 4 reg.
__global__ void __launch_bounds__(256) dense_syrk_tile_kernel(double *__restrict__ A, int64_t ld, int k, const int32_t *fail)
{
    const int bi = k + 1 + blockIdx.y, bj = k + 1 + blockIdx.x;
    if (bj > bi || *fail) return;
    __shared__ double P[TS * KP], Q[TS * KP];
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const double *Pi = A + ((int64_t)bi * TS) * ld + (int64_t)k * TS, *Qj = A + ((int64_t)bj * TS) * ld + (int64_t)k * TS;
    double4_t acc[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[nb] = (double4_t){0.0, 0.0, 0.0, 0.0};
    for (int kh = 0; kh < TS; kh += KH) {
        __syncthreads();
        for (int e = t; e < TS * KH; e += 256) {
            const int rr = e >> 5, cc = e & 31;
            P[rr * KP + cc] = Pi[rr * ld + kh + cc];
            Q[rr * KP + cc] = Qj[rr * ld + kh + cc];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KH; ks += 4) {
            const double a = P[(16 * w + (l & 15)) * KP + ks + (l >> 4)];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const double b = Q[(16 * nb + (l & 15)) * KP + ks + (l >> 4)];
                acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[nb], 0, 0, 0);
            }
        }
    }
    double *C = A + ((int64_t)bi * TS) * ld + (int64_t)bj * TS;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rr = 16 * w + (l >> 4) + 4 * q, cc = 16 * nb + (l & 15);
            if (bi != bj || cc <= rr) C[rr * ld + cc] -= acc[nb][q];
        }
}

// ---------------------------------------------------------------------------------------------------------------- the two solves
// forward step k: every workgroup solves L_kk y_k = w_k for itself; workgroup 0 stores y_k, workgroup m > 0 takes L_(k+m),k y_k off w_(k+m)
__global__ void __launch_bounds__(256) dense_forward_kernel(const double *__restrict__ A, int64_t ld, int k, double *__restrict__ w, double *__restrict__ y,
                                                            const int32_t *fail)
{
    if (*fail) return;
    __shared__ double T[TS * TP], ys[TS], part[4 * TS];
    const int t = threadIdx.x, r = t & 63, g = t >> 6;
    const double *Ak = A + ((int64_t)k * TS) * ld + (int64_t)k * TS;
    for (int e = t; e < TS * TS; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        T[rr * TP + cc] = cc <= rr ? Ak[rr * ld + cc] : 0.0;
    }
    double v = t < TS ? w[(int64_t)k * TS + t] : 0.0;
    __syncthreads();
    for (int j = 0; j < TS; ++j) {
        if (t == j) ys[j] = v / T[j * TP + j];
        __syncthreads();
        if (t > j && t < TS) v -= T[t * TP + j] * ys[j];
    }
    if (blockIdx.x == 0) {
        if (t < TS) y[(int64_t)k * TS + t] = ys[t];
        return;
    }
    const int bi = k + blockIdx.x;
    const double *Ai = A + ((int64_t)bi * TS) * ld + (int64_t)k * TS;
    __syncthreads();
    for (int e = t; e < TS * TS; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        T[rr * TP + cc] = Ai[rr * ld + cc];
    }
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) s += T[r * TP + 16 * g + c] * ys[16 * g + c];
    part[g * TS + r] = s;
    __syncthreads();
    if (t < TS) w[(int64_t)bi * TS + t] -= (part[t] + part[TS + t]) + (part[2 * TS + t] + part[3 * TS + t]);
}

// backward step k: every workgroup solves L_kk^T x_k = y_k for itself; workgroup k stores x_k[0 .. n), workgroup m < k takes L_k,m^T x_k off y_m
__global__ void __launch_bounds__(256) dense_backward_kernel(const double *__restrict__ A, int64_t ld, int k, int n, double *__restrict__ y,
                                                             double *__restrict__ x, const int32_t *fail)
{
    if (*fail) return;
    __shared__ double T[TS * TP], xs[TS], part[4 * TS];
    const int t = threadIdx.x, r = t & 63, g = t >> 6;
    const double *Ak = A + ((int64_t)k * TS) * ld + (int64_t)k * TS;
    for (int e = t; e < TS * TS; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        T[rr * TP + cc] = cc <= rr ? Ak[rr * ld + cc] : 0.0;
    }
    double v = t < TS ? y[(int64_t)k * TS + t] : 0.0;
    __syncthreads();
    for (int j = TS - 1; j >= 0; --j) {
        if (t == j) xs[j] = v / T[j * TP + j];
        __syncthreads();
        if (t < j) v -= T[j * TP + t] * xs[j];
    }
    const int bi = blockIdx.x;
    if (bi == k) {
        if (t < TS && (int64_t)k * TS + t < n) x[(int64_t)k * TS + t] = xs[t];
        return;
    }
    const double *Ai = A + ((int64_t)k * TS) * ld + (int64_t)bi * TS;
    __syncthreads();
    for (int e = t; e < TS * TS; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        T[rr * TP + cc] = Ai[rr * ld + cc];
    }
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) s += T[(16 * g + c) * TP + r] * xs[16 * g + c];
    part[g * TS + r] = s;
    __syncthreads();
    if (t < TS) y[(int64_t)bi * TS + t] -= (part[t] + part[TS + t]) + (part[2 * TS + t] + part[3 * TS + t]);
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)std::max<int64_t>((n + per - 1) / per, 1); }

}  // namespace

void launch_ba_dense_pairs(hipStream_t s, const BaPtrs &P, const int64_t *pair_off, uint32_t *keys, uint64_t *vals)
{
    if (P.no) ba_dense_pairs_kernel<<<blocks_of(P.no, 256), 256, 0, s>>>(P.no, P.nv, P.pt_off, P.obs_pt, P.obs_view, pair_off, keys, vals);
}

void launch_ba_dense_block_start(hipStream_t s, const uint32_t *keys, int64_t n_pairs, int64_t n_keys, int32_t *start)
{
    ba_dense_block_start_kernel<<<blocks_of(n_keys + 1, 256), 256, 0, s>>>(keys, n_pairs, n_keys, start);
}

void launch_ba_dense_form(hipStream_t s, const BaPtrs &P, const BaDense &D)
{
    if (P.no) ba_dense_g_kernel<<<blocks_of(P.no, 256), 256, 0, s>>>(P.st, P.no, P.rec, P.obs_pt, P.V, D.G);
    ba_dense_form_kernel<<<dim3((unsigned)P.nv, (unsigned)P.nv), 64, 0, s>>>(P.nv, D.ld, P.B, P.Dd, D.G, D.pairs, D.blk_start, D.S);
}

void launch_ba_dense_veto(hipStream_t s, const BaPtrs &P, const BaDense &D) { ba_dense_veto_kernel<<<1, 1, 0, s>>>(P.st, D.fail); }

void launch_dense_pad(hipStream_t s, double *A, int64_t ld, int n)
{
    if (ld > n) dense_pad_kernel<<<dim3(blocks_of(ld, 256), (unsigned)(ld - n)), 256, 0, s>>>(A, ld, n);
}

void launch_dense_cholesky(hipStream_t s, double *A, int64_t ld, int32_t *fail)
{
    const int nt = (int)(ld / TS);
    for (int k = 0; k < nt; ++k) {
        dense_potrf_tile_kernel<<<1, 256, 0, s>>>(A, ld, k, fail);
        const int m = nt - k - 1;
        if (m == 0) break;
        dense_trsm_tile_kernel<<<(unsigned)m, 256, 0, s>>>(A, ld, k, fail);
        dense_syrk_tile_kernel<<<dim3((unsigned)m, (unsigned)m), 256, 0, s>>>(A, ld, k, fail);
    }
}

void launch_dense_solve(hipStream_t s, const double *A, int64_t ld, int n, const double *b, double *w, double *y, double *x, const int32_t *fail)
{
    const int nt = (int)(ld / TS);
    dense_rhs_kernel<<<blocks_of(ld, 256), 256, 0, s>>>(b, n, ld, w, x);
    for (int k = 0; k < nt; ++k) dense_forward_kernel<<<(unsigned)(nt - k), 256, 0, s>>>(A, ld, k, w, y, fail);
    for (int k = nt - 1; k >= 0; --k) dense_backward_kernel<<<(unsigned)(k + 1), 256, 0, s>>>(A, ld, k, n, y, x, fail);
}
