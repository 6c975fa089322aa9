// libsfd2hip: what bundle_kernels.hip and api_bundle.hip share -- the device-side state word block of the Levenberg-Marquardt loop and
// the launchers of its passes.  fp64 throughout; every launcher queues on the given stream and returns.
#pragma once
#include "sfd2_internal.h"

#define SFD2_BA_REC 20                // doubles per observation record: Jc[2][6], Jp[2][3], r[2], all weighted by sqrt(rho')
#define SFD2_BA_LONG_TRACK 64         // a point with more observations than this gets a wave of its own, else one lane
#define SFD2_BA_VIEW_WG 256           // threads of a view's workgroup
#define SFD2_BA_VEC_WG 1024           // threads of the one workgroup that owns the 6 x n_views vectors
#define SFD2_BA_RED_WG 256            // threads of a reduction block ...
#define SFD2_BA_RED_CHUNK 2048        // ... and the elements it covers
#define SFD2_BA_GATE_NONE 0           // a kernel runs always,
#define SFD2_BA_GATE_ACCEPTED 1       //   only behind an accepted step,
#define SFD2_BA_GATE_PCG 2            //   only while the conjugate gradients have not stopped
#define SFD2_BA_OP_SUM 0
#define SFD2_BA_OP_ABSMAX 1

struct BaState {                      // one per call, in device memory; the host reads it once per LM iteration and once per PCG batch
    double cost, prev_cost, trial_cost, lambda, gmax;
    double rz, r0sq, rsq;             // PCG: r.z, |r_0|^2, |r_k|^2
    int32_t accepted, n_accepted, pcg_done, pcg_iters;
};

struct BaPtrs {                       // the call's device arrays
    BaState *st;
    const PoseCam *cams;              // [nv]
    const unsigned char *vconst, *pconst;
    const int64_t *pt_off;            // [np + 1]
    const int32_t *obs_view, *obs_pt; // [no]
    const double2 *obs_xy;            // [no]
    const int64_t *view_off;          // [nv + 1]: the by-view CSR,
    const int32_t *view_obs;          //   observation indices ascending inside a view
    const int32_t *short_ids, *long_ids;   // points by mapping
    double *pose, *pose_trial;        // [nv][12]: R row-major, t
    double *xyz, *xyz_trial;          // [np][3]
    double *rec, *err, *obs_cost;     // [no][SFD2_BA_REC], [no], [no]
    double *V, *gp, *Vinv, *zg, *z;   // per point: 6 (symmetric), 3, 6, 3, 3
    double *B, *gc, *Minv, *Dd;       // per view: 36, 6, 36, 6
    double *b, *x, *r, *zz, *p, *q;   // 6 x nv vectors of the reduced system
    double *partial;                  // reduction partials
    int nv, np, n_short, n_long;
    int64_t no;
};

// device helpers of bundle_kernels.hip and bundle_cam_kernels.hip
static __device__ __forceinline__ bool ba_gated(const BaState *st, int gate)
{
    return (gate == SFD2_BA_GATE_ACCEPTED && !st->accepted) || (gate == SFD2_BA_GATE_PCG && st->pcg_done);
}

// a[0..K) summed over the NT threads of the block by a fixed tree; sh holds K * NT doubles; every thread gets the sums
template <int K, int NT> static __device__ __forceinline__ void ba_tree_sum(double *a, double *sh)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k * NT + t] = a[k];
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k * NT + t] += sh[k * NT + t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = sh[k * NT];
    __syncthreads();
}

void launch_ba_linearise(hipStream_t st, const BaPtrs &P, int gate, bool full, bool trial, int loss, double c2);
void launch_ba_reduce(hipStream_t st, const BaPtrs &P, int gate, const double *src, int64_t n, int op, double *dst, bool combine);
void launch_ba_point_build(hipStream_t st, const BaPtrs &P, int gate);
void launch_ba_point_invert(hipStream_t st, const BaPtrs &P);
void launch_ba_point_apply(hipStream_t st, const BaPtrs &P, int gate, const double *x);
void launch_ba_view_build(hipStream_t st, const BaPtrs &P, int gate);
void launch_ba_view_precond(hipStream_t st, const BaPtrs &P);
void launch_ba_view_apply(hipStream_t st, const BaPtrs &P, int gate, bool rhs);
void launch_ba_pcg_init(hipStream_t st, const BaPtrs &P);
void launch_ba_pcg_step(hipStream_t st, const BaPtrs &P, double tol2, int max_iters);
void launch_ba_update(hipStream_t st, const BaPtrs &P);
void launch_ba_decide_commit(hipStream_t st, const BaPtrs &P);

// ---- the dense solver of the reduced camera system (bundle_dense_kernels.hip)
#define SFD2_BA_DENSE_TILE 64         // the factorisation's tile; the matrix is padded to whole tiles with an identity diagonal

struct BaDense {                      // the dense solver's device arrays; allocated only when it is chosen
    double *S;                        // [ld][ld], ld = 6 nv rounded up to whole tiles; only the lower triangle is written and read
    int64_t ld;
    double *G;                        // [no][18]: E_o L_p^-T per observation, 6 x 3
    const uint64_t *pairs;            // the pair list sorted by block: (a << 32) | b
    const int32_t *blk_start;         // [nv nv + 1]: where block i nv + j starts in it
    double *w, *y;                    // [ld] each: the solves' work vectors
    int32_t *fail;                    // 0, or 1 + the index of the first pivot that was <= 0 or not finite
};

// once per call: the pairs of every observation from pair_off[a] on, keyed view(a) nv + view(b); where every key starts in the sorted keys
void launch_ba_dense_pairs(hipStream_t st, const BaPtrs &P, const int64_t *pair_off, uint32_t *keys, uint64_t *vals);
void launch_ba_dense_block_start(hipStream_t st, const uint32_t *keys, int64_t n_pairs, int64_t n_keys, int32_t *start);
// per LM iteration: G and the lower triangle of S (behind ba_point_invert and ba_view_precond); trial_cost = inf when the pivot word is raised
void launch_ba_dense_form(hipStream_t st, const BaPtrs &P, const BaDense &D);
void launch_ba_dense_veto(hipStream_t st, const BaPtrs &P, const BaDense &D);
// A [ld][ld], ld a multiple of SFD2_BA_DENSE_TILE: rows n .. ld of the lower triangle <- identity; A <- its Cholesky factor (lower triangle);
// x[0 .. n) <- A^-1 b by the factor (w, y: ld doubles each).  *fail must be 0 before the factorisation; behind a raised word x is zero.
void launch_dense_pad(hipStream_t st, double *A, int64_t ld, int n);
void launch_dense_cholesky(hipStream_t st, double *A, int64_t ld, int32_t *fail);
void launch_dense_solve(hipStream_t st, const double *A, int64_t ld, int n, const double *b, double *w, double *y, double *x, const int32_t *fail);
