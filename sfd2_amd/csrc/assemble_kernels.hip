// libsfd2hip: matches -> 2D-3D correspondences, the device side of sfd2_assemble_2d3d (api_assemble.hip).  Replaces the per-key-point
// Python loops of it_loc/localize_cv2.py:286-360 (covisibility stage, with the reprojection gate) and :571-632 (cluster stage).
//
// A job is one query against its k database images.  The reference walks image 0..k-1, key point 0..n-1 and appends what
// survives; the output order (image, then key point) is therefore a stream compaction of the [k][n] grid, done in four launches
// over every job of the batch, blocks of SFD2_ASM_WG key points of one (job, image):
//   1. resolve: match index -> row of the point table (bounds checked, track-length filter), written to rows[k][n];
//   2. flag:    the de-duplication look-back over the earlier images' resolved rows of the same key point (coalesced rows of an
//               L2-resident array, O(k) per matched key point), then the reprojection gate in fp64 through the camera code of the
//               pose refinement (pose_camera.h); the block's survivor count by ballot + popcount;
//   3. scan:    one workgroup per job turns the job's block counts into exclusive offsets (per-thread segments, an LDS scan over the
//               256 segment sums), the per-image counts and m, and checks m against the capacity;
//   4. scatter: ballot + v_mbcnt ranks inside the block, the block's offset from the scan.
// No atomics decide a position (the only atomic is an OR into the job's status word), so the output bytes depend on the job
// alone: not on the batch, its order or the scheduling.  Every loop is bounded by k, n or the block size.
#include "sfd2_internal.h"
#include "pose_camera.h"

namespace {

constexpr int kWG = SFD2_ASM_WG;
constexpr int kWaves = kWG / 64;

__global__ __launch_bounds__(kWG) void assemble_resolve_kernel(const AsmJobDev *__restrict__ jobs, const int32_t *__restrict__ track,
                                                               int n_points, int32_t *__restrict__ rows, AsmResDev *res)
{
    const AsmJobDev &J = jobs[blockIdx.y];
    const int b = blockIdx.x;
    if (b >= J.k * J.nchunk) return;
    const int i = b / J.nchunk, idx = (b - i * J.nchunk) * kWG + (int)threadIdx.x;
    if (idx >= J.n) return;
    const AsmImgDev im = J.imgs[i];
    int r = -1;
    if (im.n1 > 0 && im.mrow >= 0) {
        const long long m = J.matches0[(int64_t)im.mrow * J.n + idx];
        if (m >= im.n1) {
            atomicOr(&res[blockIdx.y].status, SFD2_ASM_ST_MATCH_RANGE);
        } else if (m >= 0) {
            const int row = im.tab[m];
            if (row >= n_points) atomicOr(&res[blockIdx.y].status, SFD2_ASM_ST_ROW_RANGE);
            else if (row >= 0 && !((double)track[row] < J.obs_th)) r = row;     // `len(image_ids) < obs_th: continue`
        }
    }
    rows[J.ws_off + (int64_t)i * J.n + idx] = r;
}

__global__ __launch_bounds__(kWG) void assemble_flag_kernel(const AsmJobDev *__restrict__ jobs, const double *__restrict__ xyz,
                                                            const int32_t *__restrict__ rows, unsigned char *__restrict__ keep,
                                                            int32_t *__restrict__ blk)
{
    __shared__ int wcnt[kWaves];
    const AsmJobDev &J = jobs[blockIdx.y];
    const int b = blockIdx.x;
    if (b >= J.k * J.nchunk) return;
    const int i = b / J.nchunk, idx = (b - i * J.nchunk) * kWG + (int)threadIdx.x;
    bool ok = false;
    if (idx < J.n) {
        const int32_t *rw = rows + J.ws_off + idx;
        const int r = rw[(int64_t)i * J.n];
        if (r >= 0) {
            ok = true;
            for (int j = 0; j < i; ++j)                     // an earlier image took this 3D point for this key point (gated out or not)
                if (rw[(int64_t)j * J.n] == r) { ok = false; break; }
            if (ok && J.gate) {
                const double X[3] = {xyz[3 * (int64_t)r], xyz[3 * (int64_t)r + 1], xyz[3 * (int64_t)r + 2]};
                double Pc[3], px, py;
#pragma unroll
                for (int a = 0; a < 3; ++a) Pc[a] = J.R[3 * a] * X[0] + J.R[3 * a + 1] * X[1] + J.R[3 * a + 2] * X[2] + J.t[a];
                project_px(J.cam, Pc, px, py);
                const double dx = (double)J.kpq[2 * idx] - px, dy = (double)J.kpq[2 * idx + 1] - py;   // the key point without the +0.5
                if (sqrt(dx * dx + dy * dy) > J.radius) ok = false;                                    // a NaN error is kept
            }
        }
        keep[J.ws_off + (int64_t)i * J.n + idx] = ok ? 1 : 0;
    }
    const unsigned long long bal = __ballot(ok);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += wcnt[w];
        blk[J.blk_off + b] = s;
    }
}

__global__ __launch_bounds__(kWG) void assemble_scan_kernel(const AsmJobDev *__restrict__ jobs, int32_t *__restrict__ blk,
                                                            int32_t *__restrict__ counts, AsmResDev *res)
{
    __shared__ int part[kWG];
    const AsmJobDev &J = jobs[blockIdx.x];
    const int tid = threadIdx.x;
    const int T = J.k * J.nchunk, seg = (T + kWG - 1) / kWG;
    int32_t *b = blk + J.blk_off;
    const int lo = (int)min((int64_t)tid * seg, (int64_t)T), hi = min(lo + seg, T);
    int s = 0;
    for (int e = lo; e < hi; ++e) s += b[e];
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < kWG; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - s;
    for (int e = lo; e < hi; ++e) {
        const int c = b[e];
        b[e] = run;
        run += c;
    }
    const int m = part[kWG - 1];
    __syncthreads();
    for (int i = tid; i < J.k; i += kWG) {
        int c = 0;
        if (J.nchunk > 0) c = ((i + 1 < J.k) ? b[(i + 1) * J.nchunk] : m) - b[i * J.nchunk];      // (a query without key points has no blocks)
        counts[J.cnt_off + i] = c;
    }
    if (tid == 0) {
        res[blockIdx.x].m = m;
        if (m > J.cap) atomicOr(&res[blockIdx.x].status, SFD2_ASM_ST_CAPACITY);
    }
}

__global__ __launch_bounds__(kWG) void assemble_scatter_kernel(const AsmJobDev *__restrict__ jobs, const double *__restrict__ xyz,
                                                               const int32_t *__restrict__ rows, const unsigned char *__restrict__ keep,
                                                               const int32_t *__restrict__ blk, const AsmResDev *__restrict__ res)
{
    __shared__ int wcnt[kWaves];
    const AsmJobDev &J = jobs[blockIdx.y];
    const int b = blockIdx.x;
    if (b >= J.k * J.nchunk) return;
    if (res[blockIdx.y].status != 0) return;                // an input error or m above the capacity: nothing is written
    const int i = b / J.nchunk, idx = (b - i * J.nchunk) * kWG + (int)threadIdx.x;
    const int64_t at = J.ws_off + (int64_t)i * J.n + idx;
    const bool ok = idx < J.n && keep[at] != 0;
    const unsigned long long bal = __ballot(ok);
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wcnt[w] = __popcll(bal);
    __syncthreads();
    if (!ok) return;
    int o = blk[J.blk_off + b] + rank;
#pragma unroll
    for (int v = 0; v < kWaves; ++v)
        if (v < w) o += wcnt[v];
    if (o >= J.cap) return;                                 // (cannot happen with status 0: m <= cap)
    const int r = rows[at];
    J.p2[2 * (int64_t)o] = (double)J.kpq[2 * idx] + 0.5;
    J.p2[2 * (int64_t)o + 1] = (double)J.kpq[2 * idx + 1] + 0.5;
#pragma unroll
    for (int a = 0; a < 3; ++a) J.p3[3 * (int64_t)o + a] = xyz[3 * (int64_t)r + a];
    J.prow[o] = r;
    J.qidx[o] = idx;
    J.iidx[o] = i;
    J.score[o] = J.scores ? J.scores[idx] : 0.0f;
}

}  // namespace

void launch_assemble(hipStream_t st, const AsmJobDev *jobs, int n_jobs, int max_blocks, const double *xyz, const int32_t *track, int n_points,
                     int32_t *rows, unsigned char *keep, int32_t *blk, int32_t *counts, AsmResDev *res)
{
    if (n_jobs <= 0) return;
    const dim3 grid((unsigned)max_blocks, (unsigned)n_jobs);
    if (max_blocks > 0) {
        hipLaunchKernelGGL(assemble_resolve_kernel, grid, dim3(kWG), 0, st, jobs, track, n_points, rows, res);
        hipLaunchKernelGGL(assemble_flag_kernel, grid, dim3(kWG), 0, st, jobs, xyz, rows, keep, blk);
    }
    hipLaunchKernelGGL(assemble_scan_kernel, dim3((unsigned)n_jobs), dim3(kWG), 0, st, jobs, blk, counts, res);
    if (max_blocks > 0)
        hipLaunchKernelGGL(assemble_scatter_kernel, grid, dim3(kWG), 0, st, jobs, xyz, rows, keep, blk, res);
}
