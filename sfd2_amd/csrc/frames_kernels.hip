// Frame selection of the covisibility stage (it_loc/localize_cv2.py:120-233 get_covisibility_frames and
// get_covisibility_frames_by_pose) on gfx950: sfd2_covis_frames, rules and status protocol in include/sfd2_hip.h.
//
// One 256-thread workgroup per task, grid-striding over the tasks.
//
//   counters    32 bits per image: bit 31 = "connected" (the image occurs in the track of a point row of the task), bits 0..30 = count
//               (rows with a long enough track whose seen list holds the image).  In LDS up to SFD2_FRAMES_LDS_IMAGES images, else (or
//               with the flag) a row of global scratch per workgroup.  The atomic that moves an entry away from 0 appends the image to
//               the workgroup's touched list (a row of global scratch); the task ends by zeroing exactly those entries, so its cost
//               does not grow with the map.
//   candidates  the touched images with the connected bit (pos: and not excluded) get a slot of the sort arrays in LDS, at most
//               SFD2_FRAMES_MAX_CANDIDATES; the thread that owns the slot computes the pose errors in fp64 and the sort key:
//                 obs   (2^31 - 1 - count) << 32 | image        value: image, bit 31 = set aside by the pose test
//                 pos   bits of t_error                          for q_error <= q_th   (non-negative doubles order as integers)
//                       1 << 63 | (2^31 - 1 - count) << 32 | image   for the others
//   selection   bitonic sort of (key, value) ascending -- both orders are total, so the arrival order of the candidates does not
//               show; obs then ranks the taken and the set-aside frames with one block scan and applies the <= 3 fall-back, pos
//               takes the head of the sorted list.
// A task's status is decided before anything of its row is written; a row is written only with status 0.  Integer atomics on the
// counters and the list lengths only.  Every index read from the map is range-checked before it is followed (status 3), which costs
// a compare and keeps a damaged device-resident map from being written through.
#include "sfd2_internal.h"

namespace {

#define FR_MAX FRAMES_MAX_CANDIDATES
#define FR_CONNECTED 0x80000000u
#define FR_DEG (180.0 / 3.14159265358979323846)

template <bool GLOBAL>
__device__ __forceinline__ unsigned fr_load(unsigned *p)
{
    return GLOBAL ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// normalised quaternion and camera centre -R^T t of (qvec, tvec), compute_pose_error's formulas (it_loc/common.py:298-317)
__device__ __forceinline__ void fr_pose(const double *q, const double *t, double &w, double &x, double &y, double &z, double &cx, double &cy, double &cz)
{
    w = q[0], x = q[1], y = q[2], z = q[3];
    const double n = sqrt(w * w + x * x + y * y + z * z);
    w /= n, x /= n, y /= n, z /= n;
    const double r00 = 1 - 2 * (y * y + z * z), r01 = 2 * (x * y - w * z), r02 = 2 * (x * z + w * y);
    const double r10 = 2 * (x * y + w * z), r11 = 1 - 2 * (x * x + z * z), r12 = 2 * (y * z - w * x);
    const double r20 = 2 * (x * z - w * y), r21 = 2 * (y * z + w * x), r22 = 1 - 2 * (x * x + y * y);
    cx = -(r00 * t[0] + r10 * t[1] + r20 * t[2]);
    cy = -(r01 * t[0] + r11 * t[1] + r21 * t[2]);
    cz = -(r02 * t[0] + r12 * t[1] + r22 * t[2]);
}

__device__ __forceinline__ bool fr_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

template <bool GLOBAL>
__global__ __launch_bounds__(256) void covis_frames_kernel(FramesMapDev m, const FramesTaskDev *__restrict__ tasks, int n_tasks,
                                                           const int64_t *__restrict__ ref_off, const int32_t *__restrict__ ref_points, int cap,
                                                           int *scratch, int32_t *__restrict__ out)
{
    extern __shared__ __align__(16) unsigned char frames_smem[];
    __shared__ unsigned long long skey[FR_MAX];
    __shared__ int sval[FR_MAX];
    __shared__ int scan_t[256], scan_a[256];
    __shared__ int s_nt, s_nc, s_flags, s_ab;
    __shared__ double s_pose[8];                                   // the task's pose: normalised quaternion, centre, its norm
    const int tid = threadIdx.x;
    // scratch: per workgroup the touched list and, GLOBAL, the counters behind it; out: (n_out, status) per task, then the rows
    int *touched = scratch + (size_t)blockIdx.x * m.n_images * (GLOBAL ? 2 : 1);
    unsigned *cnt = GLOBAL ? reinterpret_cast<unsigned *>(touched + m.n_images) : reinterpret_cast<unsigned *>(frames_smem);
    if (!GLOBAL) {                                                 // the global rows arrive zeroed and every task leaves them so
        for (int j = tid; j < m.n_images; j += 256) cnt[j] = 0;
    }
    for (int q = blockIdx.x; q < n_tasks; q += gridDim.x) {
        const FramesTaskDev *tk = tasks + q;
        const int frame = tk->frame, cf = tk->covisibility_frame, obs_th = tk->obs_th;
        const bool pos = tk->kind == FRAMES_KIND_POS, posed = pos || tk->has_pose != 0;
        const int32_t *vrows = tk->use_ref ? ref_points : m.obs_point;
        const int64_t v0 = tk->use_ref ? ref_off[q] : m.obs_off[frame], v1 = tk->use_ref ? ref_off[q + 1] : m.obs_off[frame + 1];
        int flags = 0;                                             // 1: band, 4: a map index out of range
        if (tid == 0) {
            s_nt = 0, s_nc = 0, s_flags = 0, s_ab = -1;
            if (posed) {
                double w, x, y, z, cx, cy, cz;
                fr_pose(tk->qvec, tk->tvec, w, x, y, z, cx, cy, cz);
                const double cn = sqrt(cx * cx + cy * cy + cz * cz);
                s_pose[0] = w, s_pose[1] = x, s_pose[2] = y, s_pose[3] = z, s_pose[4] = cx, s_pose[5] = cy, s_pose[6] = cz, s_pose[7] = cn;
                if (!fr_finite(w + x + y + z) || !fr_finite(cn)) flags |= 1;
            }
        }
        __syncthreads();
        if (v0 < 0 || v1 < v0 || (!tk->use_ref && v1 > m.n_obs)) flags |= 4;
        // ---- counters: a thread per point row
        for (int64_t o = v0 + tid; o < v1 && !(flags & 4); o += 256) {
            const int p = vrows[o];
            if ((unsigned)p >= (unsigned)m.n_points) { flags |= 4; break; }
            const int64_t t0 = m.trk_off[p], t1 = m.trk_off[p + 1], s0 = m.seen_off[p], s1 = m.seen_off[p + 1];
            if (t0 < 0 || t1 < t0 || t1 > m.n_track || s0 < 0 || s1 < s0 || s1 > m.n_seen) { flags |= 4; break; }
            for (int64_t t = t0; t < t1; ++t) {
                const int im = m.trk_img[t];
                if ((unsigned)im >= (unsigned)m.n_images) { flags |= 4; continue; }
                if (fr_load<GLOBAL>(cnt + im) & FR_CONNECTED) continue;
                if (atomicOr(cnt + im, FR_CONNECTED) == 0) touched[atomicAdd(&s_nt, 1)] = im;
            }
            if (t1 - t0 < (int64_t)obs_th) continue;
            for (int64_t s = s0; s < s1; ++s) {
                const int im = m.seen_img[s];
                if ((unsigned)im >= (unsigned)m.n_images) { flags |= 4; continue; }
                if (atomicAdd(cnt + im, 1u) == 0) touched[atomicAdd(&s_nt, 1)] = im;
            }
        }
        __threadfence();                                           // the touched list and the global counters are read by other threads
        __syncthreads();
        // ---- candidates: pose errors and sort keys
        const int nt = s_nt;
        const double pw = s_pose[0], px = s_pose[1], py = s_pose[2], pz = s_pose[3], pcx = s_pose[4], pcy = s_pose[5], pcz = s_pose[6], pcn = s_pose[7];
        const double q_th = pos ? tk->q_th : 30.0;
        for (int i = tid; i < nt; i += 256) {
            const int im = touched[i];
            const unsigned c = fr_load<GLOBAL>(cnt + im);
            if (!(c & FR_CONNECTED)) continue;
            if (pos && m.excluded[im]) continue;
            const int slot = atomicAdd(&s_nc, 1);
            if (slot >= FR_MAX) continue;
            const unsigned long long by_count = ((unsigned long long)(0x7fffffffu - (c & 0x7fffffffu)) << 32) | (unsigned)im;
            unsigned long long key = by_count;
            int val = im;
            if (posed) {
                double w, x, y, z, cx, cy, cz;
                fr_pose(m.qvec + 4 * (size_t)im, m.tvec + 3 * (size_t)im, w, x, y, z, cx, cy, cz);
                const double dot = fmin(fabs(pw * w + px * x + py * y + pz * z), 1.0);
                const double q_err = 2 * acos(dot) * FR_DEG;
                const double dx = pcx - cx, dy = pcy - cy, dz = pcz - cz;
                const double t_err = sqrt(dx * dx + dy * dy + dz * dz);
                const double cn = sqrt(cx * cx + cy * cy + cz * cz);
                // acos near 1 turns a rounding of the dot product into sqrt(that) of angle: the second term covers it
                const double q_band = 1e-9 + fmin(1e-13 / sqrt(fmax(1 - dot * dot, 0.0)), 1e-5);
                const double t_band = 1e-9 * (1 + pcn + cn);
                if (!fr_finite(q_err) || !fr_finite(t_err) || !fr_finite(cn) || fabs(q_err - q_th) <= q_band) flags |= 1;
                if (pos) {
                    key = q_err <= q_th ? (unsigned long long)__double_as_longlong(t_err) : (1ull << 63) | by_count;
                } else {
                    if (fabs(t_err - 30.0) <= t_band) flags |= 1;
                    if (q_err >= 30.0 || t_err >= 30.0 || (c & 0x7fffffffu) <= 30u) val |= (int)FR_CONNECTED;
                }
            }
            skey[slot] = key;
            sval[slot] = val;
        }
        if (flags) atomicOr(&s_flags, flags);
        __syncthreads();
        const int nc = s_nc;
        const bool overflow = nc > FR_MAX;
        const int n = overflow ? 0 : nc;
        int npad = 1;
        while (npad < n) npad <<= 1;
        for (int i = n + tid; i < npad; i += 256) skey[i] = ~0ull, sval[i] = 0x7fffffff;
        __syncthreads();
        // ---- bitonic sort, ascending by (key, value)
        for (int k = 2; k <= npad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < npad; i += 256) {
                    const int l = i ^ j;
                    if (l > i) {
                        const unsigned long long ka = skey[i], kb = skey[l];
                        const int va = sval[i], vb = sval[l];
                        const bool gt = ka > kb || (ka == kb && (unsigned)va > (unsigned)vb);
                        if (gt == ((i & k) == 0)) skey[i] = kb, skey[l] = ka, sval[i] = vb, sval[l] = va;
                    }
                }
                __syncthreads();
            }
        }
        int n_res = 0, n_taken = 0, n_app = 0;
        const int chunk = (npad + 255) >> 8, p0 = tid * chunk, p1 = min(p0 + chunk, n);
        int ex_t = 0, ex_a = 0;
        if (pos) {
            int n1 = 0;                                            // frames with q_error <= q_th: the head of the sorted list
            for (int p = p0; p < p1; ++p) n1 += (skey[p] >> 63) ? 0 : 1;
            scan_t[tid] = n1;
            __syncthreads();
            n1 = 0;
            for (int t = 0; t < 256; ++t) n1 += scan_t[t];
            n_res = cf > 0 ? min(cf, n) : n1;
            // two neighbours in t_error order among the first cf + 1 closer than the band: numpy's argsort has no defined order there
            const int lim = cf > 0 ? min(n1, cf + 1) : n1;
            int tie = 0;
            for (int p = max(p0, 1); p < min(p1, lim); ++p) {
                const double ta = __longlong_as_double((long long)skey[p - 1]), tb = __longlong_as_double((long long)skey[p]);
                // |C_d| <= |C_pred| + t_error: the band of the farther frame, without its pose
                if (tb - ta < 1e-9 * (1 + 2 * pcn + tb)) tie = 1;
            }
            if (tie) atomicOr(&s_flags, 1);
        } else {
            int mt = 0, ma = 0;                                    // frames the walk takes / sets aside, in this thread's positions
            for (int p = p0; p < p1; ++p) {
                if (sval[p] < 0) ++ma;
                else ++mt;
            }
            scan_t[tid] = mt, scan_a[tid] = ma;
            __syncthreads();
            int tot_t = 0, tot_a = 0;
            for (int t = 0; t < 256; ++t) {
                const int a = scan_t[t], b = scan_a[t];
                if (t < tid) ex_t += a, ex_a += b;
                tot_t += a, tot_a += b;
            }
            n_taken = cf > 0 ? min(cf, tot_t) : tot_t;
            if (cf > 0 && ex_t < cf && cf <= ex_t + mt) {          // the walk stops in this thread's positions: set-aside frames met so far
                int a = ex_a, t = ex_t;
                for (int p = p0; p < p1 && t < cf; ++p) {
                    if (sval[p] < 0) ++a;
                    else ++t;
                }
                s_ab = a;
            }
            __syncthreads();
            const int ab = s_ab < 0 ? tot_a : s_ab;
            n_app = (n_taken <= 3 && ab > 0) ? min(ab, max(1, cf - n_taken)) : 0;
            n_res = n_taken + n_app;
        }
        __syncthreads();
        const int fl = s_flags;
        const int status = (fl & 4) ? 3 : (overflow || n_res > cap) ? 2 : (fl & 1) ? 1 : 0;
        if (status == 0) {
            int qv = q, nv = n_tasks, cv = cap;                    // the row address in vector registers: as loop invariants its parts
            asm volatile("" : "+v"(qv), "+v"(nv), "+v"(cv));       // would be scalar registers live across the whole task, and spill
            int32_t *row = out + 2 * (size_t)nv + (size_t)qv * cv;
            if (pos) {
                for (int p = tid; p < n_res; p += 256) row[p] = sval[p];
            } else {
                int t = ex_t, a = ex_a;
                for (int p = p0; p < p1; ++p) {
                    const int v = sval[p];
                    if (v < 0) {
                        if (a < n_app) row[n_taken + a] = v & 0x7fffffff;
                        ++a;
                    } else {
                        if (t < n_taken) row[t] = v;
                        ++t;
                    }
                }
            }
        }
        if (tid == 0) out[2 * q] = status == 0 ? n_res : 0, out[2 * q + 1] = status;
        // ---- leave the counters as they were found
        for (int i = tid; i < nt; i += 256) {
            if (GLOBAL) __hip_atomic_store(cnt + touched[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else cnt[touched[i]] = 0;
        }
        __threadfence();
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_covis_frames(hipStream_t st, const FramesMapDev &m, const FramesTaskDev *tasks, int n_tasks, const int64_t *ref_off,
                               const int32_t *ref_points, int cap, int global_counters, int blocks, int *scratch, int32_t *out)
{
    if (global_counters) {
        covis_frames_kernel<true><<<dim3(blocks), dim3(256), 0, st>>>(m, tasks, n_tasks, ref_off, ref_points, cap, scratch, out);
    } else {
        const size_t lds = ((size_t)m.n_images * 4 + 15) & ~(size_t)15;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(covis_frames_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        covis_frames_kernel<false><<<dim3(blocks), dim3(256), lds, st>>>(m, tasks, n_tasks, ref_off, ref_points, cap, scratch, out);
    }
    return hipGetLastError();
}
