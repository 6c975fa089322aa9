// libsfd2hip: sfd2_covis_clusters -- checks the inputs (every index the kernel follows is bounds-checked here, before anything is
// uploaded or written), uploads the map and the query lists, one launch of cluster_kernels.hip on the context's stream, results back.
#include "sfd2_ctx.h"
#include "api_scratch.h"

namespace {

}  // namespace

extern "C" int sfd2_covis_clusters(sfd2_ctx *c, const int64_t *obs_offsets, const int32_t *obs_point, int n_images, const int64_t *track_offsets,
                                   const int32_t *track_image, int n_points, const int64_t *frame_offsets, const int32_t *frames, int nq,
                                   int32_t *cluster, int32_t *n_clusters, int flags)
{
    const std::string F("sfd2_covis_clusters: ");
    if (!c || !obs_offsets || !track_offsets || !frame_offsets || !n_clusters) return fail(F + "null argument");
    if (n_images < 1 || n_points < 0 || nq < 1) return fail(F + "n_images and nq must be positive and n_points non-negative");
    if (flags & ~SFD2_CLUSTER_FLAG_GLOBAL_SLOTS) return fail(F + "unknown flags");
    if (!monotone(obs_offsets, n_images)) return fail(F + "obs_offsets must start at 0 and not decrease");
    if (!monotone(track_offsets, n_points)) return fail(F + "track_offsets must start at 0 and not decrease");
    if (!monotone(frame_offsets, nq)) return fail(F + "frame_offsets must start at 0 and not decrease");
    const int64_t O = obs_offsets[n_images], T = track_offsets[n_points], N = frame_offsets[nq];
    if ((O > 0 && !obs_point) || (T > 0 && !track_image) || (N > 0 && (!frames || !cluster))) return fail(F + "null argument");
    if (const int64_t o = first_outside(obs_point, O, n_points); o < O) return fail(F + "observation " + std::to_string(o) + ": point row out of range");
    if (const int64_t t = first_outside(track_image, T, n_images); t < T) return fail(F + "track element " + std::to_string(t) + ": image index out of range");
    {
        std::vector<int32_t> seen((size_t)n_images, -1);           // the query that listed the image last
        for (int q = 0; q < nq; ++q) {
            if (frame_offsets[q + 1] - frame_offsets[q] > SFD2_CLUSTER_MAX_FRAMES)
                return fail(F + "query " + std::to_string(q) + " lists " + std::to_string(frame_offsets[q + 1] - frame_offsets[q]) + " frames, more than " +
                            std::to_string(SFD2_CLUSTER_MAX_FRAMES));
            for (int64_t p = frame_offsets[q]; p < frame_offsets[q + 1]; ++p) {
                const int32_t f = frames[p];
                if (f < 0 || f >= n_images) return fail(F + "query " + std::to_string(q) + ": image index out of range");
                if (seen[f] == q) return fail(F + "query " + std::to_string(q) + " lists image " + std::to_string(f) + " twice");
                seen[f] = q;
            }
        }
    }
    const int global = (flags & SFD2_CLUSTER_FLAG_GLOBAL_SLOTS) || n_images > SFD2_CLUSTER_LDS_IMAGES;
    // global rows: at most 256 MB of scratch
    const int blocks = global ? (int)std::max<size_t>(1, std::min<size_t>(std::min(nq, 512), ((size_t)256 << 20) / (2 * (size_t)n_images))) : std::min(nq, 512);
    HIPCHECK(hipSetDevice(c->device));
    Carve in, ws;
    const size_t o_oo = in.take(8 * (size_t)(n_images + 1)), o_op = in.take(4 * (size_t)O), o_to = in.take(8 * (size_t)(n_points + 1)),
                 o_ti = in.take(4 * (size_t)T), o_fo = in.take(8 * (size_t)(nq + 1)), o_fr = in.take(4 * (size_t)N);
    const size_t o_cl = ws.take(4 * (size_t)N), o_n = ws.take(4 * (size_t)nq), o_scr = ws.take(global ? 2 * (size_t)blocks * n_images : 0);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->pairs_in, in.off));
    HIPCHECK(grow(c->pairs_ws, ws.off));
    char *di = c->pairs_in.as<char>(), *dw = c->pairs_ws.as<char>();
    HIPCHECK(hipMemcpyAsync(di + o_oo, obs_offsets, 8 * (size_t)(n_images + 1), hipMemcpyHostToDevice, c->stream));
    if (O) HIPCHECK(hipMemcpyAsync(di + o_op, obs_point, 4 * (size_t)O, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(di + o_to, track_offsets, 8 * (size_t)(n_points + 1), hipMemcpyHostToDevice, c->stream));
    if (T) HIPCHECK(hipMemcpyAsync(di + o_ti, track_image, 4 * (size_t)T, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(di + o_fo, frame_offsets, 8 * (size_t)(nq + 1), hipMemcpyHostToDevice, c->stream));
    if (N) HIPCHECK(hipMemcpyAsync(di + o_fr, frames, 4 * (size_t)N, hipMemcpyHostToDevice, c->stream));
    if (global) HIPCHECK(hipMemsetAsync(dw + o_scr, 0xff, 2 * (size_t)blocks * n_images, c->stream));
    {
        ProfScope ps(c, "covis_clusters", global ? "covis_cluster<global>" : "covis_cluster<lds>", 0.0, 4.0 * (double)(O + T + N));
        HIPCHECK(launch_covis_clusters(c->stream, at<const int64_t>(di, o_oo), at<const int32_t>(di, o_op), n_images, at<const int64_t>(di, o_to),
                                       at<const int32_t>(di, o_ti), at<const int64_t>(di, o_fo), at<const int32_t>(di, o_fr), nq, global, blocks,
                                       at<uint16_t>(dw, o_scr), at<int32_t>(dw, o_cl), at<int32_t>(dw, o_n)));
    }
    if (N) HIPCHECK(hipMemcpyAsync(cluster, dw + o_cl, 4 * (size_t)N, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(n_clusters, dw + o_n, 4 * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}
