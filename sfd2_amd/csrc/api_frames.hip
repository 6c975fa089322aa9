// libsfd2hip: sfd2_covis_frames -- checks the tasks and whatever of the map lies on the host (every index the kernel follows from a
// host array is bounds-checked here, before anything is uploaded or written; of a device-resident map the three offset ends are read
// back and compared with the stated sizes, and the kernel range-checks what it reads), uploads the tasks, one launch of
// frames_kernels.hip on the context's stream, results back.
#include "sfd2_ctx.h"
#include "api_scratch.h"

namespace {

static_assert(sizeof(FramesTaskDev) == sizeof(sfd2_frames_task) && offsetof(FramesTaskDev, q_th) == offsetof(sfd2_frames_task, q_th) &&
                  offsetof(FramesTaskDev, tvec) == offsetof(sfd2_frames_task, tvec),
              "FramesTaskDev is sfd2_frames_task");
static_assert(FRAMES_MAX_CANDIDATES == SFD2_FRAMES_MAX_CANDIDATES && FRAMES_KIND_POS == SFD2_FRAMES_POS, "frames constants");

}  // namespace

extern "C" int sfd2_covis_frames(sfd2_ctx *c, const sfd2_frames_map *map, const sfd2_frames_task *tasks, int n_tasks, const int64_t *ref_offsets,
                                 const int32_t *ref_points, int cap, int32_t *idx, int32_t *n_out, int32_t *status, int flags)
{
    const std::string F("sfd2_covis_frames: ");
    if (!c || !map || !tasks || !idx || !n_out || !status) return fail(F + "null argument");
    const int n_images = map->n_images, n_points = map->n_points;
    const int64_t O = map->n_obs, T = map->n_track, S = map->n_seen;
    if (n_images < 1 || n_points < 0 || n_tasks < 1 || O < 0 || T < 0 || S < 0)
        return fail(F + "n_images and n_tasks must be positive, n_points and the array sizes non-negative");
    if (cap < 1) return fail(F + "cap must be at least 1");
    if (flags & ~SFD2_FRAMES_FLAG_GLOBAL_COUNTERS) return fail(F + "unknown flags");
    if (!map->obs_offsets || !map->track_offsets || !map->seen_offsets || (O > 0 && !map->obs_point) || (T > 0 && !map->track_image) ||
        (S > 0 && !map->seen_image))
        return fail(F + "null map array");
    // ---- tasks (always host arrays)
    bool any_pos = false, any_pose = false, any_ref = false;
    for (int q = 0; q < n_tasks; ++q) {
        const sfd2_frames_task &t = tasks[q];
        const std::string Q = F + "task " + std::to_string(q) + ": ";
        if (t.frame < 0 || t.frame >= n_images) return fail(Q + "image index out of range");
        if (t.kind != SFD2_FRAMES_OBS && t.kind != SFD2_FRAMES_POS) return fail(Q + "kind must be SFD2_FRAMES_OBS or SFD2_FRAMES_POS");
        if (t.covisibility_frame < 0) return fail(Q + "covisibility_frame must not be negative");
        if (t.kind == SFD2_FRAMES_POS && !t.has_pose) return fail(Q + "the pos rule needs a pose");
        any_pos |= t.kind == SFD2_FRAMES_POS;
        any_pose |= t.has_pose != 0;
        any_ref |= t.use_ref != 0;
    }
    if (any_pos && !map->excluded) return fail(F + "the pos rule needs the excluded bytes");
    if (any_pose && (!map->qvec || !map->tvec)) return fail(F + "tasks with a pose need the images' qvec and tvec");
    int64_t R = 0;
    if (any_ref) {
        if (!ref_offsets) return fail(F + "use_ref without ref_offsets");
        if (!monotone(ref_offsets, n_tasks)) return fail(F + "ref_offsets must start at 0 and not decrease");
        R = ref_offsets[n_tasks];
        if (R > 0 && !ref_points) return fail(F + "use_ref without ref_points");
        for (int q = 0; q < n_tasks; ++q)
            if (tasks[q].use_ref && !in_range(ref_points + ref_offsets[q], ref_offsets[q + 1] - ref_offsets[q], n_points))
                return fail(F + "task " + std::to_string(q) + ": ref_points row out of range");
    }
    // ---- the map
    const int on_device = map->inputs_on_device != 0;
    HIPCHECK(hipSetDevice(c->device));
    if (on_device) {
        int64_t ends[3] = {-1, -1, -1};
        HIPCHECK(hipStreamSynchronize(c->stream));
        HIPCHECK(hipMemcpy(ends + 0, map->obs_offsets + n_images, 8, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(ends + 1, map->track_offsets + n_points, 8, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(ends + 2, map->seen_offsets + n_points, 8, hipMemcpyDeviceToHost));
        if (ends[0] != O || ends[1] != T || ends[2] != S) return fail(F + "the offsets of the device-resident map do not end at n_obs / n_track / n_seen");
    } else {
        if (!monotone(map->obs_offsets, n_images) || map->obs_offsets[n_images] != O) return fail(F + "obs_offsets must start at 0, not decrease and end at n_obs");
        if (!monotone(map->track_offsets, n_points) || map->track_offsets[n_points] != T)
            return fail(F + "track_offsets must start at 0, not decrease and end at n_track");
        if (!monotone(map->seen_offsets, n_points) || map->seen_offsets[n_points] != S) return fail(F + "seen_offsets must start at 0, not decrease and end at n_seen");
        if (!in_range(map->obs_point, O, n_points)) return fail(F + "obs_point: point row out of range");
        if (!in_range(map->track_image, T, n_images)) return fail(F + "track_image: image index out of range");
        if (!in_range(map->seen_image, S, n_images)) return fail(F + "seen_image: image index out of range");
    }
    const int global = (flags & SFD2_FRAMES_FLAG_GLOBAL_COUNTERS) || n_images > SFD2_FRAMES_LDS_IMAGES;
    // rows of global scratch per workgroup (touched list, counters): at most 256 MB; blocks does not depend on the flag
    const int blocks = (int)std::max<size_t>(1, std::min<size_t>(std::min(n_tasks, 256), ((size_t)256 << 20) / (8 * (size_t)n_images)));
    Carve in, ws;
    const size_t o_tk = in.take(sizeof(sfd2_frames_task) * (size_t)n_tasks), o_ro = in.take(any_ref ? 8 * (size_t)(n_tasks + 1) : 0),
                 o_rp = in.take(4 * (size_t)R);
    size_t o_oo = 0, o_op = 0, o_to = 0, o_ti = 0, o_so = 0, o_si = 0, o_ex = 0, o_qv = 0, o_tv = 0;
    if (!on_device) {
        o_oo = in.take(8 * (size_t)(n_images + 1)), o_op = in.take(4 * (size_t)O), o_to = in.take(8 * (size_t)(n_points + 1)), o_ti = in.take(4 * (size_t)T);
        o_so = in.take(8 * (size_t)(n_points + 1)), o_si = in.take(4 * (size_t)S), o_ex = in.take((size_t)n_images);
        o_qv = in.take(32 * (size_t)n_images), o_tv = in.take(24 * (size_t)n_images);
    }
    const size_t n_res = 2 * (size_t)n_tasks + (size_t)n_tasks * cap, scr = (size_t)blocks * n_images * (global ? 2 : 1);
    const size_t o_out = ws.take(4 * n_res), o_scr = ws.take(4 * scr);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->pairs_in, in.off));
    HIPCHECK(grow(c->pairs_ws, ws.off));
    char *di = c->pairs_in.as<char>(), *dw = c->pairs_ws.as<char>();
    HIPCHECK(hipMemcpyAsync(di + o_tk, tasks, sizeof(sfd2_frames_task) * (size_t)n_tasks, hipMemcpyHostToDevice, c->stream));
    if (any_ref) HIPCHECK(hipMemcpyAsync(di + o_ro, ref_offsets, 8 * (size_t)(n_tasks + 1), hipMemcpyHostToDevice, c->stream));
    if (R) HIPCHECK(hipMemcpyAsync(di + o_rp, ref_points, 4 * (size_t)R, hipMemcpyHostToDevice, c->stream));
    FramesMapDev dm;
    dm.obs_off = map->obs_offsets, dm.obs_point = map->obs_point, dm.trk_off = map->track_offsets, dm.trk_img = map->track_image;
    dm.seen_off = map->seen_offsets, dm.seen_img = map->seen_image, dm.excluded = map->excluded, dm.qvec = map->qvec, dm.tvec = map->tvec;
    dm.n_obs = O, dm.n_track = T, dm.n_seen = S, dm.n_images = n_images, dm.n_points = n_points;
    if (!on_device) {
        HIPCHECK(hipMemcpyAsync(di + o_oo, map->obs_offsets, 8 * (size_t)(n_images + 1), hipMemcpyHostToDevice, c->stream));
        if (O) HIPCHECK(hipMemcpyAsync(di + o_op, map->obs_point, 4 * (size_t)O, hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(di + o_to, map->track_offsets, 8 * (size_t)(n_points + 1), hipMemcpyHostToDevice, c->stream));
        if (T) HIPCHECK(hipMemcpyAsync(di + o_ti, map->track_image, 4 * (size_t)T, hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(di + o_so, map->seen_offsets, 8 * (size_t)(n_points + 1), hipMemcpyHostToDevice, c->stream));
        if (S) HIPCHECK(hipMemcpyAsync(di + o_si, map->seen_image, 4 * (size_t)S, hipMemcpyHostToDevice, c->stream));
        if (map->excluded) HIPCHECK(hipMemcpyAsync(di + o_ex, map->excluded, (size_t)n_images, hipMemcpyHostToDevice, c->stream));
        if (map->qvec) HIPCHECK(hipMemcpyAsync(di + o_qv, map->qvec, 32 * (size_t)n_images, hipMemcpyHostToDevice, c->stream));
        if (map->tvec) HIPCHECK(hipMemcpyAsync(di + o_tv, map->tvec, 24 * (size_t)n_images, hipMemcpyHostToDevice, c->stream));
        dm.obs_off = at<const int64_t>(di, o_oo), dm.obs_point = at<const int32_t>(di, o_op);
        dm.trk_off = at<const int64_t>(di, o_to), dm.trk_img = at<const int32_t>(di, o_ti);
        dm.seen_off = at<const int64_t>(di, o_so), dm.seen_img = at<const int32_t>(di, o_si);
        dm.excluded = at<const uint8_t>(di, o_ex);
        dm.qvec = at<const double>(di, o_qv), dm.tvec = at<const double>(di, o_tv);
    }
    HIPCHECK(hipMemsetAsync(dw + o_out, 0xff, 4 * n_res, c->stream));           // slots a row does not fill hold -1
    if (global) HIPCHECK(hipMemsetAsync(dw + o_scr, 0, 4 * scr, c->stream));
    {
        ProfScope ps(c, "covis_frames", global ? "covis_frames<global>" : "covis_frames<lds>", 0.0, 0.0);
        HIPCHECK(launch_covis_frames(c->stream, dm, at<const FramesTaskDev>(di, o_tk), n_tasks, at<const int64_t>(di, o_ro), at<const int32_t>(di, o_rp), cap,
                                     global, blocks, at<int>(dw, o_scr), at<int32_t>(dw, o_out)));
    }
    // into a buffer of the call's own first: the caller's arrays stay untouched when a copy or the kernel fails
    std::vector<int32_t> h(n_res);
    HIPCHECK(hipMemcpyAsync(h.data(), dw + o_out, 4 * n_res, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int q = 0; q < n_tasks; ++q)
        if (h[2 * (size_t)q + 1] == 3) return fail(F + "task " + std::to_string(q) + ": the device-resident map holds an index out of range");
    for (int q = 0; q < n_tasks; ++q) n_out[q] = h[2 * (size_t)q], status[q] = h[2 * (size_t)q + 1];
    std::copy(h.begin() + 2 * (size_t)n_tasks, h.end(), idx);
    return 0;
}
