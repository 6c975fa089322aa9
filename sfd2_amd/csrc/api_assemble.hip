// libsfd2hip: sfd2_assemble_2d3d -- checks and packs the jobs, the four launches of assemble_kernels.hip on the context's stream,
// results back.  The job and image descriptors (and host-side key points / scores) go up in one copy.
#include "sfd2_ctx.h"
#include "api_scratch.h"
#include "pose_camera.h"

namespace {

constexpr size_t kRowBytes = 16 + 24 + 4 + 4 + 4 + 4;     // one output row over the six arrays

}  // namespace

extern "C" int sfd2_assemble_2d3d(sfd2_ctx *c, const sfd2_point_table *map, sfd2_assemble_job *jobs, int n_jobs, int out_on_device, int flags)
{
    const std::string F("sfd2_assemble_2d3d: ");
    if (!c || !map || (n_jobs > 0 && !jobs)) return fail(F + "null argument");
    if (n_jobs < 0 || n_jobs > 65535) return fail(F + "the number of jobs must lie in [0, 65535]");
    if (flags != 0) return fail(F + "unknown flags");
    if (map->n_points < 0 || (map->n_points > 0 && (!map->xyz || !map->track_len))) return fail(F + "bad point table");
    if (n_jobs == 0) return 0;
    // ---- checks and the layout of the three device blocks
    std::vector<AsmJobDev> jd(n_jobs);
    size_t n_img = 0, ws_elems = 0, blk_elems = 0, out_rows = 0;
    Carve host_in;                                             // the host key points and scores, as the packing loop below carves them
    int max_blocks = 0;
    for (int j = 0; j < n_jobs; ++j) {
        sfd2_assemble_job &J = jobs[j];
        const std::string at = F + "job " + std::to_string(j) + ": ";
        J.m = 0;
        J.status = 0;
        if (J.k < 0 || J.n < 0 || J.match_rows < 0 || J.capacity < 0) return fail(at + "negative size");
        if (J.k > 0 && !J.images) return fail(at + "null images");
        if ((int64_t)J.k * J.n > 0x7fffffffLL) return fail(at + "k * n must stay below 2^31");
        if (J.n > 0 && !J.keypoints) return fail(at + "null keypoints");
        if (J.k > 0 && !J.image_counts) return fail(at + "null image_counts");
        if (J.capacity > 0 && (!J.points2D || !J.points3D || !J.point_row || !J.query_idx || !J.image_idx || !J.score))
            return fail(at + "null output buffer");
        if (std::isnan(J.obs_th)) return fail(at + "obs_th is NaN");
        AsmJobDev &d = jd[j];
        memset(&d, 0, sizeof(d));
        for (int i = 0; i < J.k; ++i) {
            const sfd2_assemble_image &im = J.images[i];
            if (im.n1 < 0 || (im.n1 > 0 && !im.point_rows)) return fail(at + "image " + std::to_string(i) + ": bad table");
            if (im.match_row >= J.match_rows) return fail(at + "image " + std::to_string(i) + ": match_row beyond matches0");
            if (im.match_row >= 0 && J.n > 0 && !J.matches0) return fail(at + "null matches0");
        }
        if (J.gate) {
            std::string why;
            if (!sfd2_pose_cam(J.model, J.params, d.cam, why)) return fail(at + why);
            double nq = 0;
            for (int a = 0; a < 4; ++a) nq += J.qvec[a] * J.qvec[a];
            nq = std::sqrt(nq);
            bool fin = std::isfinite(nq) && nq > 0 && !std::isnan(J.radius);
            for (int a = 0; a < 3; ++a) fin = fin && std::isfinite(J.tvec[a]);
            if (!fin) return fail(at + "the gate needs a finite pose with a non-zero quaternion and a radius");
            quat_to_rot(J.qvec[0] / nq, J.qvec[1] / nq, J.qvec[2] / nq, J.qvec[3] / nq, d.R);
            for (int a = 0; a < 3; ++a) d.t[a] = J.tvec[a];
            d.radius = J.radius;
        }
        d.k = J.k;
        d.n = J.n;
        d.nchunk = (J.n + SFD2_ASM_WG - 1) / SFD2_ASM_WG;
        d.gate = J.gate ? 1 : 0;
        d.cap = J.capacity;
        d.obs_th = J.obs_th;
        d.ws_off = (int64_t)ws_elems;
        d.blk_off = (int64_t)blk_elems;
        d.cnt_off = (int64_t)n_img;
        ws_elems += (size_t)J.k * J.n;
        blk_elems += (size_t)J.k * d.nchunk;
        n_img += (size_t)J.k;
        max_blocks = std::max(max_blocks, J.k * d.nchunk);
        if (!J.inputs_on_device) host_in.take((size_t)J.n * 8);
        if (!J.inputs_on_device && J.scores) host_in.take((size_t)J.n * 4);
        if (!out_on_device) out_rows += (size_t)J.capacity;
    }
    HIPCHECK(hipSetDevice(c->device));
    // in: jobs | images | host key points and scores;  ws: rows | keep | block counts | image counts | results;  out: the rows of host-bound jobs
    Carve ci, cw;
    const size_t o_job = ci.take(sizeof(AsmJobDev) * n_jobs), o_img = ci.take(sizeof(AsmImgDev) * n_img), o_hin = ci.off;
    const size_t in_bytes = o_hin + host_in.off;
    const size_t o_rows = cw.take(4 * ws_elems), o_keep = cw.take(ws_elems), o_blk = cw.take(4 * blk_elems), o_cnt = cw.take(4 * n_img),
                 o_res = cw.take(sizeof(AsmResDev) * n_jobs);
    HIPCHECK(grow(c->asm_in, in_bytes));       // (hipFree waits for the device: an earlier call's kernels have finished with the old block)
    HIPCHECK(grow(c->asm_ws, cw.off));
    // six arrays per job, each at most 255 bytes of padding -- or, of a job with capacity 0, one 256-byte slot: 6 * 256 per job covers both
    if (!out_on_device) HIPCHECK(grow(c->asm_out, std::max<size_t>(out_rows, 1) * kRowBytes + 6 * 256 * (size_t)n_jobs));
    char *in = c->asm_in.as<char>(), *ws = c->asm_ws.as<char>(), *out = c->asm_out.as<char>();
    std::vector<char> stage(in_bytes, 0);
    {
        AsmImgDev *im = at<AsmImgDev>(stage.data(), o_img);
        Carve hin{o_hin}, oo;
        size_t ii = 0;
        for (int j = 0; j < n_jobs; ++j) {
            const sfd2_assemble_job &J = jobs[j];
            AsmJobDev &d = jd[j];
            d.matches0 = reinterpret_cast<const long long *>(J.matches0);
            d.imgs = at<const AsmImgDev>(in, o_img) + ii;
            for (int i = 0; i < J.k; ++i, ++ii) {
                im[ii].tab = J.images[i].point_rows;
                im[ii].n1 = J.images[i].n1;
                im[ii].mrow = J.images[i].match_row < 0 ? -1 : J.images[i].match_row;
            }
            if (J.inputs_on_device) {
                d.kpq = J.keypoints;
                d.scores = J.scores;
            } else {
                const size_t o_kp = hin.take((size_t)J.n * 8);
                if (J.n) memcpy(stage.data() + o_kp, J.keypoints, (size_t)J.n * 8);
                d.kpq = at<const float>(in, o_kp);
                if (J.scores) {
                    const size_t o_sc = hin.take((size_t)J.n * 4);
                    if (J.n) memcpy(stage.data() + o_sc, J.scores, (size_t)J.n * 4);
                    d.scores = at<const float>(in, o_sc);
                }
            }
            if (out_on_device) {
                d.p2 = J.points2D; d.p3 = J.points3D; d.prow = J.point_row; d.qidx = J.query_idx; d.iidx = J.image_idx; d.score = J.score;
            } else {
                const size_t cap = (size_t)J.capacity;
                d.p2 = at<double>(out, oo.take(16 * cap));
                d.p3 = at<double>(out, oo.take(24 * cap));
                d.prow = at<int32_t>(out, oo.take(4 * cap));
                d.qidx = at<int32_t>(out, oo.take(4 * cap));
                d.iidx = at<int32_t>(out, oo.take(4 * cap));
                d.score = at<float>(out, oo.take(4 * cap));
            }
        }
        memcpy(stage.data() + o_job, jd.data(), sizeof(AsmJobDev) * n_jobs);
    }
    HIPCHECK(hipMemcpyAsync(in, stage.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
    AsmResDev *res = at<AsmResDev>(ws, o_res);
    HIPCHECK(hipMemsetAsync(res, 0, sizeof(AsmResDev) * n_jobs, c->stream));
    {
        ProfScope ps(c, "assemble_2d3d", "assemble_resolve+flag+scan+scatter", 0.0, (double)ws_elems * 18.0);
        launch_assemble(c->stream, at<const AsmJobDev>(in, o_job), n_jobs, max_blocks, map->xyz, map->track_len, map->n_points, at<int32_t>(ws, o_rows),
                        at<unsigned char>(ws, o_keep), at<int32_t>(ws, o_blk), at<int32_t>(ws, o_cnt), res);
    }
    HIPCHECK(hipGetLastError());
    std::vector<AsmResDev> r(n_jobs);
    std::vector<int32_t> cnt(std::max<size_t>(n_img, 1));
    HIPCHECK(hipMemcpyAsync(r.data(), res, sizeof(AsmResDev) * n_jobs, hipMemcpyDeviceToHost, c->stream));
    if (n_img) HIPCHECK(hipMemcpyAsync(cnt.data(), ws + o_cnt, 4 * n_img, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    int bad = -1;
    for (int j = 0; j < n_jobs; ++j) {
        sfd2_assemble_job &J = jobs[j];
        J.m = r[j].m;
        J.status = r[j].status;
        for (int i = 0; i < J.k; ++i) J.image_counts[i] = cnt[jd[j].cnt_off + i];
        if (J.status && bad < 0) bad = j;
        if (!out_on_device && !J.status && J.m > 0) {
            const size_t m = (size_t)J.m;
            HIPCHECK(hipMemcpyAsync(J.points2D, jd[j].p2, 16 * m, hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(J.points3D, jd[j].p3, 24 * m, hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(J.point_row, jd[j].prow, 4 * m, hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(J.query_idx, jd[j].qidx, 4 * m, hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(J.image_idx, jd[j].iidx, 4 * m, hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(J.score, jd[j].score, 4 * m, hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIPCHECK(hipStreamSynchronize(c->stream));
    if (bad >= 0) {
        const sfd2_assemble_job &J = jobs[bad];
        std::string why;
        if (J.status & SFD2_ASM_ST_MATCH_RANGE) why += " a match index beyond its image's key points;";
        if (J.status & SFD2_ASM_ST_ROW_RANGE) why += " a table entry beyond the point table;";
        if (J.status & SFD2_ASM_ST_CAPACITY) why += " m = " + std::to_string(J.m) + " above the capacity " + std::to_string(J.capacity) + ";";
        return fail(F + "job " + std::to_string(bad) + ":" + why);
    }
    return 0;
}
