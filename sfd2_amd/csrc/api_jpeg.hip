// libsfd2hip: sfd2_jpeg_decode -- a prepared baseline JPEG (jpeg_parse.hip) to a device RGBX image (jpeg_kernels.hip).
#include "sfd2_ctx.h"

namespace {

hipError_t grow(ScratchBuf &b, size_t bytes, sfd2_ctx *c, bool &synced)
{
    if (bytes <= b.cap) return hipSuccess;
    if (!synced) {                                  // queued decodes may still use the old buffer
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return e;
        synced = true;
    }
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    const size_t want = bytes + bytes / 4;          // headroom: the next image is rarely the same size
    hipError_t e = hipMalloc(&b.p, want);
    if (e == hipSuccess) b.cap = want;
    return e;
}

// the frame's geometry for the kernels; false when the info does not describe a supported, prepared frame
bool geometry(const sfd2_jpeg_info *info, JpegGeom &g, int64_t &tab_off, size_t &plane_bytes)
{
    memset(&g, 0, sizeof(g));
    if (!info->supported || !info->prepared || info->width < 1 || info->height < 1) return false;
    const int nc = info->n_components;
    if (nc != 1 && nc != 3) return false;
    g.ncomp = nc;
    g.W = info->width;
    g.H = info->height;
    g.mcus_x = info->mcus_x;
    g.nlanes = info->n_lanes;
    g.nint = info->n_intervals;
    if (g.nlanes < 1 || g.nint < 1) return false;
    if (nc == 1) {
        g.bpm = 1;
        g.hs[0] = g.vs[0] = 1;
        g.bw[0] = (g.W + 7) / 8;
        g.bh[0] = (g.H + 7) / 8;
        g.mode = 0;
    } else {
        const int h0 = info->h_samp[0], v0 = info->v_samp[0];
        if (!((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2))) return false;
        g.bpm = h0 * v0 + 2;
        int u = 0;
        for (int c = 0; c < 3; ++c) {
            g.hs[c] = c ? 1 : h0;
            g.vs[c] = c ? 1 : v0;
            g.bw[c] = info->mcus_x * g.hs[c];
            g.bh[c] = info->mcus_y * g.vs[c];
            for (int dy = 0; dy < g.vs[c]; ++dy)
                for (int dx = 0; dx < g.hs[c]; ++dx, ++u) { g.unit_comp[u] = c; g.unit_dx[u] = dx; g.unit_dy[u] = dy; }
        }
        g.mode = (h0 == 1) ? 1 : (v0 == 1 ? 2 : 3);
        g.cw = (g.W + h0 - 1) / h0;
        g.ch = (g.H + v0 - 1) / v0;
    }
    int64_t blocks = 0, bytes = 0;
    for (int c = 0; c < nc; ++c) {
        g.blk_base[c] = (int)blocks;
        g.plane_off[c] = bytes;
        blocks += (int64_t)g.bw[c] * g.bh[c];
        bytes += (int64_t)g.bw[c] * g.bh[c] * 64;
    }
    if (blocks != info->n_blocks || blocks * 64 > INT32_MAX) return false;
    g.total_blocks = (int)blocks;
    g.ri_blocks = info->restart_interval * g.bpm;
    tab_off = info->prepared_bytes - jpeg_tail_bytes(g.nlanes, g.nint);
    if (tab_off < 16 || (tab_off & 15)) return false;
    g.ecs_words = (uint32_t)(tab_off / 4);
    plane_bytes = (size_t)bytes;
    return true;
}

}  // namespace

extern "C" int sfd2_jpeg_decode(sfd2_ctx *c, const uint8_t *data, int64_t n, const sfd2_jpeg_info *info, int flags, uint8_t *out_rgbx_dev,
                                int64_t out_cap, uint32_t *status, int status_on_device)
{
    if (!c || !data || !info || !out_rgbx_dev || !status) return fail("sfd2_jpeg_decode: null argument");
    JpegGeom g;
    int64_t tab_off = 0;
    size_t plane_bytes = 0;
    if (!geometry(info, g, tab_off, plane_bytes)) return fail("sfd2_jpeg_decode: info does not describe a prepared, supported JPEG");
    if (n < info->prepared_bytes) return fail("sfd2_jpeg_decode: n is smaller than info->prepared_bytes");
    if (out_cap < (int64_t)4 * g.W * g.H) return fail("sfd2_jpeg_decode: output smaller than H * W * 4 bytes");
    HIPCHECK(hipSetDevice(c->device));
    JpegScratch &s = c->jpeg;
    if (!s.ev_copied[0])
        for (int i = 0; i < 2; ++i) {
            HIPCHECK(hipEventCreateWithFlags(&s.ev_copied[i], hipEventDisableTiming));
            HIPCHECK(hipEventCreateWithFlags(&s.ev_free[i], hipEventDisableTiming));
        }
    bool synced = false;
    const int slot = s.slot = (s.slot + 1) & 1;
    const size_t in_bytes = (size_t)info->prepared_bytes;
    HIPCHECK(grow(s.in[slot], in_bytes, c, synced));
    HIPCHECK(grow(s.lanes, sizeof(JpegLane) * g.nlanes, c, synced));
    const size_t ngroups = (g.nlanes + 255) / 256;
    HIPCHECK(grow(s.pre, 16 * ((size_t)g.nlanes + ngroups), c, synced));
    HIPCHECK(grow(s.coef, (size_t)g.total_blocks * 64 * sizeof(short), c, synced));
    HIPCHECK(grow(s.planes, plane_bytes, c, synced));
    HIPCHECK(grow(s.words, 4 * (SFD2_JPEG_SYNC_LAUNCHES + 1), c, synced));
    // upload: through the copy stream once this slot's previous decode has read it (pinned data: overlaps the work in front of it)
    HIPCHECK(hipStreamWaitEvent(c->copy_stream, s.ev_free[slot], 0));
    HIPCHECK(hipMemcpyAsync(s.in[slot].p, data, in_bytes, hipMemcpyHostToDevice, c->copy_stream));
    HIPCHECK(hipEventRecord(s.ev_copied[slot], c->copy_stream));
    HIPCHECK(hipStreamWaitEvent(c->stream, s.ev_copied[slot], 0));
    unsigned int *words = s.words.as<unsigned int>();
    HIPCHECK(hipMemsetAsync(words, 0, 4 * (SFD2_JPEG_SYNC_LAUNCHES + 1), c->stream));
    int *pre = s.pre.as<int>();
    launch_jpeg_decode(c->stream, s.in[slot].as<unsigned char>(), tab_off, g, s.lanes.as<JpegLane>(), pre, pre + 4 * (size_t)g.nlanes, words,
                       s.coef.as<short>(), s.planes.as<unsigned char>(), out_rgbx_dev, words + SFD2_JPEG_SYNC_LAUNCHES);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(s.ev_free[slot], c->stream));
    HIPCHECK(hipMemcpyAsync(status, words + SFD2_JPEG_SYNC_LAUNCHES, 4, status_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                            c->stream));
    if (flags & SFD2_FLAG_ASYNC) return 0;
    uint32_t st = 0;
    HIPCHECK(hipMemcpyAsync(&st, words + SFD2_JPEG_SYNC_LAUNCHES, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    if (st) return fail("sfd2_jpeg_decode: the entropy-coded data is not decodable here (status " + std::to_string(st) + ")");
    return 0;
}
