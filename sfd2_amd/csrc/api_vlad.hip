// libsfd2hip: sfd2_vlad_assign / sfd2_vlad_aggregate / sfd2_vlad_kmeans -- checks the arguments (before anything is uploaded), uploads
// the inputs, the launches of vlad_kernels.hip on the context's stream, results back.
#include "sfd2_ctx.h"
#include "api_scratch.h"

namespace {

constexpr size_t ROW = 4 * (size_t)SFD2_VLAD_DIM;                  // bytes of a row

bool k_ok(int k) { return k >= 1 && k <= SFD2_VLAD_MAX_K; }
std::string k_range() { return "k must lie in [1, " + std::to_string(SFD2_VLAD_MAX_K) + "]"; }
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int sfd2_vlad_assign(sfd2_ctx *c, const float *x, int64_t n, const float *centroids, int k, int inputs_on_device, int32_t *assign,
                                float *score, int flags)
{
    const std::string F("sfd2_vlad_assign: ");
    if (n < 1) return fail(F + "n must be positive");
    if (!k_ok(k)) return fail(F + k_range());
    if (!c || !x || !centroids || !assign) return fail(F + "null argument");
    if (flags) return fail(F + "unknown flags");
    if (inputs_on_device && (!aligned16(x) || !aligned16(centroids))) return fail(F + "device inputs must be 16-byte aligned");
    HIPCHECK(hipSetDevice(c->device));
    Carve in, ws;
    const size_t o_x = in.take(inputs_on_device ? 0 : ROW * (size_t)n), o_c = in.take(inputs_on_device ? 0 : ROW * k);
    const size_t o_h = ws.take(4 * (size_t)k), o_a = ws.take(4 * (size_t)n), o_s = ws.take(4 * (size_t)n), o_flag = ws.take(4);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->vlad_in, in.off));
    HIPCHECK(grow(c->vlad_ws, ws.off));
    char *di = c->vlad_in.as<char>(), *dw = c->vlad_ws.as<char>();
    const float *dx = x, *dc = centroids;
    if (!inputs_on_device) {
        HIPCHECK(hipMemcpyAsync(di + o_x, x, ROW * (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(di + o_c, centroids, ROW * k, hipMemcpyHostToDevice, c->stream));
        dx = at<const float>(di, o_x);
        dc = at<const float>(di, o_c);
    }
    HIPCHECK(hipMemsetAsync(dw + o_flag, 0, 4, c->stream));
    prof_step_begin(c);                                            // one profiled step per call: sfd2_get_layer_timings reports the launches
    {
        ProfScope ps(c, "vlad_assign", "pairs_finite+vlad_half_norms+vlad_assign", 2.0 * (double)n * k * SFD2_VLAD_DIM, (double)ROW * (double)(n + k));
        HIPCHECK(launch_pairs_finite(c->stream, dx, (size_t)n * SFD2_VLAD_DIM, dc, (size_t)k * SFD2_VLAD_DIM, at<int>(dw, o_flag)));
        HIPCHECK(launch_vlad_half_norms(c->stream, dc, k, at<float>(dw, o_h)));
        HIPCHECK(launch_vlad_assign(c->stream, dx, n, dc, at<const float>(dw, o_h), k, at<int32_t>(dw, o_a), at<float>(dw, o_s), nullptr));
    }
    prof_step_end(c);
    int bad = 0;
    HIPCHECK(hipMemcpyAsync(&bad, dw + o_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(assign, dw + o_a, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (score) HIPCHECK(hipMemcpyAsync(score, dw + o_s, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    if (bad) return fail(F + "non-finite descriptor or centroid");
    return 0;
}

extern "C" int sfd2_vlad_aggregate(sfd2_ctx *c, const float *x, const int64_t *offsets, int n_images, const float *centroids, int k,
                                   int inputs_on_device, int norm, float *out, int32_t *assign, int flags)
{
    const std::string F("sfd2_vlad_aggregate: ");
    if (n_images < 1) return fail(F + "n_images must be positive");
    if (!k_ok(k)) return fail(F + k_range());
    if (!c || !offsets || !centroids || !out) return fail(F + "null argument");
    if (norm != SFD2_VLAD_NORM_INTRA && norm != SFD2_VLAD_NORM_SSR && norm != SFD2_VLAD_NORM_NONE) return fail(F + "unknown norm");
    if (flags) return fail(F + "unknown flags");
    if (!monotone(offsets, n_images)) return fail(F + "offsets must start at 0 and not decrease");
    const int64_t n = offsets[n_images];
    if (n > 0 && !x) return fail(F + "null argument");
    if (inputs_on_device && ((n > 0 && !aligned16(x)) || !aligned16(centroids))) return fail(F + "device inputs must be 16-byte aligned");
    HIPCHECK(hipSetDevice(c->device));
    const size_t out_bytes = ROW * (size_t)k * (size_t)n_images;
    Carve in, ws;
    const size_t o_x = in.take(inputs_on_device ? 0 : ROW * (size_t)n), o_c = in.take(inputs_on_device ? 0 : ROW * k),
                 o_off = in.take(8 * ((size_t)n_images + 1));
    const size_t o_h = ws.take(4 * (size_t)k), o_a = ws.take(4 * (size_t)n), o_out = ws.take(out_bytes), o_flag = ws.take(4);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->vlad_in, in.off));
    HIPCHECK(grow(c->vlad_ws, ws.off));
    char *di = c->vlad_in.as<char>(), *dw = c->vlad_ws.as<char>();
    const float *dx = x, *dc = centroids;
    if (!inputs_on_device) {
        if (n) HIPCHECK(hipMemcpyAsync(di + o_x, x, ROW * (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(di + o_c, centroids, ROW * k, hipMemcpyHostToDevice, c->stream));
        dx = at<const float>(di, o_x);
        dc = at<const float>(di, o_c);
    }
    HIPCHECK(hipMemcpyAsync(di + o_off, offsets, 8 * ((size_t)n_images + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemsetAsync(dw + o_flag, 0, 4, c->stream));
    prof_step_begin(c);
    {
        ProfScope ps(c, "vlad_aggregate", "pairs_finite+vlad_half_norms+vlad_assign+vlad_aggregate", 2.0 * (double)n * k * SFD2_VLAD_DIM,
                     2.0 * (double)ROW * (double)n + (double)out_bytes);
        HIPCHECK(launch_pairs_finite(c->stream, dx, (size_t)n * SFD2_VLAD_DIM, dc, (size_t)k * SFD2_VLAD_DIM, at<int>(dw, o_flag)));
        HIPCHECK(launch_vlad_half_norms(c->stream, dc, k, at<float>(dw, o_h)));
        if (n) HIPCHECK(launch_vlad_assign(c->stream, dx, n, dc, at<const float>(dw, o_h), k, at<int32_t>(dw, o_a), nullptr, nullptr));
        HIPCHECK(launch_vlad_aggregate(c->stream, dx, n, at<const int64_t>(di, o_off), n_images, dc, k, at<const int32_t>(dw, o_a), norm,
                                       at<float>(dw, o_out), nullptr));
    }
    prof_step_end(c);
    int bad = 0;
    HIPCHECK(hipMemcpyAsync(&bad, dw + o_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    if (bad) return fail(F + "non-finite descriptor or centroid");
    HIPCHECK(hipMemcpyAsync(out, dw + o_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    if (assign && n) HIPCHECK(hipMemcpyAsync(assign, dw + o_a, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int sfd2_vlad_kmeans(sfd2_ctx *c, const float *x, int64_t n, int k, int max_iters, int inputs_on_device, float *centroids,
                                int64_t *counts, int64_t *moved, int *iters_run, int flags)
{
    const std::string F("sfd2_vlad_kmeans: ");
    if (n < 1) return fail(F + "n must be positive");
    if (!k_ok(k)) return fail(F + k_range());
    if (max_iters < 1) return fail(F + "max_iters must be positive");
    if (!c || !x || !centroids || !counts || !moved || !iters_run) return fail(F + "null argument");
    if (flags) return fail(F + "unknown flags");
    if (inputs_on_device && !aligned16(x)) return fail(F + "device inputs must be 16-byte aligned");
    HIPCHECK(hipSetDevice(c->device));
    const int64_t chunks = (n + SFD2_VLAD_CHUNK - 1) / SFD2_VLAD_CHUNK;
    Carve in, ws;
    const size_t o_x = in.take(inputs_on_device ? 0 : ROW * (size_t)n);
    const size_t o_c = ws.take(ROW * k), o_h = ws.take(4 * (size_t)k), o_a = ws.take(4 * (size_t)n), o_ps = ws.take(ROW * (size_t)k * (size_t)chunks),
                 o_pc = ws.take(4 * (size_t)k * (size_t)chunks), o_cnt = ws.take(8 * (size_t)k), o_mv = ws.take(8 * (size_t)max_iters),
                 o_flag = ws.take(4);
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(grow(c->vlad_in, in.off));
    HIPCHECK(grow(c->vlad_ws, ws.off));
    char *di = c->vlad_in.as<char>(), *dw = c->vlad_ws.as<char>();
    const float *dx = x;
    if (!inputs_on_device) {
        HIPCHECK(hipMemcpyAsync(di + o_x, x, ROW * (size_t)n, hipMemcpyHostToDevice, c->stream));
        dx = at<const float>(di, o_x);
    }
    float *dc = at<float>(dw, o_c);
    HIPCHECK(hipMemcpyAsync(dc, centroids, ROW * k, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemsetAsync(dw + o_flag, 0, 4, c->stream));
    HIPCHECK(hipMemsetAsync(dw + o_a, 0xff, 4 * (size_t)n, c->stream));       // -1: every row moves in the first iteration
    HIPCHECK(hipMemsetAsync(dw + o_mv, 0, 8 * (size_t)max_iters, c->stream));
    HIPCHECK(launch_pairs_finite(c->stream, dx, (size_t)n * SFD2_VLAD_DIM, dc, (size_t)k * SFD2_VLAD_DIM, at<int>(dw, o_flag)));
    int bad = 0;
    HIPCHECK(hipMemcpyAsync(&bad, dw + o_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    if (bad) return fail(F + "non-finite descriptor or centroid");
    for (int it = 0; it < max_iters; ++it) moved[it] = -1;
    int it = 0;
    prof_step_begin(c);                                            // one step for the call, a scope per iteration (the first PROF_SLOTS of them)
    for (; it < max_iters;) {
        unsigned long long mv = 0;
        {
            ProfScope ps(c, "vlad_kmeans", "vlad_half_norms+vlad_assign+vlad_aggregate+vlad_update", 2.0 * (double)n * k * SFD2_VLAD_DIM,
                         2.0 * (double)ROW * (double)n);
            HIPCHECK(launch_vlad_half_norms(c->stream, dc, k, at<float>(dw, o_h)));
            HIPCHECK(launch_vlad_assign(c->stream, dx, n, dc, at<const float>(dw, o_h), k, at<int32_t>(dw, o_a), nullptr,
                                        at<unsigned long long>(dw, o_mv) + it));
            HIPCHECK(launch_vlad_aggregate(c->stream, dx, n, nullptr, chunks, dc, k, at<const int32_t>(dw, o_a), -1, at<float>(dw, o_ps),
                                           at<int32_t>(dw, o_pc)));
            HIPCHECK(launch_vlad_update(c->stream, at<const float>(dw, o_ps), at<const int32_t>(dw, o_pc), chunks, k, dc, at<long long>(dw, o_cnt)));
        }
        HIPCHECK(hipMemcpyAsync(&mv, dw + o_mv + 8 * (size_t)it, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        moved[it++] = (int64_t)mv;
        if (mv == 0) break;
    }
    prof_step_end(c);
    *iters_run = it;
    HIPCHECK(hipMemcpyAsync(centroids, dc, ROW * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(counts, dw + o_cnt, 8 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}
