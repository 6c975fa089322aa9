// libsfd2hip: sfd2_match_guided_batch -- checks the pairs, uploads key points and descriptors, then one launch sequence of
// guided_match_kernels.hip for all pairs: the gate records, the gated GEMM + top-2 of both directions, the matcher's split merge and
// the decisions on the masked matrix.
#include "sfd2_ctx.h"
#include "api_scratch.h"

namespace {

size_t elt_size(int dtype) { return dtype == SFD2_DT_F64 ? 8 : (dtype == SFD2_DT_F16 ? 2 : 4); }

// a set the kernels read where it lies: the form sfd2_desc_pack makes
bool in_place(const sfd2_desc_set &s, int dim)
{
    return s.on_device && s.dtype == SFD2_DT_F16 && s.layout == SFD2_LAYOUT_ND && dim == 128;
}

size_t host_bytes(const sfd2_desc_set &s, int dim) { return s.on_device ? 0 : (size_t)s.n * dim * elt_size(s.dtype); }

const char *check_set(const sfd2_desc_set &s)
{
    if (s.rows) return ".rows must be NULL";
    if (s.n < 0) return ".n is negative";
    if (s.n > 0 && !s.data) return ".data is null";
    if (s.dtype != SFD2_DT_F32 && s.dtype != SFD2_DT_F64 && s.dtype != SFD2_DT_F16) return ".dtype is unknown";
    if (s.layout != SFD2_LAYOUT_ND && s.layout != SFD2_LAYOUT_DN) return ".layout is unknown";
    return nullptr;
}

}  // namespace

extern "C" int sfd2_match_guided_batch(sfd2_ctx *c, const sfd2_guided_problem *problems, int k, int dim, const sfd2_match_conf *conf,
                                       int64_t *matches0, float *scores0, int flags)
{
    const std::string F("sfd2_match_guided_batch");
    if (!c || !conf || (k > 0 && !problems)) return fail(F + ": null argument");
    if (k < 0 || k > 32767) return fail(F + ": k must lie in [0, 32767]");
    if (flags != 0) return fail(F + ": unknown flags");
    if (dim <= 0 || dim > 128) return fail(F + ": descriptor dimension must be in [1,128]");
    if (conf->flavour != SFD2_MATCH_HLOC) return fail(F + ": conf.flavour must be SFD2_MATCH_HLOC");
    if (conf->sim_mode != SFD2_SIM_F16) return fail(F + ": conf.sim_mode must be SFD2_SIM_F16");
    std::vector<GuidedProbDev> pd(k);
    int64_t N0 = 0, N1 = 0;
    int max_n = 0;
    size_t stage_bytes = 0;
    for (int i = 0; i < k; ++i) {
        const sfd2_guided_problem &p = problems[i];
        const std::string at = F + ": problem " + std::to_string(i) + ": ";
        if (const char *why = check_set(p.d0)) return fail(at + "d0" + why);
        if (const char *why = check_set(p.d1)) return fail(at + "d1" + why);
        if (p.model != SFD2_GUIDE_F && p.model != SFD2_GUIDE_H) return fail(at + "model must be SFD2_GUIDE_F or SFD2_GUIDE_H");
        if (!all_finite(p.M, 9)) return fail(at + "non-finite M");
        if (!(std::isfinite(p.max_error_px) && p.max_error_px > 0)) return fail(at + "max_error_px must be positive and finite");
        if ((p.d0.n > 0 && !p.xy0) || (p.d1.n > 0 && !p.xy1)) return fail(at + "null key points");
        if (!all_finite(p.xy0, 2 * (int64_t)p.d0.n)) return fail(at + "non-finite xy0");
        if (!all_finite(p.xy1, 2 * (int64_t)p.d1.n)) return fail(at + "non-finite xy1");
        GuidedProbDev &o = pd[i];
        memset(&o, 0, sizeof(o));
        for (int j = 0; j < 9; ++j) o.M[j] = p.M[j];
        o.model = p.model;
        o.n0 = p.d0.n;
        o.n1 = p.d1.n;
        o.off0 = N0;
        o.off1 = N1;
        N0 += p.d0.n;
        N1 += p.d1.n;
        max_n = std::max(max_n, std::max(p.d0.n, p.d1.n));
        stage_bytes += align256(host_bytes(p.d0, dim)) + align256(host_bytes(p.d1, dim));
    }
    if (N0 == 0) return 0;
    if (!matches0 || !scores0) return fail(F + ": null output");
    HIPCHECK(hipSetDevice(c->device));
    // candidate splits as sfd2_match_batch aims them: >= 6 work items per resident block slot (256 CUs x 3), never finer than 32 candidates
    const int blocks_per_job = (max_n + 127) / 128;
    int splits = (768 * 6 + 2 * k * blocks_per_job - 1) / (2 * k * blocks_per_job);
    splits = std::max(1, std::min(splits, std::min(8, (max_n + 31) / 32)));
    const size_t tot_part = (size_t)splits * (size_t)(N0 + N1);

    Carve ci, cw;
    // inputs: problems | key points of image 0 | of image 1 | host descriptor sets as given | jobs | finals
    const size_t o_pd = ci.take(sizeof(GuidedProbDev) * k), o_xy0 = ci.take(8 * (size_t)N0), o_xy1 = ci.take(8 * (size_t)N1);
    const size_t o_stage = ci.take(stage_bytes), o_jobs = ci.take(sizeof(GuidedJob) * 2 * k), o_fins = ci.take(sizeof(MatchFinal) * k);
    // work: fp16 sets | gate records | partials (two float arrays, one int array) | merged top-2 | outputs
    const size_t o_h0 = cw.take(256 * (size_t)N0), o_h1 = cw.take(256 * (size_t)N1), o_r0 = cw.take(16 * (size_t)N0), o_r1 = cw.take(16 * (size_t)N1);
    const size_t o_pf = cw.take(2 * sizeof(float) * tot_part), o_pi = cw.take(sizeof(int) * tot_part);
    const size_t o_red = cw.take(3 * sizeof(float) * (size_t)(N0 + N1)), o_m = cw.take(8 * (size_t)N0), o_s = cw.take(4 * (size_t)N0);
    HIPCHECK(hipStreamSynchronize(c->stream));              // earlier calls on this stream may still read the buffers
    HIPCHECK(grow(c->gm_in, ci.off));
    HIPCHECK(grow(c->gm_ws, cw.off));
    char *in = c->gm_in.as<char>(), *ws = c->gm_ws.as<char>();

    std::vector<float> xy0(2 * (size_t)N0), xy1(2 * (size_t)std::max<int64_t>(N1, 1));
    for (int i = 0; i < k; ++i) {
        if (pd[i].n0) memcpy(xy0.data() + 2 * pd[i].off0, problems[i].xy0, 8 * (size_t)pd[i].n0);
        if (pd[i].n1) memcpy(xy1.data() + 2 * pd[i].off1, problems[i].xy1, 8 * (size_t)pd[i].n1);
    }
    HIPCHECK(hipMemcpyAsync(in + o_pd, pd.data(), sizeof(GuidedProbDev) * k, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(in + o_xy0, xy0.data(), 8 * (size_t)N0, hipMemcpyHostToDevice, c->stream));
    if (N1) HIPCHECK(hipMemcpyAsync(in + o_xy1, xy1.data(), 8 * (size_t)N1, hipMemcpyHostToDevice, c->stream));
    launch_guided_prep(c->stream, at<const GuidedProbDev>(in, o_pd), k, max_n, at<const float>(in, o_xy0), at<const float>(in, o_xy1),
                       at<float4>(ws, o_r0), at<float4>(ws, o_r1));

    // every set as fp16 [n][128]: in place when it is packed already, through the matcher's conversion kernel otherwise
    size_t stage_off = o_stage;
    auto fp16_set = [&](const sfd2_desc_set &s, half_t *dst, const half_t **out) -> int {
        *out = dst;
        if (s.n == 0) return 0;
        if (in_place(s, dim)) { *out = reinterpret_cast<const half_t *>(s.data); return 0; }
        const void *src = s.data;
        if (!s.on_device) {
            HIPCHECK(hipMemcpyAsync(in + stage_off, s.data, host_bytes(s, dim), hipMemcpyHostToDevice, c->stream));
            src = in + stage_off;
            stage_off += align256(host_bytes(s, dim));
        }
        launch_match_prep(c->stream, src, s.n, s.n, nullptr, dim, s.dtype, s.layout, dst, nullptr);
        return 0;
    };
    std::vector<GuidedJob> jobs(2 * (size_t)k);
    std::vector<MatchFinal> fins(k);
    float *pf = at<float>(ws, o_pf), *red = at<float>(ws, o_red);
    int *pi = at<int>(ws, o_pi);
    size_t poff = 0, roff = 0;
    for (int i = 0; i < k; ++i) {
        const int n0 = pd[i].n0, n1 = pd[i].n1;
        const half_t *h0 = nullptr, *h1 = nullptr;
        if (fp16_set(problems[i].d0, at<half_t>(ws, o_h0) + 128 * (size_t)pd[i].off0, &h0)) return -1;
        if (fp16_set(problems[i].d1, at<half_t>(ws, o_h1) + 128 * (size_t)pd[i].off1, &h1)) return -1;
        GuidedJob &f = jobs[2 * i], &r = jobs[2 * i + 1];
        memset(&f, 0, sizeof(f));
        memset(&r, 0, sizeof(r));
        f.model = r.model = pd[i].model;
        f.t2 = r.t2 = (float)(problems[i].max_error_px * problems[i].max_error_px);
        // forward: keep the image-0 points, reduce over image 1
        f.a_hi = h1; f.b_hi = h0; f.a_rec = at<const float4>(ws, o_r1) + pd[i].off1; f.b_rec = at<const float4>(ws, o_r0) + pd[i].off0;
        f.na = n1; f.nb = n0; f.dir = 0;
        f.part_v1 = pf + 2 * poff; f.part_v2 = pf + 2 * poff + (size_t)splits * n0; f.part_i1 = pi + poff;
        poff += (size_t)splits * n0;
        // reverse: keep the image-1 points, reduce over image 0
        r.a_hi = h0; r.b_hi = h1; r.a_rec = f.b_rec; r.b_rec = f.a_rec;
        r.na = n0; r.nb = n1; r.dir = 1;
        r.part_v1 = pf + 2 * poff; r.part_v2 = pf + 2 * poff + (size_t)splits * n1; r.part_i1 = pi + poff;
        poff += (size_t)splits * n1;
        MatchFinal &fn = fins[i];
        memset(&fn, 0, sizeof(fn));
        fn.f_v1 = f.part_v1; fn.f_v2 = f.part_v2; fn.f_i1 = f.part_i1;
        fn.r_v1 = r.part_v1; fn.r_v2 = r.part_v2; fn.r_i1 = r.part_i1;
        fn.n0 = n0; fn.n1 = n1;
        fn.matches0 = at<long long>(ws, o_m) + pd[i].off0;
        fn.scores0 = at<float>(ws, o_s) + pd[i].off0;
        fn.red_f = red + 3 * roff; roff += (size_t)n0;
        fn.red_r = red + 3 * roff; roff += (size_t)n1;
    }
    HIPCHECK(hipMemcpyAsync(in + o_jobs, jobs.data(), sizeof(GuidedJob) * 2 * k, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(in + o_fins, fins.data(), sizeof(MatchFinal) * k, hipMemcpyHostToDevice, c->stream));
    launch_guided_top2(c->stream, at<const GuidedJob>(in, o_jobs), 2 * k, max_n, splits);
    launch_guided_finalize(c->stream, at<const MatchFinal>(in, o_fins), k, max_n, splits, conf->do_mutual_check, conf->ratio_threshold,
                           conf->distance_threshold);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(matches0, ws + o_m, 8 * (size_t)N0, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(scores0, ws + o_s, 4 * (size_t)N0, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return 0;
}
