// libsfd2hip: workspace, per-layer kernel dispatch and the network passes (ResSegNetV2.det up to the head outputs).
#include "sfd2_ctx.h"

// ------------------------------------------------------------------------------------------ workspace
static int down2(int n) { return (n - 1) / 2 + 1; }  // 3x3 stride 2 pad 1

// which throughput kernel takes a layer of SFD2_PREC_F16X3 from hi / lo' planes: conv3x3_rf for small outputs and stride 2 (conv2b, convPa.0 / convPa.3
// at 1600x1200, every 256-channel layer of a 640x480 image -- as in f16), conv3x3_pp for the other 3x3 stride-1 layers, none (the generic kernel) otherwise
static X3Kind x3_fast_kind(const PassPlan &p, const ConvW &L, bool has_res, int Ho, int Wo)
{
    if (!p.x3_pp || has_res || L.ks != 3 || L.cin % 64 != 0) return XK_GENERIC;
    if ((L.cout_pad == 256 || (L.cout_pad == 128 && L.stride == 2)) && conv3x3_rf_serves(3, L.stride, L.cout_pad, L.cin, Ho, Wo)) return XK_RF;
    return (L.stride == 1 && L.cout_pad % 128 == 0) ? XK_PP : XK_GENERIC;
}
// the resolution level (0: H x W ... 3: 1/8) of a strict layer's input; its output: one further with stride 2
static const int sl_level[] = {0 /* conv1b */, 1, 1 /* conv2a, conv2b */, 2, 2, 2, 2, 2, 2, 2, 2, 2 /* ... convPa.0 */, 3, 3 /* convPa.3, convPb */, 2, 2, 2};
static_assert(sizeof(sl_level) == SL_COUNT * sizeof(int), "one level per StrictLayer");
static bool on_planes(const StrictConv &s) { return s.kind == XK_PP || s.kind == XK_RF || s.kind == XK_S2D; }

// Largest part of the 1/4-resolution map (16 pixels per key point of the capacity) at which convDa.0 runs on the key points' blocks instead of densely.
// The sparse kernel's time goes by rounds of one 8-key-point tile per CU, the dense layer's by the map.  Measured at 1600x1200 / top-4096 (0.55 of
// the map): 75.0 us against conv3x3_pp's 121.3 (profiles/sparse_da0_ab.txt), i.e. 37.5 us per round against ~1.0 ns per pixel -- the two meet at 0.88
// of the map with two full rounds and at 0.44 with 1 024 key points (half a round's CUs idle).  0.6 sits between; DESIGN.md section 6.2.
#define SFD2_DA0_FRAC 0.6
// The one place that combines the options for a network pass (sfd2_ctx.h, PassPlan).  top_k and desc: sfd2_extract's arguments.
PassPlan plan_pass(const sfd2_ctx *c, PassEntry entry, int H, int W, int top_k, bool desc)
{
    PassPlan p;
    const int H2 = down2(H), W2 = down2(W), H4 = down2(H2), W4 = down2(W2);
    const bool det = entry == PASS_DET, x3 = c->precision == SFD2_PREC_F16X3;
    p.f32 = x3 || c->precision == SFD2_PREC_F32;
    p.comp = c->precision == SFD2_PREC_F16C;
    p.fuse = !p.f32 && (det ? c->fuse_det : c->fuse);   // det keeps every intermediate readable unless "fuse_det" is set
    p.alias = p.fuse && !det && c->opt_alias;
    p.generic_c = p.comp && c->opt_generic_c;
    p.no_rf_c = c->opt_no_rf_c;
    p.fp6_filters = c->opt_fp6_filters;
    p.fused_stem = p.fuse && !p.generic_c;
    p.comp_rb = p.comp && c->opt_comp_rb;
    bool wrm = true, wk = true;
    for (int b = 0; b < 3; ++b) {
        wrm = wrm && c->rb1[b].wrm.p && c->rb3[b].wrm.p;
        wk = wk && c->rb1[b].wfl.p && c->rb3[b].wfl.p && c->rb2[b].wlk.p;
    }
    // a ResBlock in plain fp16 (nets/sfd2.py:25-55): the fused kernel wherever the fused path runs (SFD2_FUSED_RB=0 in experiment builds: three kernels
    // per block, through t1 / t2 buffers that ensure_workspace then allocates)
    const char *frb = sfd2_env("SFD2_FUSED_RB");
    p.rb_fused = p.fuse && !p.comp_rb && !(frb && frb[0] == '0') && wrm;
    p.rb_inner = (p.comp_rb && !p.generic_c && wk) ? c->opt_rb_inner : 0;
    p.rb23 = p.rb_inner >= 2 && c->opt_fuse_rb23;
    if (p.comp) {
        // Option "fp6_acts": three tensors have conv3x3_pp<comp> as their only reader -- conv1b's output (-> conv2a), conv2b's (-> conv3a) and
        // conv3a's (-> conv3b).  Their corr records leave the producer as block-scaled fp6 half-records, and the consumer's correction is one
        // fp6 x fp6 scaled MFMA per unit: 33.5 cycles where a unit with fp8 on either side takes 66 (profiles/r04_mfma_probe.txt).  Decided
        // per tensor: the producer must be the kernel that can write them (the fused stem, conv3x3_rf<2,comp>, conv3x3_pp<comp>).
        const bool a6 = c->opt_fp6_acts && !p.generic_c && c->c2a.wc66.p && c->c3a.wc66.p && c->c3b.wc66.p;
        const bool s6 = a6 && p.fuse && c->w1b_stem_c6.p;
        const bool b6 = a6 && !p.no_rf_c && conv3x3_rf_c_serves(3, 2, c->c2b.cout_pad, c->c2b.cin, H4, W4);
        // Option "s2d" (throughput path only: the tensor is not readable by sfd2_debug_activation in that layout): conv2a stores its output as
        // four parity planes at quarter resolution, conv2b reads them as a stride-1 layer (conv2b_s2d_kernel.hip)
        p.a2a_s2d = c->opt_s2d && p.alias && s6 && !p.no_rf_c && conv2b_s2d_serves(H2, W2, c->c2b.cin, c->c2b.cout_pad) && H4 * 2 == H2 && W4 * 2 == W2;
        // Option "c3b_plain" (the load-time self-check decides, api_weights.hip): conv3b takes the hi plane of conv3a's output only; conv3a keeps writing
        // its records unless SFD2_C3A_KEEP_CORR says otherwise (experiment switch until measured)
        static const bool c3a_plain_out = sfd2_env("SFD2_C3A_KEEP_CORR") == nullptr;
        const bool p3b = c->opt_c3b_plain && a6 && b6 && !p.generic_c;
        const bool p3a = p3b && c3a_plain_out;
        // Option "trunk_r1": the three tensors the ResBlocks read as block input (conv3b's output, the outputs of blocks 0 and 1) with the residual
        // byte only -- their readers are conv1x1_c256_c<.., 2, ..> (value bytes rebuilt from the hi plane) and rb23_c_kernel's skip path
        const bool tr1 = c->opt_trunk_r1 && a6 && p.rb23 && c->rb1[0].wfr.p && c->rb3[0].wf8l.p;
        // option "comp_heads": the four 3x3 layers of the head branches compensated as well (their inputs then need corr planes: the
        // backbone output has one when the ResBlocks are compensated); convPb / convDb / ConvSta read hi planes either way
        // option "comp_det": the detector branch only (convPa.0, convPa.3) -- its score goes through exp(), which is what moves key points
        p.ch = p.comp_rb && c->opt_comp_heads;
        p.chp = p.ch || (p.comp_rb && c->opt_comp_det);
        // The records every stored tensor leaves its producer with, and its readers take (but conv3b with "c3b_plain": a3a_in).  "rb_inner": t1 (2) and
        // t2 (1, 2) plain fp16; "comp_rb" = 0: the ResBlocks' tensors all plain fp16.  The last block's output keeps its units for compensated heads.
        p.rec[T_CONV1A] = Rec::Unit8;
        p.rec[T_CONV1B] = s6 ? Rec::Half6 : Rec::Unit8;
        p.rec[T_CONV2A] = Rec::Unit8;
        p.rec[T_CONV2B] = b6 ? Rec::Half6 : Rec::Unit8;
        p.rec[T_CONV3A] = p3a ? Rec::None : a6 ? Rec::Half6 : Rec::Unit8;
        p.a3a_in = p3b ? Rec::None : p.rec[T_CONV3A];
        p.rec[T_CONV3B] = tr1 ? Rec::Resid8 : Rec::Unit8;
        for (int b = 0; b < 3 && p.comp_rb; ++b) {
            p.rec[T_T1_0 + b] = p.rb_inner >= 2 ? Rec::None : Rec::Unit8;
            p.rec[T_T2_0 + b] = p.rb_inner >= 1 ? Rec::None : Rec::Unit8;
            p.rec[T_OUT_0 + b] = (tr1 && (b < 2 || !p.chp)) ? Rec::Resid8 : Rec::Unit8;
        }
        p.rec[T_PA0] = p.chp ? Rec::Unit8 : Rec::None;
        p.rec[T_DA0] = p.ch ? Rec::Unit8 : Rec::None;
    }
    p.branches = c->opt_branches;
    if (entry == PASS_EXTRACT) {
        // H, W multiples of 8 (every BASELINE geometry): the score map needs no resize, so the detector soft-max and the
        // stability weighting run as ONE kernel that writes the heat map directly; the score map is never materialised
        p.skip_head = c->opt_fuse_post && H % 8 == 0 && W % 8 == 0;
        p.skip_pb = p.skip_head && c->opt_fuse_pb && p.fuse && !p.branches && c->pb.cout_pad >= 96;
        // Sparse descriptor head: convDb is 1x1 and only the bilinear corners of the selected key points are sampled, so on the
        // throughput path it runs after the selection, on 4 x K gathered pixels instead of the whole 1/4-resolution map (the
        // 61 MB fp32 descriptor map is never written; bit-identical descriptors).  Dense when more than a quarter of the map
        // would be gathered (top_k <= 0: every candidate).
        const bool few = desc && top_k > 0 && (size_t)16 * top_k <= (size_t)H4 * W4;
        p.sparse_desc = c->opt_sparse_desc && p.fuse && few;
        // ... and convDa.3 (3x3) is needed at those corners only as well: 4 x K pixels instead of the whole map (sparse_da3_kernel).
        // Not with compensated head branches (option "comp_heads": convDa.0's output then has a corr plane this kernel does not read).
        p.sparse_da3 = p.sparse_desc && c->opt_sparse_da3 && !p.ch && !p.branches;
        // SFD2_PREC_F16X3: the same two steps in that mode's arithmetic (planes of convDa.0's output, three MFMA passes, fp32 results)
        p.sparse_x3 = x3 && c->opt_sparse_desc && c->opt_sparse_da3 && c->opt_x3_pp && few;
        // ... and convDa.0 in front of it at the 4 x 4 blocks sparse_da3_kernel reads: 16 x K pixels (sparse_da0_kernel), bit-identical there.  Plain
        // descriptor branch of the fp16 family only (sparse_da3 implies it).  Option "sparse_da0" = 1: when at most SFD2_DA0_FRAC of the map is
        // computed; 2: at every size.  A 640x480 image with 4 096 key points stays dense.
        p.sparse_da0 = p.sparse_da3 && c->opt_sparse_da0 && c->da0.w.p && c->da0.ks == 3 && c->da0.stride == 1 &&
                       sparse_da0_serves(c->da0.cin, c->da0.cout_pad, H4, W4) &&
                       (c->opt_sparse_da0 >= 2 || (double)16 * top_k <= SFD2_DA0_FRAC * (double)H4 * W4);
        p.skip_db = p.sparse_desc;
        p.skip_da3 = p.sparse_da3 || p.sparse_x3;
    }
    // ConvSta before the head branches when convPb is fused into the post-processing (convDa.3 then takes the backbone output's slot); option
    // "sta_side": on the side stream (not with "branches": that option owns the side stream)
    p.sta_early = p.alias && p.skip_pb;
    p.sta_side = c->has_sta && p.sta_early && c->opt_sta_side && !p.branches;
    if (p.alias) {
        // Activation placement.  det (the parity entry point) keeps every activation in its own buffer for
        // sfd2_debug_activation.  The throughput path packs the whole chain into three 61 MB slots of one
        // arena (at 1600x1200), reusing a slot as soon as its tensor is dead, so the working set fits the 256 MB
        // Infinity Cache and a layer mostly reads what the previous one just wrote (measured: ResBlocks 400 -> 344 us;
        // four slots measure the same as three).  A ResBlock's output overwrites its own t1 (dead once conv3 starts), the
        // next block's t1 takes the slot of the previous input.
        static const int slots[T_COUNT] = {-1 /* conv1a: its own buffer */, 0, 1 /* spans slots 1-2 */, 0, 1, 2, 0, 2, 0 /* t1; x = slot 2, 0, 2 */, 1, 1, 1 /* t2 */,
                                           0, 2, 0 /* -> final x = slot 0 */, 1, 2 /* convDa.0 */, 1 /* convPa.3: behind convPa.0 */, 1 /* convDa.3 runs after convPb has consumed slot 1 */};
        for (int id = 0; id < T_COUNT; ++id) p.at[id].slot = slots[id];
        p.n_slots = p.branches ? 4 : 3;
        if (p.rb23) {
            // rb23_c_kernel reads t1 (with the halo rows of neighbouring tiles) while other tiles already write the block's
            // output: the output cannot take t1's slot.  No t2 in HBM on this path, so three slots still do.
            p.at[T_T1_0 + 1].slot = 0; p.at[T_T1_0 + 2].slot = 1;    // x = slot 2, 1, 2
            p.at[T_OUT_0].slot = 1; p.at[T_OUT_0 + 2].slot = 0;      // -> final x = slot 0
        }
        if (p.branches) p.at[T_DA].slot = 3;   // the two head branches run concurrently: no slot is shared between them
        // convPb fused into the detector-head kernel: convPa.3's output must outlive the network pass, so convDa.3
        // writes over the backbone output instead (slot 0) -- ConvSta, its last reader, then runs before the heads
        if (p.skip_pb) p.at[T_DA].slot = 0;
        const size_t P2 = (size_t)H2 * W2, P4 = (size_t)H4 * W4, P8 = (size_t)down2(H4) * down2(W4);
        size_t S = std::max(P2 * 64 * 2, P4 * 256 * 2);
        S = std::max(S, (P2 * 128 * 2 + 1) / 2);
        S = std::max(S, 2 * (P8 * 256 * 2 + 256));
        if (p.comp) S *= 2;   // hi plane + corr plane per tensor (the corr plane follows the hi plane inside the slot)
        p.slot_bytes = (S + 255) & ~(size_t)255;
        p.at[T_PA].off = (P8 * 256 * 2 * (p.comp ? 2 : 1) + 255) & ~(size_t)255;   // behind convPa.0's output (its corr plane too with "comp_heads")
    }
    p.x3_pp = x3 && c->opt_x3_pp;
    p.x3_fast = p.x3_pp && !det;     // (the parity entry point: every tensor as fp32 for sfd2_debug_activation)
    if (!p.f32) return p;
    const int Hl[4] = {H, H2, H4, down2(H4)}, Wl[4] = {W, W2, W4, down2(W4)};
    for (int i = 0; i < SL_COUNT; ++i) {
        const ConvW &L = strict_layer(c, i);
        const int lo = sl_level[i] + (L.stride == 2);
        p.sl[i].kind = x3_fast_kind(p, L, i >= SL_RB3 && i < SL_RB3 + 3 /* + skip connection */, Hl[lo], Wl[lo]);
    }
    if (p.skip_da3) p.sl[SL_DA3].kind = p.sl[SL_DB].kind = XK_SKIP;   // (sfd2_extract runs them on the sampled corners)
    if (!p.x3_fast) return p;        // every three-pass layer splits its fp32 input into the scratch planes and writes fp32
    p.x3_stem = c->w1b_stem_x3.p && c->c1a.wc.p;
    p.x3_rb = c->rb1[0].wfh.p && c->rb1[0].wfl.p && c->rb2[0].w.p && c->rb2[0].wlk.p;
    // Option "x3_desc16" (on the backbone output's planes, which the ResBlocks on planes leave behind)
    p.desc16 = p.skip_da3 && c->opt_x3_desc16 && p.x3_rb && c->da0.w.p && c->da0.scale_rawin.p && c->da3.w.p && c->db.w.p;
    if (p.x3_stem) p.sl[SL_C1B].kind = XK_SKIP;
    for (int i = SL_RB1; i < SL_RB3 + 3 && p.x3_rb; ++i) p.sl[i].kind = XK_SKIP;
    if (p.desc16) p.sl[SL_DA0].kind = XK_SKIP;
    // Option "s2d" in this mode too (round 5): conv2a (conv3x3_pp<x3>) stores its planes space-to-depth and conv2b runs as a stride-1 layer over
    // them (conv2b_s2d_kernel<x3>) instead of on the strided conv3x3_rf<2, x3>; planes out for conv3a
    if (c->opt_s2d && on_planes(p.sl[SL_C2B]) && on_planes(p.sl[SL_C3A]) && p.sl[SL_C2A].kind == XK_PP &&
        conv2b_s2d_serves(H2, W2, c->f2b.cin, c->f2b.cout_pad) && H4 * 2 == H2 && W4 * 2 == W2) {
        p.sl[SL_C2A].s2d_out = true, p.sl[SL_C2B].kind = XK_S2D;
    }
    // Plane hand-offs: a three-pass layer whose only reader takes planes writes planes and no fp32 tensor (conv2a -> conv2b -> conv3a -> conv3b ->
    // ResBlocks, convPa.0 -> convPa.3, convDa.0 -> the sparse descriptor head).  `have`: where the tensor in front of the layer at hand lives.
    // route(layer, its reader takes planes, where): where = X3_CHAIN_A stands for "the chain": buffer B when the input sits in A, A otherwise
    X3Out have = p.x3_stem ? X3_CHAIN_A : X3_F32;
    auto route = [&](int i, bool planes_out, X3Out where = X3_CHAIN_A) {
        StrictConv &s = p.sl[i];
        s.planes_in = on_planes(s) && have != X3_F32;
        if (on_planes(s) && planes_out) s.out = (where == X3_CHAIN_A && s.planes_in && have == X3_CHAIN_A) ? X3_CHAIN_B : where;
        have = s.out;
    };
    route(SL_C2A, on_planes(p.sl[SL_C2B]));
    route(SL_C2B, on_planes(p.sl[SL_C3A]));
    route(SL_C3A, on_planes(p.sl[SL_C3B]));
    route(SL_C3B, p.x3_rb, X3_RB);
    const X3Out backbone = p.x3_rb ? X3_RB : X3_F32;      // (the last ResBlock on planes writes its fp32 tensor as well: generic readers take that)
    have = backbone;
    route(SL_PA0, on_planes(p.sl[SL_PA3]));
    route(SL_PA3, false);
    have = backbone;
    if (!p.desc16) route(SL_DA0, p.skip_da3, X3_DA0);
    if (!p.skip_da3) route(SL_DA3, false);
    return p;
}

// Everything the pass about to run touches is allocated here, and nothing else: the throughput path gets the arena + head outputs, the layer-wise
// paths one buffer per activation, the strict family the fp32 set, the plane buffers its plan routes a layer through and the split filter forms its kernels
// read (ensure_strict_filters); run_network allocates nothing.  The activations are registered for sfd2_debug_activation as the plan will leave them.
int ensure_workspace(sfd2_ctx *c, const PassPlan &p, int H, int W)
{
    if (H < 8 || W < 8) return fail("image too small (need H, W >= 8)");
    if ((long long)H * W > (1ll << 30)) return fail("image too large");
    c->H = H; c->W = W;
    c->H2 = down2(H); c->W2 = down2(W);
    c->H4 = down2(c->H2); c->W4 = down2(c->W2);
    c->H8 = down2(c->H4); c->W8 = down2(c->W4);
    const size_t P1 = (size_t)H * W, P2 = (size_t)c->H2 * c->W2, P4 = (size_t)c->H4 * c->W4, P8 = (size_t)c->H8 * c->W8;
    const size_t Pl[4] = {P1, P2, P4, P8}, hb = sizeof(half_t);
    const bool layers = !p.f32 && !p.alias;      // private fp16 buffer per activation
    // not stored on the fp16 family's path at hand: conv1a's output inside the fused stem, t1 / t2 inside resblock_kernel
    auto on_chip = [&](int id) { return id == T_CONV1A ? p.fused_stem : (id >= T_T1_0 && id < T_OUT_0 && p.rb_fused); };
    for (int id = 0; id < T_COUNT; ++id) {
        const size_t n = Pl[kTensor[id].level] * kTensor[id].ch;
        // SFD2_PREC_F16C: a hi plane followed by its corr plane (same geometry; convPa.0's and convDa.0's for option "comp_heads"), none behind convPa.3's and convDa.3's outputs
        if (p.f32) HIPCHECK(c->act32[id].ensure(n * sizeof(float)));
        else if ((layers || id == T_CONV1A) && !on_chip(id)) HIPCHECK(c->act16[id].ensure(n * ((p.comp && id < T_PA) ? 2 * hb : hb)));
    }
    if (p.alias) HIPCHECK(c->arena.ensure(p.n_slots * p.slot_bytes));
    HIPCHECK(c->logits.ensure(P8 * 128 * sizeof(float)));
    HIPCHECK(c->draw.ensure(P4 * 128 * sizeof(float)));
    HIPCHECK(c->sta.ensure(P4 * 3 * sizeof(float)));
    HIPCHECK(c->score.ensure(P8 * 64 * sizeof(float)));
    HIPCHECK(c->heat.ensure(P1 * sizeof(float)));
    const size_t cap = cand_capacity(P1);
    c->cand_cap = (int)cap;
    HIPCHECK(c->cand.ensure(cap * 8));
    HIPCHECK(c->bnd.ensure(cap * 8));
    HIPCHECK(c->counters.ensure(SFD2_COUNTER_BYTES));
    for (ActInfo &a : c->acts) a.known = false;
    auto reg = [&](int id, const void *ptr, int is_f32, int planar, int pitch, Rec rec = Rec::None) -> ActInfo & {
        const TensorRow &t = kTensor[id];      // (the fp16 family stores its tensors times 2^act_exp, sfd2_ctx.h: sfd2_debug_activation divides it out)
        return c->acts[id] = ActInfo{true, ptr, is_f32, planar, t.ch, pitch, act_h(c, id), act_w(c, id), rec, (!is_f32 && t.group >= 0) ? c->act_exp[t.group] : 0};
    };
    reg(T_PB, c->logits.p, 1, 0, 128);
    reg(T_DB, c->draw.p, 1, 0, 128);
    reg(T_STA, c->sta.p, 1, 1, 0);
    if (p.f32) {
        // SFD2_PREC_F16X3 (none of this with "x3_pp" = 0): the scratch planes for the largest input split in front of its layer, each hand-off buffer for the largest output routed into it
        if (p.sparse_x3 && !p.desc16 && p.sl[SL_DA0].out != X3_DA0) return fail("f16x3: the sparse descriptor head needs convDa.0 on a three-pass kernel (planes out)");
        const size_t pb = 2 * hb;
        size_t scratch = 0, chain[2] = {p.x3_stem ? std::max(P2 * 64, P4 * 256) : 0, 0}, da0 = p.desc16 ? P4 * 256 : 0;
        for (int i = 0; i < SL_COUNT; ++i) {
            const StrictConv &s = p.sl[i];
            const ConvW &L = strict_layer(c, i);
            if (!on_planes(s)) continue;
            const size_t nout = Pl[sl_level[i] + (L.stride == 2)] * L.cout_pad;
            if (!s.planes_in) scratch = std::max(scratch, Pl[sl_level[i]] * L.cin);
            if (s.out == X3_CHAIN_A || s.out == X3_CHAIN_B) chain[s.out - X3_CHAIN_A] = std::max(chain[s.out - X3_CHAIN_A], nout);
            if (s.out == X3_DA0) da0 = nout;
        }
        HIPCHECK(c->x3_planes.ensure(scratch * pb));
        for (int k = 0; k < 2; ++k) HIPCHECK(c->x3_chain[k].ensure(chain[k] * pb));
        for (int k = 0; k < 3 && p.x3_rb; ++k) HIPCHECK(c->x3_rb_planes[k].ensure(P4 * 256 * pb));
        HIPCHECK(c->x3_da0_planes.ensure(da0 * pb));
        if (ensure_strict_filters(c, p)) return -1;
    } else if (!layers) {           // throughput path: intermediates live in aliased arena slots and are not readable
        // (convDa.0's map is a known tensor that the sparse form writes in part only: sfd2_debug_activation says "not materialised")
        if (p.sparse_da0) reg(T_DA0, act_view(c, p, T_DA0).p, 0, 0, kTensor[T_DA0].ch).absent = true;
        return 0;
    }
    for (int id = 0; id < T_COUNT; ++id) {
        // throughput path of SFD2_PREC_F16X3: from the stem to convDa.0 the tensors exist as hi / lo' planes only; the fp32 buffers are
        // written for the last ResBlock's output and convPa.3's.  sfd2_debug_activation must say so instead of handing back what an
        // earlier sfd2_det left in them
        if (p.f32) reg(id, c->act32[id].p, 1, 0, kTensor[id].ch).absent = p.x3_fast && id != T_OUT_0 + 2 && id != T_PA;
        // (SFD2_PREC_F16C: each tensor with the corr records the plan has its producer write; the head branches' tensors as their hi planes)
        else if (!on_chip(id)) reg(id, c->act16[id].p, 0, 0, kTensor[id].ch, id < T_PA0 ? p.rec[id] : Rec::None).absent = (p.rb23 && id >= T_T2_0 && id < T_OUT_0) || (p.sparse_da0 && id == T_DA0);   // (t2 stays on chip in rb23_c_kernel; convDa.0's map is written at the key points' blocks only)
    }
    return 0;
}

// one plain fp16 layer on buffers given by hand
static void conv_at(sfd2_ctx *c, const char *name, const ConvW &L, const DevPtr &in, int H, int W, const DevPtr &out,
                    int Ho, int Wo, int relu, const half_t *res = nullptr, int out_f32 = 0, const float *scale_override = nullptr)
{
    char kn[48];
    const float *scale = scale_override ? scale_override : L.scale.as<float>();
    const int bn = (L.cout_pad % 256 == 0) ? 256 : (L.cout_pad % 128 == 0 ? 128 : 64);
    snprintf(kn, sizeof(kn), "conv_igemm<%d,%d,%d%s>", L.ks, L.stride, bn, out_f32 ? ",f32" : "");
    if (!res && !out_f32 && conv3x3_pp_serves(L.ks, L.stride, L.cout_pad, L.cin)) snprintf(kn, sizeof(kn), "conv3x3_pp");
    if (!res && !out_f32 && conv3x3_rf_serves(L.ks, L.stride, L.cout_pad, L.cin, Ho, Wo)) snprintf(kn, sizeof(kn), "conv3x3_rf<%d>", L.stride);
    const double px = (double)Ho * Wo;
    const double flops = 2.0 * px * L.cout * L.cin * L.ks * L.ks;
    const double bytes = 2.0 * ((double)H * W * L.cin + (double)L.cout * L.cin * L.ks * L.ks) +
                         px * L.cout_pad * (out_f32 ? 4.0 : 2.0) + (res ? px * L.cout_pad * 2.0 : 0.0);
    static const bool no_c1 = sfd2_env("SFD2_NO_CONV1X1") != nullptr;
    if (L.wrm.p && !out_f32 && !no_c1) {
        snprintf(kn, sizeof(kn), "conv1x1_c256%s", res ? "+res" : "");
        ProfScope ps(c, name, kn, flops, bytes);
        launch_conv1x1_c256(c->cur_stream, in.as<half_t>(), Ho * Wo, L.wrm.as<half_t>(), scale, L.shift.as<float>(),
                            relu, res, reinterpret_cast<half_t *>(out.p), c->zero_page.as<half_t>());
        return;
    }
    ProfScope ps(c, name, kn, flops, bytes);
    launch_conv_igemm(c->cur_stream, in.as<half_t>(), H, W, L.cin, L.w.as<half_t>(), scale,
                      L.shift.as<float>(), L.cout_pad, L.ks, L.stride, relu, res, out.p, out_f32, Ho, Wo,
                      c->zero_page.as<half_t>());
}
// ... from tensor `in` to tensor `out` (+ the skip connection `res`): buffers and geometry by id (act_view, kTensor)
static void conv(sfd2_ctx *c, const PassPlan &p, const char *name, const ConvW &L, int in, int out, int relu, int res = T_NONE, int out_f32 = 0)
{
    conv_at(c, name, L, act_view(c, p, in), act_h(c, in), act_w(c, in), act_view(c, p, out), act_h(c, out), act_w(c, out), relu,
            res != T_NONE ? act_view(c, p, res).as<half_t>() : nullptr, out_f32);
}

// the range-status slot of a stored tensor of the compensated mode (sfd2_internal.h), null when nothing is recorded
static unsigned int *range_slot(sfd2_ctx *c, int id)
{
    return (id >= 0 && c->range_stat.p) ? c->range_stat.as<unsigned int>() + id * SFD2_RANGE_SUB : nullptr;
}
static half_t *corr_of(const DevPtr &b, size_t px, int pitch) { return b.as<half_t>() + px * (size_t)pitch; }
// conv3x3_pp<comp>'s filters for the records of a layer's input and output: the fp6 x fp6 strings over Half6 input records, the fp8 x fp6
// ones for a Half6 output or (option "fp6_filters") between Unit8 records, the fp8 units otherwise.  shift: [shift | scale bytes] with fp6.
struct PPFilters { const half_t *w; const float *shift; bool fp6; };
static PPFilters pp_filters(const PassPlan &p, const ConvW &L, Rec in, Rec out)
{
    if (in == Rec::Half6) return {L.wc66.as<half_t>(), L.sa66.as<float>(), true};
    if (in == Rec::Unit8 && (out == Rec::Half6 || (out == Rec::Unit8 && p.fp6_filters && L.wc6.p && L.sa6.p))) return {L.wc6.as<half_t>(), L.sa6.as<float>(), true};
    return {L.wc.as<half_t>(), L.shift.as<float>(), false};
}
// SFD2_PREC_F16C: one compensated layer from tensor `in` to tensor `out` (+ the skip connection `res_id`).  A compensated tensor = hi plane followed by its
// corr plane; the plan says in which format each carries its records (a plain-fp16 consumer just reads the hi plane, Rec::None); rin: conv3b's override
static void convc(sfd2_ctx *c, const PassPlan &p, const char *name, const ConvW &L, int in_id, int out_id, int relu, int res_id = T_NONE,
                  bool s2d_out = false /* option "s2d": the output stored space-to-depth */, const Rec *rin_override = nullptr)
{
    const DevPtr in = act_view(c, p, in_id), out = act_view(c, p, out_id), resv = res_id != T_NONE ? act_view(c, p, res_id) : DevPtr{}, *res = res_id != T_NONE ? &resv : nullptr;
    const int H = act_h(c, in_id), W = act_w(c, in_id), Ho = act_h(c, out_id), Wo = act_w(c, out_id);
    const Rec rin = rin_override ? *rin_override : p.rec[in_id], rout = p.rec[out_id];
    unsigned int *rs = range_slot(c, out_id < SFD2_RS_COUNT ? out_id : -1);
    char kn[48];
    const double px = (double)Ho * Wo;
    const double flops = 2.0 * px * L.cout * L.cin * L.ks * L.ks;
    const double bytes = (rin != Rec::None ? 4.0 : 2.0) * ((double)H * W * L.cin + (double)L.cout * L.cin * L.ks * L.ks) +
                         px * L.cout_pad * (rout != Rec::None ? 4.0 : 2.0) + (res ? px * L.cout_pad * 4.0 : 0.0);
    const half_t *in_c = rin != Rec::None ? corr_of(in, (size_t)H * W, L.cin) : nullptr;
    half_t *out_c = rout != Rec::None ? corr_of(out, (size_t)Ho * Wo, L.cout_pad) : nullptr;
    // conv3x3_pp's tile is 128 channels wide: in its compensated form it also takes conv2a (64 -> 128 channels, four chunks)
    const bool pp = !res && !p.generic_c && L.ks == 3 && L.stride == 1 && L.cout_pad % 128 == 0 && L.cin % 64 == 0;
    if (pp) {
        ProfScope ps(c, name, (in_c && out_c) ? "conv3x3_pp<comp>" : (in_c ? "conv3x3_pp<comp,plain out>" : "conv3x3_pp<comp out>"), flops, bytes);
        const PPFilters f = pp_filters(p, L, rin, rout);
        if (f.w && launch_conv3x3_pp_c(c->cur_stream, in.as<half_t>(), in_c, H, W, L.cin, f.w, L.scale.as<float>(), f.shift, L.cout_pad, relu,
                                       out.as<half_t>(), out_c, Ho, Wo, c->zero_page.as<half_t>(), L.sbyte, rs, rin, rout, s2d_out, f.fp6))
            return;
        ps.cancel();
    } else if (!p.generic_c && !p.no_rf_c && in_c && out_c && !res && L.ks == 3 && L.stride == 2 && L.cout_pad == 128) {   // conv2b
        ProfScope ps(c, name, "conv3x3_rf<2,comp>", flops, bytes);
        if (launch_conv3x3_rf_c(c->cur_stream, in.as<half_t>(), in_c, H, W, L.cin, L.wc.as<half_t>(), L.scale.as<float>(), L.shift.as<float>(),
                                L.cout_pad, L.stride, relu, out.as<half_t>(), out_c, Ho, Wo, c->zero_page.as<half_t>(), L.sbyte, rs, rin, rout))
            return;
        ps.cancel();     // no instantiation for this geometry: the next candidate takes the layer (and the profile row)
    }
    // (the kernels below read and write Unit8 records only)
    const bool unit8 = (rin == Rec::None || rin == Rec::Unit8) && (rout == Rec::None || rout == Rec::Unit8) && !s2d_out;
    if (pp || !unit8) {
        c->net_error = 1;
        (void)fail(std::string(name) + ": no kernel instantiation for the corr-record formats the pass plan asks for");
        return;
    }
    if (!p.generic_c && in_c && out_c && L.wfh.p && L.wfc.p) {   // the ResBlocks' 1x1 layers: persistent streaming kernel
        snprintf(kn, sizeof(kn), "conv1x1_c256<comp>%s", res ? "+res" : "");
        ProfScope ps(c, name, kn, flops, bytes);
        launch_conv1x1_c256_c(c->cur_stream, in.as<half_t>(), in_c, Ho * Wo, L.wfh.as<half_t>(), L.wfc.as<half_t>(), L.scale.as<float>(),
                              L.shift.as<float>(), relu, res ? res->as<half_t>() : nullptr,
                              res ? corr_of(*res, (size_t)Ho * Wo, L.cout_pad) : nullptr, out.as<half_t>(), out_c,
                              c->zero_page.as<half_t>(), L.sbyte, rs, rin, rout);
        return;
    }
    if (!p.generic_c && in_c && out_c && L.cout_pad % 128 == 0 && ((L.ks == 1 && L.stride == 1) || (L.ks == 3 && L.stride == 2 && !res))) {
        snprintf(kn, sizeof(kn), "conv_igemm2<%d,%d,comp>%s", L.ks, L.stride, res ? "+res" : "");
        ProfScope ps(c, name, kn, flops, bytes);
        if (!launch_conv_igemm2_c(c->cur_stream, in.as<half_t>(), in_c, H, W, L.cin, L.wc.as<half_t>(), L.scale.as<float>(),
                                 L.shift.as<float>(), L.cout_pad, L.ks, L.stride, relu, res ? res->as<half_t>() : nullptr,
                                 res ? corr_of(*res, (size_t)Ho * Wo, L.cout_pad) : nullptr, out.as<half_t>(), out_c, Ho, Wo,
                                 c->zero_page.as<half_t>(), L.sbyte, rs))
            ps.cancel();
        else
            return;
    }
    snprintf(kn, sizeof(kn), "convc_igemm<%d,%d>", L.ks, L.stride);
    ProfScope ps(c, name, kn, flops, bytes);
    launch_convc_igemm(c->cur_stream, in.as<half_t>(), in_c, H, W, L.cin, L.wc.as<half_t>(), L.scale.as<float>(), L.shift.as<float>(), L.cout_pad,
                       L.ks, L.stride, relu, res ? res->as<half_t>() : nullptr, res ? corr_of(*res, (size_t)Ho * Wo, L.cout_pad) : nullptr,
                       out.as<half_t>(), out_c, Ho, Wo, L.sbyte, rs);
}

static X3Pair planes_of(const DevBuf &b, size_t n) { return {b.as<half_t>(), b.as<half_t>() + n}; }
static const DevBuf &plane_buf(const sfd2_ctx *c, X3Out o) { return o == X3_CHAIN_A ? c->x3_chain[0] : o == X3_CHAIN_B ? c->x3_chain[1] : o == X3_RB ? c->x3_rb_planes[0] : c->x3_da0_planes; }

int convf_at(sfd2_ctx *c, const StrictConv &s, const char *name, const ConvW &L, const DevPtr &in, int H, int W, const DevPtr &out,
             int Ho, int Wo, int relu, const float *res, X3Pair *planes)
{
    char kn[64];
    const bool x3 = c->precision == SFD2_PREC_F16X3;
    if (s.kind == XK_SKIP) return fail(std::string(name) + ": the pass plan does not run this layer");
    if (s.kind != XK_GENERIC) {
        // The 3x3 layers (half of this mode's time) on the throughput kernels: the input is split ONCE into hi / lo' planes (the generic kernel
        // splits every staged piece, per tile and chunk) unless its producer left them behind, the kernel stages the planes by direct copies and runs
        // its fp16 K loop three times (hi x hi, hi x lo', lo' x hi) into one accumulator; fp32 out, or planes where the only reader takes planes.
        const size_t nin = (size_t)H * W * L.cin, nout = (size_t)Ho * Wo * L.cout_pad;
        const bool pre = s.planes_in;
        const X3Pair pi = pre ? *planes : planes_of(c->x3_planes, nin);
        const X3Pair po = s.out == X3_F32 ? X3Pair{} : planes_of(plane_buf(c, s.out), nout);
        const half_t *wp = L.wx3p.as<half_t>();
        if (planes) *planes = po;
        if (s.kind == XK_S2D) {
            ProfScope ps(c, name, "conv2b_s2d_kernel<x3>", 2.0 * (double)Ho * Wo * L.cout * L.cin * 9, 4.0 * nin + 4.0 * nout);
            launch_conv2b_s2d_x3(c->stream, pi.hi, pi.lo, Ho, Wo, wp, L.scale.as<float>(), L.shift.as<float>(), relu, po.hi, po.lo, c->zero_page.as<half_t>());
            return 0;
        }
        snprintf(kn, sizeof(kn), "%sconv3x3_%s<x3%s>", pre ? "" : "x3_split_planes + ", s.kind == XK_RF ? "rf" : "pp", po.hi ? ", planes out" : "");
        ProfScope ps(c, name, kn, 2.0 * (double)Ho * Wo * L.cout * L.cin * 9, (pre ? 4.0 : 12.0) * nin + 4.0 * nout);
        if (!pre) launch_x3_split_planes(c->stream, in.as<float>(), nin, pi.hi, pi.lo);
        if (s.kind == XK_RF && launch_conv3x3_rf_x3(c->stream, pi.hi, pi.lo, H, W, L.cin, wp, L.scale.as<float>(), L.shift.as<float>(), L.cout_pad,
                                                    L.stride, relu, po.hi, po.lo, po.hi ? nullptr : out.as<float>(), Ho, Wo, c->zero_page.as<half_t>()))
            return 0;
        if (L.stride != 1) { ps.cancel(); return fail("conv3x3_rf<x3>: no instantiation for this layer (x3_fast_kind and the launcher disagree)"); }
        launch_conv3x3_pp_x3(c->stream, pi.hi, pi.lo, H, W, L.cin, wp, L.scale.as<float>(), L.shift.as<float>(), L.cout_pad, relu,
                             po.hi, po.lo, po.hi ? nullptr : out.as<float>(), Ho, Wo, c->zero_page.as<half_t>(), (po.hi && s.s2d_out) ? 1 : 0);
        return 0;
    }
    if (planes) *planes = X3Pair{};
    // (SFD2_PREC_F16X3: the packed filters split once, ConvW::wx3 -- the kernel then stages them without arithmetic)
    snprintf(kn, sizeof(kn), "conv_igemm_%s<%d,%d,%d>", x3 ? "x3" : "f32", L.ks, L.stride, (L.cout_pad % 128 == 0) ? 128 : 64);
    const double px = (double)Ho * Wo;
    ProfScope ps(c, name, kn, 2.0 * px * L.cout * L.cin * L.ks * L.ks,
                 4.0 * ((double)H * W * L.cin + (double)L.cout * L.cin * L.ks * L.ks + px * L.cout_pad * (res ? 2 : 1)));
    (x3 ? launch_conv_igemm_x3 : launch_conv_igemm_f32)(c->stream, in.as<float>(), H, W, L.cin, x3 ? L.wx3.as<float>() : L.w.as<float>(), L.scale.as<float>(),
                          L.shift.as<float>(), L.cout_pad, L.ks, L.stride, relu, res, out.as<float>(), Ho, Wo);
    return 0;
}

// strict layer `sl` from tensor `in` to tensor `out` (+ the skip connection `res`)
static int convf(sfd2_ctx *c, const PassPlan &p, int sl, const char *name, int in, int out, int relu, int res = T_NONE, X3Pair *planes = nullptr)
{
    return convf_at(c, p.sl[sl], name, strict_layer(c, sl), act_view(c, p, in), act_h(c, in), act_w(c, in), act_view(c, p, out), act_h(c, out), act_w(c, out), relu,
                    res != T_NONE ? act_view(c, p, res).as<float>() : nullptr, planes);
}

// strict mode: identical layer sequence on fp32 activations (conv_f32_kernels.hip)
static int run_network_f32(sfd2_ctx *c, const PassPlan &p, const float *img_dev, int normalise)
{
    hipStream_t st = c->stream;
    const int H = c->H, W = c->W, H2 = c->H2, W2 = c->W2, H4 = c->H4, W4 = c->W4, H8 = c->H8, W8 = c->W8;
    const double P1 = (double)H * W, P4 = (double)H4 * W4, P8 = (double)H8 * W8;
    X3Pair pl;      // the planes of the tensor in front of the next layer, where its producer left them (plan_pass)
    if (p.x3_stem) {
        // throughput path of SFD2_PREC_F16X3: the fused stem in three-pass arithmetic (conv1a's image and filters as hi + lo fp16 as
        // in the compensated mode, conv1b on hi / lo' planes of conv1a's tile in LDS), its output as planes for conv2a
        pl = planes_of(c->x3_chain[0], (size_t)H2 * W2 * 64);
        ProfScope ps(c, "conv1a+conv1b", "fused_stem_c_kernel<x3>", 2.0 * P1 * 64 * 27 + 2.0 * (double)H2 * W2 * 64 * 576, P1 * 12 + (double)H2 * W2 * 256);
        launch_fused_stem_c(st, img_dev, H, W, normalise, c->c1a.wc.as<half_t>(), c->f1a.scale.as<float>(), c->f1a.shift.as<float>(),
                            c->w1b_stem_x3.p, c->f1b.scale.as<float>(), c->f1b.shift.as<float>(), pl.hi, pl.lo, H2, W2, -1);
    } else {
    {
        ProfScope ps(c, "conv1a", "conv1a_f32_kernel", 2.0 * P1 * 64 * 27, P1 * (12 + 256));
        launch_conv1a_f32(st, img_dev, H, W, normalise, c->f1a.w.as<float>(), c->f1a.scale.as<float>(),
                          c->f1a.shift.as<float>(), c->act32[T_CONV1A].as<float>());
    }
    if (convf(c, p, SL_C1B, "conv1b", T_CONV1A, T_CONV1B, 1)) return -1;
    }
    if (convf(c, p, SL_C2A, "conv2a", T_CONV1B, T_CONV2A, 1, T_NONE, &pl)) return -1;
    if (convf(c, p, SL_C2B, "conv2b", T_CONV2A, T_CONV2B, 1, T_NONE, &pl)) return -1;
    if (convf(c, p, SL_C3A, "conv3a", T_CONV2B, T_CONV3A, 1, T_NONE, &pl)) return -1;
    if (convf(c, p, SL_C3B, "conv3b", T_CONV3A, T_CONV3B, 1, T_NONE, &pl)) return -1;
    int x = T_CONV3B;      // the tensor in front of the next ResBlock / the heads
    if (p.x3_rb) {
        // ResBlocks of SFD2_PREC_F16X3 on the throughput path: every tensor of a block lives as hi / lo' planes (the input is split
        // once in front of the first block).  conv1 and conv3 on the streaming three-pass 1x1 kernel (filters = the fp16 set's
        // fragment-ordered hi / lo' arrays: the same split of the same fp32 weights), the grouped conv on gconv_c_kernel<X3>
        // (pre-split operands, direct plane stores); the skip connection is read from the planes (22 significant bits) and only the
        // last block also writes the fp32 tensor its generic readers (convPa.0, ConvSta) take.
        const size_t nin = (size_t)H4 * W4 * 256;
        half_t *xh = c->x3_rb_planes[0].as<half_t>(), *xl = xh + nin, *th = c->x3_rb_planes[1].as<half_t>(), *tl = th + nin;
        half_t *uh = c->x3_rb_planes[2].as<half_t>(), *ul = uh + nin;
        if (p.sl[SL_C3B].out != X3_RB) {      // conv3b on the generic kernel
            ProfScope ps(c, "conv3b planes", "x3_split_planes", 0.0, 12.0 * nin);
            launch_x3_split_planes(st, c->act32[x].as<float>(), nin, xh, xl);
        }
        for (int b = 0; b < 3; ++b) {
            {
                ProfScope ps(c, rb_layer_name(b, 1), "conv1x1_c256<x3>", 2.0 * P4 * 256.0 * 256.0, P4 * 256.0 * 8);
                launch_conv1x1_c256_x3(st, xh, xl, H4 * W4, c->rb1[b].wfh.as<half_t>(), c->rb1[b].wfl.as<half_t>(), c->frb1[b].scale.as<float>(),
                                       c->frb1[b].shift.as<float>(), 1, nullptr, nullptr, nullptr, th, tl, c->zero_page.as<half_t>());
            }
            {
                ProfScope ps(c, rb_layer_name(b, 2), "gconv_c_kernel<x3>", 2.0 * P4 * 256 * 72, P4 * 256 * 8);
                launch_gconv_c(st, th, tl, H4, W4, c->rb2[b].w.as<half_t>(), c->rb2[b].wlk.p, c->frb2[b].scale.as<float>(),
                               c->frb2[b].shift.as<float>(), uh, ul, -1, 0, H4);
            }
            {
                ProfScope ps(c, rb_layer_name(b, 3), "conv1x1_c256<x3>+res", 2.0 * P4 * 256.0 * 256.0, P4 * 256.0 * (b == 2 ? 16 : 12));
                launch_conv1x1_c256_x3(st, uh, ul, H4 * W4, c->rb3[b].wfh.as<half_t>(), c->rb3[b].wfl.as<half_t>(), c->frb3[b].scale.as<float>(),
                                       c->frb3[b].shift.as<float>(), 1, xh, xl, b == 2 ? c->act32[T_OUT_0 + b].as<float>() : nullptr, xh, xl,
                                       c->zero_page.as<half_t>());
            }
        }
        x = T_OUT_0 + 2;
        pl = {xh, xl};
    }
    for (int b = 0; b < (p.x3_rb ? 0 : 3); ++b) {
        float *t1 = c->act32[T_T1_0 + b].as<float>(), *t2 = c->act32[T_T2_0 + b].as<float>();
        if (convf(c, p, SL_RB1 + b, rb_layer_name(b, 1), x, T_T1_0 + b, 1)) return -1;
        {
            if (c->precision == SFD2_PREC_F16X3) {
                ProfScope ps(c, rb_layer_name(b, 2), "gconv_x3_kernel", 2.0 * P4 * 256 * 72, P4 * 256 * 8);
                launch_gconv_x3(st, t1, H4, W4, c->frb2[b].wx3.p, c->frb2[b].scale.as<float>(), c->frb2[b].shift.as<float>(), t2);
            } else {
                ProfScope ps(c, rb_layer_name(b, 2), "gconv_f32_kernel", 2.0 * P4 * 256 * 72, P4 * 256 * 8);
                launch_gconv_f32(st, t1, H4, W4, c->frb2[b].w.as<float>(), c->frb2[b].scale.as<float>(), c->frb2[b].shift.as<float>(), t2);
            }
        }
        if (convf(c, p, SL_RB3 + b, rb_layer_name(b, 3), T_T2_0 + b, T_OUT_0 + b, 1, x)) return -1;
        x = T_OUT_0 + b;
    }
    // (throughput path: both head branches read the backbone output's planes; convPa.0 leaves its own output as planes for convPa.3)
    const X3Pair backbone = pl;
    if (convf(c, p, SL_PA0, "convPa.0", x, T_PA0, 1, T_NONE, &pl)) return -1;
    if (convf(c, p, SL_PA3, "convPa.3", T_PA0, T_PA, 0, T_NONE, &pl)) return -1;
    if (convf(c, p, SL_PB, "convPb", T_PA, T_PB, 0)) return -1;
    pl = backbone;
    // Option "x3_desc16": the descriptor branch leaves this mode's arithmetic here -- convDa.0 as ONE fp16 pass (conv3x3_pp) over the backbone output's hi
    // plane, at the network's own scale (scale_rawin), its output (times 2^act_exp[AE_DA0], what convDa.3's folded constants expect) in the buffer
    // the planes would have taken (act_view); sfd2_extract then runs the fp16 sparse head on it.  The detector branch above is untouched.
    if (p.desc16) {
        DevPtr in;
        in.p = backbone.hi;
        conv_at(c, "convDa.0", c->da0, in, H4, W4, act_view(c, p, T_DA0), H4, W4, 1, nullptr, 0, c->da0.scale_rawin.as<float>());
    } else if (convf(c, p, SL_DA0, "convDa.0", x, T_DA0, 1, T_NONE, &pl)) return -1;
    if (!p.skip_da3) {      // (otherwise sfd2_extract's sparse descriptor head runs them on the sampled corners: on convDa.0's planes, or in fp16 with "x3_desc16")
        if (convf(c, p, SL_DA3, "convDa.3", T_DA0, T_DA, 0, T_NONE, &pl)) return -1;
        if (convf(c, p, SL_DB, "convDb", T_DA, T_DB, 0)) return -1;
    }
    if (c->has_sta) {
        ProfScope ps(c, "ConvSta", "convsta_f32_kernel", 2.0 * P4 * 3 * 256, P4 * (1024 + 12));
        launch_convsta_f32(st, c->act32[x].as<float>(), H4 * W4, c->sta_w.as<float>(), c->sta_b.as<float>(), c->sta.as<float>());
    }
    if (!p.skip_head) {
        ProfScope ps(c, "detector_head", "detector_head_kernel", 0.0, P8 * (65 * 4 + 256));
        launch_detector_head(st, c->logits.as<float>(), 128, H8, W8, c->score.as<float>());
    }
    HIPCHECK(hipGetLastError());
    return 0;
}

// ResSegNetV2.det up to the three head outputs (nets/sfd2.py:314-328, :340-345)
int run_network(sfd2_ctx *c, const PassPlan &p, const float *img_dev, int normalise)
{
    c->cur_stream = c->stream;
    g_sfd2_cu_limit = c->opt_cu_limit;
    if (p.f32) return run_network_f32(c, p, img_dev, normalise);
    const bool comp = p.comp, alias = p.alias;
    hipStream_t st = c->stream;
    const int H = c->H, W = c->W, H2 = c->H2, W2 = c->W2, H4 = c->H4, W4 = c->W4, H8 = c->H8, W8 = c->W8;
    const double P1 = (double)H * W, P4 = (double)H4 * W4, P8 = (double)H8 * W8;
    auto V = [&](int id) { return act_view(c, p, id); };      // where tensor `id` lives for this pass (plan_pass's placement)
    int x = T_CONV3B;      // the tensor in front of the next ResBlock / the heads
    // one ResBlock (nets/sfd2.py:25-55) in plain fp16
    auto rb_f16 = [&](int b) {
        const int t1 = T_T1_0 + b, t2 = T_T2_0 + b, ob = T_OUT_0 + b;
        if (p.rb_fused) {
            const int o = alias ? t1 : ob;   // the fused kernel must not write over its own input: with the arena the output takes t1's slot
            ProfScope ps(c, kTensor[ob].act, "resblock_kernel", 2.0 * P4 * 256 * (256 + 72 + 256), P4 * 256 * 4);
            launch_resblock(st, V(x).as<half_t>(), H4, W4, c->rb1[b].wrm.as<half_t>(), c->rb1[b].scale.as<float>(),
                            c->rb1[b].shift.as<float>(), c->rb2[b].wgc.as<half_t>(), c->rb2[b].scale.as<float>(),
                            c->rb2[b].shift.as<float>(), c->rb3[b].wrm.as<half_t>(), c->rb3[b].scale.as<float>(),
                            c->rb3[b].shift.as<float>(), V(o).as<half_t>(), c->zero_page.as<half_t>());
            x = o;
            return;
        }
        conv(c, p, rb_layer_name(b, 1), c->rb1[b], x, t1, 1);
        {
            ProfScope ps(c, rb_layer_name(b, 2), "gconv3x3_g8_kernel", 2.0 * P4 * 256 * 72, P4 * 256 * 4);
            launch_gconv3x3_g8(st, V(t1).as<half_t>(), H4, W4, c->rb2[b].w.as<half_t>(),
                               c->rb2[b].scale.as<float>(), c->rb2[b].shift.as<float>(), V(t2).as<half_t>());
        }
        conv(c, p, rb_layer_name(b, 3), c->rb3[b], t2, ob, 1, x);
        x = ob;
    };
    auto conv_sta = [&]() {
        ProfScope ps(c, "ConvSta", "convsta_kernel", 2.0 * P4 * 3 * 256, P4 * (512 + 12));
        launch_convsta(c->cur_stream, V(x).as<half_t>(), H4 * W4, c->sta_w16.as<float>(), c->sta_b.as<float>(), c->sta.as<float>());
    };
    if (comp) {
        // SFD2_PREC_F16C backbone: every activation carries a corr plane, every layer adds the fp8 correction terms (the formats: plan_pass)
        if (p.fused_stem) {
            ProfScope ps(c, "conv1a+conv1b", "fused_stem_c_kernel", 2.0 * P1 * 64 * 27 + 2.0 * (double)H2 * W2 * 64 * 576,
                         P1 * 12 + (double)H2 * W2 * 256);
            launch_fused_stem_c(st, img_dev, H, W, normalise, c->c1a.wc.as<half_t>(), c->c1a.scale.as<float>(),
                                c->c1a.shift.as<float>(), p.rec[T_CONV1B] == Rec::Half6 ? c->w1b_stem_c6.p : c->w1b_stem_c.p, c->c1b.scale.as<float>(),
                                c->c1b.shift.as<float>(), V(T_CONV1B).as<half_t>(), corr_of(V(T_CONV1B), (size_t)H2 * W2, 64), H2, W2, c->c1b.sbyte,
                                c->range_stat.as<unsigned int>(), p.rec[T_CONV1B]);
        } else {
            {
                ProfScope ps(c, "conv1a", "conv1a_c_kernel", 2.0 * P1 * 64 * 27, P1 * (12 + 256));
                launch_conv1a_c(st, img_dev, H, W, normalise, c->c1a.wc.as<half_t>(), c->c1a.scale.as<float>(),
                                c->c1a.shift.as<float>(), V(T_CONV1A).as<half_t>(), corr_of(V(T_CONV1A), (size_t)H * W, 64), range_slot(c, T_CONV1A));
            }
            convc(c, p, "conv1b", c->c1b, T_CONV1A, T_CONV1B, 1);
        }
        convc(c, p, "conv2a", c->c2a, T_CONV1B, T_CONV2A, 1, T_NONE, p.a2a_s2d);
        if (p.a2a_s2d) {
            const ConvW &L = c->c2b;
            ProfScope ps(c, "conv2b", "conv2b_s2d_kernel", 2.0 * P4 * L.cout * L.cin * 9, 4.0 * ((double)H2 * W2 * L.cin + (double)L.cout * L.cin * 9) + P4 * L.cout_pad * 4.0);
            launch_conv2b_s2d(st, V(T_CONV2A).as<half_t>(), corr_of(V(T_CONV2A), (size_t)H2 * W2, L.cin), H4, W4, L.wc.as<half_t>(), L.scale.as<float>(), L.shift.as<float>(), 1,
                              V(T_CONV2B).as<half_t>(), corr_of(V(T_CONV2B), (size_t)H4 * W4, L.cout_pad), c->zero_page.as<half_t>(), L.sbyte, range_slot(c, T_CONV2B), p.rec[T_CONV2B]);
        } else
        convc(c, p, "conv2b", c->c2b, T_CONV2A, T_CONV2B, 1);
        convc(c, p, "conv3a", c->c3a, T_CONV2B, T_CONV3A, 1);
        convc(c, p, "conv3b", c->c3b, T_CONV3A, T_CONV3B, 1, T_NONE, false, &p.a3a_in);
        for (int b = 0; b < 3; ++b) {  // ResBlock (nets/sfd2.py:25-55)
            if (!p.comp_rb) { rb_f16(b); continue; }   // option "comp_rb" = 0: this block in plain fp16 on the hi planes
            const int t1i = T_T1_0 + b, t2i = T_T2_0 + b, obi = T_OUT_0 + b;
            const DevPtr xv = V(x), t1 = V(t1i), t2 = V(t2i), ob = V(obi);
            // the records of the block's input, t1, t2 and output (plan_pass)
            const Rec x_rec = p.rec[x], t1_rec = p.rec[t1i], t2_rec = p.rec[t2i], o_rec = p.rec[obi];
            if (p.rb_inner) {
                // Option "rb_inner": the tensors INSIDE the block as plain fp16 (1: t2, 2: t1 and t2).  These kernels are bound
                // by HBM bytes, a plain tensor is half of a compensated one; the filters stay compensated (over a plain input the
                // residual term x * lo_w is a second fp16 pass: there is no fp8 value byte of x to feed the scaled MFMA).
                const size_t PP = (size_t)H4 * W4;
                const ConvW &L1 = c->rb1[b], &L2 = c->rb2[b], &L3 = c->rb3[b];
                const bool t1p = t1_rec == Rec::None;
                if (t1p) {
                    const bool x_r1 = x_rec == Rec::Resid8;
                    ProfScope ps(c, rb_layer_name(b, 1), "conv1x1_c256<comp,plain out>", 2.0 * P4 * 256.0 * 256.0, P4 * 256.0 * (x_r1 ? 5 : 6));
                    launch_conv1x1_c256_c(st, xv.as<half_t>(), corr_of(xv, PP, 256), (int)PP, L1.wfh.as<half_t>(), x_r1 ? L1.wfr.as<half_t>() : L1.wfc.as<half_t>(),
                                          L1.scale.as<float>(), L1.shift.as<float>(), 1, nullptr, nullptr, t1.as<half_t>(), nullptr,
                                          c->zero_page.as<half_t>(), L1.sbyte, range_slot(c, t1i), x_rec, t1_rec);
                } else {
                    convc(c, p, rb_layer_name(b, 1), L1, x, t1i, 1);
                }
                if (p.rb23) {
                    ProfScope ps(c, rb_layer_name(b, 3), "rb23_c_kernel", 2.0 * P4 * 256 * 72 + 2.0 * P4 * 256.0 * 256.0,
                                 P4 * 256.0 * (10 - (x_rec == Rec::Resid8) - (o_rec == Rec::Resid8)));
                    launch_rb23_c(st, t1.as<half_t>(), H4, W4, L2.w.as<half_t>(), L2.wlk.as<half_t>(), L2.scale.as<float>(), L2.shift.as<float>(),
                                  L3.wfh.as<half_t>(), L3.wfl.as<half_t>(), L3.scale.as<float>(), L3.shift.as<float>(), xv.as<half_t>(),
                                  corr_of(xv, PP, 256), ob.as<half_t>(), corr_of(ob, PP, 256), c->zero_page.as<half_t>(),
                                  range_slot(c, t2i), range_slot(c, obi), x_rec, o_rec, L3.wf8l.as<half_t>(), L3.sbyte);
                    x = obi;
                    continue;
                }
                {
                    ProfScope ps(c, rb_layer_name(b, 2), t1p ? "gconv_c_kernel<plain>" : "gconv_c_kernel<plain out>", 2.0 * P4 * 256 * 72, P4 * 256 * (t1p ? 4 : 6));
                    launch_gconv_c(st, t1.as<half_t>(), t1p ? nullptr : corr_of(t1, PP, 256), H4, W4, L2.w.as<half_t>(),
                                   t1p ? L2.wlk.p : L2.wc.p, L2.scale.as<float>(), L2.shift.as<float>(), t2.as<half_t>(), nullptr, L2.sbyte, 0, H4,
                                   range_slot(c, t2i));
                }
                {
                    ProfScope ps(c, rb_layer_name(b, 3), "conv1x1_c256<comp,plain in>+res", 2.0 * P4 * 256.0 * 256.0, P4 * 256.0 * 10);
                    launch_conv1x1_c256_c(st, t2.as<half_t>(), nullptr, (int)PP, L3.wfh.as<half_t>(), L3.wfl.as<half_t>(), L3.scale.as<float>(),
                                          L3.shift.as<float>(), 1, xv.as<half_t>(), corr_of(xv, PP, 256), ob.as<half_t>(), corr_of(ob, PP, 256),
                                          c->zero_page.as<half_t>(), L3.sbyte, range_slot(c, obi), t2_rec, o_rec);
                }
            } else {
                convc(c, p, rb_layer_name(b, 1), c->rb1[b], x, t1i, 1);
                {
                    ProfScope ps(c, rb_layer_name(b, 2), "gconv_c_kernel", 2.0 * P4 * 256 * 72, P4 * 256 * 8);
                    launch_gconv_c(st, t1.as<half_t>(), corr_of(t1, (size_t)H4 * W4, 256), H4, W4, c->rb2[b].w.as<half_t>(),
                                   c->rb2[b].wc.p, c->rb2[b].scale.as<float>(), c->rb2[b].shift.as<float>(), t2.as<half_t>(),
                                   corr_of(t2, (size_t)H4 * W4, 256), c->rb2[b].sbyte, 0, H4, range_slot(c, t2i));
                }
                convc(c, p, rb_layer_name(b, 3), c->rb3[b], t2i, obi, 1, x);
            }
            x = obi;
        }
    } else {
    if (p.fused_stem) {
        ProfScope ps(c, "conv1a+conv1b", "fused_stem_kernel", 2.0 * P1 * 64 * 27 + 2.0 * (double)H2 * W2 * 64 * 576,
                     P1 * 12 + (double)H2 * W2 * 128);
        launch_fused_stem(st, img_dev, H, W, normalise, c->c1a.w.as<half_t>(), c->c1a.scale.as<float>(),
                          c->c1a.shift.as<float>(), c->w1b_fused.as<half_t>(), c->c1b.scale.as<float>(),
                          c->c1b.shift.as<float>(), V(T_CONV1B).as<half_t>(), H2, W2);
    } else {
        {
            ProfScope ps(c, "conv1a", "conv1a_kernel", 2.0 * P1 * 64 * 27, P1 * (12 + 128));
            launch_conv1a(st, img_dev, H, W, normalise, c->c1a.w.as<half_t>(), c->c1a.scale.as<float>(),
                          c->c1a.shift.as<float>(), V(T_CONV1A).as<half_t>());
        }
        conv(c, p, "conv1b", c->c1b, T_CONV1A, T_CONV1B, 1);
    }
    conv(c, p, "conv2a", c->c2a, T_CONV1B, T_CONV2A, 1);
    conv(c, p, "conv2b", c->c2b, T_CONV2A, T_CONV2B, 1);
    conv(c, p, "conv3a", c->c3a, T_CONV2B, T_CONV3A, 1);
    conv(c, p, "conv3b", c->c3b, T_CONV3A, T_CONV3B, 1);
    for (int b = 0; b < 3; ++b) rb_f16(b);
    }
    // The two head branches read the backbone output and nothing of each other (nets/sfd2.py:328-342).  The detector
    // branch works on the 1/8 map (convPa.3: 133 tiles for 256 CUs at 1600x1200), so on its own it leaves part of the
    // chip idle; with option "branches" it runs on a side stream beside the descriptor branch (fork / join by events;
    // inside a captured hipGraph this becomes a fork in the graph).  Measured (tools/ab_branches.py, interleaved A/B at
    // 1600x1200): 1.260 -> 1.238 ms per extract (-1.7 %), outputs bit-identical.  Off by default: overlapped launches
    // stretch each other's event-timed durations, and bench.py's per-kernel roofline wants uncontended ones.
    // Option "sta_side" (round 6): ConvSta -- 63 MB read at HBM speed, 16 us -- on the side stream beside convPa.0 / convPa.3 / convDa.0 (matrix-bound, another part of
    // the chip's budget); fork here, join at the end of this function (the heat-map kernel behind it is the first reader of its output).  Inside a captured hipGraph: a
    // fork in the graph.  Same kernel, same bits.
    const bool sta_side = p.sta_side;
    if (c->has_sta && p.sta_early) {
        if (sta_side) {
            HIPCHECK(hipEventRecord(c->ev_fork, st));
            HIPCHECK(hipStreamWaitEvent(c->side_stream, c->ev_fork, 0));
            c->cur_stream = c->side_stream;
        }
        conv_sta();
        if (sta_side) {
            HIPCHECK(hipEventRecord(c->ev_join, c->side_stream));
            c->cur_stream = st;
        }
    }
    const bool fork = p.branches;
    if (fork) {
        HIPCHECK(hipEventRecord(c->ev_fork, st));
        HIPCHECK(hipStreamWaitEvent(c->side_stream, c->ev_fork, 0));
        c->cur_stream = c->side_stream;
    }
    if (p.chp) {      // options "comp_heads" / "comp_det" (plan_pass)
        convc(c, p, "convPa.0", c->pa0, x, T_PA0, 1);
        convc(c, p, "convPa.3", c->pa3, T_PA0, T_PA, 0);
    } else {
        conv(c, p, "convPa.0", c->pa0, x, T_PA0, 1);
        conv(c, p, "convPa.3", c->pa3, T_PA0, T_PA, 0);
    }
    if (!p.skip_pb) conv(c, p, "convPb", c->pb, T_PA, T_PB, 0, T_NONE, 1);
    if (!p.skip_head) {
        ProfScope ps(c, "detector_head", "detector_head_kernel", 0.0, P8 * (65 * 4 + 256));
        launch_detector_head(c->cur_stream, c->logits.as<float>(), 128, H8, W8, c->score.as<float>());
    }
    if (fork) {
        HIPCHECK(hipEventRecord(c->ev_join, c->side_stream));
        c->cur_stream = st;
    }
    if (p.ch) {
        convc(c, p, "convDa.0", c->da0, x, T_DA0, 1);
        convc(c, p, "convDa.3", c->da3, T_DA0, T_DA, 0);
    } else {
        // "sparse_da0": sfd2_extract runs the layer after the selection, on the key points' blocks; the backbone output must outlive this pass untouched
        // (its arena slot is 0; convPa.0 / convPa.3 write slot 1, convDa.0's map is slot 2, and convDa.3 -- the one layer that would take slot 0 -- is skipped)
        if (p.sparse_da0) c->da0_in = V(x);
        else conv(c, p, "convDa.0", c->da0, x, T_DA0, 1);
        if (!p.skip_da3) conv(c, p, "convDa.3", c->da3, T_DA0, T_DA, 0);
    }
    if (!p.skip_db) conv(c, p, "convDb", c->db, T_DA, T_DB, 0, T_NONE, 1);
    if (c->has_sta && !p.sta_early) conv_sta();
    if (fork || sta_side) HIPCHECK(hipStreamWaitEvent(st, c->ev_join, 0));
    HIPCHECK(hipGetLastError());
    if (c->net_error) { c->net_error = 0; return -1; }      // (a layer helper recorded an error: sfd2_last_error has its text)
    return 0;
}
