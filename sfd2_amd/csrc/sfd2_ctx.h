// libsfd2hip, host side: the context and what the api_*.hip translation units share.  Host C++ only (no kernels).
//   api_core.hip     context life cycle, options, profiling, timings, status
//   api_weights.hip  BatchNorm folding, filter packing for every kernel family, sfd2_load_weights
//   api_network.hip  workspace, per-layer kernel dispatch, the network passes of the four precisions
//   api_extract.hip  sfd2_det / sfd2_extract / pyramids / spp variants / stage entry points
//   api_match.hip    the matcher entry points
//   api_graph.hip    sfd2_extract_match and its hipGraph cache
#pragma once
#include "../../include/sfd2_hip.h"
#include "sfd2_internal.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

int sfd2_fail(const std::string &m);          // sets the thread's last-error text, returns -1
#define fail sfd2_fail
struct PoseCam;
bool sfd2_pose_cam(int model, const double *params, PoseCam &c, std::string &why);   // api_pose.hip: a COLMAP camera in the kernels' form
#define HIPCHECK(expr)                                                                           \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(std::string(#expr) + ": " + hipGetErrorString(e_) + " @" + std::to_string(__LINE__)); \
    } while (0)

extern std::atomic<unsigned long long> g_alloc_gen;   // (process-wide, contexts may live on different threads) bumped whenever a workspace buffer is (re)allocated: captured graphs hold raw pointers

// A device pointer with its capacity.  DevPtr is a non-owning view (arena slots, per-call aliases of the context's buffers);
// DevBuf owns its allocation and frees it when it goes away, so tearing a context or a layer down needs no list of members
// (the hand-kept list had missed six of them).
struct DevPtr {
    void *p = nullptr;
    size_t cap = 0;
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};
struct DevBuf : DevPtr {
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        ++g_alloc_gen;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct ConvW {                 // one folded + packed layer
    int cin = 0, cout = 0, cout_pad = 0, ks = 0, stride = 1;
    DevBuf w, scale, shift;    // fp16 packed filters, fp32 [cout_pad]
    DevBuf scale_rawin;        // convDa.0: scale for an input at the network's own scale (2^e_out only; option "x3_desc16" feeds it f16x3's hi plane)
    DevBuf wsl;                // convDa.3: w in sparse_da3_kernel's fragment order -- [chunk][tap][cout_pad / 32][2][64 lanes][8]: a fragment load reads one contiguous kilobyte
    DevBuf wrm;                // 1x1 256 -> 256 layers: the same filters as plain [cout][cin] fp16 (conv1x1_c256_kernel)
    DevBuf wfh, wfc, wfl;      // conv1x1_c256_c_kernel: the same filters, their corr units and fp16 of (w - fp16(w)) * 2^11 (the second
                               // fp16 pass over a PLAIN input, option "rb_inner") in the kernel's fragment order [8 waves][8][64 lanes][16]
    DevBuf wlk;                // grouped 3x3: the same residuals in w's fragment layout (gconv_c_kernel<false, false>)
    DevBuf wgc;                // grouped 3x3: compact [256 oc][9 taps][8 in] fp16 (resblock_kernel)
    DevBuf wx3;                // fp32 layers, SFD2_PREC_F16X3: every float4 of w as (4 hi, 4 lo) fp16 for the generic kernel (grouped conv: gconv_x3_kernel's packing) ...
    DevBuf wx3p;               // ... or as two planes (hi, lo') for the three-pass 3x3 kernels; both (and convDa.3's wsl in this mode) made by ensure_strict_filters for the plan about to run
    DevBuf wc;                 // SFD2_PREC_F16C: [2 * cin / 32][taps][cout_pad][32] units -- the fp16 filters in 32-wide chunks, then the
                               // corr units (fp8 of w * 2^b0, fp8 of (w - fp16(w)) * 2^(b0 + 11)); conv1a / grouped conv: hi then lo fragments
    int sbyte = 127;           // E8M0 scale byte of the layer's corr MFMAs: 127 - 9 - b0
    DevBuf wf8l;               // the 1x1 layers' filter residuals as e4m3 in rb23_c_kernel's K order (option "trunk_r1": conv3's x * lo_w term on the scaled MFMA)
    DevBuf wfr;                // the 1x1 layers' corr units in the order of the residual-only input form (option "trunk_r1")
    DevBuf wc6;                // conv3x3_pp layers: wc with the corr filter rows as fp6 (e2m3) strings, and ...
    DevBuf sa6;                // ... [shift[cout_pad] | per-output-channel E8M0 scale bytes, replicated into the four bytes of an int, [cout_pad]]
    size_t w_floats = 0;       // floats in w (fp32 layers)
    std::vector<float> h_scale, h_shift;   // host copies of the folded constants as loaded (before the activation exponents)
    std::vector<int> h_sa6;                // host copy of sa6
    DevBuf wc66, sa66;                     // the same two arrays for fp6 PIXEL records (option "fp6_acts"): the strings in the half-records' channel
    std::vector<int> h_sa66;               // order (sfd2_epi16_fp6), the scale bytes 2^(ec - 11)
};

// Activation exponents of the fp16 family (SFD2_PREC_F16 / F16C): the stored tensor of group g is 2^act_exp[g] times the network's
// tensor.  ReLU commutes with a positive factor and the factor is a power of two, so folding 2^(e_out - e_in) into a layer's scale
// and 2^e_out into its shift changes nothing but where the tensor sits in the number formats: exact in fp32, and it is what keeps
// the compensated mode's fixed-point-like corr units (e4m3 of x / 4 and of the fp16 residual * 512, tensors saturating at 1792)
// in their sweet spot whatever scale the checkpoint's activations have.  Set by sfd2_calibrate_range (api_weights.hip).
enum { AE_CONV1A, AE_CONV1B, AE_CONV2A, AE_CONV2B, AE_CONV3A, AE_TRUNK /* conv3b's and every ResBlock's output: one skip path */,
       AE_T1_0, AE_T1_1, AE_T1_2, AE_T2_0, AE_T2_1, AE_T2_2, AE_PA0, AE_DA0, AE_COUNT };

// A stored activation tensor has ONE identity: its id.  The id indexes the context's buffers (act16 / act32), the pass plan's records and arena placement,
// the registered activations, and -- for the first SFD2_RS_COUNT ids, in sfd2_internal.h's order -- is the tensor's range-status slot.  convPa.3's and
// convDa.3's outputs have no slot and no exponent group; the three head outputs behind T_COUNT live in buffers of their own (logits, draw, sta).
enum Tensor { T_CONV1A, T_CONV1B, T_CONV2A, T_CONV2B, T_CONV3A, T_CONV3B, T_T1_0, T_T2_0 = T_T1_0 + 3, T_OUT_0 = T_T2_0 + 3, T_PA0 = T_OUT_0 + 3, T_DA0,
              T_PA, T_DA, T_COUNT, T_PB = T_COUNT, T_DB, T_STA, T_ALL, T_NONE = -1 };
struct TensorRow { const char *act /* sfd2_debug_activation */, *range /* sfd2_range_tensor_name */; int level /* 0: H x W ... 3: 1/8 */, ch, group /* AE_*, -1: none */; };
inline constexpr TensorRow kTensor[] = {
    {"conv1a", "conv1a", 0, 64, AE_CONV1A}, {"bn1b", "conv1b", 1, 64, AE_CONV1B}, {"conv2a", "conv2a", 1, 128, AE_CONV2A},
    {"bn2b", "conv2b", 2, 128, AE_CONV2B}, {"conv3a", "conv3a", 2, 256, AE_CONV3A}, {"bn3b", "conv3b", 2, 256, AE_TRUNK},
    {"conv4.0.bn1", "conv4.0.t1", 2, 256, AE_T1_0}, {"conv4.1.bn1", "conv4.1.t1", 2, 256, AE_T1_1}, {"conv4.2.bn1", "conv4.2.t1", 2, 256, AE_T1_2},
    {"conv4.0.bn2", "conv4.0.t2", 2, 256, AE_T2_0}, {"conv4.1.bn2", "conv4.1.t2", 2, 256, AE_T2_1}, {"conv4.2.bn2", "conv4.2.t2", 2, 256, AE_T2_2},
    {"conv4.0", "conv4.0", 2, 256, AE_TRUNK}, {"conv4.1", "conv4.1", 2, 256, AE_TRUNK}, {"conv4.2", "conv4.2", 2, 256, AE_TRUNK},
    {"convPa.0", "convPa.0", 3, 256, AE_PA0}, {"convDa.0", "convDa.0", 2, 256, AE_DA0}, {"convPa", "", 3, 256, -1}, {"convDa", "", 2, 256, -1},
    {"convPb", "", 3, 65, -1}, {"convDb", "", 2, 128, -1}, {"ConvSta", "", 2, 3, -1}};
static_assert(sizeof(kTensor) == T_ALL * sizeof(TensorRow), "one row per tensor id");
static_assert(T_PA == SFD2_RS_COUNT, "the ids with a range-status slot come first (SFD2_RS_COUNT == SFD2_RANGE_TENSORS: api_core.hip)");
static_assert(T_CONV1A == SFD2_RS_CONV1A && T_CONV1B == SFD2_RS_CONV1B && T_CONV2A == SFD2_RS_CONV2A && T_CONV2B == SFD2_RS_CONV2B && T_CONV3A == SFD2_RS_CONV3A &&
              T_CONV3B == SFD2_RS_CONV3B && T_T1_0 == SFD2_RS_T1_0 && T_T1_0 + 2 == SFD2_RS_T1_2 && T_T2_0 == SFD2_RS_T2_0 && T_T2_0 + 2 == SFD2_RS_T2_2 &&
              T_OUT_0 == SFD2_RS_OUT_0 && T_OUT_0 + 2 == SFD2_RS_OUT_2 && T_PA0 == SFD2_RS_PA0 && T_DA0 == SFD2_RS_DA0, "a tensor's range-status slot is its id");
// the profile-row name of a ResBlock layer: "conv4.<b>.conv<k>" (k = 1, 2, 3)
inline const char *rb_layer_name(int b, int k)
{
    static const char *n[3][3] = {{"conv4.0.conv1", "conv4.0.conv2", "conv4.0.conv3"}, {"conv4.1.conv1", "conv4.1.conv2", "conv4.1.conv3"}, {"conv4.2.conv1", "conv4.2.conv2", "conv4.2.conv3"}};
    return n[b][k - 1];
}

struct ActInfo { bool known = false; /* registered by the last ensure_workspace */ const void *p; int f32; int planar; int c, pitch, h, w; Rec rec = Rec::None; /* f16c: the format of the corr records (their plane follows the hi plane) */ int exp2 = 0; /* stored = value * 2^exp2 (activation exponents of the fp16 family) */ bool absent = false; /* stays on chip on the path taken */ };

// A device block that is scratch of one entry point: its own hipMalloc, NOT a DevBuf.  Growing it never bumps g_alloc_gen, so it
// never drops the captured graphs of the network (api_graph.hip), which never read these blocks.  Users: the JPEG decoder
// (api_jpeg.hip, with a grow() of its own that synchronises and leaves headroom) and every geometry entry point (api_pose /
// assemble / triangulate / pairs / cluster / frames .hip), which lay the block out with api_scratch.h's Carve.
struct ScratchBuf {
    void *p = nullptr;
    size_t cap = 0;
    ScratchBuf() = default;
    ScratchBuf(const ScratchBuf &) = delete;
    ScratchBuf &operator=(const ScratchBuf &) = delete;
    ~ScratchBuf() { if (p) (void)hipFree(p); }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};
// at least `bytes`; the old block is freed first (hipFree waits for the device), the contents are not kept
inline hipError_t grow(ScratchBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return hipSuccess;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e == hipSuccess) b.cap = bytes;
    return e;
}
struct JpegScratch {
    ScratchBuf in[2];                     // prepared buffers, uploaded through the copy stream (two, so the next upload overlaps this decode)
    hipEvent_t ev_copied[2] = {}, ev_free[2] = {};
    int slot = 0;
    ScratchBuf lanes, pre, coef, planes;
    ScratchBuf words;                     // sync flags (SFD2_JPEG_SYNC_LAUNCHES) and the status word
    ~JpegScratch()
    {
        for (int i = 0; i < 2; ++i) {
            if (ev_copied[i]) (void)hipEventDestroy(ev_copied[i]);
            if (ev_free[i]) (void)hipEventDestroy(ev_free[i]);
        }
    }
};

struct sfd2_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_jobs = nullptr;      // guards reuse of the pinned job descriptors below
    // host images go through a copy stream into one of two staging slots, so the upload of image i + 1 overlaps the
    // network of image i when the caller runs extracts back to back (SFD2_FLAG_ASYNC + pinned host memory)
    hipStream_t copy_stream = nullptr;
    // (SFD2_IMG_SLOTS slots, not two: an upload that has to WAIT for its slot's previous reader stalls the copy engine's queue in front of every other
    //  context's uploads -- two pipelined contexts on one device then run at half the rate of one (CHANGELOG round 5) -- so the ring is longer than the images
    //  a driver keeps in flight per context)
#define SFD2_IMG_SLOTS 4
    hipEvent_t ev_copied[SFD2_IMG_SLOTS] = {}, ev_img_free[SFD2_IMG_SLOTS] = {};
    DevBuf img2[SFD2_IMG_SLOTS];
    int img_slot = 0, img_slot_used = -1;
    void *pin_jobs = nullptr;
    size_t pin_cap = 0;
    bool weights_loaded = false;
    bool counters_clean = false;       // the kernel in front of the selection cleared the counters (pb_heads_heat_kernel)
    bool has_sta = false;              // ConvSta present in the loaded state_dict (absent for require_stability=False models)
    int opt_alias = 1;                 // sfd2_set_option "alias"
    int act_exp[AE_COUNT] = {};        // activation exponents of the fp16 family (above)
    float act_max[AE_COUNT] = {};      // what the calibration measured (largest |x| of the group's tensors on the calibration image)
    int opt_range_fallback = 1;        // sfd2_set_option "range_fallback": a synchronous f16c extract that saturated a tensor is re-run in f16x3
    int range_fallbacks = 0;           // how often that happened
    int in_fallback = 0;               // set around the re-run
    int prof_step_entry = 0;           // profile step at the entry of the running extraction: the repeat starts there again
    float range_hist[SFD2_RS_COUNT] = {};   // maxima (stored units) folded away from the device words by a fallback's reset
    int opt_auto_range = 1;            // sfd2_set_option "auto_range": sfd2_load_weights calibrates the exponents on a built-in probe image
    std::vector<float> h_sta_w;        // ConvSta filters as loaded (the uploaded copy carries 2^-act_exp[AE_TRUNK])
    int opt_cu_limit = 0;              // sfd2_set_option "cu_limit": persistent kernels of THIS context launch at most so many blocks
    int fuse_det = 0;                  // sfd2_set_option "fuse_det"
    int use_graphs = 0;                // sfd2_set_option "graphs"
    DevBuf x3_chain[2];                // f16x3 tensors as hi / lo' planes (hi, then lo'; who reads and writes which buffer: PassPlan::sl).  X3_CHAIN_A / B: handed from one 3x3 layer to the next
    DevBuf x3_rb_planes[3];            // a ResBlock's input (X3_RB), conv1's and the grouped conv's outputs
    int opt_fuse_post = 1;             // sfd2_set_option "fuse_post": heads -> heat map -> NMS in one kernel on the extract path
    int opt_sparse_desc = 1;           // sfd2_set_option "sparse_desc": extract path runs convDb on the sampled corner pixels only
    DevBuf da3_sparse;                 // [sel_cap][4][256] fp16: convDa.3 on the sampled corner pixels
    int opt_fp6_acts = 1;              // sfd2_set_option "fp6_acts": the corr records of the three tensors only conv3x3_pp<comp> reads (conv1b's, conv2b's,
                                       // conv3a's output) as block-scaled fp6 half-records, their consumers' corr MFMAs fp6 x fp6 (33.5 cycles instead of 66)
    int net_error = 0;                 // set by a layer helper of run_network that cannot return an error itself; run_network returns -1 and clears it
    int opt_trunk_r1 = 1;              // sfd2_set_option "trunk_r1": conv3b's output and the outputs of ResBlocks 0 and 1 carry ONE correction byte per channel (the
                                       // residual) instead of the (residual, value) unit: 3 bytes per channel through the HBM-bound ResBlock kernels instead of 4
    int opt_s2d = 1;                   // sfd2_set_option "s2d": on the throughput path conv2a stores its output space-to-depth and conv2b runs as a stride-1 layer
                                       // over it (conv2b_s2d_kernel.hip) instead of conv3x3_rf<2,comp>
    int opt_fp6_filters = 0;           // sfd2_set_option "fp6_filters": conv3x3_pp<comp> takes its corr filters as block-scaled fp6 (fp8 x fp6 MFMA).
                                       // Measured: conv3b 212.0 -> 212.1 us, extract 1.5188 -> 1.5165 ms, descriptors <=5.2e-4 (<=4.9e-4 without): the
                                       // mixed-format MFMA's shorter issue time in the probe does not show in the layer; off by default, kept as the
                                       // packing / layout groundwork for fp6 on both sides
    int opt_x3_pp = 1;                 // sfd2_set_option "x3_pp": SFD2_PREC_F16X3 runs its 3x3 stride-1 layers on conv3x3_pp (pre-split planes, three passes)
    int opt_auto_margin = 1;           // sfd2_set_option "auto_margin": sfd2_load_weights measures SFD2_PREC_F16C's descriptor error on the built-in probe against the
                                       // SFD2_PREC_F32 pass it runs anyway and, above SFD2_MARGIN_TARGET, turns on the accuracy options that bring it back (api_weights.hip)
    float margin_err[4] = {-1.0f, -1.0f, -1.0f, -1.0f};   // probe error with the options as set / rb_inner = 0 / comp_heads = 1 / both (-1: not measured)
    int margin_choice = -1;            // which of the four the context now runs (-1: no self-check has run)
    int opt_c3b_plain = 0;             // effective: conv3b (SFD2_PREC_F16C) runs its K loop over the hi plane of conv3a's output only -- no correction chunks (the
                                       // output's corr bytes still come from the fp32 accumulators) -- and conv3a then writes no corr plane.  -62 us of 184 at 1600x1200
                                       // for ~ x 1.4 on the descriptor error (tools/relax_study.py), so it is never on unverified:
    int user_c3b_plain = -1;           // sfd2_set_option "c3b_plain": -1 (default) = on only when the load-time self-check measured the probe inside SFD2_MARGIN_TARGET
                                       // WITH it (option "auto_margin"; off otherwise), 1 = on, 0 = off
    bool margin_done = false, margin_pending = false;   // the self-check ran on the loaded weights / waits for the context to enter SFD2_PREC_F16C
    float relax_err = -1.0f;           // the probe's error with "c3b_plain" on and the other options as set (-1: not measured)
    bool user_set_rb_inner = false, user_set_comp_heads = false;   // the caller set the key explicitly: the self-check reports, but does not override it
    int user_rb_inner = 2, user_comp_heads = 0;   // what sfd2_set_option last asked for: the self-check of a LATER sfd2_load_weights starts from these, not from its own earlier choice
    int opt_x3_desc16 = 0;             // sfd2_set_option "x3_desc16": SFD2_PREC_F16X3 on sfd2_extract with the DESCRIPTOR branch (convDa.0, convDa.3 at the sampled corners,
                                       // convDb) in plain fp16 on the backbone output's hi plane: the key points are this mode's own, the descriptors carry the
                                       // fp16 head's error only (<= 1e-3: north_star's tolerance, not this mode's 2e-5)
    DevBuf x3_planes;                  // scratch planes: the fp32 input of a three-pass 3x3 layer whose producer left no planes, split in front of it
    DevBuf x3_da0_planes;              // X3_DA0: convDa.0's output as planes (sparse descriptor head of f16x3); with "x3_desc16" its fp16 output
    DevBuf db_sparse;                  // [sel_cap][4][128] fp32: convDb on the sampled corners (f16x3)
    int opt_sparse_da3 = 1;            // sfd2_set_option "sparse_da3": with the sparse descriptor head, convDa.3 on the sampled corners only
    int opt_sparse_da0 = 1;            // sfd2_set_option "sparse_da0": with "sparse_da3", convDa.0 on the 4 x 4 blocks that kernel reads only (sparse_da0_kernel.hip):
                                       // 1 = where the plan expects it to pay (plan_pass), 0 = always dense, 2 = wherever the arithmetic allows (tests, A/B runs at small sizes)
    DevPtr da0_in;                     // ... the backbone output's fp16 plane as the last run_network left it: sfd2_extract's sparse convDa.0 reads it after the selection
    int opt_fuse_pb = 1;               // sfd2_set_option "fuse_pb": convPb inside the fused detector-head / heat-map kernel
    int opt_comp_rb = 1;               // sfd2_set_option "comp_rb": SFD2_PREC_F16C compensates the ResBlocks too (0: fused fp16 ResBlock kernel)
    int opt_rb_inner = 2;              // sfd2_set_option "rb_inner": SFD2_PREC_F16C ResBlocks, 1 = t2 (the grouped conv's output) stored as plain
                                       // fp16, 2 (default) = t1 and t2, 0 = both compensated; the filters stay compensated either way
                                       // (second fp16 pass with their residuals).  Measured at 1600x1200: 1.82 / 1.75 / 1.67 ms per
                                       // extract for 0 / 1 / 2, descriptors <= 3.5e-4 / 3.8e-4 / 4.9e-4 over the BASELINE geometries.
    int opt_fuse_rb23 = 1;             // sfd2_set_option "fuse_rb23": with rb_inner = 2, ResBlock.conv2 + conv3 + residual in one kernel (t2 stays in LDS)
    int opt_comp_det = 0;              // sfd2_set_option "comp_det": SFD2_PREC_F16C compensates the detector branch's 3x3 layers (convPa.0, convPa.3) only
    int opt_comp_heads = 0;            // sfd2_set_option "comp_heads": SFD2_PREC_F16C compensates the 3x3 layers of the two head branches too
    int opt_no_rf_c = 0;               // sfd2_set_option "no_rf_c": conv2b on conv_igemm2<comp> instead of conv3x3_rf<comp> (A/B switch)
    int opt_generic_c = 0;             // sfd2_set_option "generic_c": SFD2_PREC_F16C layers on the generic reference kernel (tests)
    int opt_branches = 0;              // sfd2_set_option "branches": detector branch on a second stream beside the descriptor branch
    int opt_sta_side = 0;              // sfd2_set_option "sta_side": ConvSta on the side stream beside the head branches' 3x3 layers (throughput path)
    hipStream_t side_stream = nullptr; // the detector branch (convPa.0 -> convPa.3 -> convPb -> detector_head)
    hipStream_t cur_stream = nullptr;  // stream the conv()/ProfScope helpers launch on (main or side)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    struct GraphEntry *graphs = nullptr;   // hipGraph cache of sfd2_extract_match (see below)
    int n_graphs = 0;
    unsigned long long graph_clock = 0;
    // weights
    ConvW c1a, c1b, c2a, c2b, c3a, c3b, rb1[3], rb2[3], rb3[3], pa0, pa3, da0, da3, pb, db;
    DevBuf sta_w16;                                // ConvSta filters times 2^-act_exp[AE_TRUNK]: what the fp16 family launches with
    DevPtr range_stat;                             // (a view: the words live behind the zero page) SFD2_RS_COUNT x SFD2_RANGE_SUB words: running maxima of the compensated mode's stored tensors (sticky until read with reset)
    DevPtr range_hist_dev;                         // (a view behind range_stat) SFD2_RS_COUNT words: maxima folded away from the running words on the device
    DevPtr extract_rec;                            // (a view behind range_hist_dev) the four words of sfd2_extract_record_async
    DevBuf range_scratch;                          // AE_COUNT words: absolute maxima of a calibration pass
    DevBuf sta_w, sta_b, zero_page, w1b_fused;   // w1b_fused: conv1b filters as [9][64][64] for the fused stem
    DevBuf w1b_stem_c6;                            // ... with the corr fragments as fp6 strings + scale byte (option "fp6_acts")
    DevBuf w1b_stem_c;                             // the same as register fragments (hi K slices + corr) for the compensated fused stem
    DevBuf w1b_stem_x3;                            // ... with the lo' fragments (fp16 of (w - fp16(w)) * 2^11) in place of the corr fragment: f16x3
    int fuse = 1;                                  // fused kernels on the extract path (SFD2_NO_FUSE=1 disables)
    // strict fp32 mode
    int precision = SFD2_PREC_F16;
    ConvW f1a, f1b, f2a, f2b, f3a, f3b, frb1[3], frb2[3], frb3[3], fpa0, fpa3, fda0, fda3, fpb, fdb;
    DevBuf act32[T_COUNT];             // fp32 NHWC activations, by tensor id
    // geometry of the current workspace
    int H = 0, W = 0, H2 = 0, W2 = 0, H4 = 0, W4 = 0, H8 = 0, W8 = 0;
    // activations (NHWC fp16 unless noted), by tensor id
    DevBuf img, act16[T_COUNT];
    DevBuf logits /*f32 [P8][128]*/, draw /*f32 [P4][128]*/, sta /*f32 [3][P4]*/, score /*f32*/, heat /*f32*/;
    DevBuf stab /*f32 [H][W]*/, desc_nchw, tmp_f32;
    // selection
    DevBuf cand, bnd, sel, sorted, counters, kpts, kscores, kdesc;
    DevBuf kdesc64;                    // SFD2_FLAG_DESC_STORE64: the descriptors as float64 [128][capacity] on their way to a host buffer
    DevBuf g_keys, g_state0, g_state1, g_kept;   // greedy NMS (extract.py variant)
    int cand_cap = 0;
    int last_sel_cap = 0;
    float *kpts_cur = nullptr, *kscores_cur = nullptr;   // where the last selection wrote its key points
    // scale pyramid staging (sfd2_extract_multiscale)
    DevBuf arena;   // aliased activation slots of the throughput path (placed by plan_pass, sized by ensure_workspace)
    DevBuf img_u8_packed;              // SFD2_FLAG_IMG_U8_X: the image as three bytes per pixel (unpack_rgbx_kernel)
    JpegScratch jpeg;                  // sfd2_jpeg_decode
    // scratch of the geometry entry points (ScratchBuf: growing one drops no captured graph; grow() above, layouts by api_scratch.h's Carve)
    ScratchBuf asm_in, asm_ws, asm_out;     // sfd2_assemble_2d3d (api_assemble.hip): descriptors and host inputs, per-(image, key point) work, host-bound outputs
    ScratchBuf pose_in, pose_ws, pose_out;  // sfd2_absolute_pose_batch / sfd2_pose_refine_batch (api_pose.hip): inputs, per-point work, results
    ScratchBuf tv_in, tv_ws, tv_out;        // sfd2_relative_pose_batch (api_two_view.hip): inputs, normalised points and the trials' matrices, results
    ScratchBuf fm_in, fm_ws, fm_out;        // sfd2_fundamental_batch / sfd2_homography_batch (api_fundamental.hip pairs_batch): inputs, normalised points, results
    ScratchBuf gm_in, gm_ws;                // sfd2_match_guided_batch (api_guided.hip): uploaded key points, descriptors and job descriptors; fp16 sets, gate records, partials and results
    ScratchBuf tri_in, tri_ws;             // sfd2_verify_matches_batch / sfd2_build_tracks / sfd2_triangulate_tracks (api_triangulate.hip): inputs, work and results
    ScratchBuf pairs_in, pairs_ws;          // sfd2_pairs_retrieval / _covisibility / _poses (api_pairs.hip), sfd2_covis_clusters (api_cluster.hip) and sfd2_covis_frames (api_frames.hip): uploaded inputs, partial lists / counters / slot rows and results
    ScratchBuf vlad_in, vlad_ws;            // sfd2_vlad_assign / _aggregate / _kmeans (api_vlad.hip): uploaded rows, centroids and offsets; assignments, sums, partials and results
    ScratchBuf ba_in, ba_ws;                // sfd2_bundle_adjust (api_bundle.hip): uploaded inputs and the two CSRs; state, Jacobian records, blocks, PCG vectors and results
    ScratchBuf map_in, map_ws;              // sfd2_mapper_restrict / _filter / _visible / _assemble (api_mapper.hip): uploaded tables and lists; flags, scans, per-observation work and results
    DevBuf img_scaled, ms_kp, ms_sc, ms_de, ms_keys, ms_sorted, ms_cnt;
    unsigned int ms_cand_seen[8] = {};
    int ms_cand_cap[8] = {};
    // matcher
    DevBuf m_stage, m_hi0, m_lo0, m_hi1, m_lo1, m_part_f, m_part_i, m_red, m_jobs, m_fins, m_out_m, m_out_s, m_rkeys;
    sfd2_timings tim = {};
    ActInfo acts[T_ALL] = {};          // by tensor id; sfd2_debug_activation searches kTensor's names
    // per-launch profiling (sfd2_set_profiling)
    int prof_max_steps = 0, prof_step = 0, prof_slot = 0;
    std::vector<hipEvent_t> prof_ev;          // [max_steps][PROF_SLOTS][2]
    std::vector<sfd2_layer_timing> prof_tab;  // slot -> descriptor + accumulators
    std::vector<int> prof_used;               // [max_steps] slots recorded in that step
    std::vector<int> prof_row;                // [max_steps][PROF_SLOTS] -> row of prof_tab
    std::string prof_filter;                  // only kernel labels containing this are timed
};

void graphs_release(sfd2_ctx *c);
// api_fundamental.hip: the checking, packing and scratch layer of the camera-less pair estimators, one launch of `launch`
typedef void (*PairsLaunch)(hipStream_t, const FmProbDev *, int, const TvConfDev &, const double *, const double *, double2 *, double2 *,
                            unsigned char *, FmResDev *);
int pairs_batch(const char *name, int sample_size, PairsLaunch launch, sfd2_ctx *c, const sfd2_fundamental_problem *problems, int k,
                const sfd2_two_view_conf *conf, sfd2_fundamental_result *results, uint8_t *inlier_mask_u8, int flags);
#define PROF_SLOTS 48
struct ProfScope {   // records an event pair around one launch when profiling is on
    sfd2_ctx *c; int slot;
    ProfScope(sfd2_ctx *c_, const char *name, const char *kernel, double flops, double bytes) : c(c_), slot(-1)
    {
        if (c->prof_max_steps <= 0 || c->prof_step >= c->prof_max_steps || c->prof_slot >= PROF_SLOTS) return;
        if (!c->prof_filter.empty() && strstr(kernel, c->prof_filter.c_str()) == nullptr) return;
        slot = c->prof_slot++;
        int row = -1;  // table rows are keyed by stage name (extract and match steps interleave)
        for (size_t i = 0; i < c->prof_tab.size(); ++i)
            if (strncmp(c->prof_tab[i].name, name, sizeof(c->prof_tab[i].name) - 1) == 0) { row = (int)i; break; }
        if (row < 0) {
            c->prof_tab.push_back(sfd2_layer_timing{});
            row = (int)c->prof_tab.size() - 1;
            snprintf(c->prof_tab[row].name, sizeof(c->prof_tab[row].name), "%s", name);
            snprintf(c->prof_tab[row].kernel, sizeof(c->prof_tab[row].kernel), "%s", kernel);
        }
        c->prof_tab[row].flops = flops;
        c->prof_tab[row].bytes = bytes;
        c->prof_row[(size_t)c->prof_step * PROF_SLOTS + slot] = row;
        (void)hipEventRecord(c->prof_ev[((size_t)c->prof_step * PROF_SLOTS + slot) * 2], c->cur_stream);
    }
    void cancel()   // the launch did not happen (a launcher declined the geometry): give the slot back
    {
        if (slot >= 0 && slot == c->prof_slot - 1) c->prof_slot--;
        slot = -1;
    }
    ~ProfScope()
    {
        if (slot >= 0) (void)hipEventRecord(c->prof_ev[((size_t)c->prof_step * PROF_SLOTS + slot) * 2 + 1], c->cur_stream);
    }
};
static inline void prof_step_begin(sfd2_ctx *c) { c->prof_slot = 0; }
static inline void prof_step_end(sfd2_ctx *c)
{
    if (c->prof_max_steps > 0 && c->prof_step < c->prof_max_steps) {
        c->prof_used[c->prof_step] = c->prof_slot;
        c->prof_step++;
    }
}

// api_weights.hip
int apply_act_exponents(sfd2_ctx *c);                   // re-uploads the fp16 family's scale / shift arrays with c->act_exp folded in
// api_core.hip
int read_range_status(sfd2_ctx *c, sfd2_range_status *out, int reset);
// after a synchronous extraction in SFD2_PREC_F16C: 1 = a compensated tensor saturated and the call is to be repeated in SFD2_PREC_F16X3
// (the device words are folded into the context's history and cleared), 0 = fine / not applicable, -1 = error
int range_wants_fallback(sfd2_ctx *c);
int range_fold_before_sync_extract(sfd2_ctx *c);        // earlier asynchronous calls' maxima -> device-side history, running words cleared (no host sync)
int sfd2_margin_selfcheck_if_pending(sfd2_ctx *c);    // api_weights.hip: the F16C self-check of a context loaded in another precision
int reset_range_records(sfd2_ctx *c);                   // the exponents changed: running words, device and host history cleared
struct FallbackScope {      // the repeat: strict arithmetic, no recursion
    sfd2_ctx *c; int prec;
    explicit FallbackScope(sfd2_ctx *c_) : c(c_), prec(c_->precision)
    {
        c->precision = SFD2_PREC_F16X3; c->in_fallback = 1; c->range_fallbacks++;
        if (c->prof_step > c->prof_step_entry) c->prof_step = c->prof_step_entry;   // the saturated pass is not a profiled step: its slots are recorded again
    }
    ~FallbackScope() { c->precision = prec; c->in_fallback = 0; }
};
// api_network.hip.  What one network pass runs, decided once per call (plan_pass) from the options, the precision, the entry point, the
// geometry and which packed weight arrays exist; ensure_workspace allocates and registers the activations from it, the dispatch reads it.
enum PassEntry { PASS_DET /* parity: every activation readable unless "fuse_det" */, PASS_DENSE /* throughput kernels, dense head maps (pyramids,
                 spp) */, PASS_EXTRACT /* sfd2_extract: the heads fused into the post-processing, the sparse descriptor head */ };
// The conv layers of the strict pass (SFD2_PREC_F32 / F16X3) that go through convf, in pass order; the ResBlocks' 1x1 layers: + block
enum StrictLayer { SL_C1B, SL_C2A, SL_C2B, SL_C3A, SL_C3B, SL_RB1, SL_RB3 = SL_RB1 + 3, SL_PA0 = SL_RB3 + 3, SL_PA3, SL_PB, SL_DA0, SL_DA3, SL_DB, SL_COUNT };
template <class Ctx> auto &strict_layer(Ctx *c, int i)     // (Ctx: sfd2_ctx or const sfd2_ctx)
{
    decltype(&c->f1b) t[] = {&c->f1b, &c->f2a, &c->f2b, &c->f3a, &c->f3b, &c->frb1[0], &c->frb1[1], &c->frb1[2], &c->frb3[0], &c->frb3[1], &c->frb3[2],
                             &c->fpa0, &c->fpa3, &c->fpb, &c->fda0, &c->fda3, &c->fdb};
    static_assert(sizeof(t) == SL_COUNT * sizeof(t[0]), "one entry per StrictLayer");
    return *t[i];
}
// The kernel such a layer runs on: the generic igemm (fp32 in / out: conv_igemm_f32, conv_igemm_x3) or one of SFD2_PREC_F16X3's three-pass 3x3 kernels on hi / lo' planes
// (conv3x3_pp<x3>, conv3x3_rf<x3>, conv2b_s2d_kernel<x3>).  XK_SKIP: not run by this pass (the fused stem, the ResBlocks on planes, sfd2_extract's sparse descriptor head)
enum X3Kind { XK_GENERIC, XK_PP, XK_RF, XK_S2D, XK_SKIP };
enum X3Out { X3_F32, X3_CHAIN_A, X3_CHAIN_B, X3_RB, X3_DA0 };   // where its output goes: the fp32 tensor, or planes only in one of the context's plane buffers
struct StrictConv { X3Kind kind = XK_GENERIC; bool planes_in = false; X3Out out = X3_F32; bool s2d_out = false; };   // planes_in: the producer left the input as planes (otherwise split into x3_planes first); s2d_out: planes stored space-to-depth (conv2a, for XK_S2D)
struct X3Pair { half_t *hi = nullptr, *lo = nullptr; };   // the planes of one tensor
struct PassPlan {
    bool f32 = false, comp = false;          // the fp32 buffers (SFD2_PREC_F32 / F16X3); SFD2_PREC_F16C
    bool fuse = false, alias = false;        // fused kernels; the arena slots instead of one buffer per activation
    bool fused_stem = false, rb_fused = false;   // conv1a + conv1b in one kernel; plain fp16 ResBlocks on resblock_kernel (t1, t2 never stored)
    bool comp_rb = false;                    // SFD2_PREC_F16C: compensated ResBlocks (otherwise plain fp16 on the hi planes)
    int rb_inner = 0;                        // ... "rb_inner" in effect; rb23: 2 with ResBlock.conv2 + conv3 in rb23_c_kernel (t2 stays on chip)
    bool rb23 = false, generic_c = false, no_rf_c = false, fp6_filters = false;
    // SFD2_PREC_F16C: the corr records of every stored tensor from conv1a's output to convPa.0's / convDa.0's (Rec::None in other modes)
    Rec rec[T_COUNT] = {};
    Rec a3a_in = Rec::None;                  // a3a as conv3b reads it: None with "c3b_plain", also where conv3a still stores Half6 (SFD2_C3A_KEEP_CORR)
    bool a2a_s2d = false;                    // "s2d": conv2a's output stored space-to-depth, conv2b on conv2b_s2d_kernel
    bool ch = false, chp = false;            // compensated head branches ("comp_heads"); compensated detector branch ("comp_heads" or "comp_det")
    bool branches = false, sta_early = false, sta_side = false;   // detector branch on the side stream; ConvSta before the heads / on the side stream
    bool skip_head = false, skip_pb = false, skip_db = false, skip_da3 = false;   // layers left to sfd2_extract's post-processing
    bool sparse_desc = false, sparse_da3 = false, sparse_x3 = false;           // its sparse descriptor head: fp16, fp16 with convDa.3, f16x3
    bool sparse_da0 = false;                 // ... with sparse_da3: convDa.0 as well, on the 4 x 4 blocks around the key points' corners (run_network skips the layer)
    struct { int slot = -1; size_t off = 0; } at[T_COUNT];   // alias: each tensor's arena slot (-1: its own buffer) and its byte offset inside the slot
    int n_slots = 0;                         // ... slots in all, bytes per slot
    size_t slot_bytes = 0;
    bool x3_pp = false, x3_fast = false;     // f16x3: 3x3 layers on the three-pass kernels ("x3_pp"); the throughput path's plane hand-offs
    bool x3_stem = false, x3_rb = false;     // ... the fused three-pass stem (planes in X3_CHAIN_A); ResBlocks on the planes
    bool desc16 = false;                     // "x3_desc16": the descriptor branch in fp16 on the backbone's hi plane
    StrictConv sl[SL_COUNT];                 // f32 / f16x3: every layer's kernel and where its planes come from and go
};
PassPlan plan_pass(const sfd2_ctx *c, PassEntry entry, int H, int W, int top_k = 0, bool desc = false);
int ensure_workspace(sfd2_ctx *c, const PassPlan &p, int H, int W);   // allocates every buffer the pass touches and makes the filter forms it reads
int run_network(sfd2_ctx *c, const PassPlan &p, const float *img_dev, int normalise);   // launches only
// Where a tensor lives for the pass at hand (a non-owning view): the fp32 buffer on the strict family (convDa.0 with "x3_desc16": the fp16 output in the
// plane buffer), the arena slot on the throughput path, the fp16 buffer otherwise; the head outputs in their own buffers
inline DevPtr act_view(const sfd2_ctx *c, const PassPlan &p, int id)
{
    if (id >= T_COUNT) return id == T_PB ? c->logits : id == T_DB ? c->draw : c->sta;
    if (p.f32) return (id == T_DA0 && p.desc16) ? c->x3_da0_planes : c->act32[id];
    if (!p.alias || p.at[id].slot < 0) return c->act16[id];
    DevPtr v;
    v.p = c->arena.as<char>() + (size_t)p.at[id].slot * p.slot_bytes + p.at[id].off;
    return v;
}
inline int act_h(const sfd2_ctx *c, int id) { const int h[4] = {c->H, c->H2, c->H4, c->H8}; return h[kTensor[id].level]; }
inline int act_w(const sfd2_ctx *c, int id) { const int w[4] = {c->W, c->W2, c->W4, c->W8}; return w[kTensor[id].level]; }
inline size_t cand_capacity(size_t P1) { return std::min(std::max<size_t>(65536, P1 / 8), P1); }   // candidates the selection keeps for an image of P1 pixels
// one layer of the strict family on buffers given by hand (sfd2_extract's sparse head).  planes: in, the input's planes where s.planes_in; out, the output's (null pair: it went to the fp32 tensor)
int convf_at(sfd2_ctx *c, const StrictConv &s, const char *name, const ConvW &L, const DevPtr &in, int H, int W, const DevPtr &out, int Ho, int Wo,
             int relu, const float *res = nullptr, X3Pair *planes = nullptr);
// api_weights.hip
int ensure_strict_filters(sfd2_ctx *c, const PassPlan &p);   // SFD2_PREC_F16X3: the split filter forms (ConvW::wx3, wx3p, wsl) the plan's kernels read
// api_extract.hip
int copy_out(sfd2_ctx *c, void *dst, const void *src_dev, size_t bytes, int dst_on_device);
