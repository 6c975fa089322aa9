/*
 * libsfd2hip -- C-ABI of the MI355X-native SFD2 extract + match hot path.
 *
 * One shared object, plain pointers and sizes, no torch types.  Every entry point
 * names the reference interface (feixue94/sfd2, file:line) it replaces.  The
 * Python host side (sfd2_amd/) binds these with ctypes; INTEGRATION.md shows the
 * stub a maintainer of the reference would add.
 *
 * Conventions
 *   - return value 0 = ok, negative = error; text in sfd2_last_error() (thread local)
 *   - a context is bound to ONE device and ONE HIP stream; it is not thread-safe;
 *     use one context per GPU (any number per process)
 *   - the caller owns every input/output buffer; the library owns the context,
 *     packed weights and workspace only
 *   - `*_on_device` flags: 0 = host pointer (pageable ok), 1 = device pointer on the
 *     context's device
 *   - all calls are synchronous with respect to the host unless SFD2_FLAG_ASYNC is
 *     passed (then the caller synchronises the stream from sfd2_get_stream())
 */
#ifndef SFD2_HIP_H
#define SFD2_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfd2_ctx sfd2_ctx;

#define SFD2_DESC_DIM 128
#define SFD2_FLAG_ASYNC 1          /* do not synchronise the stream before returning     */
#define SFD2_FLAG_NO_STABILITY 2   /* use_stability = False (extract_localization.py:31) */
#define SFD2_FLAG_IMG_NORMALISED 4 /* input already passed through norm_RGB               */
#define SFD2_FLAG_IMG_U8_HWC 8     /* sfd2_extract: img is uint8 [H][W][3]; the device does the
                                    * astype(float32) / 255. of extract_localization.py:168,186 */
#define SFD2_FLAG_IMG_BGR 16       /* with IMG_U8_HWC: channel order is cv2's BGR (:162-165)    */
#define SFD2_FLAG_MATCH_OUT16 64    /* sfd2_match_batch: matches0 is int16 [k][n], scores0 IEEE half [k][n] -- the types the reference STORES (.short() /
                                    * .half(): hloc/match_features.py:114,118), converted on the device: a third of the bytes to the host and no
                                    * host-side cast of the [k][n] blocks in the batch driver's writer */
#define SFD2_FLAG_DESC_STORE64 128 /* sfd2_extract: `desc` is double [128][cap_out] -- the descriptors as the reference STORES them (transposed,
                                    * extract_localization.py:253, and float64, :269-272), columns >= the key-point count zero.  The cast is exact and the
                                    * values are those of the float [n][128] form; what moves to the device is the writer threads' cast + transposing
                                    * copy (4 MB per image: the host is the scarce side of an 8-GPU node, tools/host_soak.py).  cap_out >= 1 required. */
#define SFD2_FLAG_IMG_U8_X 32      /* with IMG_U8_HWC (sfd2_extract, sfd2_preprocess): pixels are FOUR bytes, the fourth ignored
                                    * (RGBX / BGRX: the in-memory layout of PIL's RGB images, which a decoder thread can hand
                                    * over without the interpreter-locked repacking to three bytes); unpacked on the device */

/* One named fp32 tensor of the reference state_dict (torch layout), host memory.
 * Replaces: model.load_state_dict(torch.load(p)['model'])  extract_localization.py:213-215 */
typedef struct {
    const char *name;   /* e.g. "conv1a.0.weight", "conv4.1.bn2.running_var" */
    const float *data;  /* contiguous fp32                                   */
    int32_t ndim;
    int64_t shape[4];
} sfd2_tensor;

/* matcher flavours */
#define SFD2_MATCH_HLOC 0       /* hloc/matchers/nearest_neighbor.py:38-57                  */
#define SFD2_MATCH_ITLOC_NNM 1  /* it_loc/matcher.py:122-130 (+ scores :113)               */
#define SFD2_MATCH_ITLOC_NNR 2  /* it_loc/matcher.py:165-194                               */
/* descriptor element types / layouts accepted by the matcher */
#define SFD2_DT_F32 0
#define SFD2_DT_F64 1
#define SFD2_DT_F16 2
#define SFD2_LAYOUT_ND 0  /* [n][dim]  (it_loc/matcher.py: [N,128])                        */
#define SFD2_LAYOUT_DN 1  /* [dim][n]  (hloc feature files: [128,N], match_features.py:99) */
/* similarity arithmetic */
#define SFD2_SIM_F16 0       /* fp16 operands, fp32 accumulate: |err| < 1e-3 on unit vectors */
#define SFD2_SIM_F16X2 1     /* hi+lo fp16 split (3 MFMA products): ~fp32 accuracy            */

typedef struct {
    int32_t flavour;          /* SFD2_MATCH_*                                                */
    int32_t do_mutual_check;  /* hloc only (default_conf, nearest_neighbor.py:28-32)          */
    float ratio_threshold;    /* hloc: <=0 means None.  itloc nnr: the Lowe ratio (0.9)       */
    float distance_threshold; /* hloc: <=0 means None                                         */
    int32_t sim_mode;         /* SFD2_SIM_*                                                   */
} sfd2_match_conf;

typedef struct {
    float ms_total;      /* last sfd2_extract / sfd2_match* call, device time (hip events) */
    float ms_backbone;   /* conv stack incl. heads                                          */
    float ms_post;       /* heat map, NMS, selection, descriptor sampling                   */
    float ms_match;
    int64_t n_candidates; /* N0 after NMS + threshold + border of the last extract          */
} sfd2_timings;

int sfd2_version(void);   /* 100 = rounds 1-4; 105 adds sfd2_extract_record_async, sfd2_desc_pack and host outputs with SFD2_FLAG_ASYNC; 106 adds sfd2_get_margin_status; 107 adds sfd2_get_relax_status (option "c3b_plain"); 108 adds sfd2_get_option, sfd2_device_pci_bus_id, SFD2_FLAG_DESC_STORE64; 109 adds the baseline JPEG decoder (sfd2_jpeg_*); 112 adds the SfM map (sfd2_verify_matches_batch, sfd2_build_tracks, sfd2_triangulate_tracks); 113 adds the pair selection (sfd2_pairs_retrieval, sfd2_pairs_covisibility, sfd2_pairs_poses); 114 adds sfd2_covis_clusters; 115 adds sfd2_covis_frames; 116 adds the VLAD global descriptors (sfd2_vlad_assign, sfd2_vlad_aggregate, sfd2_vlad_kmeans); 117 adds sfd2_relative_pose_batch; 118 adds sfd2_bundle_adjust; 119 adds the mapper's bookkeeping (sfd2_mapper_restrict, sfd2_mapper_filter, sfd2_mapper_visible, sfd2_mapper_assemble); 120 adds sfd2_fundamental_batch; 121 adds sfd2_homography_batch; 122 adds sfd2_match_guided_batch; 123 adds sfd2_bundle_adjust_cameras; 124 adds sfd2_spd_solve and sfd2_ba_conf.solver (SFD2_BA_SOLVER_DENSE) */
const char *sfd2_last_error(void);

int sfd2_ctx_create(int device, sfd2_ctx **out);
/* (version 108) PCI address "dddd:bb:dd.f" of a device and HIP's device count: what a one-process-per-GPU launcher needs to place a rank's decoder and writer
 * threads on the socket its GPU hangs off (/sys/bus/pci/devices/<address>/local_cpulist; sfd2_amd/sharding.py).  The reference leaves CPU placement to its
 * DataLoader worker processes (extract_localization.py:230-233).  out: at least 13 bytes; n_devices may be null. */
int sfd2_device_pci_bus_id(int device, char *out, int len, int *n_devices);
void sfd2_ctx_destroy(sfd2_ctx *ctx);
/* HIP stream (hipStream_t) all of this context's kernels are launched on. */
void *sfd2_get_stream(sfd2_ctx *ctx);

/* Folds Conv bias + BatchNorm (eval) into fp32 per-channel scale/shift, converts the
 * filters to fp16 MFMA-friendly layouts and uploads them.  Unknown names
 * (num_batches_tracked ...) are ignored; missing ones are an error.
 * Replaces: ResSegNetV2.__init__ / load_state_dict  (nets/sfd2.py:259-303). */
int sfd2_load_weights(sfd2_ctx *ctx, const sfd2_tensor *tensors, int n);

/* Arithmetic of the conv stack.  SFD2_PREC_F16 (default): fp16 MFMA operands, fp32 accumulate,
 * fp16 activations -- the throughput mode.  SFD2_PREC_F32: exact fp32 on the f32-input MFMA with
 * fp32 activations -- the parity mode (differs from the fp32 reference by summation order only).
 * SFD2_PREC_F16X3: the parity mode's buffers, filters and layer sequence with the 3x3 / 1x1 convolutions on the fp16
 * matrix path in three passes (operands split into hi + lo fp16 while they are staged; ~2^-22 per product against
 * fp32's 2^-24, fp32 accumulation) -- descriptors within 2e-5 of the reference like SFD2_PREC_F32, ~1.9x its speed.
 * SFD2_PREC_F16C: compensated fp16 -- the throughput mode's layout and kernels, with the backbone (conv1a .. conv4.2)
 * carrying a second 2-byte plane per activation and per filter that holds the fp16 rounding residual and the value at
 * fp8 precision; every backbone layer adds the two first-order error terms with ONE block-scaled MFMA per 32
 * channels (measured matrix time relative to the plain fp16 layer: 2.03x with fp8 operands, 1.52x with fp6 on both sides -- option
 * "fp6_acts", the default for conv2a / conv3a / conv3b; profiles/r04_mfma_probe.txt).  Operands then carry ~15 significant bits: descriptors within
 * 1e-3 of the fp32 reference (measured <= 5e-4), which is the tolerance BASELINE.json's north_star states.  The head
 * branches stay plain fp16 (they contribute 2.4e-4 on their own).  Option "comp_heads" extends it to convPa / convDa.
 * RANGE: the compensated tensors saturate at +-1792 in stored units and lose their correction bits below ~0.03 (the fp32
 * reference has neither limit): see "Range management" below for what keeps real checkpoints inside and reports it. */
#define SFD2_PREC_F16 0
#define SFD2_PREC_F32 1
#define SFD2_PREC_F16X3 2
#define SFD2_PREC_F16C 3
int sfd2_set_precision(sfd2_ctx *ctx, int mode);

/* Execution options of a context (the reference has none: its layers are stock torch modules).
 *   "fuse"      1 (default): sfd2_extract runs the fused kernels (stem, ResBlocks) over the aliased
 *               activation arena; 0: one kernel per layer, private buffers.
 *   "fuse_det"  0 (default): sfd2_det keeps every intermediate activation readable through
 *               sfd2_debug_activation; 1: sfd2_det runs the throughput path's fused kernels on private
 *               buffers (conv1a, conv4.b.bn1 / bn2 are then not materialised) -- how the parity tests
 *               reach the kernels sfd2_extract uses.
 *   "alias"     1 (default): the throughput path packs activations into the three-slot arena.
 *   "graphs"    0 (default) / 1: sfd2_extract_match (below) replays a cached hipGraph per geometry.
 *   "fuse_post" 1 (default): on the extract path, for H and W multiples of 8, detector soft-max + depth-to-space and
 *               stability weighting run as one kernel that writes the heat map (no score map in memory); 0: two
 *               kernels.  Bit-identical key points either way.
 *   "fuse_pb"   1 (default): with "fuse_post", convPb runs inside that kernel as well (the logits never reach memory).
 *   "sparse_desc" 1 (default): on the extract path (top_k > 0, 16 * top_k <= descriptor-map pixels) convDb runs after
 *               the selection on the 4 * top_k bilinear corner pixels only, the dense descriptor map is not written;
 *               0: dense map, then sampling.  Bit-identical descriptors either way.
 *   "branches"  0 (default) / 1: the detector branch (convPa, convPb, soft-max) runs on a second HIP stream beside
 *               the descriptor branch (convDa, convDb) -- they share only the backbone output (-1.7 % per extract).
 *   "sta_side"  0 (default) / 1: on the throughput path ConvSta (nets/sfd2.py:344: 256 -> 3 channels, a 63 MB read) runs on the context's side stream beside
 *               convPa.0 / convPa.3 / convDa.0 and joins in front of the heat-map kernel; a fork inside a captured hipGraph.  Bit-identical.  Not together with "branches".
 *   "comp_rb"   1 (default) / 0: SFD2_PREC_F16C compensates the three ResBlocks as well (descriptors within ~3e-4 of
 *               the fp32 reference); 0 runs them on the fused fp16 ResBlock kernel (~7e-4, still inside 1e-3, and faster).
 *   "rb_inner"  2 (default) / 1 / 0: SFD2_PREC_F16C stores the tensors INSIDE the ResBlocks as plain fp16 (1: the grouped
 *               conv's output, 2: conv1's output too, 0: both compensated); the block's input / output / skip path and all
 *               filters stay compensated.  These layers are bound by HBM bytes: 1.82 / 1.75 / 1.67 ms per 1600x1200 extract
 *               for 0 / 1 / 2, descriptors <= 3.5e-4 / 3.8e-4 / 4.9e-4 (tests assert 7e-4 for 1 and 2, 1e-3 everywhere).
 *   "x3_pp"     1 (default) / 0: SFD2_PREC_F16X3 on its throughput kernels -- 3x3 stride-1 layers on conv3x3_pp over pre-split hi / lo'
 *               planes, and on sfd2_extract (not sfd2_det) the fused three-pass stem, the streaming three-pass 1x1 kernel in the
 *               ResBlocks and the sparse descriptor head; 0 = the generic three-pass kernel everywhere (same tolerances, 1.6x slower).
 *   "auto_margin" 1 (default) / 0: the load-time self-check of SFD2_PREC_F16C (sfd2_get_margin_status below); set it BEFORE sfd2_load_weights.  It runs when
 *               the context is in SFD2_PREC_F16C at the load (or the first time it enters that precision afterwards) and leaves alone a key the caller set.
 *   "c3b_plain" -1 (default) / 0 / 1: conv3b without its correction chunks when the self-check finds the room (sfd2_get_relax_status below).
 *   "x3_desc16" 0 (default) / 1: SFD2_PREC_F16X3 on sfd2_extract with the DESCRIPTOR branch in plain fp16 -- convDa.0 as one fp16 pass over the
 *               backbone output's hi plane, convDa.3 / convDb on the sampled corners on the fp16 kernels (wherever the sparse descriptor head
 *               runs: 16 x top_k <= the 1/4-resolution map; elsewhere the option does nothing).  Key points and scores are this mode's own, bit for
 *               bit; descriptors within 1e-3 of the reference (measured <= 2.9e-4) instead of 2e-5; 2.46 -> 2.18 ms per 1600x1200 extract.  This
 *               is north_star's contract as written (key-point list equal up to near-ties, descriptors within 1e-3).  Python: precision "f16x3d".
 *   "fp6_filters" 0 (default) / 1: SFD2_PREC_F16C, conv2a / conv3a / conv3b: the correction filters as e2m3 (fp6) with one power-of-two
 *               scale per output channel instead of e4m3 (fp8 x fp6 scaled MFMA).  Same tolerance (descriptors <= 5.2e-4 measured),
 *               no measurable speed difference on MI355X: an experiment switch.
 *   "fp6_acts"  1 (default) / 0: SFD2_PREC_F16C, the correction records of the three tensors whose only reader is conv3x3_pp<comp>
 *               (conv1b's, conv2b's and conv3a's output) as block-scaled fp6: per pixel and 16 channels 32 e2m3 codes (residual * 2^11 and
 *               value of every channel) and one E8M0 exponent, written by the producers' epilogues (v_cvt_scalef32_2xpk16_fp6_f32); conv2a /
 *               conv3a / conv3b then correct with ONE fp6 x fp6 scaled MFMA per unit (33.5 cycles; 66 with fp8 on either side).
 *               -37 us per 1600x1200 extract (profiles/r04n_ab_fp6_acts.txt); descriptor rms error +1 .. 2.4 % of the fp8 records'
 *               (profiles/r04n_fp6_record_formats.txt), same 1e-3 tolerance asserted.  Decided per tensor: a producer that is not the
 *               tuned kernel ("fuse" 0, "no_rf_c", "generic_c") keeps its records fp8.  0 = fp8 records everywhere.
 *   "trunk_r1"  1 (default) / 0: SFD2_PREC_F16C (with "rb_inner" 2, "fuse_rb23", "fp6_acts"): conv3b's output and the ResBlocks' outputs carry ONE
 *               correction byte per channel -- the residual e4m3((x - fp16(x)) * 2^9) -- instead of the (residual, value) unit: 3 bytes per channel
 *               through the HBM-bound ResBlock kernels instead of 4.  The skip path never used the value byte; ResBlock.conv1 rebuilds it from
 *               the hi plane in registers (v_cvt_scalef32_pk_fp8_f16).  conv2 + conv3 + residual 92 -> 83 us per block, extract 1.468 -> 1.431 ms
 *               at 1600x1200; the rebuilt byte is e4m3(fp16(x) / 4) where the stored one was e4m3(x / 4): second-order, same tolerances.
 *   "s2d"       1 (default) / 0: SFD2_PREC_F16C on the throughput path (sfd2_extract / sfd2_extract_match; image sides multiples of 4, fp6_acts on):
 *               conv2a stores its output space-to-depth (four parity planes at quarter resolution) and conv2b runs as a stride-1 layer over
 *               it (conv2b_s2d_kernel.hip: filters through the LDS once per 512 pixels; conv3x3_rf<2,comp> loads 1.18 MB of filter fragments per
 *               128).  conv2b 147 -> 98 us at 1600x1200; same products, another fp32 summation order (descriptors within 5e-4 of the strided
 *               kernel's, both <= 1e-3 against the reference).  sfd2_det keeps the strided kernel (its tensors stay readable).
 *   "cu_limit"  0 (default) / n: persistent kernels of THIS context launch at most n blocks (experiment: with two streams, two kernels
 *               side by side on half the chip each measure the same throughput as taking turns on all of it).
 *   "auto_range" 1 (default) / 0: sfd2_load_weights calibrates the activation exponents on a built-in probe image (see
 *               sfd2_calibrate_range below); 0 = all exponents zero until the caller calibrates.  The probe is one 192x256
 *               SFD2_PREC_F32 pass (its fp32 workspace is released again); the exponents apply to SFD2_PREC_F16 as well as
 *               F16C, so both modes' results depend on what the context was calibrated on.
 *   "range_fallback" 1 (default) / 0: a synchronous sfd2_extract in SFD2_PREC_F16C that saturated a tensor is re-run in
 *               SFD2_PREC_F16X3 before it returns.
 *   "sparse_da3" 1 (default) / 0: on the extract path (with "sparse_desc"), convDa.3 runs on the 4 x K bilinear corner pixels of the
 *               selected key points only instead of the whole 1/4-resolution map (-77 us per 1600x1200 / top-4096 extract;
 *               descriptors within 4e-5 of the dense path's: another fp32 summation order).  0 = dense.
 *   "sparse_da0" 1 (default) / 0 / 2: with "sparse_da3" in effect (SFD2_PREC_F16 / F16C, plain descriptor branch), convDa.0 runs after the
 *               selection on the 4 x 4 blocks of its map that convDa.3's sparse form reads -- 16 x K pixels -- instead of densely inside the
 *               network pass; bit-identical outputs (the dense kernel's summation order at the same map size).  1 = where it pays:
 *               16 x top_k <= 0.6 of the 1/4-resolution map (1600x1200 / top-4096: on, -45 us; 640x480 / top-4096: dense); 0 = always
 *               dense; 2 = wherever the sparse head runs, whatever the size (tests, A/B runs).  After such an extract
 *               sfd2_debug_activation("convDa.0") answers "not materialised": the map is written at the key points' blocks only.
 *   "fuse_rb23" 1 (default) / 0: with rb_inner = 2, ResBlock.conv2 + conv3 + residual in one kernel (the grouped conv's output tile
 *               stays in LDS); 0 = two launches.  Bit-identical.
 *   "comp_heads" 0 (default) / 1: SFD2_PREC_F16C compensates the four 3x3 layers of the two head branches as well
 *               (descriptors ~1.5e-4 instead of ~3e-4, key points closer to the reference's list; ~0.25 ms more per image).
 *   "comp_det"  0 (default) / 1: SFD2_PREC_F16C compensates the detector branch's two 3x3 layers (convPa.0, convPa.3) only: the score goes
 *               through exp(), so its error is what moves key points; the descriptor branch stays plain (and keeps its sparse head).
 *   "no_rf_c"   0 (default) / 1: conv2b of SFD2_PREC_F16C on conv_igemm2<comp> instead of conv3x3_rf<comp> (A/B switch).
 *   "generic_c" 0 (default) / 1: SFD2_PREC_F16C layers all run on the generic compensated kernel (the reference
 *               implementation of that arithmetic) instead of the tuned kernels' compensated instantiations; the two
 *               differ by fp32 summation order only.
 * Unknown keys are an error. */
int sfd2_set_option(sfd2_ctx *ctx, const char *key, int value);
/* (version 108) What the context runs with for a key of sfd2_set_option: the value last set, or, for the keys the load-time self-check decides
 * ("rb_inner", "comp_heads", "c3b_plain"), its choice.  The reference has no counterpart (one fp32 arithmetic, nets/sfd2.py:313-326); a caller that keeps
 * several contexts per GPU copies these from the first so that all of them compute the same bits (sfd2_amd/model.py replica()). */
int sfd2_get_option(sfd2_ctx *ctx, const char *key, int *value);

/* ResSegNetV2.det (nets/sfd2.py:313-354).  x: [3][H][W] fp32, normalised image
 * (pass SFD2_FLAG_IMG_NORMALISED) or raw [0,1] RGB (normalised on the fly).
 * score [8*H8][8*W8], stability [H][W], desc [128][Hc][Wc] (L2-normalised), fp32.
 * Any output pointer may be NULL.  *hs,*ws receive the score map size. */
int sfd2_det(sfd2_ctx *ctx, const float *x, int x_on_device, int H, int W, int flags,
             float *score, float *stability, float *desc, int out_on_device,
             int *hs, int *ws, int *hc, int *wc);

/* extract_resnet_return, single scale, mask=None (nets/extractor.py:97-338):
 * img [3][H][W] fp32 in [0,1] (or uint8 [H][W][3] with SFD2_FLAG_IMG_U8_HWC: a quarter of the
 * host->device bytes, converted while conv1a stages its patch) -> up to top_k key points sorted
 * by score descending.
 * kpts_xy [cap][2] (x, y), scores [cap], desc [cap][128] fp32, cap = top_k (>0).
 * top_k <= 0 keeps every candidate (cap_out entries are then written at most).
 * nms_radius 4 and border 4 are the reference's constants (:143-144). */
int sfd2_extract(sfd2_ctx *ctx, const void *img, int img_on_device, int H, int W,
                 float conf_th, int top_k, int flags,
                 float *kpts_xy, float *scores, float *desc, int out_on_device,
                 int64_t cap_out, int *n_out);
/* extract_resnet_return with kwargs scales=[...] (nets/extractor.py:113-124,211-236,322-330):
 * every pyramid level int(H*s) x int(W*s) is the bilinear resize (align_corners=False) of the
 * normalised image; levels are merged by score on the device (top_k > 0) or concatenated in
 * scale order (top_k <= 0).  Key points are returned in original-image coordinates.
 * Reference behaviour kept: the 4-pixel border is tested against the ORIGINAL W, H in level
 * coordinates (:181-184).  scales: n_scales (<= 8) doubles.  Synchronous. */
int sfd2_extract_multiscale(sfd2_ctx *ctx, const void *img, int img_on_device, int H, int W,
                            const double *scales, int n_scales, float conf_th, int top_k, int flags,
                            float *kpts_xy, float *scores, float *desc, int out_on_device,
                            int64_t cap_out, int *n_out);

/* The decoder's uint8 image to the network's input, ImageDataset.__getitem__ (extract_localization.py:168-186):
 * astype(float32) -> cv2.resize(..., (new_w, new_h), INTER_CUBIC) when the size changes (the caller applies the
 * resize_max / resize_force rule of :172-177) -> HWC to CHW -> / 255.  img_hwc uint8 [H][W][3] (SFD2_FLAG_IMG_BGR:
 * cv2.imread order), host or device; out_chw_dev fp32 [3][new_h][new_w] on the device, ready for sfd2_extract.
 * The cubic kernel restates OpenCV's published float32 algorithm (a = -0.75, replicated border, horizontal
 * pass first); cv2 is not available to pin it against -- see oracle/oracle.py cv2_resize_cubic. */
int sfd2_preprocess(sfd2_ctx *ctx, const unsigned char *img_hwc, int on_device, int H, int W, int flags,
                    int new_h, int new_w, float *out_chw_dev);

/* After an SFD2_FLAG_ASYNC extract: number of key points, once the stream is idle. */
int sfd2_extract_count(sfd2_ctx *ctx, int *n_out);

/* Pipelined callers (the DataLoader-fed loop of extract_localization.py:230-250 with several images in flight):
 * sfd2_extract with SFD2_FLAG_ASYNC returns as soon as the image's work is queued; img may be a (pinned) host buffer -- it goes
 * through the context's copy stream into one of two staging slots, so the upload of image i + 1 overlaps the network of image i --
 * and the outputs may be (pinned) host buffers too: kpts_xy / scores / desc then receive the full capacity (top_k rows) by
 * asynchronous copies and hold the result once the stream is synchronised (an event recorded on sfd2_get_stream()).
 * sfd2_extract_record_async queues, behind that extract, the image's record into `rec` (pinned host or device memory):
 *   n            key points written (already clipped to the capacity)
 *   n_candidates NMS survivors (sfd2_timings.n_candidates of the synchronous call)
 *   saturated    bit i: tensor i (sfd2_range_tensor_name) reached the saturation of SFD2_PREC_F16C ON THIS IMAGE -- the caller
 *                repeats such an image with a synchronous sfd2_extract (which falls back to SFD2_PREC_F16X3 by itself)
 *   flags        bit 0: candidate buffer overflow (the synchronous call's error)
 * and folds the range maxima into the context's history (sfd2_get_range_status reports them); a tensor that saturated starts the next
 * image with a clean record, so `saturated` speaks for this image alone (tensors below the saturation keep their running maxima: that
 * is what spares the recording kernels their atomics).  One call per asynchronous extract, before the next extract is queued. */
typedef struct {
    int32_t n;
    int32_t n_candidates;
    uint32_t saturated;
    uint32_t flags;
} sfd2_extract_record;
int sfd2_extract_record_async(sfd2_ctx *ctx, sfd2_extract_record *rec, int rec_on_device);

/* extract_spp_feats_singlescale (extract.py:205-277), the older SuperPoint-style variant:
 * candidates heat >= conf_th, greedy grid NMS in score order (nms_fast, extract.py:17-84,
 * Chebyshev radius 4), border 4, descriptor sampling, NO top-K.  x is the NORMALISED image
 * (this variant's caller applies norm_RGB, extract.py:280-287).  Also returns, if non-NULL, the
 * heat map [H][W] and the dense L2-normalised descriptor map [128][Hc][Wc] the reference returns. */
int sfd2_extract_spp(sfd2_ctx *ctx, const float *x, int x_on_device, int H, int W, float conf_th, int flags,
                     float *kpts_xy, float *scores, float *desc, int64_t cap_out, int *n_out,
                     float *heat_out, float *desc_full_out);
/* extrat_spp_feats_multiscale (extract.py:87-201): the caller supplies the level schedule (nh, nw per level, emit = the
 * level passes the max_scale / max_size test; Python's float arithmetic and round() decide it); level 0 is the
 * NORMALISED image itself, every further level the bilinear resize of the PREVIOUS one.  Per emitted level: detector
 * score resized to the level (no stability weighting, as the reference), heat >= conf_th, greedy NMS radius 4,
 * confidence order, border 4 against the ORIGINAL W, H, descriptors sampled at level coordinates.  kpts_xy are in
 * LEVEL coordinates, concatenated level by level; level_count[l] = key points of level l.  Host buffers. */
int sfd2_extract_spp_levels(sfd2_ctx *ctx, const float *x, int x_on_device, int H, int W, int n_levels,
                            const int32_t *nh, const int32_t *nw, const int32_t *emit, float conf_th, int flags,
                            float *kpts_xy, float *scores, float *desc, int64_t cap_out, int32_t *level_count);
/* nms_fast on a dense map: kept[y][x] = heat if the pixel survives greedy NMS else 0 (host buffers) */
int sfd2_nms_fast(sfd2_ctx *ctx, const float *heat, int H, int W, float conf_th, int dist, float *kept_out);

/* Stage entry points (parity tests; each is the device kernel the pipeline uses). */
/* simple_nms(scores, 4) (nets/extractor.py:20-35): heat [H][W] -> nms [H][W] */
int sfd2_simple_nms(sfd2_ctx *ctx, const float *heat, int H, int W, int radius, float *nms_out);
/* NMS + threshold + border + sort + top-K (nets/extractor.py:157-183,322-326).  conf_th must be >= 0 and not NaN, here
 * and in every extract call (an error otherwise): candidates are the scores > conf_th, ordered by their float bits, which
 * is the order of the values only for non-negative scores.  More candidates than min(max(65536, H*W/8), H*W) is the
 * "candidate buffer overflow" error; the context stays usable.  At most cap_out rows are written. */
int sfd2_select_keypoints(sfd2_ctx *ctx, const float *heat, int H, int W, float conf_th,
                          int radius, int border, int top_k,
                          float *kpts_xy, float *scores, int64_t cap_out, int *n_out);
/* bilinear descriptor sampling + renormalisation (nets/extractor.py:199-208);
 * desc_map [128][hc][wc] fp32 (raw or normalised), kpts [n][2] */
int sfd2_sample_descriptors(sfd2_ctx *ctx, const float *desc_map, int hc, int wc, int nh, int nw,
                            const float *kpts_xy, int n, float *desc_out);
/* heat = resize(score) * stability (nets/extractor.py:137-141), with stability from the
 * 3-class logits sta [3][hc][wc] (nets/sfd2.py:345-347).  score [hs][ws]. sta may be NULL. */
int sfd2_heatmap(sfd2_ctx *ctx, const float *score, int hs, int ws, const float *sta, int hc, int wc,
                 int H, int W, float *heat_out);
/* Reads back an intermediate activation of the last sfd2_det/sfd2_extract as fp32 [c][h][w].
 * Names: conv1a bn1b conv2a bn2b conv3a bn3b conv4.0.bn1 conv4.0.bn2 conv4.0 conv4.1 conv4.2
 *        convPa.0 convPa convDa.0 convDa convPb convDb ConvSta */
int sfd2_debug_activation(sfd2_ctx *ctx, const char *name, float *out, int64_t cap, int *c, int *h, int *w);

/* Nearest-neighbour matcher.  d0 [n0 x dim], d1 [n1 x dim] (dtype/layout as given).
 * matches0 [n0] int64 (-1 = no match); scores0 [n0] fp32 (hloc: (sim+1)/2 or 0;
 * itloc: raw row maximum).  Replaces NearestNeighbor._forward
 * (hloc/matchers/nearest_neighbor.py:38-57) and Matcher.forward (it_loc/matcher.py:91-119).
 * Ratio modes (hloc ratio_threshold > 0, SFD2_MATCH_ITLOC_NNR) compare the best similarity s1 of a row (column) with the
 * second best s2, counted with multiplicity: a duplicated maximum has s2 == s1 and passes no ratio below 1.  A direction
 * with ONE candidate (n1 == 1 for the rows, n0 == 1 for the columns) has no second best, where the reference's topk(2)
 * raises: here s2 = -inf, so d1 = 2 (1 - s2) = +inf and that direction's ratio test passes -- hloc: d0 <= r^2 inf,
 * it_loc: sqrt(d0) / (inf + 1e-8) = 0 <= ratio; the distance threshold and the other direction decide as usual.
 * n1 == 0: every row -1 with score 0. */
int sfd2_match(sfd2_ctx *ctx, const void *d0, int n0, const void *d1, int n1, int dim,
               int dtype, int layout, int on_device, const sfd2_match_conf *conf,
               int64_t *matches0, float *scores0, int out_on_device);

/* Segmented (block-masked) matcher: rows [seg0[s], seg0[s+1]) of d0 against rows [seg1[s], seg1[s+1]) of d1 only, all
 * n_seg segments in one launch -- the same-label phase of the label-aware matcher once both sets are ordered by label
 * (Matcher.matcher_with_label, it_loc/matcher.py:239-264).  seg0 / seg1: n_seg + 1 ascending HOST offsets starting at
 * 0 and ending at n0 / n1 (an empty range on either side = no matches for that segment's rows).
 * matches0 [n0]: global row of d1 or -1; scores0 [n0] as sfd2_match, within the segment. */
int sfd2_match_segments(sfd2_ctx *ctx, const void *d0, int n0, const void *d1, int n1, int dim,
                        int dtype, int layout, int on_device, int n_seg, const int32_t *seg0, const int32_t *seg1,
                        const sfd2_match_conf *conf, int64_t *matches0, float *scores0, int out_on_device);

/* One descriptor set handed to the batched matcher. */
typedef struct {
    const void *data;   /* [n][dim] or [dim][n], see layout                          */
    int32_t n;
    int32_t dtype;      /* SFD2_DT_*                                                  */
    int32_t layout;     /* SFD2_LAYOUT_*                                              */
    int32_t on_device;  /* 0 host, 1 device                                           */
    const int32_t *rows; /* HOST array of n_rows row indices into data, or NULL: only these rows
                          * take part and matches0 reports THEIR indices -- the db_3D_ids != -1
                          * mask and the index remap of feature_matching
                          * (it_loc/localize_cv2.py:531-534,557-559) done on the device     */
    int32_t n_rows;
    int32_t reserved;
} sfd2_desc_set;

/* One descriptor set into the matcher's resident form: fp16 [n][128] row-major on the device (columns beyond dim zero), made by
 * the conversion kernel every sfd2_match* call runs on its inputs -- a set packed once and then passed as (SFD2_DT_F16,
 * SFD2_LAYOUT_ND, on_device = 1) gives bit-identical matches to passing the original every time.  This is what lets a batch
 * driver keep the database sets of hloc/match_features.py:99-105 (read + .float() + .cuda() per PAIR there) resident in HBM
 * across pairs.  src->rows selects / orders rows as in sfd2_match_batch; dst_f16_dev: caller-owned device buffer of
 * (rows ? n_rows : n) * 128 * 2 bytes.  flags: SFD2_FLAG_ASYNC (a host source must stay valid until the stream is synchronised). */
int sfd2_desc_pack(sfd2_ctx *ctx, const sfd2_desc_set *src, int dim, void *dst_f16_dev, int flags);

/* One query against k database images in one launch (the localiser's inner loop,
 * it_loc/localize_cv2.py:705-715 -> feature_matching :511-560 -> Matcher.forward).
 * matches0 [k][q->n] int64, scores0 [k][q->n] fp32.  Device-resident fp16 [n][128] database
 * sets (SFD2_DT_F16, SFD2_LAYOUT_ND, sim_mode SFD2_SIM_F16) are used in place, no conversion. */
int sfd2_match_batch(sfd2_ctx *ctx, const sfd2_desc_set *q, const sfd2_desc_set *db, int k, int dim,
                     const sfd2_match_conf *conf, int64_t *matches0, float *scores0, int out_on_device,
                     int flags);

/* One query unit as pure stream work: sfd2_extract (SFD2_FLAG_ASYNC semantics, device-resident image
 * and outputs, capacity top_k > 0) followed by sfd2_match_batch of the top_k descriptor rows against k
 * device-resident database sets -- the per-query body of the localiser (it_loc/localizer.py:87 ->
 * localize_cv2.py:705-715) with nothing returned to the host; the caller synchronises sfd2_get_stream().
 * With sfd2_set_option("graphs", 1) the unit is captured into a hipGraph the second time a geometry
 * (sizes, pointers, matcher conf) is seen and replayed afterwards; up to 16 geometries are cached per
 * context (least recently used evicted), entries are dropped when the workspace is reallocated.
 * k = 0 extracts only. */
int sfd2_extract_match(sfd2_ctx *ctx, const void *img_dev, int H, int W, float conf_th, int top_k, int flags,
                       float *kpts_xy, float *scores, float *desc, const sfd2_desc_set *db, int k, int dim,
                       const sfd2_match_conf *conf, int64_t *matches0, float *scores0);

int sfd2_get_timings(sfd2_ctx *ctx, sfd2_timings *out);

/* ---- Range management of the fp16 family (SFD2_PREC_F16 / SFD2_PREC_F16C).  The reference computes in fp32 and has nothing
 * of the kind (nets/sfd2.py:313-326); this is what keeps a reduced-precision path honest on a checkpoint nobody has seen.
 *
 * The compensated mode stores every backbone tensor as fp16 + two e4m3 bytes with FIXED scalings (value / 4, fp16 residual
 * * 512) and saturates it at 1792 (so that neither byte can overflow e4m3's 448).  That suits tensors whose largest
 * entry lies between ~0.2 and ~500 (descriptors within 5e-4 of the fp32 reference there; 1.1e-3 at 0.03; garbage above
 * 1792: tools/conditioning_sweep.py).  Three mechanisms keep it there and make leaving it visible:
 *   1. sfd2_load_weights normalises every filter per output channel by a power of two (the factor goes into the folded
 *      BatchNorm scale: exact), so no channel's filter sits in fp16's subnormals or below the e4m3 units' range.
 *   2. Activation exponents: the stored tensor of group g is 2^e[g] times the network's tensor, the factors folded into
 *      the layers' scale / shift constants (exact: powers of two commute with ReLU and with fp32 rounding).
 *      sfd2_calibrate_range measures every group's largest |x| on an image (one pass in SFD2_PREC_F32) and sets e[g] so
 *      that it lands at 16; sfd2_load_weights does that on a built-in probe image (option "auto_range", default 1).
 *   3. Range status: every kernel that writes a tensor of the compensated mode records the largest value it WOULD have
 *      stored, before the saturation.  sfd2_get_range_status reports them; a synchronous sfd2_extract that saturated a
 *      tensor is re-run in SFD2_PREC_F16X3 before it returns (option "range_fallback", default 1) and counted.
 *      Asynchronous calls (SFD2_FLAG_ASYNC, sfd2_extract_match) cannot look at the counters: the caller polls
 *      sfd2_get_range_status at its own synchronisation points, or takes the per-image record of sfd2_extract_record_async.
 *      A fallback's first SFD2_PREC_F16X3 pass allocates that mode's workspace: captured sfd2_extract_match graphs of the
 *      context are dropped and re-captured on their next use.  Recalibration (sfd2_calibrate_range, sfd2_set_act_exponents)
 *      clears the recorded maxima: they were measured under the previous scaling. */
#define SFD2_RANGE_TENSORS 17
#define SFD2_RANGE_GROUPS 14
typedef struct {
    int32_t n_tensors;                        /* SFD2_RANGE_TENSORS                                                      */
    float max_stored[SFD2_RANGE_TENSORS];     /* largest value in front of the saturation, as stored (x 2^exponent), since
                                                 the last reset; 0 = the tensor was not produced by a recording kernel   */
    float max_value[SFD2_RANGE_TENSORS];      /* the same in the network's own units                                      */
    int32_t exponent[SFD2_RANGE_TENSORS];     /* the tensor's activation exponent                                         */
    uint32_t saturated;                       /* bit i: tensor i reached 1792 (values were clamped: results are wrong)    */
    uint32_t low;                             /* bit i: tensor i never exceeded 2^-5 (the corr units have lost their bits:
                                                 plain-fp16 accuracy, ~2e-3 on descriptors)                               */
    int32_t fallbacks;                        /* synchronous extracts re-run in SFD2_PREC_F16X3 since the context exists  */
} sfd2_range_status;
int sfd2_get_range_status(sfd2_ctx *ctx, sfd2_range_status *out, int reset);
/* "conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4.b.t1", "conv4.b.t2", "conv4.b" (b = 0..2), "convPa.0", "convDa.0" */
const char *sfd2_range_tensor_name(int i);
/* img: [3][H][W] fp32 as for sfd2_det (flags: SFD2_FLAG_IMG_NORMALISED).  Replaces the exponents; captured graphs are dropped. */
int sfd2_calibrate_range(sfd2_ctx *ctx, const float *img, int img_on_device, int H, int W, int flags);
/* exps / maxima [SFD2_RANGE_GROUPS]: conv1a, conv1b, conv2a, conv2b, conv3a, trunk (conv3b's and the ResBlocks' outputs share the
 * skip path), t1 of block 0..2, t2 of block 0..2, convPa.0, convDa.0.  maxima = what the last calibration measured. */
int sfd2_get_act_exponents(sfd2_ctx *ctx, int32_t *exps, float *maxima, int cap, int *n);
int sfd2_set_act_exponents(sfd2_ctx *ctx, const int32_t *exps, int n /* SFD2_RANGE_GROUPS, or 0 = all zero */);
/* Self-check of SFD2_PREC_F16C at sfd2_load_weights (option "auto_margin", default 1).  The compensated mode's distance from the fp32 reference depends on
 * the checkpoint (heavy-tailed or biased filters cost margin), so the library measures it: the built-in probe image goes through sfd2_det in SFD2_PREC_F32 and
 * in SFD2_PREC_F16C, and while the largest difference of the two L2-normalised descriptor maps exceeds the target (7e-4) the accuracy options are turned on in
 * order of cost -- "rb_inner" = 0 (+6 % per extract), "comp_heads" = 1 (+24 %), both -- the first that meets the target stays.  errs4: the probe error with the
 * options as they were / rb_inner = 0 / comp_heads = 1 / both (-1 = not measured: an earlier one met the target); *choice: 0..3 = which of them the context
 * now runs (bit 0: rb_inner = 0, bit 1: comp_heads = 1), -1 = no self-check has run (option off, auto_range off).  sfd2_set_option afterwards overrides. */
int sfd2_get_margin_status(sfd2_ctx *ctx, float *errs4, int *choice, float *target);
/* Option "c3b_plain" (version 107).  conv3b (nets/sfd2.py:276-278: 256 -> 256 channels at 1/4 resolution, the largest layer of the backbone) can run its
 * K loop over the fp16 plane of conv3a's output alone -- no correction chunks, the output's correction bytes still come from the fp32 accumulators, and
 * conv3a then writes no correction plane: -62 us of that layer's 184 at 1600x1200 for ~1.4x the descriptor error (tools/relax_study.py).  It is never on
 * unverified: with the default -1 the self-check above also measures the probe WITH it and keeps it only when the options as set met the target and the probe
 * with it stays inside 6.5e-4 (tighter than the 7e-4 that buys margin back: an extraction's error is up to 1.1x the probe's, profiles/r06p_relax_probe_8seeds.txt);
 * 1 forces it (the self-check then runs every candidate with it), 0 forbids it.  *err_plain: the probe error with it (-1 = not measured),
 * *c3b_plain: whether the context now runs it.  A rounds-1..5 caller sees the same entry points; the descriptor tolerance (1e-3) is unchanged. */
int sfd2_get_relax_status(sfd2_ctx *ctx, float *err_plain, int *c3b_plain);

/* Blocks until every kernel queued on the context's stream has finished. */
int sfd2_sync(sfd2_ctx *ctx);

/* Per-launch device timing (HIP events recorded on the context's stream around every kernel
 * launch of sfd2_det / sfd2_extract / sfd2_match*).  The reference only has wall-clock prints
 * (it_loc/localizer.py:151-156); this is what bench.py's roofline block is computed from.
 * max_steps = number of extract/match calls that may be in flight before the table is read. */
typedef struct {
    char name[32];      /* layer / stage, e.g. "conv3b", "nms_select"                       */
    char kernel[48];    /* kernel family, e.g. "conv_igemm<3,1,256>"                        */
    double flops;       /* algorithmic FLOPs of ONE launch (2*MAC; 0 for non-GEMM stages)    */
    double bytes;       /* algorithmic HBM bytes of ONE launch (each tensor once)            */
    double ms_total;    /* summed device time of all recorded launches                       */
    int32_t launches;
} sfd2_layer_timing;
int sfd2_set_profiling(sfd2_ctx *ctx, int max_steps /* 0 = off */);
/* Only launches whose kernel-family label contains `substr` are timed (NULL or "" = all): every
 * event pair costs ~2-4 us of stream time, so a timed run brackets the kernel it reports on only. */
int sfd2_set_profile_filter(sfd2_ctx *ctx, const char *substr);
int sfd2_get_layer_timings(sfd2_ctx *ctx, sfd2_layer_timing *out, int cap, int *n);

/* ------------------------------------------------------------------------------------------------ baseline JPEG decoder
 * The decoder in front of extract_localization.py:162-165 (cv2.imread / PIL), on the device.  The host parses the headers
 * (sfd2_jpeg_parse) and removes the byte stuffing in place (sfd2_jpeg_prepare); the device does the Huffman decoding
 * (self-synchronising, one lane per 256-bit subsequence), dequantisation, the accurate integer IDCT, "fancy" chroma
 * upsampling and YCbCr -> RGB with libjpeg's fixed-point arithmetic, so the pixels equal what PIL / libjpeg(-turbo) decode
 * with its defaults (JDCT_ISLOW, do_fancy_upsampling).  Output: uint8 [H][W][4] RGBX on the device, what sfd2_extract /
 * sfd2_preprocess take with SFD2_FLAG_IMG_U8_HWC | SFD2_FLAG_IMG_U8_X and img_on_device = 1.
 *
 * Supported (anything else: supported = 0 and a reason, the caller decodes that file on the CPU):
 *   SOF0 / SOF1, 8-bit, Huffman; one interleaved scan; 1 component (grey, replicated to RGB) or 3 components YCbCr with
 *   luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; any DQT / DHT; DRI with RSTn markers. */
#define SFD2_JPEG_OK 0
#define SFD2_JPEG_NOT_JPEG 1      /* no SOI, or not a JPEG at all (PNG, ...)                         */
#define SFD2_JPEG_TRUNCATED 2     /* a segment, the scan or the EOI lies beyond the end of the data   */
#define SFD2_JPEG_PROGRESSIVE 3   /* SOF2 / SOF6                                                      */
#define SFD2_JPEG_ARITHMETIC 4    /* SOF9 .. SOF15 (except the hierarchical lossless ones), DAC       */
#define SFD2_JPEG_PRECISION 5     /* sample precision other than 8 bits                              */
#define SFD2_JPEG_COLOUR 6        /* 2 or 4 components, Adobe transform 0, 'R','G','B' component ids  */
#define SFD2_JPEG_SAMPLING 7      /* a sampling layout other than the ones above                     */
#define SFD2_JPEG_MULTI_SCAN 8    /* more than one scan, or a scan that does not hold every component */
#define SFD2_JPEG_PROCESS 9       /* lossless or hierarchical SOF, DNL                                */
#define SFD2_JPEG_MALFORMED 10    /* inconsistent segments, tables, RSTn sequence or image size        */
typedef struct {
    int32_t width, height;
    int32_t n_components;
    int32_t h_samp[3], v_samp[3];
    int32_t restart_interval;     /* MCUs per restart interval (DRI), 0 = none                        */
    int32_t supported;            /* 1: sfd2_jpeg_decode can take this file                           */
    int32_t reason;               /* SFD2_JPEG_* (0 when supported)                                   */
    int32_t mcus_x, mcus_y;       /* MCU grid of the scan                                             */
    int32_t n_intervals;          /* restart intervals of the scan (RSTn markers + 1)                 */
    int32_t n_blocks;             /* 8x8 blocks the scan codes                                        */
    int64_t file_bytes;           /* n of the parse                                                   */
    int64_t scan_begin, scan_end; /* entropy-coded data: [scan_begin, scan_end), scan_end = offset of the EOI */
    int64_t prepared_cap;         /* bytes the buffer handed to sfd2_jpeg_prepare must hold (>= file_bytes) */
    /* filled by sfd2_jpeg_prepare */
    int64_t prepared_bytes;       /* bytes of the prepared buffer sfd2_jpeg_decode uploads             */
    int32_t n_lanes;              /* Huffman decoding lanes                                           */
    int32_t prepared;             /* 1 once the buffer holds the prepared form                        */
} sfd2_jpeg_info;

/* Reads the headers and walks the entropy-coded data (RSTn count and order, the EOI behind the scan).  Host only: no context,
 * no device.  Never reads outside [data, data + n).  Returns 0 with info->supported = 1, or -1 with info->reason set (and
 * width / height / components when the frame header was read) and the reason in sfd2_last_error(). */
int sfd2_jpeg_parse(const uint8_t *data, int64_t n, sfd2_jpeg_info *info);

/* In place: buf holds the file in [0, info->file_bytes) and has room for info->prepared_cap bytes.  Parses again, moves the
 * entropy-coded data to the front with the byte stuffing (FF 00) and the RSTn markers removed, each restart interval starting
 * on a byte, and writes behind it the Huffman lookup tables, quantisation tables and the lane table.  The headers are
 * overwritten.  Returns 0 (info->prepared = 1, info->prepared_bytes set) or -1. */
int sfd2_jpeg_prepare(uint8_t *buf, int64_t cap, sfd2_jpeg_info *info);

/* Decodes a prepared buffer (data: host, n >= info->prepared_bytes) into out_rgbx_dev (device, uint8 [H][W][4], out_cap bytes).
 * *status (host, or device when status_on_device) receives 0, or a non-zero anomaly mask (bit 0 invalid Huffman code or a run
 * past coefficient 63, bit 1 block count / restart interval mismatch, bit 2 an interval that does not end at its marker,
 * bit 3 the lanes did not synchronise) -- the pixels are then not valid and the caller decodes the file on the CPU.
 * SFD2_FLAG_ASYNC: data may be pinned host memory; it goes up through the context's copy stream, the decode is queued on
 * sfd2_get_stream() and *status is written in stream order (a host status must then be pinned too); data and status must stay
 * valid until the stream has passed.  Without the flag the call synchronises and returns -1 on a non-zero status.
 * The decoder's scratch belongs to the context, grows on demand and is separate from the network's workspace. */
int sfd2_jpeg_decode(sfd2_ctx *ctx, const uint8_t *data, int64_t n, const sfd2_jpeg_info *info, int flags,
                     uint8_t *out_rgbx_dev, int64_t out_cap, uint32_t *status, int status_on_device);

/* ------------------------------------------------------------------------------------------------ absolute pose
 * pycolmap.absolute_pose_estimation (it_loc/localize_cv2.py:731, :390) and pycolmap.pose_refinement (:451) on the device, for
 * many problems of any sizes in one launch.  LO-RANSAC over P3P (Lambda Twist) with fp32 scoring on centred coordinates and an
 * fp64 local optimisation, then the refinement of pycolmap's RefineAbsolutePose with the intrinsics fixed: Cauchy loss (1 px
 * scale) on the reprojection error in pixels over the RANSAC inliers.  Results depend on the problem and the seed only (not on
 * the batch, its order or the scheduling) and are bit-reproducible.
 * Pose convention (COLMAP): x_cam = R(qvec) X + tvec, qvec = (w, x, y, z) unit, world to camera; points2D are pixel coordinates
 * as given (the localiser adds its +0.5, localize_cv2.py:647). */
#define SFD2_CAM_SIMPLE_PINHOLE 0   /* f, cx, cy                          (COLMAP camera model ids and parameter order) */
#define SFD2_CAM_PINHOLE 1          /* fx, fy, cx, cy                                                                      */
#define SFD2_CAM_SIMPLE_RADIAL 2    /* f, cx, cy, k                                                                        */
#define SFD2_CAM_OPENCV 4           /* fx, fy, cx, cy, k1, k2, p1, p2                                                      */
typedef struct {
    int32_t n;                      /* correspondences                                                                     */
    int32_t model;                  /* SFD2_CAM_*; any other id is an error                                                */
    const double *points2D;         /* host [n][2] pixels                                                                  */
    const double *points3D;         /* host [n][3] world                                                                   */
    double params[8];               /* the model's parameters in COLMAP order (unused tail ignored)                       */
    int32_t width, height;
    double max_error_px;            /* RANSAC inlier threshold in pixels (the `thresh` of localize_cv2.py:731)             */
} sfd2_pose_problem;
typedef struct {
    double min_inlier_ratio;        /* limits max_num_trials as COLMAP's RANSAC does                                       */
    int64_t min_num_trials, max_num_trials;
    double confidence;
    uint64_t seed;                  /* trial i of every problem draws its sample from (seed, i) only                      */
} sfd2_pose_conf;
typedef struct {
    int32_t success;                /* 0: fewer than 4 correspondences or no pose with >= 3 inliers (outputs finite)       */
    int32_t num_inliers;            /* RANSAC inliers (absolute pose) or the mask's count (refinement)                     */
    int32_t num_trials;             /* RANSAC trials run (0 for the refinement)                                            */
    int32_t reserved;
    double qvec[4];                 /* w, x, y, z                                                                          */
    double tvec[3];
} sfd2_pose_result;

/* k problems; results[k]; inlier_mask_u8: host, sum(n) bytes, the problems' RANSAC inlier masks concatenated in problem order.
 * Non-finite input or a bad model / parameter is an error (-1).  flags: 0.  Replaces pycolmap.absolute_pose_estimation(mkpq,
 * mp3d, cfg, thresh), it_loc/localize_cv2.py:731. */
int sfd2_absolute_pose_batch(sfd2_ctx *ctx, const sfd2_pose_problem *problems, int k, const sfd2_pose_conf *conf,
                             sfd2_pose_result *results, uint8_t *inlier_mask_u8, int flags);
/* The refinement alone, from qvec_tvec_in[k][7] (qw qx qy qz tx ty tz) over the inliers of inlier_mask_u8 (host, sum(n) bytes,
 * problems concatenated).  max_error_px is not used.  flags: 0.  Replaces pycolmap.pose_refinement(tvec, qvec, mkpq, mp3d,
 * inlier_mask, cfg), it_loc/localize_cv2.py:451. */
int sfd2_pose_refine_batch(sfd2_ctx *ctx, const sfd2_pose_problem *problems, int k, const double *qvec_tvec_in,
                           const uint8_t *inlier_mask_u8, sfd2_pose_result *results, int flags);

/* ------------------------------------------------------------------------------------------------ absolute pose, unknown focal
 * (version 125) pycolmap.absolute_pose_estimation's estimate_focal_length / refine_focal_length / refine_extra_params.
 * Focal samples: with S = num_focal_length_samples, sample i = 0..S is the given camera with its focal parameters (f, or fx and fy)
 * multiplied by a_i = min_ratio + (max_ratio - min_ratio) (i / S)^2; the principal point and the extras stay as given.
 * Sweep: every (problem, sample) runs the solver's RANSAC (no refinement) at its camera, threshold (max_error_px / mean focal)^2 at
 * that camera, with the call's seed, confidence and min_inlier_ratio and both trial limits clipped to sweep_max_num_trials.
 * Select: more inliers, then the smaller residual sum in squared pixels (fp32), then the smaller i; no sample with 3 inliers:
 * success 0 and the camera as given.  Main run: sfd2_absolute_pose_batch at the winning camera, bit for bit (num_trials, mask, pose).
 * Refinement with intrinsics (either refine flag): Levenberg-Marquardt as the solver's (Cauchy at 1 px, fp64, <= 100 iterations) over
 * the pose and, with additive steps, the focal group and / or the extra group (k; k1 k2 p1 p2), never the principal point; a trial
 * state with a non-finite word or a focal length that is not positive or outside [min_ratio, max_ratio] x the given one is rejected
 * like a cost increase.  At most three refinements: after one, every point is re-scored in fp64 pixels (depth > 0, squared error <=
 * max_error_px^2); if the count grew, the next refinement runs over the new mask.  The pose, the camera and the mask reported are the
 * last refinement's, so num_inliers >= ransac_num_inliers.  Without estimate_focal_length the main run uses the given camera. */
typedef struct {
    int32_t estimate_focal_length, refine_focal_length, refine_extra_params;   /* 0 / non-zero                                */
    int32_t num_focal_length_samples;      /* S, 1..64 (COLMAP: 30)                                                        */
    double min_focal_length_ratio;         /* 0 < min <= max, finite (COLMAP: 0.2 and 5)                                   */
    double max_focal_length_ratio;
    int64_t sweep_max_num_trials;          /* >= 1: the sweep's cap on min_num_trials and max_num_trials                   */
    int64_t reserved[2];                   /* zero; anything else is an error                                              */
} sfd2_pose_focal_conf;
typedef struct {
    int32_t success;
    int32_t num_inliers;            /* the count of the mask the reported pose was refined over                            */
    int32_t num_trials;             /* of the main run                                                                     */
    int32_t reserved;
    double qvec[4];
    double tvec[3];
    double params[8];               /* the camera's parameters in COLMAP order after the sweep and the refinement          */
    int32_t focal_sample;           /* the winning sample, -1 without a sweep or when no sample has 3 inliers              */
    int32_t ransac_num_inliers;     /* the main run's RANSAC count                                                         */
    double focal_factor;            /* a_focal_sample (1 without a sweep)                                                  */
} sfd2_pose_focal_result;
typedef struct {
    int32_t cnt, num_trials;        /* the sample's RANSAC inliers (0 below 3) and trials                                  */
    float sum_px;                   /* (sum fm) fm in fp32: the winner's residual sum, fm the sample's mean focal in fp32  */
    int32_t pad;
} sfd2_pose_sweep_record;

/* As sfd2_absolute_pose_batch, with the options of focal_conf.  sweep_out: NULL, or host [k][S + 1] records (written with
 * estimate_focal_length only). */
int sfd2_absolute_pose_focal_batch(sfd2_ctx *ctx, const sfd2_pose_problem *problems, int k, const sfd2_pose_conf *conf,
                                   const sfd2_pose_focal_conf *focal_conf, sfd2_pose_focal_result *results, uint8_t *inlier_mask_u8,
                                   sfd2_pose_sweep_record *sweep_out, int flags);
/* As sfd2_pose_refine_batch, with the camera's groups that focal_conf's refine flags select: one refinement from the given pose over
 * the given mask, no re-scoring.  The ratios bound the focal lengths; the sweep's fields are checked and not used. */
int sfd2_pose_refine_camera_batch(sfd2_ctx *ctx, const sfd2_pose_problem *problems, int k, const double *qvec_tvec_in,
                                  const uint8_t *inlier_mask_u8, const sfd2_pose_focal_conf *focal_conf,
                                  sfd2_pose_focal_result *results, int flags);

/* ------------------------------------------------------------------------------------------------ relative pose
 * The calibrated two-view geometry of a matched pair, which COLMAP estimates inside matches_importer (hloc/triangulation.py:114,
 * hloc/reconstruction.py:145), for many pairs of any sizes in one launch: LO-RANSAC over the five-point solver with fp64 scoring
 * on the squared Sampson error, a refinement of the 5 pose parameters on the same error over the RANSAC inliers, and the choice
 * among the four decompositions by the points in front of both cameras.  Essential matrix only: a rotation-only
 * pair shows in the triangulation angles.  Results depend on the pair and the seed only and are bit-reproducible. */
typedef struct {
    int32_t n;                      /* correspondences                                                                     */
    int32_t model0, model1;         /* SFD2_CAM_* of the two images; any other id is an error                              */
    int32_t reserved;
    double params0[8], params1[8];  /* the models' parameters in COLMAP order (unused tail ignored)                       */
    const double *points2D_0;       /* host [n][2] pixels in image 0                                                       */
    const double *points2D_1;       /* host [n][2] pixels in image 1                                                       */
    double max_error_px;            /* inlier threshold in pixels: (max_error_px / mean of the two mean focal lengths)^2
                                       bounds the squared Sampson error in normalised coordinates                         */
} sfd2_two_view_problem;
typedef struct {
    double min_inlier_ratio;        /* limits max_num_trials as COLMAP's RANSAC does                                       */
    int64_t min_num_trials, max_num_trials;
    double confidence;
    uint64_t seed;                  /* trial i of every pair draws its sample from (seed, i) only                         */
    int32_t min_num_inliers;        /* success needs at least this many RANSAC inliers                                     */
    int32_t reserved;
} sfd2_two_view_conf;
typedef struct {
    int32_t success;                /* 1: num_inliers >= min_num_inliers and a decomposition has points in front of both
                                       cameras; 0 otherwise, also with fewer than 5 correspondences (outputs finite)       */
    int32_t num_inliers;            /* RANSAC inliers                                                                      */
    int32_t num_trials;             /* RANSAC trials run                                                                   */
    int32_t reserved;
    double qvec[4];                 /* w, x, y, z: camera 0 to camera 1, x1 = R(qvec) x0 + tvec                            */
    double tvec[3];                 /* unit length                                                                         */
    double E[9];                    /* [tvec]x R(qvec), row-major: x1^T E x0 = 0 in normalised coordinates                 */
} sfd2_two_view_result;

/* k pairs; results[k]; inlier_mask_u8 and tri_angle_deg: host, sum(n) entries, the pairs concatenated in order: the RANSAC inlier
 * mask, and the angle in degrees at the (midpoint-)triangulated point between the rays to the two centres, NaN for an outlier
 * and for a point not in front of both cameras.  Non-finite input or a bad model / parameter is an error (-1).  flags: 0. */
int sfd2_relative_pose_batch(sfd2_ctx *ctx, const sfd2_two_view_problem *problems, int k, const sfd2_two_view_conf *conf,
                             sfd2_two_view_result *results, uint8_t *inlier_mask_u8, double *tri_angle_deg, int flags);

/* ------------------------------------------------------------------------------------------------ fundamental matrix (version 120)
 * The uncalibrated two-view geometry of a matched pair, which COLMAP estimates for a pair without a trusted focal length
 * (EstimateUncalibrated), for many pairs of any sizes in one launch: LO-RANSAC over the seven-point solver with fp64 scoring on the
 * squared Sampson error in pixels, then a refinement of 7 parameters of a rank-2 chart on the same error over the RANSAC inliers
 * (DESIGN.md 16).  No camera, no pose, no cheirality test; H is sfd2_homography_batch below, and the decision between E, F and H
 * is the caller's (sfd2_amd.two_view.decide_two_view_geometry).  Results depend on the pair and the seed
 * only and are bit-reproducible.  sfd2_two_view_conf is taken as sfd2_relative_pose_batch takes it (sample size 7). */
typedef struct {
    int32_t n;                      /* correspondences                                                                     */
    int32_t reserved;
    const double *points2D_0;       /* host [n][2] pixels in image 0                                                       */
    const double *points2D_1;       /* host [n][2] pixels in image 1                                                       */
    double max_error_px;            /* inlier threshold in pixels: max_error_px^2 bounds the squared Sampson error         */
} sfd2_fundamental_problem;
typedef struct {
    int32_t success;                /* 1: num_inliers >= min_num_inliers; 0 otherwise, also with fewer than 7 correspondences
                                       or point sets without extent (F = 0, mask 0, num_trials 0)                          */
    int32_t num_inliers;            /* RANSAC inliers                                                                      */
    int32_t num_trials;             /* RANSAC trials run                                                                   */
    int32_t reserved;
    double F[9];                    /* row-major, x1^T F x0 = 0 in pixels; rank 2, unit Frobenius norm, the first entry of
                                       largest magnitude positive; all 0 without a result                                  */
} sfd2_fundamental_result;

/* k pairs; results[k]; inlier_mask_u8: host, sum(n) bytes, the pairs' RANSAC inlier masks concatenated in order.  Non-finite input
 * is an error (-1).  flags: 0. */
int sfd2_fundamental_batch(sfd2_ctx *ctx, const sfd2_fundamental_problem *problems, int k, const sfd2_two_view_conf *conf,
                           sfd2_fundamental_result *results, uint8_t *inlier_mask_u8, int flags);

/* ------------------------------------------------------------------------------------------------ homography (version 121)
 * The homography of a matched pair, which COLMAP estimates next to E and F for every pair to tell a plane or a panorama from a
 * general scene, for many pairs of any sizes in one launch: LO-RANSAC over the closed-form four-point solver with fp64 scoring on the
 * squared one-sided transfer error |x1 - pi(H x0)|^2 in image 1, then a refinement of 8 parameters (the entry of largest magnitude
 * held constant) on the same error over the RANSAC inliers.  No camera, no decomposition, no pose.  Results depend
 * on the pair and the seed only and are bit-reproducible.  sfd2_two_view_conf is taken as sfd2_relative_pose_batch takes it
 * (sample size 4). */
typedef struct {
    int32_t n;                      /* correspondences                                                                     */
    int32_t reserved;
    const double *points2D_0;       /* host [n][2] pixels in image 0                                                       */
    const double *points2D_1;       /* host [n][2] pixels in image 1                                                       */
    double max_error_px;            /* inlier threshold in pixels: max_error_px^2 bounds the squared transfer error        */
} sfd2_homography_problem;
typedef struct {
    int32_t success;                /* 1: num_inliers >= min_num_inliers; 0 otherwise, also with fewer than 4 correspondences
                                       or point sets without extent (H = 0, mask 0, num_trials 0)                          */
    int32_t num_inliers;            /* RANSAC inliers                                                                      */
    int32_t num_trials;             /* RANSAC trials run                                                                   */
    int32_t reserved;
    double H[9];                    /* row-major, x1 ~ H x0 in pixels; unit Frobenius norm, the first entry of largest
                                       magnitude positive; all 0 without a result                                          */
} sfd2_homography_result;

/* k pairs; results[k]; inlier_mask_u8: host, sum(n) bytes, the pairs' RANSAC inlier masks concatenated in order.  Non-finite input
 * is an error (-1).  flags: 0. */
int sfd2_homography_batch(sfd2_ctx *ctx, const sfd2_homography_problem *problems, int k, const sfd2_two_view_conf *conf,
                          sfd2_homography_result *results, uint8_t *inlier_mask_u8, int flags);

/* ------------------------------------------------------------------------------------------------ guided matching (version 122)
 * A pair matched AGAIN under its two-view model, what COLMAP has next to its two-view estimation as guided_matching:
 * sim[i][j] = d0_i . d1_j where the key points i and j agree with the model within max_error_px, -inf elsewhere, and on that masked
 * matrix the rule of SFD2_MATCH_HLOC -- per row the best value at the first index on a tie, the second best counted with multiplicity
 * among the gated candidates only, ratio / distance / mutual tests as sfd2_match applies them.  A row without a gated candidate gives
 * -1 and score 0; a row (column) with one gated candidate passes the ratio test.  The gate, on per-point records computed once per key
 * point in fp64 from M and rounded to fp32, the test itself in fp32:
 *   F: l = F (x0, y0, 1), m = F^T (x1, y1, 1), r = x1 l0 + y1 l1 + l2; the pair passes iff r^2 <= max_error_px^2 (l0^2 + l1^2 + m0^2 + m1^2)
 *      (the four-term Sampson error of sfd2_fundamental_batch without the division)
 *   H: p = pi(H (x0, y0, 1)); iff p is finite and |x1 - p|^2 <= max_error_px^2 (the one-sided transfer error of sfd2_homography_batch)
 * Both directions of the mutual check evaluate ONE function on the same records, so they see the same mask bit for bit.  An essential
 * matrix is served through F = K1^-T E K0^-1.  Only SFD2_MATCH_HLOC with SFD2_SIM_F16; key points as stored (no +0.5: M must be in the
 * same pixel frame as xy0 / xy1). */
#define SFD2_GUIDE_F 0
#define SFD2_GUIDE_H 1
typedef struct {
    sfd2_desc_set d0, d1;        /* as sfd2_match_batch takes them (host or device-resident packed fp16); rows must be NULL */
    const float *xy0, *xy1;      /* host [n][2] pixels */
    int32_t model, reserved;     /* SFD2_GUIDE_* */
    double M[9];                 /* row-major; F: x1^T F x0 = 0, H: x1 ~ H x0, pixels */
    double max_error_px;
} sfd2_guided_problem;

/* k pairs in one launch sequence; matches0 / scores0: host, sum(d0.n) entries, the pairs concatenated in order.  Non-finite key points
 * or matrix, max_error_px <= 0, an unknown model, a flavour other than SFD2_MATCH_HLOC, a sim_mode other than SFD2_SIM_F16 or a
 * non-NULL rows give -1 with sfd2_last_error() naming the pair and the field.  d0.n == 0 or d1.n == 0 is no error (rows -1, score 0).
 * The candidates of a direction are swept in `splits` chunks of ceil(n / splits) rounded up to 32; the result does not depend on
 * splits.  flags: 0. */
int sfd2_match_guided_batch(sfd2_ctx *ctx, const sfd2_guided_problem *problems, int k, int dim, const sfd2_match_conf *conf,
                            int64_t *matches0, float *scores0, int flags);

/* ------------------------------------------------------------------------------------------------ 2D-3D assembly
 * Matches -> 2D-3D correspondences for a batch of jobs in one call: the per-key-point loops of it_loc/localize_cv2.py:571-632
 * (match_cluster_2D) and :286-360 (pose_refinement_covisibility, with the reprojection gate).  A job is one query against its k
 * database images.  For image i = 0..k-1, query key point idx ascending, a match is dropped when matches0 < 0, when the image's
 * table has no 3D point for the matched key point, when the point's track length is < obs_th, when an earlier image of the job
 * already took the same 3D point for this idx (the entry is made BEFORE the gate: a gated-out point still blocks its later
 * duplicates), and, with gate != 0, when the point projected with (qvec, tvec, camera) in fp64 lies more than radius pixels from
 * the key point (compared as `error > radius`, so a NaN error is kept; no depth test; the key point WITHOUT the +0.5 the output
 * adds).  What survives is appended: order = image ascending, then idx ascending.  The order comes from prefix sums, never from
 * atomics, so a job's output bytes depend on the job alone, not on the batch, its order or the run. */
typedef struct {
    const double *xyz;              /* device [n_points][3]                                                                */
    const int32_t *track_len;       /* device [n_points]: len(points3D[id].image_ids)                                      */
    int32_t n_points;
    int32_t reserved;
} sfd2_point_table;
typedef struct {
    const int32_t *point_rows;      /* device [n1]: key point -> row of the point table, or -1                             */
    int32_t n1;                     /* 0: the image is skipped (localize_cv2.py:293-296, :577-580)                         */
    int32_t match_row;              /* row of the job's matches0 that holds this image's matches; -1: an image without
                                     * matches (one the <= 3 rule kept away from the matcher, :537-538)                     */
} sfd2_assemble_image;
typedef struct {
    const int64_t *matches0;        /* device [match_rows][n], as sfd2_match_batch(out_on_device = 1) writes it: indices into
                                     * the image's UNMASKED key points, < 0 = none.  An index >= n1 is an input error.      */
    const sfd2_assemble_image *images;  /* host [k]                                                                         */
    int32_t k, n, match_rows;
    int32_t inputs_on_device;       /* keypoints / scores: 0 host, 1 device                                                */
    const float *keypoints;         /* [n][2], as the feature store holds them                                             */
    const float *scores;            /* [n] or NULL (output scores are then 0)                                              */
    double obs_th;                  /* compared as (double)track_len < obs_th                                              */
    int32_t gate;                   /* 0: no reprojection gate (the cluster stage)                                         */
    int32_t model;                  /* gate: SFD2_CAM_*, params, pose and radius                                           */
    double params[8];
    double qvec[4], tvec[3];        /* qvec is normalised as the reference's scipy call does                               */
    double radius;
    int32_t capacity;               /* rows of every output buffer below                                                   */
    int32_t m;                      /* OUT: correspondences of the job (also when m > capacity)                            */
    int32_t status;                 /* OUT: 0, or bits: 1 a match index >= n1, 2 a table entry >= n_points, 4 m > capacity  */
    int32_t reserved;
    double *points2D;               /* OUT [m][2]: key point + 0.5                                                         */
    double *points3D;               /* OUT [m][3]                                                                          */
    int32_t *point_row;             /* OUT [m]: row of the point table                                                     */
    int32_t *query_idx;             /* OUT [m]                                                                             */
    int32_t *image_idx;             /* OUT [m]: position in images[]                                                       */
    float *score;                   /* OUT [m]                                                                             */
    int32_t *image_counts;          /* OUT, HOST [k]: correspondences per image                                            */
} sfd2_assemble_job;
/* Runs on sfd2_get_stream() behind whatever was queued there (an sfd2_match_batch with SFD2_FLAG_ASYNC and out_on_device = 1
 * needs no synchronisation in between) and synchronises before it returns.  out_on_device: the six row buffers of every job are
 * device (1) or host (0) memory; m, status and image_counts are always host.  Returns -1 when any job has a non-zero status (every
 * job's m and status are filled; a job with a non-zero status writes no rows, the others are complete) or on a bad argument.
 * flags: 0. */
int sfd2_assemble_2d3d(sfd2_ctx *ctx, const sfd2_point_table *map, sfd2_assemble_job *jobs, int n_jobs, int out_on_device, int flags);

/* ------------------------------------------------------------------------------------------------ SfM map
 * The map hloc/triangulation.py gets from `colmap matches_importer` and `colmap point_triangulator`, with the reference poses and the
 * intrinsics fixed (triangulation.py:134-142): known-pose verification of the matches, tracks as connected components, robust
 * multi-view triangulation with a per-point refinement.  Every call takes concatenated arrays plus offsets, runs on
 * sfd2_get_stream(), synchronises before it returns, returns -1 on a bad argument or non-finite input and reports per-item trouble
 * through status words.  Results depend on the inputs (and the seed) only: not on the batch, its order or the scheduling. */
typedef struct {
    int32_t model, reserved;        /* SFD2_CAM_*; any other id is an error                                                */
    double params[8];               /* the model's parameters in COLMAP order                                              */
    double qvec[4], tvec[3];        /* world to camera, qvec = (w, x, y, z), normalised by the call                         */
} sfd2_tri_view;
/* Known-pose geometric verification.  views[n_views]; kp_offsets[n_views + 1] and keypoints[kp_offsets[n_views]][2] (host, as the
 * feature store holds them: the call adds COLMAP's +0.5, triangulation.py:64); pair p matches view pair_views[2p] against
 * pair_views[2p + 1] with matches[match_offsets[p] .. match_offsets[p + 1])[2] = (key point in the first, key point in the second),
 * host, IN/OUT.  A match survives when its point-to-epipolar-line distance in normalised coordinates is <= max_error_px / mean focal
 * in both images; a pair with fewer than min_num_inliers survivors loses all.  Rejected entries become (-1, -1); entries that come
 * in negative stay rejected, and a pair of a view with itself loses all.  pair_counts[p]: the survivors before the min_num_inliers rule; pair_status[p]: 0 or 1 = an index
 * beyond the image's key points (the call then returns -1).  flags: 0. */
int sfd2_verify_matches_batch(sfd2_ctx *ctx, const sfd2_tri_view *views, int n_views, const int64_t *kp_offsets, const float *keypoints,
                              const int32_t *pair_views, const int64_t *match_offsets, int n_pairs, int32_t *matches,
                              double max_error_px, int min_num_inliers, int32_t *pair_counts, int32_t *pair_status, int flags);
/* Connected components over n_nodes nodes and edges[n_edges][2] (host; an edge with a negative end is skipped).  labels[n_nodes]:
 * the smallest node of the node's component.  The components of two or more nodes as a CSR ordered by label, nodes ascending:
 * track_offsets (capacity n_nodes / 2 + 2) and track_nodes (capacity n_nodes), their lengths in *n_tracks (+ 1) and *n_track_nodes.
 * status[0]: 0, 1 = an edge beyond n_nodes, 2 = not converged within max_rounds hooking rounds (both return -1, nothing else is
 * written); status[1]: rounds run.  flags: 0. */
int sfd2_build_tracks(sfd2_ctx *ctx, int64_t n_nodes, const int32_t *edges, int64_t n_edges, int max_rounds, int32_t *labels,
                      int32_t *track_offsets, int32_t *track_nodes, int64_t *n_tracks, int64_t *n_track_nodes, int32_t *status, int flags);
#define SFD2_TRI_MAX_POINTS 4       /* points per track                                                                    */
typedef struct {
    double min_tri_angle_deg;           /* hypotheses and the final filter (1.5)                                           */
    double create_max_angle_error_deg;  /* inliers of a hypothesis (2)                                                     */
    double filter_max_reproj_error;     /* completion and filter, pixels (4)                                               */
    uint64_t seed;                      /* a long track's hypothesis h of pass p is drawn from (seed, label, 64 p + h) only */
    int32_t max_refine_iterations;      /* Levenberg-Marquardt steps per refinement (50)                                   */
    int32_t reserved;
} sfd2_tri_conf;
/* Track t holds the observations track_offsets[t] .. track_offsets[t + 1] (host arrays): obs_view (index into views; the
 * observations of one view must be consecutive, as sfd2_build_tracks' ascending nodes are) and obs_xy (key point as stored, the call
 * adds +0.5); track_labels[t] keys the random draws.  Up to SFD2_TRI_MAX_POINTS points per track, slot s = t * SFD2_TRI_MAX_POINTS +
 * pass: xyz[s][3], error[s] (mean reprojection error, pixels), n_obs[s] (0: no point); obs_point[o]: the pass that took observation
 * o, or -1; track_status[t]: 0, 1 = fewer than two observations, 2 = a refinement left the finite numbers.  A track that returns to
 * a view after leaving it is refused (-1, the error names the observation); the views of a track may come in any order.  flags: 0. */
int sfd2_triangulate_tracks(sfd2_ctx *ctx, const sfd2_tri_view *views, int n_views, const int64_t *track_offsets, const int64_t *track_labels,
                            int n_tracks, const int32_t *obs_view, const float *obs_xy, const sfd2_tri_conf *conf, double *xyz, double *error,
                            int32_t *n_obs, int8_t *obs_point, int32_t *track_status, int flags);

/* ------------------------------------------------------------------------------------------------ bundle adjustment
 * Levenberg-Marquardt over camera poses and 3D points with the points eliminated (Schur complement) and the reduced camera system
 * solved by matrix-free preconditioned conjugate gradients, block-Jacobi preconditioned, or (version 124,
 * conf.solver = SFD2_BA_SOLVER_DENSE) formed as a dense matrix and solved by a Cholesky factorisation: an exact
 * step instead of an inexact one, for up to SFD2_BA_DENSE_MAX_VIEWS views, sfd2_bundle_adjust only.  Conventions of the
 * SfM-map section: host arrays, the call runs on sfd2_get_stream() and synchronises before it returns, returns -1 with
 * sfd2_last_error() set on a bad argument, non-finite input or an index out of range (the message names the first offending index).
 * fp64, fixed-order sums, no floating-point atomics: the result depends on the inputs (and the flags) only, two calls give the same
 * bytes.  Intrinsics are constant in sfd2_bundle_adjust; sfd2_bundle_adjust_cameras refines them. */
#define SFD2_BA_LOSS_TRIVIAL 0
#define SFD2_BA_LOSS_CAUCHY 1          /* rho(s) = c^2 log(1 + s / c^2), c = loss_scale, as an IRLS weight rho'(s)               */
#define SFD2_BA_ST_GRADIENT 0          /* result status: max |g| <= gradient_tolerance                                          */
#define SFD2_BA_ST_FUNCTION 1          /*   relative cost change of an accepted step <= function_tolerance                      */
#define SFD2_BA_ST_MAX_ITERATIONS 2    /*   max_iterations steps were tried                                                      */
#define SFD2_BA_ST_LAMBDA 3            /*   lambda grew past 1e12: no further progress (the best accepted state is returned)    */
#define SFD2_BA_ST_NONFINITE 4         /*   the cost of the given state is not finite: nothing was written                      */
#define SFD2_BA_FLAG_POINT_LANE 1      /* every point's sums by one lane, whatever its track length                             */
#define SFD2_BA_FLAG_POINT_WAVE 2      /* every point's sums by one wave (default: a wave beyond 64 observations, else a lane)  */
#define SFD2_BA_SOLVER_PCG 0           /* conf.solver: matrix-free preconditioned conjugate gradients (a zeroed conf)            */
#define SFD2_BA_SOLVER_DENSE 1         /*   the reduced camera system as a dense fp64 matrix, Cholesky; result.pcg_iterations = 0 */
#define SFD2_BA_DENSE_MAX_VIEWS 2048   /* the dense solver's limit: S is stored as a full [6 n_views]^2 fp64 matrix, 1.2 GB here  */
typedef struct {
    int32_t max_iterations;         /* LM steps tried at the most (100)                                                    */
    int32_t pcg_max_iterations;     /* conjugate-gradient iterations per step at the most (100)                            */
    int32_t loss;                   /* SFD2_BA_LOSS_*                                                                      */
    int32_t pcg_batch;              /* PCG iterations queued between two reads of the stopping word; 0: 16                 */
    double gradient_tolerance;      /* 1e-10                                                                               */
    double function_tolerance;      /* 0                                                                                   */
    double pcg_tolerance;           /* PCG stops at |r_k| <= pcg_tolerance |r_0| (0.1)                                     */
    double loss_scale;              /* c of the Cauchy loss, pixels                                                        */
    double initial_lambda;          /* 1e-4                                                                                */
    int32_t solver;                 /* SFD2_BA_SOLVER_* (0: PCG); any other value is refused                               */
    int32_t reserved[3];            /* zero                                                                                */
} sfd2_ba_conf;
typedef struct {
    int32_t status;                 /* SFD2_BA_ST_*                                                                        */
    int32_t iterations;             /* LM steps tried                                                                      */
    int32_t accepted_steps;
    int32_t pcg_iterations;         /* over all steps                                                                      */
    double initial_cost, final_cost;   /* 1/2 sum rho(|r|^2), pixels^2                                                      */
    double gradient_max;            /* max |g| at the returned state                                                       */
    double lambda;                  /* the damping the next step would have used                                           */
} sfd2_ba_result;
/* views[n_views]: IN/OUT poses (a view that is constant or has no observation keeps its words bit for bit; the others come back
 * with a unit qvec, w >= 0); view_constant[n_views] and point_constant[n_points]: non-zero = fixed; xyz[n_points][3]: IN/OUT;
 * point p holds the observations point_offsets[p] .. point_offsets[p + 1]: obs_view (index into views) and obs_xy[.][2] (pixels as
 * given: a model's xys already carry the +0.5).  The residual is the camera model's projection of R X + t minus obs_xy, without a
 * depth test.  obs_error[n_obs]: the reprojection error of every observation at the returned state, pixels. */
int sfd2_bundle_adjust(sfd2_ctx *ctx, sfd2_tri_view *views, int n_views, const uint8_t *view_constant, double *xyz, int n_points,
                       const uint8_t *point_constant, const int64_t *point_offsets, const int32_t *obs_view, const double *obs_xy,
                       const sfd2_ba_conf *conf, sfd2_ba_result *result, double *obs_error, int flags);
/* The same adjustment with camera intrinsics among the unknowns.  cameras[n_cameras]: IN/OUT; view_camera[n_views]
 * maps every view to one (one shared camera, one per view, or anything between).  refine selects COLMAP's three parameter groups; a
 * group the model does not have contributes nothing, refine == 0 is a constant camera.  The views' own model / params words are not
 * read; on return they hold their camera's final values.  A camera that is constant, or whose views have no observation, comes back
 * bit for bit, as does every camera when no step was accepted.  A trial state with a non-finite camera parameter or a focal length
 * <= 0 is rejected as a non-finite cost is.  Every other argument, the result and the flags: as sfd2_bundle_adjust.  -1 also on a
 * camera index out of range, unknown refine bits, a bad model or non-finite parameters (the message names the first offending index). */
#define SFD2_BA_REFINE_FOCAL 1         /* f, or fx and fy (SIMPLE_* models: the one f)                                          */
#define SFD2_BA_REFINE_PRINCIPAL 2     /* cx, cy                                                                                */
#define SFD2_BA_REFINE_EXTRA 4         /* k; k1, k2, p1, p2                                                                     */
typedef struct {
    int32_t model, refine;          /* SFD2_CAM_*, SFD2_BA_REFINE_* bits                                                   */
    double params[8];               /* the model's parameters in COLMAP order, IN/OUT                                      */
} sfd2_ba_camera;
int sfd2_bundle_adjust_cameras(sfd2_ctx *ctx, sfd2_ba_camera *cameras, int n_cameras, const int32_t *view_camera, sfd2_tri_view *views,
                               int n_views, const uint8_t *view_constant, double *xyz, int n_points, const uint8_t *point_constant,
                               const int64_t *point_offsets, const int32_t *obs_view, const double *obs_xy, const sfd2_ba_conf *conf,
                               sfd2_ba_result *result, double *obs_error, int flags);

/* (version 124) A x = b for a symmetric positive definite A by the dense solver's kernels: a blocked fp64 Cholesky factorisation on
 * the device and two triangular solves.  Host arrays; A is [n][n] row-major and only its lower triangle is read; 1 <= n <= 6 *
 * SFD2_BA_DENSE_MAX_VIEWS.  Returns 0 with *info = 0 and x[n] written; 0 with *info = k + 1 when pivot k is the first that is <= 0 or
 * not finite (A is not positive definite to working precision), x untouched; -1 with sfd2_last_error() set on a bad argument or a
 * non-finite entry of the lower triangle or of b.  Fixed-order sums: two calls give the same bytes. */
int sfd2_spd_solve(sfd2_ctx *ctx, const double *A, int n, const double *b, double *x, int32_t *info);

/* ------------------------------------------------------------------------------------------------ incremental mapper
 * The bookkeeping between relative pose, absolute pose, triangulation and bundle adjustment in a round of sfd2_amd.reconstruction
 * (DESIGN.md section 15).  Conventions of the SfM-map section: host arrays in and out, the calls run on sfd2_get_stream() and
 * synchronise before they return, and return -1 with sfd2_last_error() set on a bad argument, non-finite input or an index out of
 * range (the message names the first offending index).  The track table is sfd2_build_tracks': track t holds the observations
 * track_offsets[t] .. track_offsets[t + 1] of obs_view (index into the n_views views) and obs_xy (key point as stored, float32).
 * Integer work is exact; atomics are integer adds only, sums have a fixed order: results depend on the inputs (and the flags) only. */
#define SFD2_MAPPER_FLAG_TRACK_LANE 1  /* every track's (point's) observations by one lane, whatever its length                */
#define SFD2_MAPPER_FLAG_TRACK_WAVE 2  /* every track's (point's) by one wave (default: a wave beyond 64 observations, else a lane) */
/* The tracks with observations in at least two distinct views that registered[n_views] marks (non-zero), in track order, each
 * with its registered observations in observation order.  sub_track (capacity n_tracks): the source track; sub_offsets (capacity
 * n_tracks + 1); sub_obs (the source observation index), sub_view and sub_xy[.][2] (capacity track_offsets[n_tracks]); the two lengths
 * in *n_sub_tracks and *n_sub_obs.  flags: 0 or one SFD2_MAPPER_FLAG_*; both mappings give the same bytes. */
int sfd2_mapper_restrict(sfd2_ctx *ctx, const int64_t *track_offsets, int n_tracks, const int32_t *obs_view, const float *obs_xy,
                         const uint8_t *registered, int n_views, int32_t *sub_track, int64_t *sub_offsets, int32_t *sub_obs, int32_t *sub_view,
                         float *sub_xy, int64_t *n_sub_tracks, int64_t *n_sub_obs, int flags);
/* Point p holds the observations point_offsets[p] .. point_offsets[p + 1]: obs_view and obs_xy[.][2] (double pixels as
 * sfd2_bundle_adjust takes them: the +0.5 applied).  e = |project(cam, R X + t) - xy|; obs_keep[o] = depth > 0 and e <=
 * max_reproj_error (a NaN is not kept).  point_live[p] = kept observations in two distinct views and point_angle[p] >=
 * min_tri_angle_deg; point_error[p]: the mean e of the kept (0 when none), summed in observation order (lane) or as 64 strided partial
 * sums joined by a fixed tree (wave); point_angle[p]: the largest angle at X between the rays to the centres of two kept
 * observations, degrees (NaN below two kept).  fp64.  flags: 0 or one SFD2_MAPPER_FLAG_*. */
int sfd2_mapper_filter(sfd2_ctx *ctx, const sfd2_tri_view *views, int n_views, const double *xyz, int n_points, const int64_t *point_offsets,
                       const int32_t *obs_view, const double *obs_xy, double max_reproj_error, double min_tri_angle_deg, uint8_t *obs_keep,
                       uint8_t *point_live, double *point_error, double *point_angle, int flags);
/* The points are point_track[n_points] (their track, ascending, at most SFD2_TRI_MAX_POINTS per track) with point_live[n_points].
 * counts[n_views]: for an unregistered view the sum, over its observations, of the live points of the observation's track (the
 * correspondences sfd2_mapper_assemble would write for it); 0 for a registered view.  flags: 0. */
int sfd2_mapper_visible(sfd2_ctx *ctx, const int64_t *track_offsets, int n_tracks, const int32_t *obs_view, const uint8_t *registered, int n_views,
                        const int32_t *point_track, const uint8_t *point_live, int n_points, int64_t *counts, int flags);
/* The 2D-3D problems of the views cand[k]: per candidate every (observation of the view, live point of its track) pair, ordered by
 * observation index and then by point index.  offsets[k + 1]; rows offsets[c] .. offsets[c + 1] of points2D[.][2] (stored xy + 0.5),
 * points3D[.][3] (the point's xyz), src_obs and src_point.  capacity: rows the four arrays hold; when offsets[k] is larger the call
 * returns -1 with only the offsets written (the sum of sfd2_mapper_visible's counts over the candidates is the size).  flags: 0. */
int sfd2_mapper_assemble(sfd2_ctx *ctx, const int64_t *track_offsets, int n_tracks, const int32_t *obs_view, const float *obs_xy, int n_views,
                         const int32_t *point_track, const uint8_t *point_live, const double *xyz, int n_points, const int32_t *cand, int k,
                         int64_t capacity, int64_t *offsets, double *points2D, double *points3D, int32_t *src_obs, int32_t *src_point, int flags);

/* ------------------------------------------------------------------------------------------------ pair selection
 * The image pairs the stages above are run on: hloc/pairs_from_retrieval.py (query-db pairs by global-descriptor similarity),
 * hloc/pairs_from_covisibility.py (db-db pairs by shared 3D points) and hloc/pairs_from_poses.py (pairs by distance under a
 * rotation gate).  All three are "the k best of n scored candidates per row" under ONE total order: the better score first, then
 * the smaller candidate index.  A row's result depends on the inputs only -- not on tiling, split count, batch or scheduling.
 * Conventions of the SfM-map section: concatenated arrays plus offsets (host memory unless said otherwise), the calls run on
 * sfd2_get_stream() and synchronise before they return, and return -1 with sfd2_last_error() set on a bad argument or non-finite
 * input.  1 <= k <= SFD2_PAIRS_MAX_K (sfd2_pairs_poses, whose lists are per image and not per strip of rows: <=
 * SFD2_PAIRS_POSES_MAX_K).  Rows are best first; slots a row does not fill hold index -1. */
#define SFD2_PAIRS_MAX_K 256
#define SFD2_PAIRS_POSES_MAX_K 1024
#define SFD2_PAIRS_FLAG_GLOBAL_COUNTERS 1   /* covisibility: counters in global scratch even where they would fit LDS           */
#define SFD2_PAIRS_FLAG_CENTRES 2           /* poses: positions are the camera centres -R^T t (see sfd2_pairs_poses)            */
#define SFD2_PAIRS_SPLITS(n) ((n) << 8)     /* retrieval: flags bits 8..15 = number of db splits (0: chosen by the call)         */
/* query[nq][d] . db[nd][d]^T in fp32 (f32-input MFMA: an fmaf chain over ascending element index, so a similarity has the same
 * bits whatever the batch or the split count) and per query the k most similar db rows: idx[nq][k], sim[nq][k] (host).  Replaces
 * the einsum + topk of pairs_from_retrieval.py:60-61.  inputs_on_device: query and db are host (0) or device (1) pointers.  Any
 * d, nq, nd >= 1; k > nd is an error, as torch.topk raises.  The split count is clamped to the number of 128-row db tiles. */
int sfd2_pairs_retrieval(sfd2_ctx *ctx, const float *query, int nq, const float *db, int nd, int d, int k, int inputs_on_device,
                         int32_t *idx, float *sim, int flags);
/* The map as two CSRs: obs_offsets[n_images + 1] / obs_point = per image the point-table row of every key point that has a 3D
 * point; track_offsets[n_points + 1] / track_image = per point the image index of every track element.  Duplicates on either side
 * are counted, as the loops of pairs_from_covisibility.py:20-24 count them; the image itself is excluded.  Per image the k other
 * images with the largest counts > 0: idx[n_images][k], count[n_images][k], n_found[n_images] (<= k; 0: no covisibility). */
int sfd2_pairs_covisibility(sfd2_ctx *ctx, const int64_t *obs_offsets, const int32_t *obs_point, int n_images,
                            const int64_t *track_offsets, const int32_t *track_image, int n_points, int k, int32_t *idx,
                            int32_t *count, int32_t *n_found, int flags);
/* qvec[n][4] (w x y z, used as stored: COLMAP's qvec2rotmat does not normalise) and tvec[n][3], world to camera, fp64 throughout.
 * Per pair dist = |p_i - p_j| and dR = deg(acos(clip((tr(R_i^T R_j) - 1) / 2, -1, 1))); a candidate is valid when
 * dR < rotation_threshold_deg and j != i; per image the k nearest valid ones, nearest first: idx[n][k], dist[n][k] (unfilled:
 * infinity), n_found[n].  The position p is -R t, which is what pairs_from_poses.py:25-26 computes (it multiplies before it
 * transposes); with SFD2_PAIRS_FLAG_CENTRES it is the camera centre -R^T t.  k >= n is no error: a row has at most n - 1 entries. */
int sfd2_pairs_poses(sfd2_ctx *ctx, const double *qvec, const double *tvec, int n, int k, double rotation_threshold_deg,
                     int32_t *idx, double *dist, int32_t *n_found, int flags);

/* ------------------------------------------------------------------------------------------------ covisibility clustering
 * it_loc/localize_cv2.py:87-117 do_covisibility_clustering for many queries in one call, over the two CSRs of
 * sfd2_pairs_covisibility (the conventions of the pair-selection section hold: host arrays, the call runs on sfd2_get_stream(),
 * synchronises before it returns, and returns -1 with sfd2_last_error() set on a bad argument, writing nothing).  Query q lists the
 * images frames[frame_offsets[q] .. frame_offsets[q + 1]) in retrieval order: at most SFD2_CLUSTER_MAX_FRAMES of them, each an
 * index in [0, n_images), none twice (drop repeats before the call: the reference's visited set skips them).
 *   - There is an edge i -> j when image j occurs in the track of a point that image i observes.  The rule is directed: j need not
 *     observe the point itself.
 *   - The list is walked in order; a frame not yet visited opens a cluster that takes every not-yet-visited frame OF THE LIST
 *     reachable from it over those edges (paths run through frames of the list only).
 *   - The clusters are ordered by size, largest first; equal sizes keep their order of creation (Python's sorted(key=len,
 *     reverse=True) is stable), and creation order is the order of each cluster's earliest list position.
 * cluster[p] is the rank of list position p's cluster in that order, n_clusters[q] the number of clusters (0 for an empty query).
 * Deviation: the order of the members INSIDE a cluster is not part of the result (the reference's is whatever set.pop() yields);
 * callers list them by ascending list position.  Integer and bit operations only: a query's output does not depend on the batch,
 * its order, the grid or the flag.  The image -> list-position table sits in LDS up to SFD2_CLUSTER_LDS_IMAGES images, beyond that
 * (or with the flag) in a row of global scratch per workgroup. */
#define SFD2_CLUSTER_MAX_FRAMES 256
#define SFD2_CLUSTER_LDS_IMAGES 65536
#define SFD2_CLUSTER_FLAG_GLOBAL_SLOTS 1   /* image -> list-position table in global scratch even where it fits LDS             */
int sfd2_covis_clusters(sfd2_ctx *ctx, const int64_t *obs_offsets, const int32_t *obs_point, int n_images,
                        const int64_t *track_offsets, const int32_t *track_image, int n_points, const int64_t *frame_offsets,
                        const int32_t *frames, int nq, int32_t *cluster, int32_t *n_clusters, int flags);

/* ------------------------------------------------------------------------------------------------ covisible frame selection
 * it_loc/localize_cv2.py:120-169 get_covisibility_frames (SFD2_FRAMES_OBS) and :172-233 get_covisibility_frames_by_pose
 * (SFD2_FRAMES_POS) for many tasks in one call.  The map is the two CSRs of sfd2_covis_clusters plus
 *   - the SEEN CSR: seen_offsets[n_points + 1] / seen_image = per point the distinct images whose key points hold the point,
 *     ascending: the de-duplicated inverse of obs.  The reference takes connectivity from the tracks and the count from
 *     np.isin(points, image.point3D_ids); the two differ when a track lists an image that does not observe the point, or an image
 *     lists a point twice;
 *   - excluded[n_images]: one byte per image, set when its name holds "left" or "right" (POS only; may be NULL without POS tasks);
 *   - qvec[n_images][4] (w x y z), tvec[n_images][3]: the images' poses, fp64 (may be NULL when no task has a pose);
 *   - n_obs, n_track, n_seen: the lengths of obs_point, track_image, seen_image, which the offsets must end at.
 * Image indices must ascend with the image ids (ties are broken by index where the reference breaks them by id).  With
 * inputs_on_device every map array is a device pointer and nothing of the map is uploaded: the call reads the three offset ends
 * back and the kernel range-checks every index it follows.  Tasks, ref_offsets / ref_points and the outputs are host arrays.
 *
 * A task: frame (image index), kind, covisibility_frame (cf, 0 = no limit), obs_th, q_th (POS), has_pose with qvec / tvec (POS needs
 * one), use_ref.  V, the task's point rows, is the frame's obs segment, or with use_ref ref_points[ref_offsets[i] .. ref_offsets[i + 1])
 * (the reference's ref_3Dpoints; repeats count, as the reference counts them).
 *   connected  every image in the track of any row of V -- the frame itself too; the track length is not tested here.
 *   count(d)   the entries of V with track length >= obs_th (track_offsets, duplicates counted) whose seen list holds d.
 *   pose error against an image's pose, fp64, compute_pose_error's formulas: both quaternions normalised, the centres -R^T t,
 *              t_error = |C_pred - C_d|, q_error = 2 acos(min(1, |q . q_d|)) in degrees.
 * OBS: the connected frames are walked by larger count first, then smaller index.  With a pose a frame is set aside when
 * q_error >= 30, t_error >= 30 or count <= 30; the others are taken until cf are (cf = 0: all).  If at most 3 were taken, the
 * frames set aside before the walk ended are appended in order, stopping after the append that brings the length to >= cf.
 * POS: excluded images leave connected.  The frames with q_error <= q_th come by ascending t_error, up to cf; cf = 0 ends here.
 * If fewer than cf, the list is filled by (larger count, smaller index) from the frames not yet taken, up to cf.
 *
 * idx[n_tasks][cap]: image indices in result order, -1 beyond n_out[i].  status[i]:
 *   0  the row is the reference's result;
 *   1  a decision lay inside a rounding band -- the row is empty, n_out 0, and the caller must decide on the host:
 *        a q_error within 1e-9 + min(1e-13 / sin(q_error / 2), 1e-5) degrees of its threshold (the second term is what acos does
 *        to a rounding of the dot product near 1), for any connected frame of a task with a pose;
 *        OBS: a t_error within 1e-9 (1 + |C_pred| + |C_d|) of 30;
 *        POS: two neighbours in t_error order among the first cf + 1 (cf = 0: all) closer than 1e-9 (1 + 2 |C_pred| + t_error), the
 *        farther one's t_error (|C_d| <= |C_pred| + t_error: the band above without a second look at the pose) -- numpy's default
 *        argsort is not stable, a tie has no defined order;
 *        a non-finite value in the task's pose, an image's pose or an error;
 *   2  capacity, same consequence: more than cap results, or more than SFD2_FRAMES_MAX_CANDIDATES connected frames.
 * Counts and the (count, index) order are integer and exact.  A task's outputs do not depend on the batch, its order, the grid
 * or the flag.  The counters sit in LDS up to SFD2_FRAMES_LDS_IMAGES images, beyond that (or with the flag) in a row of global
 * scratch per workgroup.  Returns -1 with sfd2_last_error() set, writing nothing, on a bad argument: an index out of range in any
 * host array, negative sizes, cap < 1, offsets that do not end at the stated sizes; and, after the launch, when the kernel's range
 * check met a bad index in a device-resident map (no output array is written then either). */
#define SFD2_FRAMES_OBS 0
#define SFD2_FRAMES_POS 1
#define SFD2_FRAMES_MAX_CANDIDATES 4096
#define SFD2_FRAMES_LDS_IMAGES 16384
#define SFD2_FRAMES_FLAG_GLOBAL_COUNTERS 1   /* counters in global scratch even where they fit LDS                              */
typedef struct {
    const int64_t *obs_offsets;     /* [n_images + 1]                                                                      */
    const int32_t *obs_point;       /* [n_obs] point rows                                                                  */
    const int64_t *track_offsets;   /* [n_points + 1]                                                                      */
    const int32_t *track_image;     /* [n_track] image indices, duplicates kept                                            */
    const int64_t *seen_offsets;    /* [n_points + 1]                                                                      */
    const int32_t *seen_image;      /* [n_seen] image indices, distinct and ascending per point                            */
    const uint8_t *excluded;        /* [n_images] or NULL                                                                  */
    const double *qvec, *tvec;      /* [n_images][4], [n_images][3] or NULL                                                */
    int64_t n_obs, n_track, n_seen;
    int32_t n_images, n_points;
    int32_t inputs_on_device, reserved;
} sfd2_frames_map;
typedef struct {
    int32_t frame, kind, covisibility_frame, obs_th;
    int32_t has_pose, use_ref;
    double q_th;
    double qvec[4], tvec[3];        /* world to camera, qvec = (w, x, y, z)                                                */
} sfd2_frames_task;
int sfd2_covis_frames(sfd2_ctx *ctx, const sfd2_frames_map *map, const sfd2_frames_task *tasks, int n_tasks, const int64_t *ref_offsets,
                      const int32_t *ref_points, int cap, int32_t *idx, int32_t *n_out, int32_t *status, int flags);

/* ------------------------------------------------------------------------------------------------ global descriptors (VLAD)
 * What sfd2_pairs_retrieval ranks by: per image one vector aggregated from its local descriptors (Jegou et al. 2010, with the
 * intra-normalisation of Arandjelovic & Zisserman 2013) over a k-means vocabulary learnt by Lloyd iterations on the device.  The
 * project's own choice, not a port: the reference retrieves with NetVLAD / AP-GeM descriptors extracted by another project.
 * Conventions of the pair-selection section: outputs and offsets are host arrays, inputs_on_device says whether x and centroids
 * are host (0) or device (1) pointers, the calls run on sfd2_get_stream() and synchronise before they return, and return -1 with
 * sfd2_last_error() set on a bad argument (before anything is uploaded) or on non-finite input.  Rows and centroids are
 * SFD2_VLAD_DIM floats; 1 <= k <= SFD2_VLAD_MAX_K, any k.  flags must be 0.  The arithmetic is part of the interface:
 *   h_j     = 0.5f * (fmaf chain of c_j[e] * c_j[e] over ascending e, from 0)
 *   dot_j   = fmaf chain of x[e] * c_j[e] over ascending e, from 0 (the f32-input MFMA)
 *   s_j     = dot_j - h_j, one fp32 subtraction; a row goes to the j of largest s_j, a tie to the smaller j
 *   V[j][e] = the sum, over the segment's rows i in ascending order with assignment j, of (x[i][e] - c_j[e]): an fp32 subtraction,
 *             then an fp32 addition (k-means sums x[i][e] itself and counts the rows)
 *   norms   in fp64 from the fp32 sums, every output component rounded to fp32 once.  INTRA: each centroid's 128 values divided by
 *           their L2 norm (a zero block stays zero), then the whole vector by its L2 norm; SSR: sign(v) sqrt(|v|) per component,
 *           then the L2 norm; NONE: the L2 norm only.  A zero vector stays zero: nothing is ever NaN.
 * A row's or an image's result depends on that row or image and the centroids only -- not on the batch, its order or the grid.
 * No floating-point atomics. */
#define SFD2_VLAD_DIM 128
#define SFD2_VLAD_MAX_K 256
#define SFD2_VLAD_CHUNK 4096
#define SFD2_VLAD_NORM_INTRA 0
#define SFD2_VLAD_NORM_SSR 1
#define SFD2_VLAD_NORM_NONE 2
/* x[n][128], centroids[k][128]: assign[n] and, unless NULL, score[n] = s of the chosen centroid.  n >= 1. */
int sfd2_vlad_assign(sfd2_ctx *ctx, const float *x, int64_t n, const float *centroids, int k, int inputs_on_device,
                     int32_t *assign, float *score /* or NULL */, int flags);
/* Image i owns the rows offsets[i] .. offsets[i + 1] - 1 of x (offsets[n_images + 1], from 0, not decreasing; an image may have
 * any number of rows, 0 included: its vector is zero).  out[n_images][k * 128]; assign, unless NULL, receives offsets[n_images]
 * assignments.  n_images >= 1. */
int sfd2_vlad_aggregate(sfd2_ctx *ctx, const float *x, const int64_t *offsets, int n_images, const float *centroids, int k,
                        int inputs_on_device, int norm, float *out /* [n_images][k * 128] */, int32_t *assign /* or NULL */, int flags);
/* Lloyd iterations from the k start centroids in centroids[k][128] (always a host array, overwritten with the result); x stays on
 * the device across the iterations.  An iteration assigns, sums the rows and counts them per centroid within every chunk of
 * SFD2_VLAD_CHUNK consecutive rows (fp32, row order), adds the chunks' partial sums in ascending chunk order in fp64 and sets
 * centroid = (float)(sum / count); a centroid without rows keeps its value.  moved[it] is the number of rows whose assignment
 * differs from the previous iteration's (n for the first); the call stops after the first iteration with moved == 0 or after
 * max_iters (>= 1).  counts[k]: the rows per centroid under the last iteration's assignment; moved[max_iters], -1 for an iteration
 * that did not run; *iters_run. */
int sfd2_vlad_kmeans(sfd2_ctx *ctx, const float *x, int64_t n, int k, int max_iters, int inputs_on_device,
                     float *centroids /* in: start, out: result */, int64_t *counts, int64_t *moved, int *iters_run, int flags);

#ifdef __cplusplus
}
#endif
#endif /* SFD2_HIP_H */
