// convDa.0 (3x3, 256 -> 256, BN + ReLU: nets/sfd2.py:340-342) on the pixels the sparse descriptor head reads only.  On the extract path
// convDa.0's one consumer is sparse_da3_kernel, which reads the 4 x 4 block (y0 - 1 .. y0 + 2, x0 - 1 .. x0 + 2) around each selected key
// point's corner (sd_corner): 16 x K pixels -- 65 536 of 120 000 at 1600x1200 / top-4096 -- so this kernel computes the layer there and
// nowhere else, and stores the results into the dense map at their true positions (overlapping blocks of neighbouring key points store
// the same bits twice; pixels no key point needs keep whatever they held and are never read).
//
// The kernel is conv3x3_rf_kernel<1> (conv3rf_kernels.hip) with another address generation on both sides: the same 128-pixel x
// 256-channel tile, filters from L2 straight into a register ring of nine units, the patch through three LDS buffers of one 32-channel
// chunk each (buffer_load ... lds, two chunks ahead, one piece per unit), counted waits, one barrier per chunk, persistent blocks whose
// pipeline runs across the tile boundary, the same epilogue.  Per output element the MFMAs come in the order of the dense kernel that
// would run the layer at this geometry -- chunks ascending, the two K halves inside a tap, and the nine taps of a chunk row by row
// (conv3x3_rf) or COLUMN by column (conv3x3_pp with its default KXM schedule: kx outside, ky inside) -- so the pixels come out bit for
// bit as the dense layer writes them: template parameter KXM, chosen by the launcher as launch_conv_igemm chooses the kernel.
//
//   tile    8 key points = eight 4 x 4 output blocks laid out as a virtual 8 x 16 tile, two block rows x four block columns: key point
//           k of the tile sits at block row k >> 2, block column k & 3.  A pixel fragment is still "2 output rows x 16 pixels".
//   patch   per key point a CELL of 6 rows x 8 records (64 B = 32 channels of one pixel; 6 x 6 used: input pixels y0 - 2 .. y0 + 3,
//           x0 - 2 .. x0 + 3), 48 records per cell, 384 per chunk = 24 pieces of 1 KB, three per wave.  Output (r, c) of a block
//           reads record (r + ky) * 8 + (c + kx) of its cell: per-lane base + compile-time tap offset.  Pixels outside the map, the
//           two pad records of a row and the cells of key points beyond the count get an offset beyond the buffer: zeros.
//   slots   a record's four 16-byte slots are XOR-swizzled by the cell's BLOCK COLUMN (k & 3).  ds_read_b128 serves a wave in the
//           lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} (+ 32): four runs of four consecutive records of the block
//           columns {0, 3} of one fragment row and {1, 2} of the other (or the reverse).  Cell and row pitch are multiples of
//           four records, so a run covers each record residue mod 4 once, and the four runs of a group differ in the block column:
//           sixteen different slots of the 256-byte bank row for every tap.  (conv3x3_rf's (record >> 2) & 3 relies on the sixteen
//           records of a fragment row being consecutive, which they are not here.)  The term does not depend on the tap or the
//           fragment, so a lane's read address is one of two bases (K half) + a constant.
#include "sfd2_internal.h"

#define S0_KP 8                          // key points per tile
#define S0_RP 8                          // records per cell row (six used)
#define S0_CELL (6 * S0_RP)              // records per cell
#define S0_NPIECE (S0_KP * S0_CELL / 16) // 24 pieces of 16 records
#define S0_PPW (S0_NPIECE / 8)           // pieces per wave
#define S0_XBYTES (S0_NPIECE * 1024)
#define S0_CC 32
#define S0_C 256                         // input and (padded) output channels
#ifndef SFD2_PP_KXM                      // conv3x3_pp's tap schedule (conv3_kernels.hip; an experiment build sets it for every file)
#define SFD2_PP_KXM 1
#endif

typedef __attribute__((address_space(3))) void s0_lds_t;

// one LDS-DMA piece: 64 lanes x 16 bytes from base + voff (+ soff) to 1 KB of LDS at dst; offsets beyond nbytes read zeros
// (buffer_load ... lds: conv3rf_kernels.hip says why not global_load ... lds)
__device__ __forceinline__ void s0_copy_piece(const half_t *base, int nbytes, unsigned char *dst, int voff, int soff)
{
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t *>(base), 0, nbytes, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (s0_lds_t *)dst, 16, voff, soff, 0, 0);
}

__device__ __forceinline__ h4_t s0_cvt4(float a, float b, float c, float d)
{
    h4_t r;
    r[0] = (half_t)a; r[1] = (half_t)b; r[2] = (half_t)c; r[3] = (half_t)d;
    return r;
}

// in: the backbone output [H][W][256] fp16 (the hi plane in SFD2_PREC_F16C); out: convDa.0's dense map [H][W][256]; kpts / count: the
// selection's key points and their number on the device (what sparse_da3_kernel reads); half_w / half_h: sd_corner's arguments.
// Persistent: tiles blockIdx.x, + gridDim.x, ... of ceil(count / 8); blocks without a tile return at once.
// KXM: unit t of a chunk is tap (ky, kx) = (t % 3, t / 3) instead of (t / 3, t % 3)
#define S0_TAP(t_) (KXM ? ((t_) % 3) * 3 + (t_) / 3 : (t_))
template <bool KXM>
__global__ __launch_bounds__(512, 2)
void sparse_da0_kernel(const half_t *__restrict__ in, int H, int W, const half_t *__restrict__ wpk /*[8 chunks of 32][9 taps][256][32]*/,
                       const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                       const float *__restrict__ kpts, const unsigned int *__restrict__ count, int n_max, float half_w, float half_h,
                       half_t *__restrict__ out)
{
    constexpr int NCH = S0_C / S0_CC;                      // chunks per tile
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *Xs = smem;                              // [3][S0_XBYTES]
    int *geo = reinterpret_cast<int *>(smem + 3 * S0_XBYTES);   // [2 tiles in flight][S0_KP][x0, y0]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lhi = lane >> 5, l32 = lane & 31, ly = l32 >> 4, lx = l32 & 15;
    const int n0 = wave * 32;                              // this wave's output channels; every wave all four pixel fragments

    int n = n_max;
    { const unsigned int cnt = *count; if ((unsigned int)n > cnt) n = (int)cnt; }
    const int n_tiles = (n + S0_KP - 1) / S0_KP;
    const int n_my = (n_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;   // tiles of this block
    if (n_my <= 0) return;
    const int TC = n_my * NCH;                             // chunks of this block

    // ---- per-lane staging sources of ONE tile: piece wave + 8 i = records 16 (wave + 8 i) ..: two rows of cell (wave + 8 i) / 3.
    // The key point of a piece is wave-uniform: its corner is computed per wave from scalar loads (no vector-memory operation joins
    // the counted ones) and left in `geo` for the tile's epilogue; rows of the list beyond the count are not converted (sparse_da3_kernel)
    const int in_bytes = (int)((size_t)H * W * S0_C * sizeof(half_t));
    int xoff[S0_PPW];
    int xoff_seq = -1;                                     // which of this block's tiles xoff describes
#define S0_SETUP_X(seq_)                                                                               \
    {                                                                                                  \
        const int tile_ = (int)blockIdx.x + (seq_) * (int)gridDim.x;                                   \
        _Pragma("unroll") for (int i = 0; i < S0_PPW; ++i) {                                           \
            const int piece = wave + 8 * i;                                                            \
            const int kpl = piece / 3, pr = piece - kpl * 3;                                           \
            const int kp = tile_ * S0_KP + kpl;                                                        \
            const bool live = kp < n;                                                                  \
            const int kpc = live ? kp : n - 1;                                                         \
            const float kx_ = kpts[2 * kpc], ky_ = kpts[2 * kpc + 1];                                  \
            int x0_, y0_;                                                                              \
            sd_corner(live ? kx_ : 0.0f, live ? ky_ : 0.0f, half_w, half_h, H, W, x0_, y0_);           \
            if (lane == 0) {                                                                           \
                geo[(((seq_) & 1) * S0_KP + kpl) * 2] = x0_;                                           \
                geo[(((seq_) & 1) * S0_KP + kpl) * 2 + 1] = y0_;                                       \
            }                                                                                          \
            const int r = lane >> 2;                                                                   \
            const int cy = pr * 2 + (r >> 3), cx = r & 7;                                              \
            const int slot = (lane & 3) ^ (kpl & 3);                                                   \
            const int iy = y0_ - 2 + cy, ix = x0_ - 2 + cx;                                            \
            int off = (int)0x80000000;                                                                 \
            if (live && cx < 6 && iy >= 0 && iy < H && ix >= 0 && ix < W)                              \
                off = ((iy * W + ix) * S0_C + slot * 8) * (int)sizeof(half_t);                         \
            xoff[i] = off;                                                                             \
        }                                                                                              \
        xoff_seq = (seq_);                                                                             \
    }
#define S0_ISSUE_X1(chunk_, buf_, i_) \
    s0_copy_piece(in, in_bytes, Xs + (buf_)*S0_XBYTES + (wave + 8 * (i_)) * 1024, xoff[i_], (chunk_)*S0_CC * (int)sizeof(half_t))
#define S0_ISSUE_X(chunk_, buf_) \
    _Pragma("unroll") for (int i_ = 0; i_ < S0_PPW; ++i_) S0_ISSUE_X1(chunk_, buf_, i_);

    // A fragments: lane -> filter row n0 + (lane & 31), K slice (lane >> 5) + 2 * kk of the unit's [256][32] tile
    const int aoff = (n0 + l32) * S0_CC + lhi * 8;
#define S0_LOAD_A(u_, dst_)                                                                            \
    do {                                                                                               \
        int ao_ = aoff;                                                                                \
        asm volatile("" : "+v"(ao_));                                                                  \
        const half_t *ap_ = wpk + (size_t)(u_)*S0_C * S0_CC + ao_;                                     \
        dst_[0] = *reinterpret_cast<const h8_t *>(ap_);                                                \
        dst_[1] = *reinterpret_cast<const h8_t *>(ap_ + 16);                                           \
    } while (0)

    // B fragments: byte address of (fragment 0, tap 0, K half kk) for this lane; unit t_'s tap adds (ky * 8 + kx) records, fragment f
    // (f >> 1) block rows = four cells and 2 (f & 1) cell rows
    const int bcol = lx >> 2;
    const int qb = bcol * S0_CELL + ly * S0_RP + (lx & 3);
    const int bb0 = qb * 64 + ((lhi ^ bcol) << 4), bb1 = qb * 64 + (((2 + lhi) ^ bcol) << 4);
#define S0_READ_B(xs_, t_, kk_, dst_)                                                                  \
    do {                                                                                               \
        const int to_ = (S0_TAP(t_) / 3) * S0_RP + S0_TAP(t_) % 3;                                     \
        int b_ = (kk_) ? bb1 : bb0;                                                                    \
        asm volatile("" : "+v"(b_));                                                                   \
        const unsigned char *bp_ = (xs_) + b_ + to_ * 64;                                              \
        _Pragma("unroll") for (int f_ = 0; f_ < 4; ++f_)                                               \
            dst_[f_] = *reinterpret_cast<const h8_t *>(bp_ + ((f_ >> 1) * 4 * S0_CELL + (f_ & 1) * 2 * S0_RP) * 64); \
    } while (0)

    f32x16_t acc[4];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[f][r] = 0.0f;
    h8_t fa[9][2], fb[3][4];

    // scale / shift of this wave's 32 channels stay in registers
    float4 sc[4], sh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sc[q] = *reinterpret_cast<const float4 *>(scale + n0 + 4 * lhi + 8 * q);
        sh[q] = *reinterpret_cast<const float4 *>(shift + n0 + 4 * lhi + 8 * q);
    }
    const float lo = relu ? 0.0f : -__builtin_huge_valf();   // branch-free ReLU (this file is compiled with -fno-honor-nans)

    S0_SETUP_X(0)
    S0_ISSUE_X(0, 0)
    S0_ISSUE_X(1, 1)
#pragma unroll
    for (int u = 0; u < 9; ++u) S0_LOAD_A(S0_TAP(u), fa[u]);
    SFD2_BARRIER_DRAIN();
    S0_READ_B(Xs, 0, 0, fb[0]);
    S0_READ_B(Xs, 0, 1, fb[1]);

    int bc = 0;                                            // C % 3: three patch buffers
    int c = 0, seq = 0, C = 0;                             // chunk within the tile, tile of this block, chunk of this block
    auto chunk = [&]() {
        const int bn = bc == 2 ? 0 : bc + 1, bnn = bn == 2 ? 0 : bn + 1;
        const unsigned char *xs = Xs + bc * S0_XBYTES;
        const unsigned char *xn = Xs + bn * S0_XBYTES;
        // the patch two chunks ahead (of this or of the next tile) goes into the buffer chunk C - 1 used, one piece per unit; the
        // block's last two chunks re-request its last patch (branch-free: the in-flight counts stay what the waits assume)
        const int Cx = C + 2 < TC ? C + 2 : TC - 1;
        const int seq_x = Cx / NCH, cx = Cx - seq_x * NCH;
        if (seq_x != xoff_seq) S0_SETUP_X(seq_x)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (t < S0_PPW) S0_ISSUE_X1(cx, bnn, t);
            if (t == 8) {
                // chunk boundary: my pieces of the next patch have landed -- younger and possibly still in flight are the filter
                // loads of units 2..8 and 0..7 (2 each) and the three pieces of the patch after it: 33 -- my reads of this one
                // are done; then the whole block's.  The last chunk's look-ahead reads return stale records no MFMA consumes.
                static_assert(2 * (10 - S0_PPW) + 16 + S0_PPW == 33, "chunk-boundary wait count");
                asm volatile("s_waitcnt vmcnt(33) lgkmcnt(0)\n\ts_barrier" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int h = 2 * t + kk;                  // K half of the chunk; its fragments sit in fb[h % 3]
                if (h + 2 < 18) S0_READ_B(xs, (h + 2) / 2, (h + 2) % 2, fb[(h + 2) % 3]);
                else S0_READ_B(xn, (h + 2 - 18) / 2, (h + 2) % 2, fb[(h + 2) % 3]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int f = 0; f < 4; ++f)
                    acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[t][kk], fb[h % 3][f], acc[f], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // the same unit of the next chunk: the same filters serve every tile, so the ring wraps at a tile's last chunk
            const int cn = c + 1 == NCH ? 0 : c + 1;
            S0_LOAD_A(cn * 9 + S0_TAP(t), fa[t]);
            __builtin_amdgcn_sched_barrier(0);
        }
        bc = bn;
        ++C;
    };
    // a tile's epilogue: y = acc * scale + shift (ReLU), regrouped with v_permlane32_swap into 16-byte stores at the pixels' true
    // positions; the next tile's first operands are already in registers / in flight
    auto epilogue = [&]() {
        const int tile = (int)blockIdx.x + seq * (int)gridDim.x;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int kpl = (f >> 1) * 4 + bcol;
            const int x0 = geo[((seq & 1) * S0_KP + kpl) * 2], y0 = geo[((seq & 1) * S0_KP + kpl) * 2 + 1];
            const int oy = y0 - 1 + 2 * (f & 1) + ly, ox = x0 - 1 + (lx & 3);
            const bool inb = tile * S0_KP + kpl < n && oy >= 0 && oy < H && ox >= 0 && ox < W;
            const size_t pix = (size_t)(inb ? oy : 0) * W + (inb ? ox : 0);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const size_t o16 = pix * S0_C + n0 + 8 * (2 * m + lhi);
                uint2 pk[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int q = 2 * m + j;
                    float v0 = acc[f][4 * q + 0] * sc[q].x + sh[q].x;
                    float v1 = acc[f][4 * q + 1] * sc[q].y + sh[q].y;
                    float v2 = acc[f][4 * q + 2] * sc[q].z + sh[q].z;
                    float v3 = acc[f][4 * q + 3] * sc[q].w + sh[q].w;
                    v0 = fmaxf(v0, lo); v1 = fmaxf(v1, lo); v2 = fmaxf(v2, lo); v3 = fmaxf(v3, lo);
                    const h4_t hv = s0_cvt4(v0, v1, v2, v3);
                    __builtin_memcpy(&pk[j], &hv, 8);
                }
                const auto t0 = __builtin_amdgcn_permlane32_swap(pk[0].x, pk[1].x, false, false);
                const auto t1 = __builtin_amdgcn_permlane32_swap(pk[0].y, pk[1].y, false, false);
                if (inb) *reinterpret_cast<uint4 *>(out + o16) = make_uint4(t0[0], t1[0], t0[1], t1[1]);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[f][r] = 0.0f;
        }
        c = 0;
        ++seq;
    };
    while (C < TC) {
        chunk();
        if (++c == NCH) epilogue();
    }
#undef S0_ISSUE_X
#undef S0_ISSUE_X1
#undef S0_LOAD_A
#undef S0_READ_B
#undef S0_SETUP_X
}
#undef S0_TAP

// the geometries the kernel takes: 256 -> 256 channels, the map addressed through a buffer descriptor with 32-bit byte offsets
bool sparse_da0_serves(int cin, int CoutP, int hc, int wc)
{
    return cin == S0_C && CoutP == S0_C && (long long)hc * wc * S0_C * (long long)sizeof(half_t) < (1ll << 31);
}

// nh x nw: the image (sd_corner's half sizes, as launch_sparse_da3 passes them).  The tap order is that of the dense kernel launch_conv_igemm would
// pick for the layer at this map size: conv3x3_rf where it serves (small maps), conv3x3_pp otherwise (conv3_kernels.hip: SFD2_PP_KXM, default 1).  The grid is fixed by the capacity n_max, not by the count
// (which stays on the device): min(CUs, ceil(n_max / 8)) persistent blocks, so the launch can be captured into a hipGraph.
void launch_sparse_da0(hipStream_t st, const half_t *in, int hc, int wc, int nh, int nw, const half_t *wpk, const float *scale, const float *shift,
                       int relu, const float *kpts, const unsigned int *count, int n_max, half_t *out)
{
    if (n_max <= 0) return;
    constexpr size_t lds = (size_t)3 * S0_XBYTES + 2 * S0_KP * 2 * sizeof(int);
    static bool attr_done = false;
    static int slots = 256;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(sparse_da0_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(sparse_da0_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            slots = cus;                                   // one resident block per CU
        attr_done = true;
    }
    const int n_tiles = (n_max + S0_KP - 1) / S0_KP;
    const int grid = n_tiles < sfd2_slots(slots) ? n_tiles : sfd2_slots(slots);
    const bool kxm = SFD2_PP_KXM && !conv3x3_rf_serves(3, 1, S0_C, S0_C, hc, wc) && conv3x3_pp_serves(3, 1, S0_C, S0_C);
    hipLaunchKernelGGL(kxm ? sparse_da0_kernel<true> : sparse_da0_kernel<false>, dim3(grid), dim3(512), lds, st, in, hc, wc, wpk, scale, shift, relu,
                       kpts, count, n_max, (float)nw / 2.0f, (float)nh / 2.0f, out);
}
