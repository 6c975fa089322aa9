// libsfd2hip: the device side of the baseline JPEG decoder (layout of the prepared buffer: sfd2_internal.h).
//
//   jpeg_sync_kernel    self-synchronising Huffman decoding (Weissenberger & Schmidt, ICPP 2018 / HiPC 2021): every lane starts at its
//                       256-bit subsequence, guessing "first block of an MCU", and decodes whole blocks until it has passed the end of its
//                       subsequence.  A lane then restarts from where its predecessor stopped, until no lane's start changes: inside a
//                       workgroup by a barrier loop, across workgroups by a fixed number of launches that return at once when the
//                       previous one changed nothing, then (only if those did not settle) one workgroup walking the groups in order.
//                       Restart intervals begin at exact starts.
//   jpeg_scan_*         exclusive scans of the lanes' block counts (output block of every lane) and DC difference sums (the DC
//                       predictor at every lane's start: the sums since the lane's restart interval began)
//   jpeg_write_kernel   decodes once more from the agreed starts and writes the coefficients; checks block counts, interval ends, sync
//   jpeg_idct_kernel    libjpeg's accurate integer IDCT (jidctint.c, "islow": 13-bit constants, two passes, range limit around 128) with
//                       the 16-bit arithmetic of libjpeg-turbo's SIMD version (wrapping sums, saturating packs, the DC-only shortcut)
//   jpeg_color_kernel   libjpeg's "fancy" chroma upsampling (h2v1 / h2v2 triangle filters, replicated edges) and YCbCr -> RGB with its
//                       16-bit fixed-point tables; writes RGBX
// Safety: every read of the bit buffer is clamped to its words, every coefficient write to block < total_blocks; an anomaly sets a
// status bit and never a fault or a loop without bound.
#include "sfd2_internal.h"

namespace {

constexpr int kSyncWG = 64;
constexpr int kScanWG = 256;

__constant__ uint8_t c_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Bits {                      // 64-bit window over the big-endian words; words beyond the data read as zero
    const uint32_t *d;
    uint32_t nw, wi;
    uint64_t win;
    __device__ uint32_t ld(uint32_t i) const { return i < nw ? __builtin_bswap32(d[i]) : 0u; }
    __device__ void init(const uint32_t *data, uint32_t nwords, uint32_t pos)
    {
        d = data;
        nw = nwords;
        wi = pos >> 5;
        win = ((uint64_t)ld(wi) << 32) | ld(wi + 1);
    }
    __device__ uint32_t peek(uint32_t pos)
    {
        const uint32_t w = pos >> 5;
        if (w != wi) {
            win = (w == wi + 1) ? (win << 32) | ld(w + 1) : ((uint64_t)ld(w) << 32) | ld(w + 1);
            wi = w;
        }
        return (uint32_t)(win >> (32 - (pos & 31)));
    }
};

__device__ inline int huff_decode(const JpegHuff &h, uint32_t v, int &len)
{
    const uint32_t e = h.lut[v >> 23];
    if (e) { len = (int)(e >> 8); return (int)(e & 255); }
    for (int l = 10; l <= 16; ++l) {
        const int c = (int)(v >> (32 - l));
        if (c <= h.maxcode[l]) { len = l; return h.vals[(h.valoff[l] + c) & 255]; }
    }
    len = 0;
    return -1;
}

__device__ inline int extend(uint32_t x, int s) { return (int)x < (1 << (s - 1)) ? (int)x - (1 << s) + 1 : (int)x; }

// One block (T.81 F.2.2): DC difference, then the AC run/size symbols up to EOB or coefficient 63.  coef (natural order) is
// written only when W; false on an invalid code, a DC size above 11 or a run past coefficient 63.
template <bool W>
__device__ inline bool decode_block(Bits &br, uint32_t &pos, const JpegHuff &dc, const JpegHuff &ac, int &diff, short *coef)
{
    int len;
    uint32_t v = br.peek(pos);
    int s = huff_decode(dc, v, len);
    if (s < 0 || s > 11) return false;
    diff = s ? extend((v << len) >> (32 - s), s) : 0;
    pos += len + s;
    for (int k = 1; k < 64;) {
        v = br.peek(pos);
        const int rs = huff_decode(ac, v, len);
        if (rs < 0) return false;
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) return false;
            if (W) coef[c_natural[k]] = (short)extend((v << len) >> (32 - s), s);
            pos += len + s;
            ++k;
        } else {
            pos += len;
            if (r != 15) break;   // EOB
            k += 16;              // ZRL
        }
    }
    return true;
}

struct LaneCtx {
    uint32_t start, end;
    bool head, last_in_int;
    int interval;
};

__device__ inline LaneCtx lane_ctx(const uint32_t *lane_start, const uint32_t *lane_int, const uint32_t *int_first, int i)
{
    LaneCtx l;
    l.start = lane_start[i];
    l.end = lane_start[i + 1];
    l.interval = (int)lane_int[i];
    l.head = int_first[l.interval] == (uint32_t)i;
    l.last_in_int = int_first[l.interval + 1] == (uint32_t)(i + 1);
    return l;
}

// Decodes whole blocks from (pos, u) while pos is before the lane's end.  The last lane of an interval stops at the interval's
// end when fewer than 8 bits remain and all are ones (the padding in front of a marker: no Huffman code is all ones).
// W: also writes the blocks (base = output block of the first, pred = DC predictors).
template <bool W>
__device__ inline void decode_lane(Bits &br, const JpegHuff (*tab)[2], const JpegGeom &g, const LaneCtx &lc, uint32_t pos, int u,
                                   JpegLane &rec, int base, int *pred, short *coef, unsigned int *status)
{
    rec.spos = pos;
    rec.su = u;
    rec.bad = 0;
    rec.cnt = 0;
    rec.dc[0] = rec.dc[1] = rec.dc[2] = 0;
    br.init(br.d, br.nw, pos);
    while (pos < lc.end) {
        if (lc.last_in_int && lc.end - pos < 8) {
            const uint32_t nb = lc.end - pos;
            if ((br.peek(pos) >> (32 - nb)) == (1u << nb) - 1) { pos = lc.end; break; }
        }
        const int c = g.unit_comp[u];
        int diff = 0;
        short *blk = nullptr;
        if (W) {
            const int b = base + rec.cnt;
            if (b >= g.total_blocks) { atomicOr(status, SFD2_JPEG_BAD_COUNT); break; }
            const int mcu = b / g.bpm, mx = mcu % g.mcus_x, my = mcu / g.mcus_x;
            const int bx = mx * g.hs[c] + g.unit_dx[u], by = my * g.vs[c] + g.unit_dy[u];
            blk = coef + (int64_t)(g.blk_base[c] + by * g.bw[c] + bx) * 64;
            const int4 z = make_int4(0, 0, 0, 0);
            for (int q = 0; q < 8; ++q) reinterpret_cast<int4 *>(blk)[q] = z;
        }
        if (!decode_block<W>(br, pos, tab[c][0], tab[c][1], diff, blk)) { rec.bad = 1; break; }
        if (W) {
            pred[c] += diff;
            blk[0] = (short)pred[c];
        }
        rec.dc[c] += diff;
        ++rec.cnt;
        u = (u + 1 == g.bpm) ? 0 : u + 1;
    }
    rec.epos = pos;
    rec.eu = u;
}

__device__ inline void load_tables(const unsigned char *in, int64_t tab_off, int ncomp, JpegHuff (*tab)[2])
{
    const uint4 *src = reinterpret_cast<const uint4 *>(in + tab_off);
    uint4 *dst = reinterpret_cast<uint4 *>(&tab[0][0]);
    const int n = (int)(ncomp * 2 * sizeof(JpegHuff) / sizeof(uint4));
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

struct Prepared {
    const uint32_t *words, *lane_start, *lane_int, *int_first;
};

__device__ inline Prepared prepared(const unsigned char *in, int64_t tab_off, const JpegGeom &g)
{
    Prepared p;
    p.words = reinterpret_cast<const uint32_t *>(in);
    p.lane_start = reinterpret_cast<const uint32_t *>(in + tab_off + sizeof(JpegTables));
    p.lane_int = p.lane_start + g.nlanes + 1;
    p.int_first = p.lane_int + g.nlanes;
    return p;
}

struct SyncShared {
    JpegHuff tab[3][2];
    uint32_t xpos[kSyncWG];
    int xu[kSyncWG];
    int any;
};

// One workgroup's lanes: each starts where its predecessor's last record stopped (group-first lanes read it from the previous group),
// decodes when its start differs from its record, and the group iterates until no start changes.  Writes the records that changed;
// returns (in every thread) whether any did.  first: the first launch (no records yet; non-head lanes guess "block 0 at their start").
__device__ bool sync_group(SyncShared &sh, const Prepared &P, const JpegGeom &g, JpegLane *lanes, int grp, bool first)
{
    const int t = threadIdx.x, i = grp * kSyncWG + t;
    const bool valid = i < g.nlanes;
    LaneCtx lc = {};
    JpegLane old = {}, rec = {};
    uint32_t spos = 0;
    int su = 0;
    if (valid) {
        lc = lane_ctx(P.lane_start, P.lane_int, P.int_first, i);
        spos = lc.start;
        if (!first) {
            old = lanes[i];
            if (!lc.head) {
                const JpegLane pv = lanes[i - 1];     // (another workgroup may be rewriting it: the next launch sees the change)
                if (!pv.bad && pv.epos >= lc.start) { spos = pv.epos; su = pv.eu; }
            }
        }
        su = su < 0 || su >= g.bpm ? 0 : su;
    }
    Bits br;
    br.d = P.words;
    br.nw = g.ecs_words;
    bool need = valid && (first || spos != old.spos || su != old.su);
    if (valid && !need) rec = old;
    if (t == 0) sh.any = 0;
    __syncthreads();
    for (int round = 0; round <= kSyncWG; ++round) {
        if (need) {
            decode_lane<false>(br, sh.tab, g, lc, spos, su, rec, 0, nullptr, nullptr, nullptr);
            need = false;
        }
        sh.xpos[t] = rec.epos;
        sh.xu[t] = (!valid || rec.bad) ? -1 : rec.eu;
        __syncthreads();
        bool moved = false;
        if (valid && t > 0 && !lc.head) {
            uint32_t np = lc.start;
            int nu = 0;
            if (sh.xu[t - 1] >= 0 && sh.xpos[t - 1] >= lc.start) { np = sh.xpos[t - 1]; nu = sh.xu[t - 1]; }
            if (np != spos || nu != su) { spos = np; su = nu; need = true; moved = true; }
        }
        if (!__syncthreads_or(moved)) break;
    }
    const bool changed = valid && (first || rec.spos != old.spos || rec.su != old.su || rec.epos != old.epos || rec.eu != old.eu ||
                                   rec.bad != old.bad);
    if (changed) lanes[i] = rec;
    return __syncthreads_or(changed);
}

__global__ __launch_bounds__(kSyncWG) void jpeg_sync_kernel(const unsigned char *in, int64_t tab_off, JpegGeom g, JpegLane *lanes,
                                                            unsigned int *flags, int it)
{
    if (it > 0 && flags[it - 1] == 0) return;          // the previous launch changed nothing: synchronised
    __shared__ SyncShared sh;
    load_tables(in, tab_off, g.ncomp, sh.tab);
    const Prepared P = prepared(in, tab_off, g);
    if (sync_group(sh, P, g, lanes, blockIdx.x, it == 0) && threadIdx.x == 0) flags[it] = 1;
}

// When the launches above did not settle (a stream that resynchronises only after many subsequences -- noise at quality 100 decoded with
// the wrong MCU phase can run on for thousands of bits): one workgroup walks the groups in order, each starting from its predecessor's
// final record, which makes the chain exact.  Returns at once when the last launch changed nothing.
__global__ __launch_bounds__(kSyncWG) void jpeg_sync_serial_kernel(const unsigned char *in, int64_t tab_off, JpegGeom g, JpegLane *lanes,
                                                                   unsigned int *flags)
{
    if (flags[SFD2_JPEG_SYNC_LAUNCHES - 1] == 0) return;
    __shared__ SyncShared sh;
    load_tables(in, tab_off, g.ncomp, sh.tab);
    const Prepared P = prepared(in, tab_off, g);
    const int ng = (g.nlanes + kSyncWG - 1) / kSyncWG;
    for (int grp = 0; grp < ng; ++grp) sync_group(sh, P, g, lanes, grp, false);
    __syncthreads();
    if (threadIdx.x == 0) flags[SFD2_JPEG_SYNC_LAUNCHES - 1] = 0;
}

// exclusive scan of (cnt, dc0, dc1, dc2) over the lanes of each 256-lane group; group totals to wg_sum
__global__ __launch_bounds__(kScanWG) void jpeg_scan_local_kernel(const JpegLane *lanes, int nl, int4 *pre, int4 *wg_sum)
{
    __shared__ int4 s[kScanWG];
    const int t = threadIdx.x, i = blockIdx.x * kScanWG + t;
    int4 v = make_int4(0, 0, 0, 0);
    if (i < nl) { const JpegLane l = lanes[i]; v = make_int4(l.cnt, l.dc[0], l.dc[1], l.dc[2]); }
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < kScanWG; off <<= 1) {
        int4 a = t >= off ? s[t - off] : make_int4(0, 0, 0, 0);
        __syncthreads();
        s[t] = make_int4(s[t].x + a.x, s[t].y + a.y, s[t].z + a.z, s[t].w + a.w);
        __syncthreads();
    }
    if (i < nl) pre[i] = make_int4(s[t].x - v.x, s[t].y - v.y, s[t].z - v.z, s[t].w - v.w);
    if (t == kScanWG - 1) wg_sum[blockIdx.x] = s[t];
}

// one workgroup: exclusive scan of the group totals (in place)
__global__ __launch_bounds__(kScanWG) void jpeg_scan_top_kernel(int4 *wg, int ng)
{
    __shared__ int4 s[kScanWG];
    __shared__ int4 carry;
    const int t = threadIdx.x;
    if (t == 0) carry = make_int4(0, 0, 0, 0);
    __syncthreads();
    for (int base = 0; base < ng; base += kScanWG) {
        const int4 v = base + t < ng ? wg[base + t] : make_int4(0, 0, 0, 0);
        s[t] = v;
        __syncthreads();
        for (int off = 1; off < kScanWG; off <<= 1) {
            int4 a = t >= off ? s[t - off] : make_int4(0, 0, 0, 0);
            __syncthreads();
            s[t] = make_int4(s[t].x + a.x, s[t].y + a.y, s[t].z + a.z, s[t].w + a.w);
            __syncthreads();
        }
        const int4 c = carry;
        if (base + t < ng) wg[base + t] = make_int4(c.x + s[t].x - v.x, c.y + s[t].y - v.y, c.z + s[t].z - v.z, c.w + s[t].w - v.w);
        __syncthreads();
        if (t == kScanWG - 1) carry = make_int4(c.x + s[t].x, c.y + s[t].y, c.z + s[t].z, c.w + s[t].w);
        __syncthreads();
    }
}

__device__ inline int4 prefix(const int4 *pre, const int4 *wg, int i)
{
    const int4 a = pre[i], b = wg[i / kScanWG];
    return make_int4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

__global__ __launch_bounds__(kSyncWG) void jpeg_write_kernel(const unsigned char *in, int64_t tab_off, JpegGeom g, const JpegLane *lanes,
                                                             const int4 *pre, const int4 *wg, const unsigned int *flags, short *coef,
                                                             unsigned int *status)
{
    __shared__ JpegHuff tab[3][2];
    if (flags[SFD2_JPEG_SYNC_LAUNCHES - 1]) {          // the last launch still changed a lane: not synchronised
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, SFD2_JPEG_NO_SYNC);
        return;
    }
    load_tables(in, tab_off, g.ncomp, tab);
    __syncthreads();
    const Prepared P = prepared(in, tab_off, g);
    const int i = blockIdx.x * kSyncWG + threadIdx.x;
    if (i >= g.nlanes) return;
    const LaneCtx lc = lane_ctx(P.lane_start, P.lane_int, P.int_first, i);
    const JpegLane rec = lanes[i];
    if (rec.bad) { atomicOr(status, SFD2_JPEG_BAD_CODE); return; }
    const int4 me = prefix(pre, wg, i), hd = prefix(pre, wg, (int)P.int_first[lc.interval]);
    const int base = me.x;
    if (base % g.bpm != rec.su) atomicOr(status, SFD2_JPEG_BAD_COUNT);
    if (lc.head && base != (g.ri_blocks ? lc.interval * g.ri_blocks : 0)) atomicOr(status, SFD2_JPEG_BAD_COUNT);
    if (i == g.nlanes - 1 && base + rec.cnt != g.total_blocks) atomicOr(status, SFD2_JPEG_BAD_COUNT);
    if (lc.last_in_int && rec.epos != lc.end) atomicOr(status, SFD2_JPEG_BAD_END);
    int pred[3] = {me.y - hd.y, me.z - hd.z, me.w - hd.w};
    Bits br;
    br.d = P.words;
    br.nw = g.ecs_words;
    JpegLane again;
    decode_lane<true>(br, tab, g, lc, rec.spos, rec.su, again, base, pred, coef, status);
    if (again.bad || again.cnt != rec.cnt) atomicOr(status, SFD2_JPEG_BAD_CODE);
}

// ---------------------------------------------------------------------------------------------------- IDCT (jidctint.c, islow)
constexpr int kIdctBlocks = 32;    // 8 threads per block

// The arithmetic of libjpeg-turbo's SIMD "islow" (what PIL runs on x86-64), pinned against PIL's output on blocks of one to four
// coefficients under 16-bit quantisation tables (tests/test_gpu_jpeg_crafted.py): the dequantised coefficient is the low 16 bits of
// coef * quantval; the sums in0 +- in4, in7 + in3 and in5 + in1 of both passes are 16-bit word additions that wrap; pass 1's outputs are
// saturated to 16 bits and the samples to [0, 255] around 128; and a block whose rows 1-7 hold no coefficient skips pass 1 for a 16-bit
// shift of row 0, which wraps where the full pass would saturate.  Where nothing leaves 16 bits -- every valid 8-bit stream short of
// extreme quantisation -- this is jidctint.c's C arithmetic exactly.
__device__ inline int sat16(int x) { return x < -32768 ? -32768 : x > 32767 ? 32767 : x; }
__device__ inline int wrap16(int x) { return (int)(short)x; }

__device__ inline unsigned char idct_limit(int x)
{
    x += 128;
    return (unsigned char)(x < 0 ? 0 : x > 255 ? 255 : x);
}

#define FIX_0_298631336 2446
#define FIX_0_390180644 3196
#define FIX_0_541196100 4433
#define FIX_0_765366865 6270
#define FIX_0_899976223 7373
#define FIX_1_175875602 9633
#define FIX_1_501321110 12299
#define FIX_1_847759065 15137
#define FIX_1_961570560 16069
#define FIX_2_053119869 16819
#define FIX_2_562915447 20995
#define FIX_3_072711026 25172

// the 1-D 8-point IDCT of both passes; in[] already dequantised / scaled, out[] before the final descale
__device__ inline void idct8(const int *in, int *out, int shift)
{
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * FIX_0_541196100;
    int tmp2 = z1 + z3 * (-FIX_1_847759065);
    int tmp3 = z1 + z2 * FIX_0_765366865;
    z2 = in[0];
    z3 = in[4];
    int tmp0 = wrap16(z2 + z3) * (1 << 13);
    int tmp1 = wrap16(z2 - z3) * (1 << 13);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7];
    tmp1 = in[5];
    tmp2 = in[3];
    tmp3 = in[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = wrap16(tmp0 + tmp2);
    int z4 = wrap16(tmp1 + tmp3);
    const int z5 = (z3 + z4) * FIX_1_175875602;
    tmp0 = tmp0 * FIX_0_298631336;
    tmp1 = tmp1 * FIX_2_053119869;
    tmp2 = tmp2 * FIX_3_072711026;
    tmp3 = tmp3 * FIX_1_501321110;
    z1 = z1 * (-FIX_0_899976223);
    z2 = z2 * (-FIX_2_562915447);
    z3 = z3 * (-FIX_1_961570560);
    z4 = z4 * (-FIX_0_390180644);
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const int rnd = 1 << (shift - 1);
    out[0] = (tmp10 + tmp3 + rnd) >> shift;
    out[7] = (tmp10 - tmp3 + rnd) >> shift;
    out[1] = (tmp11 + tmp2 + rnd) >> shift;
    out[6] = (tmp11 - tmp2 + rnd) >> shift;
    out[2] = (tmp12 + tmp1 + rnd) >> shift;
    out[5] = (tmp12 - tmp1 + rnd) >> shift;
    out[3] = (tmp13 + tmp0 + rnd) >> shift;
    out[4] = (tmp13 - tmp0 + rnd) >> shift;
}

__global__ __launch_bounds__(kIdctBlocks * 8) void jpeg_idct_kernel(const unsigned char *in, int64_t tab_off, JpegGeom g,
                                                                    const short *coef, unsigned char *planes)
{
    __shared__ int ws[kIdctBlocks][64];
    const int lb = threadIdx.x >> 3, t = threadIdx.x & 7;
    const int b = blockIdx.x * kIdctBlocks + lb;
    const bool active = b < g.total_blocks;
    const JpegTables *tabs = reinterpret_cast<const JpegTables *>(in + tab_off);
    int c = 0;
    if (active) {
        c = (g.ncomp == 3 && b >= g.blk_base[2]) ? 2 : (g.ncomp == 3 && b >= g.blk_base[1]) ? 1 : 0;
        // pass 1: column t, dequantised (libjpeg: coef * quantval), scaled up by PASS1_BITS = 2
        const short *cb = coef + (int64_t)b * 64;
        const uint16_t *q = tabs->q[c];
        int x[8], y[8];
        int ac = 0;                                        // any coefficient in rows 1-7 of the block (its 8 threads share a wave)
        for (int r = 1; r < 8; ++r) ac |= cb[r * 8 + t];
        for (int m = 1; m < 8; m <<= 1) ac |= __shfl_xor(ac, m, 8);
        for (int r = 0; r < 8; ++r) x[r] = wrap16((int)cb[r * 8 + t] * (int)q[r * 8 + t]);
        if (ac) {
            idct8(x, y, 13 - 2);
            for (int r = 0; r < 8; ++r) ws[lb][r * 8 + t] = sat16(y[r]);
        } else {
            for (int r = 0; r < 8; ++r) ws[lb][r * 8 + t] = wrap16(x[0] * 4);
        }
    }
    __syncthreads();
    if (!active) return;
    int x[8], y[8];
    for (int k = 0; k < 8; ++k) x[k] = ws[lb][t * 8 + k];
    idct8(x, y, 13 + 2 + 3);
    const int local = b - g.blk_base[c], bx = local % g.bw[c], by = local / g.bw[c];
    const int pitch = g.bw[c] * 8;
    unsigned char *o = planes + g.plane_off[c] + (int64_t)(by * 8 + t) * pitch + bx * 8;
    uint32_t lo = 0, hi = 0;
    for (int k = 0; k < 4; ++k) lo |= (uint32_t)idct_limit(y[k]) << (8 * k);
    for (int k = 0; k < 4; ++k) hi |= (uint32_t)idct_limit(y[4 + k]) << (8 * k);
    *reinterpret_cast<uint2 *>(o) = make_uint2(lo, hi);
}

// ---------------------------------------------------------------------------------------------------- upsampling + colour
// h2v1 fancy (jdsample.c): out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2, the end samples copied
__device__ inline int up_h2v1(const unsigned char *row, int cw, int x)
{
    const int i = x >> 1;
    if (cw <= 2) return row[i];                          // libjpeg upsamples so narrow a component by replication
    const int v = row[i];
    if (!(x & 1)) return i == 0 ? v : (3 * v + row[i - 1] + 1) >> 2;
    return i == cw - 1 ? v : (3 * v + row[i + 1] + 2) >> 2;
}

// h2v2 fancy: column sums 3 * nearer row + further row (rows above / below replicated at the edges), then
// (3 * this + neighbour + 8 or 7) >> 4
__device__ inline int up_h2v2(const unsigned char *plane, int pitch, int cw, int ch, int x, int y)
{
    const int i = x >> 1, j = y >> 1;
    const unsigned char *near = plane + (int64_t)j * pitch;
    if (cw <= 2) return near[i];
    const int jf = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
    const unsigned char *far = plane + (int64_t)jf * pitch;
    const int cs = 3 * near[i] + far[i];
    if (!(x & 1)) return i == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
    return i == cw - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
}

__device__ inline unsigned char clamp255(int v) { return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v); }

__global__ __launch_bounds__(256) void jpeg_color_kernel(const unsigned char *planes, JpegGeom g, unsigned char *out)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.W) return;
    const int p0 = g.bw[0] * 8;
    const int Y = planes[g.plane_off[0] + (int64_t)y * p0 + x];
    uint32_t px;
    if (g.mode == 0) {
        px = (uint32_t)Y * 0x010101u | 0xFF000000u;
    } else {
        const int p1 = g.bw[1] * 8;
        const unsigned char *P1 = planes + g.plane_off[1], *P2 = planes + g.plane_off[2];
        int cb, cr;
        if (g.mode == 1) {
            cb = P1[(int64_t)y * p1 + x];
            cr = P2[(int64_t)y * p1 + x];
        } else if (g.mode == 2) {
            cb = up_h2v1(P1 + (int64_t)y * p1, g.cw, x);
            cr = up_h2v1(P2 + (int64_t)y * p1, g.cw, x);
        } else {
            cb = up_h2v2(P1, p1, g.cw, g.ch, x, y);
            cr = up_h2v2(P2, p1, g.cw, g.ch, x, y);
        }
        // jdcolor.c: R = y + Cr_r[cr], G = y + ((Cb_g[cb] + Cr_g[cr]) >> 16), B = y + Cb_b[cb] (SCALEBITS 16)
        const int xb = cb - 128, xr = cr - 128;
        const int R = Y + ((91881 * xr + 32768) >> 16);
        const int G = Y + ((-46802 * xr + -22554 * xb + 32768) >> 16);
        const int B = Y + ((116130 * xb + 32768) >> 16);
        px = (uint32_t)clamp255(R) | (uint32_t)clamp255(G) << 8 | (uint32_t)clamp255(B) << 16 | 0xFF000000u;
    }
    reinterpret_cast<uint32_t *>(out)[(int64_t)y * g.W + x] = px;
}

}  // namespace

void launch_jpeg_decode(hipStream_t st, const unsigned char *in, int64_t tab_off, const JpegGeom &g, JpegLane *lanes, int *lane_pre,
                        int *wg_pre, unsigned int *sync_flags, short *coef, unsigned char *planes, unsigned char *out_rgbx,
                        unsigned int *status)
{
    const int nl = g.nlanes;
    const unsigned sync_grid = (unsigned)((nl + kSyncWG - 1) / kSyncWG), scan_grid = (unsigned)((nl + kScanWG - 1) / kScanWG);
    for (int it = 0; it < SFD2_JPEG_SYNC_LAUNCHES; ++it)
        hipLaunchKernelGGL(jpeg_sync_kernel, dim3(sync_grid), dim3(kSyncWG), 0, st, in, tab_off, g, lanes, sync_flags, it);
    hipLaunchKernelGGL(jpeg_sync_serial_kernel, dim3(1), dim3(kSyncWG), 0, st, in, tab_off, g, lanes, sync_flags);
    int4 *pre = reinterpret_cast<int4 *>(lane_pre), *wg = reinterpret_cast<int4 *>(wg_pre);
    hipLaunchKernelGGL(jpeg_scan_local_kernel, dim3(scan_grid), dim3(kScanWG), 0, st, lanes, nl, pre, wg);
    hipLaunchKernelGGL(jpeg_scan_top_kernel, dim3(1), dim3(kScanWG), 0, st, wg, (int)scan_grid);
    hipLaunchKernelGGL(jpeg_write_kernel, dim3(sync_grid), dim3(kSyncWG), 0, st, in, tab_off, g, lanes, pre, wg, sync_flags, coef, status);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((g.total_blocks + kIdctBlocks - 1) / kIdctBlocks)), dim3(kIdctBlocks * 8), 0, st,
                       in, tab_off, g, coef, planes);
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((g.W + 255) / 256), (unsigned)g.H), dim3(256), 0, st, planes, g, out_rgbx);
}
