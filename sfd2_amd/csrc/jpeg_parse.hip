// libsfd2hip: the host side of the baseline JPEG decoder -- header parser (sfd2_jpeg_parse) and the in-place preparation of the
// entropy-coded data for the device (sfd2_jpeg_prepare).  Host C++ only: no context, no device.
//
// Written from ITU-T T.81 (markers B.1-B.2, Huffman table specification C, restart intervals B.2.5 / F.1.2.3) and libjpeg's
// published colour-space conventions (JFIF, Adobe APP14 transform, component ids).  Every read is checked against [data, data + n).
#include "sfd2_ctx.h"

namespace {

const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Hdr {                       // what the parse keeps beyond sfd2_jpeg_info: the tables the scan uses
    uint8_t comp_id[4] = {}, tq[4] = {}, td[4] = {}, ta[4] = {};
    uint16_t qt[4][64] = {};       // natural order
    bool qt_ok[4] = {};
    uint8_t hbits[8][17] = {};     // [0..3] DC, [4..7] AC; hbits[t][l] = codes of length l
    uint8_t hvals[8][256] = {};
    int hcount[8] = {};
    bool h_ok[8] = {};
};

int reject(sfd2_jpeg_info *info, int reason, const char *what)
{
    info->supported = 0;
    info->reason = reason;
    return fail(std::string("sfd2_jpeg_parse: ") + what);
}

inline int be16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

// T.81 C.2 / libjpeg's check: codes are assigned in order of length; after the codes of length l the next code must stay
// below 2^l (so no code is all ones)
bool huff_valid(const uint8_t *bits)
{
    long code = 0;
    for (int l = 1; l <= 16; ++l) {
        code += bits[l];
        if (code >= (1L << l)) return false;
        code <<= 1;
    }
    return true;
}

void build_huff(const uint8_t *bits, const uint8_t *vals, JpegHuff *h)
{
    memset(h, 0, sizeof(*h));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        h->valoff[l] = k - code;
        h->maxcode[l] = bits[l] ? code + bits[l] - 1 : -1;
        for (int i = 0; i < bits[l]; ++i, ++code, ++k) {
            if (l <= 9) {
                const int base = code << (9 - l);
                for (int e = 0; e < (1 << (9 - l)); ++e) h->lut[base + e] = (uint16_t)((l << 8) | vals[k]);
            }
        }
        code <<= 1;
    }
    h->maxcode[0] = -1;
    h->maxcode[17] = 0x7fffffff;
    memcpy(h->vals, vals, 256);
}

// The whole parse.  Leaves info filled (supported / reason) and the scan's tables in hd.
int parse(const uint8_t *d, int64_t n, sfd2_jpeg_info *info, Hdr *hd)
{
    memset(info, 0, sizeof(*info));
    info->file_bytes = n;
    if (n < 2) return reject(info, n == 1 && d[0] == 0xFF ? SFD2_JPEG_TRUNCATED : SFD2_JPEG_NOT_JPEG, "not a JPEG (too short)");
    if (d[0] != 0xFF || d[1] != 0xD8) return reject(info, SFD2_JPEG_NOT_JPEG, "not a JPEG (no SOI)");
    int64_t pos = 2;
    bool sof = false, jfif = false;
    int adobe = -1, nf = 0, P = 0;
    for (;;) {
        if (pos >= n) return reject(info, SFD2_JPEG_TRUNCATED, "truncated before the scan");
        if (d[pos] != 0xFF) return reject(info, SFD2_JPEG_MALFORMED, "marker expected");
        while (pos < n && d[pos] == 0xFF) ++pos;                       // fill bytes
        if (pos >= n) return reject(info, SFD2_JPEG_TRUNCATED, "truncated before the scan");
        const int m = d[pos++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD9) || m == 0x00) return reject(info, SFD2_JPEG_MALFORMED, "unexpected marker before the scan");
        if (pos + 2 > n) return reject(info, SFD2_JPEG_TRUNCATED, "truncated segment length");
        const int L = be16(d + pos);
        if (L < 2) return reject(info, SFD2_JPEG_MALFORMED, "bad segment length");
        if (pos + L > n) return reject(info, SFD2_JPEG_TRUNCATED, "truncated segment");
        const uint8_t *s = d + pos + 2;
        const int sl = L - 2;
        pos += L;
        if (m == 0xC0 || m == 0xC1 || m == 0xC2 || m == 0xC6) {
            if (sof) return reject(info, SFD2_JPEG_MALFORMED, "second frame header");
            sof = true;
            if (sl < 6) return reject(info, SFD2_JPEG_MALFORMED, "short frame header");
            P = s[0];
            info->height = be16(s + 1);
            info->width = be16(s + 3);
            nf = s[5];
            if (sl < 6 + 3 * nf) return reject(info, SFD2_JPEG_MALFORMED, "short frame header");
            info->n_components = nf;
            for (int c = 0; c < nf && c < 4; ++c) {
                hd->comp_id[c] = s[6 + 3 * c];
                const int hv = s[7 + 3 * c];
                if (c < 3) { info->h_samp[c] = hv >> 4; info->v_samp[c] = hv & 15; }
                hd->tq[c] = s[8 + 3 * c];
                if ((hv >> 4) < 1 || (hv >> 4) > 4 || (hv & 15) < 1 || (hv & 15) > 4 || hd->tq[c] > 3)
                    return reject(info, SFD2_JPEG_MALFORMED, "bad component in the frame header");
            }
            if (m == 0xC2 || m == 0xC6) return reject(info, SFD2_JPEG_PROGRESSIVE, "progressive JPEG");
            if (P != 8) return reject(info, SFD2_JPEG_PRECISION, "sample precision is not 8 bits");
            if (info->height == 0) return reject(info, SFD2_JPEG_PROCESS, "height defined by DNL");
            if (info->width == 0 || nf == 0) return reject(info, SFD2_JPEG_MALFORMED, "empty frame");
            if (info->width > 65500 || info->height > 65500)       // libjpeg's JPEG_MAX_DIMENSION: the CPU decoders refuse these
                return reject(info, SFD2_JPEG_MALFORMED, "frame wider or taller than 65500");
        } else if (m == 0xC3 || m == 0xC5 || m == 0xC7) {
            return reject(info, SFD2_JPEG_PROCESS, "lossless or hierarchical JPEG");
        } else if (m >= 0xC9 && m <= 0xCF) {           // SOF9-SOF15 and DAC (0xCC)
            return reject(info, SFD2_JPEG_ARITHMETIC, "arithmetic-coded JPEG");
        } else if (m == 0xC4) {
            int o = 0;
            while (o < sl) {
                if (o + 17 > sl) return reject(info, SFD2_JPEG_MALFORMED, "short DHT");
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return reject(info, SFD2_JPEG_MALFORMED, "bad DHT class / id");
                const int t = tc * 4 + th;
                int cnt = 0;
                hd->hbits[t][0] = 0;
                for (int l = 1; l <= 16; ++l) { hd->hbits[t][l] = s[o + l]; cnt += s[o + l]; }
                if (cnt > 256 || o + 17 + cnt > sl) return reject(info, SFD2_JPEG_MALFORMED, "bad DHT counts");
                if (!huff_valid(hd->hbits[t])) return reject(info, SFD2_JPEG_MALFORMED, "bad Huffman table");
                memset(hd->hvals[t], 0, 256);
                memcpy(hd->hvals[t], s + o + 17, cnt);
                hd->hcount[t] = cnt;
                hd->h_ok[t] = true;
                o += 17 + cnt;
            }
        } else if (m == 0xDB) {
            int o = 0;
            while (o < sl) {
                const int pq = s[o] >> 4, t = s[o] & 15;
                if (pq > 1 || t > 3) return reject(info, SFD2_JPEG_MALFORMED, "bad DQT precision / id");
                if (o + 1 + 64 * (pq + 1) > sl) return reject(info, SFD2_JPEG_MALFORMED, "short DQT");
                for (int k = 0; k < 64; ++k)
                    hd->qt[t][kNatural[k]] = (uint16_t)(pq ? be16(s + o + 1 + 2 * k) : s[o + 1 + k]);
                hd->qt_ok[t] = true;
                o += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xDD) {
            if (sl < 2) return reject(info, SFD2_JPEG_MALFORMED, "short DRI");
            info->restart_interval = be16(s);
        } else if (m == 0xE0) {
            if (sl >= 14 && !memcmp(s, "JFIF\0", 5)) jfif = true;    // libjpeg: only with the 14 data bytes of a JFIF header
        } else if (m == 0xEE) {
            if (sl >= 12 && !memcmp(s, "Adobe", 5)) adobe = s[11];
        } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE) {
            // other application segments and comments (EXIF orientation is ignored, as the CPU decoders here ignore it)
        } else if (m == 0xDC) {
            return reject(info, SFD2_JPEG_PROCESS, "DNL segment");
        } else if (m == 0xDA) {
            if (!sof) return reject(info, SFD2_JPEG_MALFORMED, "scan before the frame header");
            if (sl < 1) return reject(info, SFD2_JPEG_MALFORMED, "short SOS");
            const int ns = s[0];
            if (sl < 1 + 2 * ns + 3) return reject(info, SFD2_JPEG_MALFORMED, "short SOS");
            if (nf != 1 && nf != 3) return reject(info, SFD2_JPEG_COLOUR, "neither 1 nor 3 components");
            if (ns != nf) return reject(info, SFD2_JPEG_MULTI_SCAN, "the scan does not hold every component");
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != hd->comp_id[c]) return reject(info, SFD2_JPEG_MULTI_SCAN, "scan components out of frame order");
                hd->td[c] = s[2 + 2 * c] >> 4;
                hd->ta[c] = s[2 + 2 * c] & 15;
                if (hd->td[c] > 3 || hd->ta[c] > 3 || !hd->h_ok[hd->td[c]] || !hd->h_ok[4 + hd->ta[c]] || !hd->qt_ok[hd->tq[c]])
                    return reject(info, SFD2_JPEG_MALFORMED, "the scan uses an undefined table");
                for (int k = 0; k < hd->hcount[hd->td[c]]; ++k)
                    if (hd->hvals[hd->td[c]][k] > 11) return reject(info, SFD2_JPEG_MALFORMED, "DC table symbol above 11");
            }
            const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ahal = s[3 + 2 * ns];
            if (ss != 0 || se != 63 || ahal != 0) return reject(info, SFD2_JPEG_MALFORMED, "not a sequential scan");
            if (nf == 3) {
                const bool rgb_ids = hd->comp_id[0] == 'R' && hd->comp_id[1] == 'G' && hd->comp_id[2] == 'B';
                if (!jfif && ((adobe >= 0 && adobe == 0) || (adobe < 0 && rgb_ids)))
                    return reject(info, SFD2_JPEG_COLOUR, "RGB colour space (no YCbCr transform)");
                const int h0 = info->h_samp[0], v0 = info->v_samp[0];
                const bool luma_ok = (h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2);
                for (int c = 1; c < 3; ++c)
                    if (info->h_samp[c] != 1 || info->v_samp[c] != 1) return reject(info, SFD2_JPEG_SAMPLING, "chroma sampling other than 1x1");
                if (!luma_ok) return reject(info, SFD2_JPEG_SAMPLING, "luma sampling other than 1x1, 2x1, 2x2");
                info->mcus_x = (info->width + 8 * h0 - 1) / (8 * h0);
                info->mcus_y = (info->height + 8 * v0 - 1) / (8 * v0);
                info->n_blocks = 0;
                if ((int64_t)info->width * info->height > (1 << 28)) return reject(info, SFD2_JPEG_MALFORMED, "image too large");
                info->n_blocks = info->mcus_x * info->mcus_y * (h0 * v0 + 2);
            } else {
                if ((int64_t)info->width * info->height > (1 << 28)) return reject(info, SFD2_JPEG_MALFORMED, "image too large");
                info->mcus_x = (info->width + 7) / 8;
                info->mcus_y = (info->height + 7) / 8;
                info->n_blocks = info->mcus_x * info->mcus_y;
            }
            const int64_t mcus = (int64_t)info->mcus_x * info->mcus_y;
            const int ri = info->restart_interval;
            info->n_intervals = ri ? (int)((mcus + ri - 1) / ri) : 1;
            info->scan_begin = pos;
            // the entropy-coded data: FF 00 is a stuffed FF, FF D0-D7 a restart marker (in order), fill FFs may precede a marker;
            // the first other marker ends the scan and must be the EOI
            int64_t p = pos;
            int rst = 0;
            for (;;) {
                const uint8_t *q = p < n ? static_cast<const uint8_t *>(memchr(d + p, 0xFF, (size_t)(n - p))) : nullptr;
                if (!q) return reject(info, SFD2_JPEG_TRUNCATED, "truncated scan (no EOI)");
                const int64_t at = q - d;
                if (at + 1 >= n) return reject(info, SFD2_JPEG_TRUNCATED, "truncated scan (no EOI)");
                if (d[at + 1] == 0x00) { p = at + 2; continue; }
                int64_t r = at + 1;
                while (r < n && d[r] == 0xFF) ++r;
                if (r >= n) return reject(info, SFD2_JPEG_TRUNCATED, "truncated scan (no EOI)");
                const int mk = d[r];
                if (mk == 0x00) return reject(info, SFD2_JPEG_MALFORMED, "fill bytes in front of a stuffed byte");
                if (mk >= 0xD0 && mk <= 0xD7) {
                    if ((mk & 7) != (rst & 7)) return reject(info, SFD2_JPEG_MALFORMED, "restart markers out of sequence");
                    ++rst;
                    if (rst >= info->n_intervals) return reject(info, SFD2_JPEG_MALFORMED, "more restart markers than intervals");
                    p = r + 1;
                    continue;
                }
                info->scan_end = at;
                if (mk != 0xD9) return reject(info, mk == 0x01 ? SFD2_JPEG_MALFORMED : SFD2_JPEG_MULTI_SCAN, "more than one scan");
                break;
            }
            if (rst != info->n_intervals - 1) return reject(info, SFD2_JPEG_MALFORMED, "restart marker count differs from the intervals");
            const int64_t ecs = info->scan_end - info->scan_begin;
            if (ecs > (int64_t)1 << 28) return reject(info, SFD2_JPEG_MALFORMED, "scan too large");
            const int64_t lanes_max = ecs * 8 / SFD2_JPEG_LANE_BITS + info->n_intervals + 1;
            info->prepared_cap = std::max<int64_t>(n, ((ecs + 15) & ~(int64_t)15) + 16 + jpeg_tail_bytes(lanes_max, info->n_intervals));
            info->supported = 1;
            info->reason = SFD2_JPEG_OK;
            return 0;
        } else {
            return reject(info, SFD2_JPEG_MALFORMED, "unknown marker");
        }
    }
}

}  // namespace

extern "C" int sfd2_jpeg_parse(const uint8_t *data, int64_t n, sfd2_jpeg_info *info)
{
    if (!info) return fail("sfd2_jpeg_parse: info is null");
    if (!data && n > 0) return fail("sfd2_jpeg_parse: data is null");
    if (n < 0) n = 0;
    Hdr hd;
    return parse(data, n, info, &hd);
}

extern "C" int sfd2_jpeg_prepare(uint8_t *buf, int64_t cap, sfd2_jpeg_info *info)
{
    if (!buf || !info) return fail("sfd2_jpeg_prepare: null argument");
    const int64_t n = info->file_bytes;
    if (n < 0 || n > cap) return fail("sfd2_jpeg_prepare: file_bytes exceeds the buffer");
    Hdr hd;
    if (parse(buf, n, info, &hd)) return -1;
    if (cap < info->prepared_cap) return fail("sfd2_jpeg_prepare: the buffer holds fewer than prepared_cap bytes");
    JpegTables tab;
    memset(&tab, 0, sizeof(tab));
    for (int c = 0; c < info->n_components; ++c) {
        build_huff(hd.hbits[hd.td[c]], hd.hvals[hd.td[c]], &tab.huff[c][0]);
        build_huff(hd.hbits[4 + hd.ta[c]], hd.hvals[4 + hd.ta[c]], &tab.huff[c][1]);
        memcpy(tab.q[c], hd.qt[hd.tq[c]], sizeof(tab.q[c]));
    }
    // destuff in place: the output never overtakes the input (it starts at 0, the input at scan_begin >= 2 and shrinks)
    std::vector<uint32_t> starts(1, 0);
    starts.reserve(info->n_intervals);
    int64_t w = 0, p = info->scan_begin;
    const int64_t end = info->scan_end;
    while (p < end) {
        const uint8_t *q = static_cast<const uint8_t *>(memchr(buf + p, 0xFF, (size_t)(end - p)));
        const int64_t at = q ? q - buf : end;
        if (at > p) { memmove(buf + w, buf + p, (size_t)(at - p)); w += at - p; }
        if (at >= end) break;
        if (buf[at + 1] == 0x00) { buf[w++] = 0xFF; p = at + 2; continue; }
        int64_t r = at + 1;
        while (buf[r] == 0xFF) ++r;                                // (the parse saw a marker behind these fill bytes)
        starts.push_back((uint32_t)w);                              // RSTn: the next interval starts on this byte
        p = r + 1;
    }
    if ((int)starts.size() != info->n_intervals) return fail("sfd2_jpeg_prepare: restart intervals differ from the parse");
    const int64_t tab_off = ((w + 15) & ~(int64_t)15) + 16;
    memset(buf + w, 0, (size_t)(tab_off - w));
    int64_t L = 0;
    for (int j = 0; j < info->n_intervals; ++j) {
        const int64_t bits = 8 * ((j + 1 < info->n_intervals ? (int64_t)starts[j + 1] : w) - starts[j]);
        L += std::max<int64_t>(1, (bits + SFD2_JPEG_LANE_BITS - 1) / SFD2_JPEG_LANE_BITS);
    }
    const int64_t need = tab_off + jpeg_tail_bytes(L, info->n_intervals);
    if (need > cap) return fail("sfd2_jpeg_prepare: buffer too small");
    memcpy(buf + tab_off, &tab, sizeof(tab));
    uint32_t *lane_start = reinterpret_cast<uint32_t *>(buf + tab_off + sizeof(JpegTables));
    uint32_t *lane_int = lane_start + L + 1;
    uint32_t *int_first = lane_int + L;
    int64_t l = 0;
    for (int j = 0; j < info->n_intervals; ++j) {
        const int64_t b0 = 8 * (int64_t)starts[j], b1 = 8 * (j + 1 < info->n_intervals ? (int64_t)starts[j + 1] : w);
        const int64_t nl = std::max<int64_t>(1, (b1 - b0 + SFD2_JPEG_LANE_BITS - 1) / SFD2_JPEG_LANE_BITS);
        int_first[j] = (uint32_t)l;
        for (int64_t t = 0; t < nl; ++t, ++l) {
            lane_start[l] = (uint32_t)std::min(b0 + t * SFD2_JPEG_LANE_BITS, b1);
            lane_int[l] = (uint32_t)j;
        }
    }
    lane_start[L] = (uint32_t)(8 * w);
    int_first[info->n_intervals] = (uint32_t)L;
    info->n_lanes = (int32_t)L;
    info->prepared_bytes = need;
    info->prepared = 1;
    return 0;
}
