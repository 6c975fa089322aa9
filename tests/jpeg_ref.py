"""Test-only helpers for the baseline JPEG decoder, written from ITU-T T.81: a marker-level reader / writer with edit helpers (Annex B),
a baseline Huffman entropy decoder and encoder (F.1.2 / F.2.2, byte stuffing, restart markers) that together transcode a file -- other
tables, table ids, restart intervals, padding -- without changing what it decodes to, Huffman tables from a bits / vals pair (C.2) or
from symbol counts (K.2), image content generators, and the crafted families the host and GPU tests iterate (MUST_SUPPORT,
MUST_REFUSE, SAME_OR_REFUSED).  The product never imports this file."""
import functools
import io
import re

import numpy as np

SOF0, SOF1, DHT, SOI, EOI, SOS, DQT, DRI, APP0, APP1, APP14, COM = 0xC0, 0xC1, 0xC4, 0xD8, 0xD9, 0xDA, 0xDB, 0xDD, 0xE0, 0xE1, 0xEE, 0xFE

# zigzag position k -> natural (row-major) index (T.81 figure A.6)
NATURAL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


# ------------------------------------------------------------------------------------------------ marker level
class Jpeg:
    """segs: [(marker, payload)] from behind SOI up to and including SOS; ecs: the entropy-coded bytes as they stand in the file (stuffing
    and RSTn included); tail: from the marker that ends the scan (EOI) to the end of the file."""

    def __init__(self, segs, ecs, tail):
        self.segs, self.ecs, self.tail = list(segs), bytes(ecs), bytes(tail)

    def copy(self):
        return Jpeg(self.segs, self.ecs, self.tail)

    def find(self, *markers):
        return [i for i, (m, _) in enumerate(self.segs) if m in markers]

    @property
    def sof(self):
        return self.find(SOF0, SOF1)[0]


def read(data):
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    pos, segs = 2, []
    while True:
        assert data[pos] == 0xFF, "marker expected"
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        n = (data[pos + 1] << 8) | data[pos + 2]
        segs.append((m, data[pos + 3:pos + 1 + n]))
        pos += 1 + n
        if m == SOS:
            break
    p = pos
    while True:
        p = data.index(b"\xff", p)
        q = p + 1
        while data[q] == 0xFF:
            q += 1
        if data[q] == 0 or 0xD0 <= data[q] <= 0xD7:
            p = q + 1
            continue
        break
    return Jpeg(segs, data[pos:p], data[p:])


def write(j, fill=0, fill_rst=0, fill_eoi=0):
    """The file.  fill: FF bytes in front of every header marker (an int, or {segment index: count}); fill_rst / fill_eoi: in front of every
    RSTn / of the marker that ends the scan."""
    out = bytearray(b"\xff\xd8")
    for i, (m, payload) in enumerate(j.segs):
        assert len(payload) + 2 <= 65535, "segment too long"
        out += b"\xff" * (fill.get(i, 0) if isinstance(fill, dict) else fill)
        out += bytes([0xFF, m, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + payload
    ecs = j.ecs
    if fill_rst:       # (inside the entropy-coded data FF is followed by 00 unless it starts a marker)
        ecs = re.sub(rb"\xff([\xd0-\xd7])", lambda mo: b"\xff" * (fill_rst + 1) + mo.group(1), ecs)
    return bytes(out) + ecs + b"\xff" * fill_eoi + j.tail


def frame(j):
    """The frame header: dict(marker, precision, height, width, comps=[(id, h, v, tq)])."""
    m, s = j.segs[j.sof]
    return dict(marker=m, precision=s[0], height=(s[1] << 8) | s[2], width=(s[3] << 8) | s[4],
                comps=[(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])])


def scan_header(j):
    s = j.segs[-1][1]
    return [(s[1 + 2 * c], s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(s[0])]


def restart_interval(j):
    ri = 0
    for m, s in j.segs:
        if m == DRI:
            ri = (s[0] << 8) | s[1]
    return ri


def parse_dqt(payload):
    """[(pq, id, [64 values in zigzag order])]"""
    out, o = [], 0
    while o < len(payload):
        pq, t = payload[o] >> 4, payload[o] & 15
        if pq:
            v = [(payload[o + 1 + 2 * k] << 8) | payload[o + 2 + 2 * k] for k in range(64)]
        else:
            v = list(payload[o + 1:o + 65])
        out.append((pq, t, v))
        o += 1 + 64 * (pq + 1)
    return out


def make_dqt(tables):
    out = bytearray()
    for pq, t, v in tables:
        out.append((pq << 4) | t)
        for x in v:
            out += bytes([x >> 8, x & 255]) if pq else bytes([x])
    return bytes(out)


def parse_dht(payload):
    """[(class, id, bits[16], vals)]"""
    out, o = [], 0
    while o < len(payload):
        bits = list(payload[o + 1:o + 17])
        n = sum(bits)
        out.append((payload[o] >> 4, payload[o] & 15, bits, list(payload[o + 17:o + 17 + n])))
        o += 17 + n
    return out


def make_dht(tables):
    return b"".join(bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals) for tc, th, bits, vals in tables)


def tables(j):
    """The tables in force at the scan (the last definition of each id): ({id: (pq, values)}, {(class, id): (bits, vals)})."""
    q, h = {}, {}
    for m, s in j.segs:
        if m == DQT:
            for pq, t, v in parse_dqt(s):
                q[t] = (pq, v)
        elif m == DHT:
            for tc, th, bits, vals in parse_dht(s):
                h[(tc, th)] = (bits, vals)
    return q, h


# ------------------------------------------------------------------------------------------------ edits (each returns a new Jpeg)
def remap_ids(j, ids):
    j = j.copy()
    i = j.sof
    m, s = j.segs[i]
    s = bytearray(s)
    for c, v in enumerate(ids):
        s[6 + 3 * c] = v if isinstance(v, int) else ord(v)
    j.segs[i] = (m, bytes(s))
    m, s = j.segs[-1]
    s = bytearray(s)
    for c, v in enumerate(ids):
        s[1 + 2 * c] = v if isinstance(v, int) else ord(v)
    j.segs[-1] = (m, bytes(s))
    return j


def drop(j, *markers):
    j = j.copy()
    j.segs = [sg for sg in j.segs if sg[0] not in markers]
    return j


def insert(j, index, marker, payload):
    j = j.copy()
    j.segs.insert(index, (marker, bytes(payload)))
    return j


JFIF_APP0 = b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"           # the 14 data bytes of a JFIF 1.01 APP0 without a thumbnail


def set_app0(j, payload):
    """Drops every APP0; puts one with this payload behind SOI (None: none)."""
    j = drop(j, APP0)
    return j if payload is None else insert(j, 0, APP0, payload)


def adobe_payload(transform):
    return b"Adobe" + bytes([0, 100, 0x80, 0, 0, 0, transform])


def set_app14(j, transform):
    """Drops every APP14; puts an Adobe one with this transform in front of the first table or frame header (None: none)."""
    j = drop(j, APP14)
    if transform is None:
        return j
    return insert(j, min(j.find(DQT, DHT, SOF0, SOF1)), APP14, adobe_payload(transform))


def map_dqt(j, fn):
    """fn(pq, id, values) -> (pq, id, values) over every table of every DQT segment."""
    j = j.copy()
    j.segs = [(m, make_dqt([fn(*t) for t in parse_dqt(s)])) if m == DQT else (m, s) for m, s in j.segs]
    return j


def dqt16(j, scale=1):
    return map_dqt(j, lambda pq, t, v: (1, t, [min(65535, x * scale) for x in v]))


def dqt_const(j, value):
    return map_dqt(j, lambda pq, t, v: (0 if value < 256 else 1, t, [value] * 64))


def _each(marker, payload):
    if marker == DQT:
        return [make_dqt([t]) for t in parse_dqt(payload)]
    return [make_dht([t]) for t in parse_dht(payload)]


def split_tables(j, marker):
    """One segment per table."""
    j = j.copy()
    j.segs = [x for m, s in j.segs for x in ([(m, p) for p in _each(m, s)] if m == marker else [(m, s)])]
    return j


def merge_tables(j, marker):
    """One segment holding every table, where the first one stood."""
    idx = j.find(marker)
    both = b"".join(j.segs[i][1] for i in idx)
    j = drop(j, marker)
    return insert(j, idx[0], marker, both)


def move_tables(j, marker, where):
    """where: 'front' (in front of the frame header) or 'behind' (between the frame header and SOS)."""
    segs = [sg for sg in j.segs if sg[0] == marker]
    j = drop(j, marker)
    at = j.sof if where == "front" else len(j.segs) - 1
    j.segs[at:at] = segs
    return j


def set_sof(j, marker=None, sampling=None, height=None, width=None):
    j = j.copy()
    i = j.sof
    m, s = j.segs[i]
    s = bytearray(s)
    for c, hv in enumerate(sampling or []):
        s[7 + 3 * c] = hv
    if height is not None:
        s[1:3] = bytes([height >> 8, height & 255])
    if width is not None:
        s[3:5] = bytes([width >> 8, width & 255])
    j.segs[i] = (m if marker is None else marker, bytes(s))
    return j


def insert_dri(j, n, index=None):
    return insert(j, len(j.segs) - 1 if index is None else index, DRI, bytes([n >> 8, n & 255]))


def insert_blob(j, marker, size, index=0, payload=None):
    """A COM / APPn segment with size payload bytes (seeded noise unless given)."""
    if payload is None:
        payload = np.random.RandomState(size).randint(0, 256, size, dtype=np.uint8).tobytes()
    return insert(j, index, marker, payload)


# ------------------------------------------------------------------------------------------------ Huffman tables
def huff_codes(bits, vals):
    """T.81 C.2: {symbol: (code, length)}; asserts the table is valid (no code of all ones, no overflow)."""
    enc, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            enc[vals[k]] = (code, l)
            code += 1
            k += 1
        assert code < (1 << l), "invalid Huffman table"
        code <<= 1
    return enc


def optimal_table(counts):
    """T.81 K.2: code lengths from symbol counts (with the reserved all-ones code point), limited to 16 bits -> (bits[16], vals)."""
    freq = [0] * 257
    for s, n in counts.items():
        freq[s] = n
    freq[256] = 1
    size, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        for i in range(257):                                 # least frequency, the larger symbol on a tie
            if freq[i] and (c1 < 0 or freq[i] <= freq[c1]):
                c1 = i
        for i in range(257):
            if freq[i] and i != c1 and (c2 < 0 or freq[i] <= freq[c2]):
                c2 = i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    bits = [0] * 40
    for i in range(257):
        if size[i]:
            bits[size[i]] += 1
    for i in range(39, 16, -1):                              # K.2 figure K.3: shorten codes longer than 16 bits
        while bits[i] > 0:
            k = i - 2
            while bits[k] == 0:
                k -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[k + 1] += 2
            bits[k] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                             # the reserved code point
    vals = [s for l in range(1, 40) for s in range(256) if size[s] == l]
    return bits[1:17], vals


def flat_table(symbols, length):
    """Every symbol gets a code of exactly this length."""
    symbols = sorted(symbols)
    assert len(symbols) < (1 << length)
    bits = [0] * 16
    bits[length - 1] = len(symbols)
    return bits, symbols


# ------------------------------------------------------------------------------------------------ entropy coding
def _layout(j):
    """(units, mcus_x, mcus_y): units = component index of every block of an MCU, in order (A.2.3; one component: A.2.2)."""
    f = frame(j)
    comps = f["comps"]
    if len(comps) == 1:
        return [0], -(-f["width"] // 8), -(-f["height"] // 8)
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    units = [ci for ci, c in enumerate(comps) for _ in range(c[1] * c[2])]
    return units, -(-f["width"] // (8 * hmax)), -(-f["height"] // (8 * vmax))


def _intervals(ecs):
    """The entropy-coded data split at its RSTn markers, destuffed."""
    parts = re.split(rb"\xff+[\xd0-\xd7]", ecs)
    return [p.replace(b"\xff\x00", b"\xff") for p in parts]


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def decode_scan(j):
    """The quantised coefficients in scan order: [(component index, [64 ints in zigzag order, DC absolute])]."""
    units, mx, my = _layout(j)
    sc = scan_header(j)
    _, h = tables(j)
    dec = []
    for _, td, ta in sc:
        dec.append(tuple({(l, c): s for s, (c, l) in huff_codes(*h[(tc, t)]).items()} for tc, t in ((0, td), (1, ta))))
    ri = restart_interval(j) or mx * my
    parts = _intervals(j.ecs)
    assert len(parts) == -(-mx * my // ri), "restart marker count"
    blocks = []
    for pi, part in enumerate(parts):
        nbits, padded = 8 * len(part), part + bytes(8)       # (room to peek past the end)
        pos = 0

        def peek():                                          # the 32 bits from pos on
            return (int.from_bytes(padded[pos >> 3:(pos >> 3) + 5], "big") >> (8 - (pos & 7))) & 0xFFFFFFFF

        def sym(table):
            nonlocal pos
            w = peek()
            for l in range(1, 17):
                s = table.get((l, w >> (32 - l)))
                if s is not None:
                    pos += l
                    return s
            raise ValueError("bad code")

        def take(n):
            nonlocal pos
            v = peek() >> (32 - n)
            pos += n
            return v

        pred = [0] * len(sc)
        for _ in range(min(ri, mx * my - pi * ri)):
            for ci in units:
                co = [0] * 64
                s = sym(dec[ci][0])
                pred[ci] += _extend(take(s), s) if s else 0
                co[0] = pred[ci]
                k = 1
                while k < 64:
                    rs = sym(dec[ci][1])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    co[k] = _extend(take(s), s)
                    k += 1
                blocks.append((ci, co))
        assert pos <= nbits, "scan ran past its interval"
    return blocks


def _symbols(blocks, ncomp, units, ri):
    """Per block: (component, [(symbol, extra value, extra bits)]) with DC differences restarting every ri MCUs."""
    out, pred = [], [0] * ncomp
    for b, (ci, co) in enumerate(blocks):
        if ri and b % (ri * len(units)) == 0:
            pred = [0] * ncomp
        d = co[0] - pred[ci]
        pred[ci] = co[0]
        s = abs(d).bit_length()
        ev = [(s, d if d >= 0 else d + (1 << s) - 1, s)]
        run = 0
        for k in range(1, 64):
            v = co[k]
            if v == 0:
                run += 1
                continue
            while run > 15:
                ev.append((0xF0, 0, 0))
                run -= 16
            s = abs(v).bit_length()
            ev.append(((run << 4) | s, v if v >= 0 else v + (1 << s) - 1, s))
            run = 0
        if run:
            ev.append((0x00, 0, 0))
        out.append((ci, ev))
    return out


def symbol_counts(blocks, ncomp, units, ri):
    """({component: {DC symbol: n}}, {component: {AC symbol: n}})"""
    dc, ac = {c: {} for c in range(ncomp)}, {c: {} for c in range(ncomp)}
    for ci, ev in _symbols(blocks, ncomp, units, ri):
        dc[ci][ev[0][0]] = dc[ci].get(ev[0][0], 0) + 1
        for s, _, _ in ev[1:]:
            ac[ci][s] = ac[ci].get(s, 0) + 1
    return dc, ac


def encode_scan(blocks, units, huff, ri=0, pad="ones", extra=None):
    """blocks as decode_scan gives them; huff: per component ((bits, vals) DC, (bits, vals) AC); ri: restart interval in MCUs.
    pad: the bits that fill the last byte of an interval, 'ones' (F.1.2.3) or 'zeros'.  extra: 'eoi' / 'rst' adds a 00 byte behind the
    last interval / behind the first one (in front of RST0)."""
    enc = [(huff_codes(*dc), huff_codes(*ac)) for dc, ac in huff]
    out = bytearray()
    acc = n = 0

    def put(code, length):
        nonlocal acc, n
        acc = (acc << length) | code
        n += length
        while n >= 8:
            b = (acc >> (n - 8)) & 255
            out.append(b)
            if b == 0xFF:
                out.append(0)
            n -= 8
        acc &= (1 << n) - 1

    def flush():
        if n:
            put(((1 << (8 - n)) - 1) if pad == "ones" else 0, 8 - n)

    per = ri * len(units)
    rst = 0
    for b, (ci, ev) in enumerate(_symbols(blocks, len(huff), units, ri)):
        if per and b and b % per == 0:
            flush()
            if extra == "rst" and rst == 0:
                out.append(0)
            out += bytes([0xFF, 0xD0 | (rst & 7)])
            rst += 1
        for k, (s, v, nb) in enumerate(ev):
            put(*enc[ci][0 if k == 0 else 1][s])
            if nb:
                put(v, nb)
    flush()
    if extra == "eoi":
        out.append(0)
    return bytes(out)


def transcode(data, dc_ids=None, ac_ids=None, tq_ids=None, ac_kind="optimal", dc_kind="optimal", ri=None, pad="ones", extra=None):
    """Decodes the scan and codes it again: Huffman table ids per component (dc_ids / ac_ids, components that share an id share one
    table built from their joint counts), quantisation table ids (tq_ids), table shapes (ac_kind 'optimal' / 'flat16'; dc_kind 'optimal' /
    'flat9' / 'flat10'), restart interval (None: as in the file), padding.  The coefficients, and so the pixels, do not change."""
    j = read(data)
    f = frame(j)
    nc = len(f["comps"])
    units, mx, my = _layout(j)
    blocks = decode_scan(j)
    sc = scan_header(j)
    dc_ids = list(dc_ids) if dc_ids is not None else [t[1] for t in sc]
    ac_ids = list(ac_ids) if ac_ids is not None else [t[2] for t in sc]
    ri = restart_interval(j) if ri is None else ri
    dcc, acc = symbol_counts(blocks, nc, units, ri)

    def joint(counts, ids, t):
        tot = {}
        for c in range(nc):
            if ids[c] == t:
                for s, n in counts[c].items():
                    tot[s] = tot.get(s, 0) + n
        return tot

    dct = {t: joint(dcc, dc_ids, t) for t in set(dc_ids)}
    act = {t: joint(acc, ac_ids, t) for t in set(ac_ids)}
    dct = {t: optimal_table(c) if dc_kind == "optimal" else flat_table(range(12), int(dc_kind[4:])) for t, c in dct.items()}
    act = {t: optimal_table(c) if ac_kind == "optimal" else flat_table(set(c) | {0}, int(ac_kind[4:])) for t, c in act.items()}
    ecs = encode_scan(blocks, units, [(dct[dc_ids[c]], act[ac_ids[c]]) for c in range(nc)], ri, pad, extra)
    q, _ = tables(j)
    tq = list(tq_ids) if tq_ids is not None else [c[3] for c in f["comps"]]
    qsegs = {}
    for c in range(nc):
        pq, v = q[f["comps"][c][3]]
        assert qsegs.setdefault(tq[c], (pq, tq[c], v)) == (pq, tq[c], v), "components with different tables cannot share an id"
    sof = bytearray(j.segs[j.sof][1])
    sos = bytearray(j.segs[-1][1])
    for c in range(nc):
        sof[8 + 3 * c] = tq[c]
        sos[2 + 2 * c] = (dc_ids[c] << 4) | ac_ids[c]
    segs = [sg for sg in j.segs[:-1] if sg[0] not in (DQT, DHT, DRI, SOF0, SOF1)]
    segs.append((DQT, make_dqt([qsegs[t] for t in sorted(qsegs)])))
    segs.append((j.segs[j.sof][0], bytes(sof)))
    segs.append((DHT, make_dht([(0, t, *dct[t]) for t in sorted(dct)] + [(1, t, *act[t]) for t in sorted(act)])))
    if ri:
        segs.append((DRI, bytes([ri >> 8, ri & 255])))
    segs.append((SOS, bytes(sos)))
    return write(Jpeg(segs, ecs, b"\xff\xd9"))


def from_blocks(template, blocks):
    """The template file with its scan replaced by these coefficient blocks (same tables, which must hold every symbol needed)."""
    j = read(template)
    units, _, _ = _layout(j)
    _, h = tables(j)
    huff = [(h[(0, td)], h[(1, ta)]) for _, td, ta in scan_header(j)]
    return write(Jpeg(j.segs, encode_scan(blocks, units, huff, restart_interval(j)), b"\xff\xd9"))


# ------------------------------------------------------------------------------------------------ files
MODES = {"444": dict(subsampling=0), "422": dict(subsampling=1), "420": dict(subsampling=2), "grey": {}}
COLOUR = ("444", "422", "420")


def content(kind, w, h, seed=0, colour=(200, 30, 90), tile=(16, 16), split="x"):
    """uint8 [h, w, 3]: 'noise'; 'flat' (colour); 'tiled' (a noise tile of tile = (w, h) repeated); 'half_flat_half_noise' (split along
    'x' or 'y'); 'block_checker' (alternating black and white 8x8 blocks); 'hard_edges' (saturated rectangles and one-pixel lines);
    'primaries' (saturated R / G / B / C / M / Y / white / black patches that ignore the block grid)."""
    rs = np.random.RandomState(seed)
    if kind == "noise":
        return rs.randint(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array(colour, dtype=np.uint8), (h, w, 3)).copy()
    if kind == "tiled":
        t = rs.randint(0, 256, (tile[1], tile[0], 3), dtype=np.uint8)
        return np.tile(t, (-(-h // tile[1]), -(-w // tile[0]), 1))[:h, :w].copy()
    if kind == "half_flat_half_noise":
        img = rs.randint(0, 256, (h, w, 3), dtype=np.uint8)
        if split == "x":
            img[:, :w // 2] = colour
        else:
            img[:h // 2] = colour
        return img
    if kind == "block_checker":
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((x // 8 + y // 8) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    if kind == "hard_edges":
        img = np.zeros((h, w, 3), dtype=np.uint8)
        for _ in range(12):
            x0, y0 = rs.randint(w), rs.randint(h)
            img[y0:y0 + 1 + rs.randint(h), x0:x0 + 1 + rs.randint(w)] = rs.randint(0, 2, 3) * 255
        for _ in range(6):
            img[rs.randint(h)] = rs.randint(0, 2, 3) * 255
            img[:, rs.randint(w)] = rs.randint(0, 2, 3) * 255
        return img
    if kind == "primaries":
        pal = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 255), (255, 255, 0), (255, 255, 255), (0, 0, 0)],
                       dtype=np.uint8)
        y, x = np.mgrid[0:h, 0:w]
        return pal[(x // 11 + 3 * (y // 7) + seed) % 8]
    raise ValueError(kind)


def encode(arr, mode, **kw):
    """PIL's encoder: mode '444' / '422' / '420' / 'grey'."""
    from PIL import Image, ImageFile
    im = Image.fromarray(arr)
    if mode == "grey":
        im = im.convert("L")
    b = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 8 * arr.size)              # (optimised tables on noise: PIL's default encoder buffer is too small)
    try:
        im.save(b, "JPEG", **MODES[mode], **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return b.getvalue()


def pil_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@functools.lru_cache(maxsize=None)
def base(mode, w=40, h=24, kind="noise", quality=90, seed=5):
    return encode(content(kind, w, h, seed), mode, quality=quality)


def geometry(data):
    """What sfd2_jpeg_parse must report for a supported file, from the headers alone."""
    j = read(data)
    f = frame(j)
    units, mx, my = _layout(j)
    ri = restart_interval(j)
    return dict(width=f["width"], height=f["height"], n_components=len(f["comps"]), mcus_x=mx, mcus_y=my,
                n_blocks=mx * my * len(units), restart_interval=ri, n_intervals=-(-mx * my // ri) if ri else 1,
                h_samp=[c[1] for c in f["comps"]], v_samp=[c[2] for c in f["comps"]])


# ------------------------------------------------------------------------------------------------ crafted families
# Every family is a function of a PIL-written source file (base(mode) unless a test picks another size).
def _mcus(src):
    _, mx, my = _layout(read(src))
    return mx, mx * my


def _edit(fn, **wr):
    return lambda src: write(fn(read(src)), **wr)


def _restarts(src, **wr):
    return write(read(transcode(src, ri=2)), **wr)


def _redefined(src):
    """Every DQT and DHT table is first defined with other contents (all-ones quantisation, a flat Huffman table), then properly."""
    j = read(src)
    q, h = tables(j)
    junk_q = make_dqt([(0, t, [1] * 64) for t in sorted(q)])
    junk_h = make_dht([(tc, th, *flat_table(range(12) if tc == 0 else range(1, 200), 12)) for tc, th in sorted(h)])
    return write(insert(insert(j, min(j.find(DQT)), DQT, junk_q), 0, DHT, junk_h))


def _unused_id3(src):
    j = read(src)
    j = insert(j, j.sof, DQT, make_dqt([(1, 3, [65535] * 64)]))
    return write(insert(j, len(j.segs) - 1, DHT, make_dht([(0, 3, *flat_table(range(16), 7)), (1, 3, *flat_table(range(255), 16))])))


def _embedded(src):
    return write(insert_blob(read(src), APP1, 0, 1, payload=b"Exif\0\0" + base("420", 17, 9)))


def colour_variant(ids, app0, adobe):
    """A 4:2:0 file with these component ids, this APP0 payload (None: no APP0) and this Adobe transform (None: no APP14)."""
    return write(set_app14(set_app0(remap_ids(read(base("420")), ids), app0), adobe))


ID_SETS = [(1, 2, 3), (0, 1, 2), ("R", "G", "B"), (7, 9, 200)]


def colour_cases():
    """{name: bytes}: the id sets with and without JFIF, the Adobe transforms with and without JFIF (ids 1, 2, 3), and RGB ids behind an
    APP0 that starts with JFIF\\0 but is 5...13 bytes long."""
    out = {}
    for ids in ID_SETS:
        for jf in (True, False):
            out[f"ids{'-'.join(map(str, ids))}-{'jfif' if jf else 'nojfif'}"] = colour_variant(ids, JFIF_APP0 if jf else None, None)
    for tr in (0, 1, 2):
        for jf in (True, False):
            out[f"adobe{tr}-{'jfif' if jf else 'nojfif'}"] = colour_variant((1, 2, 3), JFIF_APP0 if jf else None, tr)
    for n in range(5, 14):
        out[f"rgb-ids-jfif{n}"] = colour_variant(("R", "G", "B"), JFIF_APP0[:n], None)
    return out


def pil_is_ycbcr(data):
    """Whether PIL decodes the file to the pixels of the untouched 4:2:0 base file (None: PIL refuses the file)."""
    import struct
    try:
        return bool(np.array_equal(pil_pixels(data), pil_pixels(base("420"))))
    except (OSError, SyntaxError, ValueError, struct.error):
        return None


ALL = ("444", "422", "420", "grey")

# name -> (modes, source -> bytes).  PIL decodes every file to the source's pixels; jpeg.parse must call it supported, with
# geometry(data)'s fields, and the device must decode it to PIL's pixels.
MUST_SUPPORT = {
    "sof1": (ALL, _edit(lambda j: set_sof(j, marker=SOF1))),
    "grey-sampling-22": (("grey",), _edit(lambda j: set_sof(j, sampling=[0x22]))),
    "grey-sampling-43": (("grey",), _edit(lambda j: set_sof(j, sampling=[0x43]))),
    "dqt16": (ALL, _edit(dqt16)),
    "dqt-one-segment": (ALL, _edit(lambda j: merge_tables(j, DQT))),
    "dht-one-segment": (ALL, _edit(lambda j: merge_tables(j, DHT))),
    "eight-segments": (ALL, _edit(lambda j: split_tables(split_tables(j, DQT), DHT))),
    "tables-in-front-of-sof": (ALL, _edit(lambda j: move_tables(move_tables(j, DHT, "front"), DQT, "front"))),
    "dqt-behind-sof": (ALL, _edit(lambda j: move_tables(j, DQT, "behind"))),
    "table-defined-twice": (ALL, _redefined),
    "unused-table-id3": (ALL, _unused_id3),
    "dri-n-then-dri-0": (ALL, _edit(lambda j: insert_dri(insert_dri(j, 3, 0), 0))),
    "dri-one-interval": (ALL, lambda src: write(insert_dri(read(src), _mcus(src)[1] + 3))),
    "three-long-segments": (ALL, _edit(lambda j: insert_blob(insert_blob(insert_blob(j, COM, 65533, 1), 0xE5, 65533, 1), APP1, 65533, 1))),
    "app1-holds-a-jpeg": (ALL, _embedded),
    "fill-header": (ALL, _edit(lambda j: j, fill=3)),
    "fill-rst": (ALL, lambda src: _restarts(src, fill_rst=3)),
    "fill-eoi": (ALL, lambda src: _restarts(src, fill_eoi=3)),
    "bytes-after-eoi": (ALL, lambda src: src + b"\x00\x01garbage\xff\xd9\xff"),
    "jpeg-after-eoi": (ALL, lambda src: src + base("444", 17, 9)),
}

R_COLOUR, R_MALFORMED = "colour space", "malformed"
# name -> (reason, () -> bytes): files PIL decodes to other pixels than a YCbCr decode gives, or refuses
MUST_REFUSE = {
    "rgb-ids-nojfif": (R_COLOUR, lambda: colour_variant(("R", "G", "B"), None, None)),
    "rgb-ids-short-jfif": (R_COLOUR, lambda: colour_variant(("R", "G", "B"), JFIF_APP0[:7], None)),
    "rgb-ids-jfif13": (R_COLOUR, lambda: colour_variant(("R", "G", "B"), JFIF_APP0[:13], None)),
    "adobe0-nojfif": (R_COLOUR, lambda: colour_variant((1, 2, 3), None, 0)),
    "width-65501": (R_MALFORMED, lambda: write(set_sof(read(base("420")), width=65501))),
    "height-65535": (R_MALFORMED, lambda: write(set_sof(read(base("grey")), height=65535))),
}

# name -> (modes, source -> bytes): transcoded files that decode to the source's pixels
TRANSCODED_SAME = {
    "shared-pair-3-3": (COLOUR, lambda src: transcode(src, dc_ids=(3, 3, 3), ac_ids=(3, 3, 3))),
    "three-pairs-three-dqt": (COLOUR, lambda src: transcode(src, dc_ids=(0, 1, 2), ac_ids=(0, 1, 2), tq_ids=(0, 1, 2))),
    "ac-flat16": (ALL, lambda src: transcode(src, ac_kind="flat16")),
    "dc-flat9": (ALL, lambda src: transcode(src, dc_kind="flat9")),
    "dc-flat10": (ALL, lambda src: transcode(src, dc_kind="flat10")),
}
for _name, _ri in (("1", lambda mx, t: 1), ("2", lambda mx, t: 2), ("7", lambda mx, t: 7), ("row-1", lambda mx, t: mx - 1),
                   ("row+1", lambda mx, t: mx + 1), ("total-1", lambda mx, t: t - 1), ("total", lambda mx, t: t),
                   ("total+5", lambda mx, t: t + 5)):
    TRANSCODED_SAME[f"ri-{_name}"] = (ALL, lambda src, _ri=_ri: transcode(src, ri=_ri(*_mcus(src))))

# PIL decodes these to the source's pixels; the device decoder gives the same pixels or refuses (and the driver falls back)
SAME_OR_REFUSED = {
    "pad-zeros": (ALL, lambda src: transcode(src, pad="zeros")),
    "pad-zeros-ri2": (ALL, lambda src: transcode(src, ri=2, pad="zeros")),
    "extra-00-before-eoi": (ALL, lambda src: transcode(src, extra="eoi")),
    "extra-00-before-rst": (ALL, lambda src: transcode(src, ri=2, extra="rst")),
}

# quantisation tables outside what encoders write (test D): PIL decodes all of them, most samples at 0 or 255
QUANT_EDITS = {
    "x3": lambda j: dqt16(j, 3), "x40": lambda j: dqt16(j, 40), "x257": lambda j: dqt16(j, 257),
    "all255": lambda j: dqt_const(j, 255), "all1": lambda j: dqt_const(j, 1),
}


def probe_blocks():
    """128 blocks of one to four small coefficients that, under a large constant quantisation table, take each 16-bit sum of the IDCT
    out of range on its own: DC alone and row 0 alone (rows 1-7 empty: the decoder's shortcut), in0 +- in4, the odd columns and rows."""
    inv = np.argsort(NATURAL)                                # natural index -> zigzag position

    def blk(**nat):
        co = [0] * 64
        for k, v in nat.items():
            co[int(inv[int(k[1:])])] = v
        return (0, co)

    out = []
    for k in range(-8, 8):
        out += [blk(n0=k), blk(n0=k, n3=3), blk(n0=k, n8=1), blk(n0=k, n32=8 - abs(k)), blk(n8=k, n40=5, n24=-k, n56=7),
                blk(n1=k, n5=5, n3=-k, n7=7), blk(n0=k, n8=2 * (k % 3), n1=k % 2)]
    rs = np.random.RandomState(0)
    while len(out) < 128:
        co = [0] * 64
        for _ in range(rs.randint(1, 5)):
            co[rs.randint(64)] = int(rs.randint(-8, 9))
        out.append((0, co))
    return out


def probe_file(q):
    """A grey 128 x 64 file of probe_blocks() under a quantisation table of 64 times q."""
    return from_blocks(write(dqt_const(read(base("grey", 128, 64)), q)), probe_blocks())
