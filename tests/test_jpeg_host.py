"""CPU tests of the host side of the baseline JPEG decoder: sfd2_jpeg_parse (sizes, sampling, restart intervals, the reason of every
refusal, truncations and byte flips that never crash it), sfd2_jpeg_prepare, and ImageDataset(decoder="hip").load; then the crafted
files of tests/jpeg_ref.py: the transcoder against PIL, the verdict tables, colour-space detection and the dimension cap."""
import io

import numpy as np
import pytest

import jpeg_ref as jr
from sfd2_amd import jpeg


def _img(w, h, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)


def _encode(arr, mode="RGB", fmt="JPEG", **kw):
    from PIL import Image
    im = Image.fromarray(arr).convert(mode)
    b = io.BytesIO()
    im.save(b, fmt, **kw)
    return b.getvalue()


MATRIX = [  # (w, h, encoder options, components, luma (h, v), restart interval in MCUs or None = any > 0)
    (1600, 1200, dict(quality=90), 3, (2, 2), 0),
    (17, 9, dict(quality=90, subsampling=0), 3, (1, 1), 0),
    (33, 17, dict(quality=50, subsampling=1), 3, (2, 1), 0),
    (1601, 1199, dict(quality=100, optimize=True), 3, (2, 2), 0),
    (64, 48, dict(quality=90, restart_marker_blocks=1), 3, (2, 2), None),
    (64, 48, dict(quality=90, restart_marker_rows=1), 3, (2, 2), None),
    (1, 1, dict(quality=90), 3, (2, 2), 0),
]


@pytest.mark.parametrize("case", MATRIX, ids=[f"{c[0]}x{c[1]}-{'-'.join(map(str, c[2].items()))}" for c in MATRIX])
def test_parse_reads_pil_files(case):
    w, h, kw, nc, luma, ri = case
    info = jpeg.parse(_encode(_img(w, h), **kw))
    assert info.supported == 1 and info.reason == 0
    assert (info.width, info.height, info.n_components) == (w, h, nc)
    assert (info.h_samp[0], info.v_samp[0]) == luma and (info.h_samp[1], info.v_samp[1]) == (1, 1)
    if ri is None:
        assert info.restart_interval > 0 and info.n_intervals > 1
    else:
        assert info.restart_interval == ri and info.n_intervals == 1
    mx, my = -(-w // (8 * luma[0])), -(-h // (8 * luma[1]))
    assert (info.mcus_x, info.mcus_y) == (mx, my) and info.n_blocks == mx * my * (luma[0] * luma[1] + 2)


def test_parse_reads_grey_files():
    info = jpeg.parse(_encode(_img(23, 11), mode="L"))
    assert info.supported and info.n_components == 1 and (info.width, info.height) == (23, 11) and info.n_blocks == 3 * 2


def _sof(data):
    i = 2
    while data[i + 1] not in (0xC0, 0xC1, 0xC2):
        i += 2 + (data[i + 2] << 8 | data[i + 3])
    return i


def test_parse_reasons():
    R = {v: k for k, v in jpeg.REASONS.items()}
    base = _encode(_img(40, 30))
    assert jpeg.reason(jpeg.parse(_encode(_img(40, 30), progressive=True))) == "progressive"
    assert jpeg.reason(jpeg.parse(_encode(_img(40, 30), mode="CMYK"))) == "colour space"
    p = _sof(base)
    sof9 = bytearray(base)
    sof9[p + 1] = 0xC9
    assert jpeg.parse(bytes(sof9)).reason == R["arithmetic"]
    b12 = bytearray(base)
    b12[p + 4] = 12
    i12 = jpeg.parse(bytes(b12))
    assert i12.reason == R["precision"] and (i12.width, i12.height) == (40, 30)
    assert jpeg.reason(jpeg.parse(_encode(_img(8, 8), fmt="PNG"))) == "not a JPEG"
    assert jpeg.reason(jpeg.parse(b"")) == "not a JPEG"
    assert not jpeg.supported(b"")
    assert jpeg.supported(base)


def test_parse_truncations():
    data = _encode(_img(24, 16, 3), quality=80, restart_marker_blocks=1)
    info = jpeg.parse(data)
    assert info.supported
    for n in list(range(1, int(info.scan_begin) + 1)) + list(range(len(data) - 64, len(data))):
        t = jpeg.parse(data[:n])
        assert not t.supported and jpeg.reason(t) == "truncated", (n, jpeg.reason(t))


def test_parse_survives_flips_and_truncations():
    """Seeded truncations and byte flips over real files: an error or a consistent info, never a crash; and a supported result prepares."""
    rs = np.random.RandomState(5)
    files = [_encode(_img(40, 24, 1), quality=70), _encode(_img(33, 9, 2), subsampling=1, restart_marker_blocks=2),
             _encode(_img(16, 16, 3), mode="L", optimize=True), _encode(_img(20, 20, 4), subsampling=0, restart_marker_rows=1)]
    for k in range(1500):
        d = bytearray(files[k % len(files)])
        if k % 3 == 0:
            d = d[:rs.randint(0, len(d) + 1)]
        for _ in range(rs.randint(1, 4)):
            if len(d):
                d[rs.randint(len(d))] = rs.randint(256)
        info = jpeg.parse(bytes(d))
        if info.supported:
            assert info.reason == 0 and info.width > 0 and info.height > 0 and 0 < info.scan_begin <= info.scan_end <= len(d)
            buf = np.zeros(int(info.prepared_cap), dtype=np.uint8)
            buf[:len(d)] = np.frombuffer(bytes(d), dtype=np.uint8)
            jpeg.prepare(buf, info)
            assert info.prepared and 0 < info.prepared_bytes <= info.prepared_cap and info.n_lanes >= info.n_intervals
        else:
            assert info.reason != 0


def test_prepare_removes_stuffing_and_markers():
    data = _encode(_img(64, 48, 7), quality=95, restart_marker_blocks=1)
    info = jpeg.parse(data)
    scan = data[info.scan_begin:info.scan_end]
    buf = np.zeros(int(info.prepared_cap), dtype=np.uint8)
    buf[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    jpeg.prepare(buf, info)
    want = bytearray()
    i = 0
    while i < len(scan):           # destuff by hand: FF 00 -> FF, FF Dn dropped
        if scan[i] == 0xFF:
            if scan[i + 1] == 0:
                want.append(0xFF)
            i += 2
            continue
        want.append(scan[i])
        i += 1
    assert bytes(buf[:len(want)]) == bytes(want)
    assert info.n_lanes >= info.n_intervals == (info.mcus_x * info.mcus_y + info.restart_interval - 1) // info.restart_interval


def test_dataset_hip_items(tmp_path):
    from PIL import Image
    from sfd2_amd import extract_localization as el
    arr = _img(160, 120, 9)
    Image.fromarray(arr).save(tmp_path / "a.jpg", "JPEG", quality=90)
    Image.fromarray(arr).save(tmp_path / "b.jpg", "JPEG", progressive=True)
    Image.fromarray(arr).save(tmp_path / "c.png")
    conf = {"resize_max": 100}
    hip = el.ImageDataset(tmp_path, conf, decoder="hip")
    pil = el.ImageDataset(tmp_path, conf, decoder="pil")
    assert hip.decoder == "hip" and pil.decoder == "pil"
    for i in range(len(hip)):
        a, b = hip.load(i), pil.load(i)
        assert a["name"] == b["name"]
        assert tuple(a["original_size"]) == tuple(b["original_size"]) and tuple(a["resize"]) == tuple(b["resize"])
        if a["name"] == "a.jpg":
            buf, info = a["jpeg"]
            assert a["image"] is None and info.prepared and buf.size == info.prepared_bytes and "fallback" not in a
        else:
            assert a.get("jpeg") is None and a["fallback"] and np.array_equal(a["image"], b["image"])
    with pytest.raises(ValueError):
        el.ImageDataset(tmp_path, conf, decoder="nvjpeg")


# ------------------------------------------------------------------------------------------------ crafted files (tests/jpeg_ref.py)

def _cases(*families):
    return [(name, mode) for fam in families for name, (modes, _) in fam.items() for mode in modes]


def _build(name, mode, src):
    for fam in (jr.MUST_SUPPORT, jr.TRANSCODED_SAME, jr.SAME_OR_REFUSED):
        if name in fam:
            return fam[name][1](src)
    raise KeyError(name)


@pytest.mark.parametrize("size", [(40, 24), (33, 17)], ids=["40x24", "33x17"])
@pytest.mark.parametrize("mode", jr.ALL)
def test_transcoder_keeps_pil_pixels(mode, size):
    """The reference inside its own conditions: every way the transcoder recodes a PIL file (table ids, table shapes, restart intervals,
    padding, an extra byte) decodes in PIL to the source's pixels, the coefficients read back equal, and jpeg.parse takes the file."""
    src = jr.base(mode, *size)
    want = jr.pil_pixels(src)
    blocks = jr.decode_scan(jr.read(src))
    n = 0
    for name, m in _cases(jr.TRANSCODED_SAME, jr.SAME_OR_REFUSED):
        if m != mode:
            continue
        data = _build(name, mode, src)
        assert np.array_equal(jr.pil_pixels(data), want), name
        if name in jr.TRANSCODED_SAME:
            assert jr.decode_scan(jr.read(data)) == blocks, name
        info = jpeg.parse(data)
        assert info.supported, (name, jpeg.reason(info))
        n += 1
    assert n >= 14


def test_huffman_tables_from_counts_and_lengths():
    """optimal_table (T.81 K.2): a valid prefix code of at most 16 bits that holds every counted symbol, shorter codes for more frequent
    symbols, also for 256 symbols with Fibonacci-like counts (which need the length limit); flat_table: one length."""
    rs = np.random.RandomState(2)
    for counts in ({s: int(c) for s, c in enumerate(rs.randint(1, 1000, 200))}, {0: 5}, {3: 1, 250: 1},
                   {s: int(1.5 ** min(s, 60)) for s in range(256)}):
        bits, vals = jr.optimal_table(counts)
        enc = jr.huff_codes(bits, vals)
        assert sorted(vals) == sorted(counts) and sum(bits) == len(vals) and max(l for _, l in enc.values()) <= 16
        assert sum(2.0 ** -l for _, l in enc.values()) < 1.0                    # (the all-ones code point stays free)
        if max(l for _, l in enc.values()) < 16:                                # (no length was limited: more frequent, never longer)
            assert all(enc[a][1] <= enc[b][1] for a in counts for b in counts if counts[a] > counts[b])
    bits, vals = jr.flat_table(range(12), 9)
    assert bits[8] == 12 and sum(bits) == 12 and {l for _, l in jr.huff_codes(bits, vals).values()} == {9}


@pytest.mark.parametrize("name,mode", _cases(jr.MUST_SUPPORT), ids=lambda v: str(v))
def test_verdict_must_support(name, mode):
    """Every crafted header variant: PIL decodes it to the source's pixels, and jpeg.parse calls it supported with the geometry the
    headers state."""
    src = jr.base(mode)
    data = _build(name, mode, src)
    assert np.array_equal(jr.pil_pixels(data), jr.pil_pixels(src))
    info = jpeg.parse(data)
    assert info.supported == 1 and info.reason == 0, jpeg.reason(info)
    g = jr.geometry(data)
    for k in ("width", "height", "n_components", "mcus_x", "mcus_y", "n_blocks", "restart_interval", "n_intervals"):
        assert getattr(info, k) == g[k], (k, getattr(info, k), g[k])
    nc = g["n_components"]
    assert list(info.h_samp)[:nc] == g["h_samp"] and list(info.v_samp)[:nc] == g["v_samp"]
    assert data[info.scan_end] == 0xFF and info.scan_begin < info.scan_end


@pytest.mark.parametrize("name", list(jr.MUST_REFUSE))
def test_verdict_must_refuse(name):
    """Files PIL refuses or decodes to other pixels than the YCbCr decode of the same scan: jpeg.parse refuses them, with the reason."""
    why, fn = jr.MUST_REFUSE[name]
    data = fn()
    assert jr.pil_is_ycbcr(data) is not True
    info = jpeg.parse(data)
    assert not info.supported and jpeg.reason(info) == why, jpeg.reason(info)


def test_colour_space_follows_pil():
    """Component ids x JFIF, Adobe transforms x JFIF, and APP0 segments that start with JFIF\\0 but are shorter than a JFIF header: where
    PIL does not decode the file as YCbCr (other pixels than the untouched file's, or no image at all), parse refuses with "colour
    space"; everywhere else the file is supported.  libjpeg counts a JFIF marker only from 14 data bytes on."""
    cases = jr.colour_cases()
    assert len(cases) == 8 + 6 + 9
    other = set()
    for name, data in cases.items():
        ycc = jr.pil_is_ycbcr(data)
        info = jpeg.parse(data)
        if ycc:
            assert info.supported, (name, jpeg.reason(info))
        else:
            other.add(name)
            assert not info.supported and jpeg.reason(info) == "colour space", (name, jpeg.reason(info))
    assert other == {"idsR-G-B-nojfif", "adobe0-nojfif"} | {f"rgb-ids-jfif{n}" for n in range(5, 14)}, other


def test_dimension_cap_follows_pil():
    """libjpeg refuses frames wider or taller than 65500: a file PIL raises on is refused by parse (the driver then fails the same way
    through its CPU decoder), and 65500 itself is taken."""
    for mode in ("420", "grey"):
        for kw in (dict(width=65501), dict(width=65535), dict(height=65501), dict(height=65535)):
            data = jr.write(jr.set_sof(jr.read(jr.base(mode)), **kw))
            with pytest.raises(OSError):
                jr.pil_pixels(data)
            info = jpeg.parse(data)
            assert not info.supported and jpeg.reason(info) == "malformed", (mode, kw)
    for w, h in ((65500, 1), (1, 65500)):
        data = jr.base("420", w, h)
        info = jpeg.parse(data)
        assert jr.pil_pixels(data).shape == (h, w, 3) and info.supported and (info.width, info.height) == (w, h)


@pytest.mark.parametrize("edit", list(jr.QUANT_EDITS))
def test_extreme_quantisation_tables_are_supported(edit):
    """16-bit tables scaled x3 / x40 / x257 and 8-bit tables of all 255 / all 1: PIL decodes them, parse takes them."""
    for mode in jr.ALL:
        for kind in ("noise", "primaries"):
            data = jr.write(jr.QUANT_EDITS[edit](jr.read(jr.base(mode, 40, 24, kind))))
            assert jr.pil_pixels(data).shape == (24, 40, 3)
            info = jpeg.parse(data)
            assert info.supported, (mode, kind, jpeg.reason(info))
