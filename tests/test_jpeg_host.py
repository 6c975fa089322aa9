"""CPU tests of the host side of the baseline JPEG decoder: sfd2_jpeg_parse (sizes, sampling, restart intervals, the reason of every
refusal, truncations and byte flips that never crash it), sfd2_jpeg_prepare, and ImageDataset(decoder="hip").load."""
import io

import numpy as np
import pytest

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
