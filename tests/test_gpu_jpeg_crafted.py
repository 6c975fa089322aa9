"""GPU tests of the baseline JPEG decoder on files PIL's encoder never writes and on scans that never resynchronise by themselves
(tests/jpeg_ref.py builds them): bit-exact against np.asarray(PIL.Image.open(p).convert("RGB")) on the same bytes, no tolerance.

  A  every width and height from 1 to 18 in every sampling mode, and the longest rows and columns libjpeg takes
  B  content: flat colour (a periodic scan: only the predecessor chain and, past 12 groups of lanes, the serial walk synchronise it),
     repeated tiles, half flat / half noise, DC differences of category 11, hard edges, saturated primaries
  C  marker-level edits (jpeg_ref.MUST_SUPPORT, the colour-space cases)
  D  quantisation tables that take the IDCT out of 16 bits, and blocks of single coefficients that isolate each of its 16-bit sums
  E  transcoded files: shared / separate table ids, flat-length tables, restart intervals, padding
  F  queued decodes whose scratch buffers grow in the middle of the queue
  G  the driver's routing of refused files

Every test prints how many files it decoded and how many were refused (pytest -s shows it)."""
import functools
import os

import numpy as np
import pytest

import jpeg_ref as jr
from test_gpu_jpeg import _check, _ctx, _model

pytestmark = pytest.mark.gpu


def _diff(data):
    """test_gpu_jpeg._check's comparison as text: None when the device's pixels equal PIL's."""
    from sfd2_amd import jpeg
    info = jpeg.parse(data)
    if not info.supported:
        return f"refused by parse: {jpeg.reason(info)}"
    got = jpeg.decode(_ctx(), data).cpu().numpy()
    want = jr.pil_pixels(data)
    if got.shape[:2] != want.shape[:2]:
        return f"shape {got.shape} against {want.shape}"
    bad = np.argwhere(np.any(got[:, :, :3] != want, axis=-1))
    if bad.size:
        y, x = bad[0].tolist()
        return f"{len(bad)} pixels differ, first at (y {y}, x {x}): got {got[y, x, :3].tolist()}, PIL {want[y, x].tolist()}"
    return None


def _check_all(label, files):
    """Every file of {name: bytes} decodes on the device to PIL's pixels; all failures are reported, not only the first."""
    bad = {}
    for name, data in files.items():
        d = _diff(data)
        if d is not None:
            bad[name] = d
    print(f"[{label}] {len(files)} files, {len(files) - len(bad)} decoded equal to PIL, 0 refused")
    assert not bad, (len(bad), list(bad.items())[:10])


def _groups(data):
    """The scan's length in workgroups of 64 lanes of 256 bits (the parallel launches settle 12 of them for certain)."""
    from sfd2_amd import jpeg
    info = jpeg.parse(data)
    return (info.scan_end - info.scan_begin) * 8 / 256 / 64


# ------------------------------------------------------------------------------------------------ A: small shapes
@pytest.mark.parametrize("mode", jr.ALL)
def test_a_every_size_up_to_18x18(mode):
    """Chroma planes one and two samples wide (replicated, not interpolated), the first interpolated widths, heights whose last chroma row
    is replicated, partial MCUs in both directions."""
    files = {f"{w}x{h}": jr.encode(jr.content("noise", w, h, 100 * w + h), mode, quality=95) for w in range(1, 19) for h in range(1, 19)}
    assert len(files) == 324
    _check_all(f"A {mode} 1..18 x 1..18", files)


@pytest.mark.parametrize("mode", jr.ALL)
def test_a_longest_row_and_column(mode):
    _check_all(f"A {mode} 65500", {"65500x1": jr.base(mode, 65500, 1), "1x65500": jr.base(mode, 1, 65500)})


# ------------------------------------------------------------------------------------------------ B: content
COLOURS = [(0, 0, 0), (255, 255, 255), (200, 30, 90)]
FLAT = {"420": ("420", 1600, 1200, {}), "444": ("444", 1600, 1200, {}), "grey": ("grey", 2048, 2048, {}),
        "420-restart-blocks-1": ("420", 1600, 1200, dict(restart_marker_blocks=1)),
        "420-restart-rows-1": ("420", 1600, 1200, dict(restart_marker_rows=1))}


@pytest.mark.parametrize("layout", list(FLAT))
def test_b_flat_colour(layout):
    """Every MCU after the first is the same few bits: no lane that guessed wrongly ever resynchronises by itself.  Without restart
    markers the scans are longer than the 12 groups the parallel launches settle for certain."""
    mode, w, h, kw = FLAT[layout]
    files = {str(c): jr.encode(jr.content("flat", w, h, colour=c), mode, quality=90, **kw) for c in COLOURS}
    if not kw:
        assert min(_groups(d) for d in files.values()) > 12
    _check_all(f"B flat {layout}", files)


@pytest.mark.parametrize("tile", [(8, 8), (16, 16), (24, 24)], ids=["8x8", "16x16", "24x24"])
def test_b_repeated_tiles(tile):
    """A noise tile repeated to 640 x 480: a periodic scan of more than a hundred groups (24 x 24 is not MCU-aligned in 4:2:0)."""
    files = {m: jr.encode(jr.content("tiled", 640, 480, 3, tile=tile), m, quality=90) for m in jr.COLOUR}
    assert min(_groups(d) for d in files.values()) > 12
    _check_all(f"B tiles {tile}", files)


def test_b_half_flat_half_noise():
    files = {f"{m}-{s}": jr.encode(jr.content("half_flat_half_noise", 640, 480, 4, split=s), m, quality=90) for m in jr.ALL for s in "xy"}
    _check_all("B half flat half noise", files)


def test_b_block_checker_dc_category_11():
    files = {m: jr.encode(jr.content("block_checker", 128, 64), m, quality=100) for m in ("grey", "444")}
    for m, d in files.items():        # the DC differences between black and white blocks are +-2040
        dc = [co[0] for ci, co in jr.decode_scan(jr.read(d)) if ci == 0]
        assert max(abs(a - b) for a, b in zip(dc, dc[1:])).bit_length() == 11
    _check_all("B block checker", files)


@pytest.mark.parametrize("kind", ["hard_edges", "primaries"])
def test_b_edges_and_primaries(kind):
    """The IDCT overshoots [0, 255] and the colour conversion clamps."""
    files = {f"{m}-q{q}": jr.encode(jr.content(kind, 97, 131, 6), m, quality=q) for m in jr.ALL for q in (50, 95)}
    _check_all(f"B {kind}", files)


# ------------------------------------------------------------------------------------------------ C: marker-level edits
def _cases(fam):
    return [(name, mode) for name, (modes, _) in fam.items() for mode in modes]


@pytest.mark.parametrize("name,mode", _cases(jr.MUST_SUPPORT), ids=lambda v: str(v))
def test_c_marker_edits(name, mode):
    _check(jr.MUST_SUPPORT[name][1](jr.base(mode)))


def test_c_colour_space_cases():
    """Component ids, JFIF and Adobe markers: the files PIL decodes as YCbCr decode to PIL's pixels, the others are refused."""
    from sfd2_amd import jpeg
    files, refused = {}, 0
    for name, data in jr.colour_cases().items():
        if jr.pil_is_ycbcr(data):
            files[name] = data
        else:
            refused += 1
            assert not jpeg.supported(data), name
    assert len(files) == 12 and refused == 11
    _check_all("C colour space", files)
    print(f"[C colour space] {refused} refused by parse")


# ------------------------------------------------------------------------------------------------ D: quantisation tables
@pytest.mark.parametrize("edit", list(jr.QUANT_EDITS))
def test_d_quantisation_tables(edit):
    """Dequantised coefficients and IDCT sums that leave 16 bits; the reference is what PIL gives."""
    files = {f"{m}-{kind}": jr.write(jr.QUANT_EDITS[edit](jr.read(jr.base(m, 40, 24, kind)))) for m in jr.ALL for kind in ("noise", "primaries")}
    _check_all(f"D {edit}", files)


def test_d_idct_single_coefficient_probes():
    """Blocks of one to four coefficients under constant tables of 700, 4000, 32768 and 65535: each 16-bit sum of libjpeg-turbo's SIMD
    IDCT (in0 +- in4, in7 + in3, in5 + in1, the DC-only shortcut's shift) overflows on its own in some block."""
    _check_all("D probes", {f"q{q}": jr.probe_file(q) for q in (700, 4000, 32768, 65535)})


# ------------------------------------------------------------------------------------------------ E: transcoded files
@pytest.mark.parametrize("name,mode", _cases(jr.TRANSCODED_SAME), ids=lambda v: str(v))
def test_e_transcoded(name, mode):
    _check(jr.TRANSCODED_SAME[name][1](jr.base(mode)))


def test_e_shared_tables_long_scan():
    """One table pair for all three components: nothing in the codes tells a luma block from a chroma block, so the MCU phase of every lane
    comes through the predecessor chain alone, here over far more than 12 groups."""
    data = jr.transcode(jr.base("444", 256, 256, quality=95), dc_ids=(3, 3, 3), ac_ids=(3, 3, 3))
    assert _groups(data) > 24
    _check(data)


@pytest.mark.parametrize("name,mode", _cases(jr.SAME_OR_REFUSED), ids=lambda v: str(v))
def test_e_same_or_refused(name, mode):
    """Zero padding bits and a stray 00 byte: PIL decodes them to the source's pixels; the device gives the same pixels or raises
    ValueError (test_g_driver_routing then shows the fallback) -- never other pixels."""
    from sfd2_amd import jpeg
    data = jr.SAME_OR_REFUSED[name][1](jr.base(mode))
    assert jpeg.supported(data)
    try:
        got = jpeg.decode(_ctx(), data).cpu().numpy()
    except ValueError as e:
        print(f"[E {name} {mode}] refused: {str(e)[-60:]}")
        return
    print(f"[E {name} {mode}] decoded")
    assert np.array_equal(got[:, :, :3], jr.pil_pixels(data))


# ------------------------------------------------------------------------------------------------ F: queued decodes
@functools.lru_cache(maxsize=None)
def _queue_files():
    return [jr.encode(jr.content("noise" if w < 100 else "half_flat_half_noise", w, h, 20 + i), m, quality=90)
            for i, (w, h, m) in enumerate(((17, 9, "422"), (1600, 1200, "420"), (64, 48, "grey"), (2048, 1536, "444")))]


def test_f_queued_decodes_while_scratch_grows():
    """16 decode_async calls, sizes alternating small / large so that the scratch buffers grow in the middle of the queue, one sync:
    every output equals PIL, every status word is 0, and synchronous decodes of the same files give the same bytes."""
    import torch
    from sfd2_amd import jpeg
    ctx = _ctx()
    files = _queue_files()
    status_t = torch.full((16,), 0xFFFF, dtype=torch.int32).pin_memory()
    status = status_t.numpy().view(np.uint32)
    keep, outs = [], []
    for i in range(16):
        data = files[i % 4]
        info = jpeg.parse(data)
        assert info.supported
        t = torch.zeros(int(info.prepared_cap), dtype=torch.uint8).pin_memory()
        buf = t.numpy()
        buf[:len(data)] = np.frombuffer(data, dtype=np.uint8)
        jpeg.prepare(buf, info)
        out = torch.zeros((info.height, info.width, 4), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
        jpeg.decode_async(ctx, buf, info, out, status[i:i + 1])
        keep.append((t, info))
        outs.append(out)
    ctx.sync()
    assert status.tolist() == [0] * 16, status.tolist()
    want = [jr.pil_pixels(d) for d in files]
    for i, out in enumerate(outs):
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :, :3], want[i % 4]), i
        assert np.array_equal(got, jpeg.decode(ctx, files[i % 4]).cpu().numpy()), i
    print("[F] 16 queued decodes equal to PIL and to the synchronous decodes")


# ------------------------------------------------------------------------------------------------ G: driver routing
def test_g_driver_routing(tmp_path):
    """Crafted files from C, D and E, every same-or-refused one and every refused one, through ImageDataset(decoder="hip").load +
    device_image (test_corrupted_scans_decode_like_pil's loop) against decoder="pil": the same pixels or the same ValueError."""
    from sfd2_amd import extract_localization as el
    from sfd2_amd import synth
    model = _model(synth.make_state_dict(0), "f16c")
    files = {f"r-{name}": fn() for name, (_, fn) in jr.MUST_REFUSE.items()}
    for name, (modes, fn) in jr.SAME_OR_REFUSED.items():
        for m in ("420", "grey"):
            files[f"s-{name}-{m}"] = fn(jr.base(m))
    for name, m in (("sof1", "420"), ("grey-sampling-43", "grey"), ("fill-rst", "422"), ("jpeg-after-eoi", "444")):
        files[f"c-{name}-{m}"] = jr.MUST_SUPPORT[name][1](jr.base(m))
    files["d-x257-420"] = jr.write(jr.QUANT_EDITS["x257"](jr.read(jr.base("420", 40, 24, "primaries"))))
    files["d-probe-4000"] = jr.probe_file(4000)
    files["e-shared-420"] = jr.TRANSCODED_SAME["shared-pair-3-3"][1](jr.base("420"))
    files["e-ac-flat16-grey"] = jr.TRANSCODED_SAME["ac-flat16"][1](jr.base("grey"))
    root = tmp_path / "img"
    os.makedirs(root)
    for name, data in files.items():
        with open(root / f"{name}.jpg", "wb") as f:
            f.write(data)
    hip = el.ImageDataset(root, {}, decoder="hip")
    pil = el.ImageDataset(root, {}, decoder="pil")
    assert len(hip) == len(files) >= 20
    how = {"device": 0, "fallback": 0, "error": 0}
    for i in range(len(hip)):
        try:
            want = pil.load(i)["image"]
        except ValueError:
            want = None
        try:
            item = hip.load(i)
            if item.get("jpeg") is not None:
                img = el.device_image(model, item)
                got = img[:, :, :3].cpu().numpy() if img is not None else el.cpu_decode(item["path"])
                route = "device" if img is not None else "fallback"
            else:
                got = item["image"]
                route = "fallback"
        except ValueError:
            got = None
            route = "error"
        how[route] += 1
        name = str(hip.paths[i])
        assert (want is None) == (got is None), name
        if want is not None:
            assert np.array_equal(want, got), name
        if name.startswith("r-"):
            assert route != "device", name
    print(f"[G] {len(files)} files: {how}")
    assert how["error"] == 2 and how["device"] >= 8, how
