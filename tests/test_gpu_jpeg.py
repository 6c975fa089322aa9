"""GPU tests of the baseline JPEG decoder (sfd2_amd/jpeg.py, include/sfd2_hip.h sfd2_jpeg_decode): bit-exact against
np.asarray(PIL.Image.open(p).convert("RGB")) over sizes, subsampling, quality, optimised tables and restart markers; the extraction
driver with decoder="hip" writes the stores decoder="pil" writes, serial and pipelined, with per-file CPU fallbacks; and corrupted
scans give what PIL gives."""
import io
import os

import numpy as np
import pytest

from sfd2_amd import synth

pytestmark = pytest.mark.gpu


def _ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no MI355X visible: GPU tests cannot run (there is no CPU fallback)")
    from sfd2_amd import _lib
    return _lib.default_context(0)


def _content(w, h, kind, seed):
    rs = np.random.RandomState(seed)
    if kind == "noise":
        return rs.randint(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([128 + 100 * np.sin(x / 23.0 + seed), 128 + 90 * np.cos(y / 17.0), 128 + 60 * np.sin((x + y) / 31.0)], -1)
    return np.clip(img + rs.standard_normal(img.shape) * 3, 0, 255).astype(np.uint8)


def _encode(arr, grey=False, **kw):
    from PIL import Image, ImageFile
    im = Image.fromarray(arr)
    if grey:
        im = im.convert("L")
    b = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 8 * arr.size)       # (optimised tables on noise: PIL's default encoder buffer is too small)
    try:
        im.save(b, "JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return b.getvalue()


def _pil(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _check(data):
    ctx = _ctx()
    from sfd2_amd import jpeg
    info = jpeg.parse(data)
    assert info.supported, jpeg.reason(info)
    got = jpeg.decode(ctx, data).cpu().numpy()
    want = _pil(data)
    assert got.shape[:2] == want.shape[:2]
    bad = np.argwhere(np.any(got[:, :, :3] != want, axis=-1))
    assert bad.size == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])][:3].tolist(), want[tuple(bad[0])].tolist())


SIZES = [(1600, 1200), (1600, 1063), (1601, 1199), (2048, 1536), (17, 9), (8, 8), (1, 1)]
MODES = [("444", dict(subsampling=0)), ("422", dict(subsampling=1)), ("420", dict(subsampling=2)), ("grey", {})]


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_bit_exact_sizes_and_subsampling(size, mode):
    w, h = size
    name, kw = mode
    for i, kind in enumerate(("noise", "smooth")):
        _check(_encode(_content(w, h, kind, 7 + i), grey=name == "grey", quality=90, **kw))


OPTS = [dict(quality=50), dict(quality=100), dict(quality=90, optimize=True), dict(quality=50, optimize=True),
        dict(quality=90, restart_marker_blocks=1), dict(quality=90, restart_marker_blocks=4), dict(quality=100, restart_marker_rows=1),
        dict(quality=90, optimize=True, restart_marker_blocks=4)]


@pytest.mark.parametrize("opts", OPTS, ids=["-".join(f"{k}{v}" for k, v in o.items()) for o in OPTS])
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_bit_exact_quality_tables_and_restarts(opts, mode):
    name, kw = mode
    for i, (w, h, kind) in enumerate(((331, 257, "noise"), (640, 481, "smooth"))):
        _check(_encode(_content(w, h, kind, 11 + i), grey=name == "grey", **kw, **opts))


# ------------------------------------------------------------------------------------------------ the extraction driver
def _model(sd, precision, **opts):
    _ctx()
    from sfd2_amd.model import ResSegNetV2
    m = ResSegNetV2(outdim=128, require_stability=True, precision=precision).eval()
    m.cuda(0)
    for k, v in opts.items():
        m.context.set_option(k, v)
    m.load_state_dict(sd)
    return m


def _stores_equal(a_path, b_path):
    from sfd2_amd.feature_io import open_store
    a, b = open_store(a_path, "r"), open_store(b_path, "r")
    assert list(a.keys()) == list(b.keys()) and len(list(a.keys())) > 0, (list(a.keys()), list(b.keys()))
    for k in a.keys():
        assert sorted(a[k].keys()) == sorted(b[k].keys()), k
        for ds in b[k].keys():
            x, y = np.asarray(a[k][ds].__array__()), np.asarray(b[k][ds].__array__())
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (k, ds)


def _write_images(root, extra=False):
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    shapes = [(128, 96, dict(quality=90)), (160, 120, dict(quality=75, subsampling=1)), (200, 150, dict(quality=95, subsampling=0)),
              (97, 131, dict(quality=90, restart_marker_blocks=2)), (64, 48, {})]
    for i, (w, h, kw) in enumerate(shapes):
        arr = (synth.make_image(h, w, 900 + i).transpose(1, 2, 0) * 255).astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, f"im{i}.jpg"), "JPEG", **kw)
    n_extra = 0
    if extra:
        arr = (synth.make_image(96, 128, 950).transpose(1, 2, 0) * 255).astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, "p0.png"))
        Image.fromarray(arr).save(os.path.join(root, "p1.jpg"), "JPEG", progressive=True)
        Image.fromarray(arr).convert("L").save(os.path.join(root, "g2.jpg"), "JPEG")      # grey: on the device
        n_extra = 2
    return n_extra


@pytest.mark.parametrize("precision", ["f16c", "f16x3"])
@pytest.mark.parametrize("workers", [0, 2])
def test_driver_hip_decoder_writes_the_pil_store(tmp_path, synth_sd, precision, workers):
    """extract_localization.main with decoder="hip" against decoder="pil": the same groups, bit for bit, serial and pipelined (two lanes),
    with and without the device resize (resize_max 150)."""
    from sfd2_amd import extract_localization as el
    _write_images(str(tmp_path / "img"))
    model = _model(synth_sd, precision)
    name, conf = next(iter(el.confs.items()))
    conf = {**conf, "model": {**conf["model"], "max_keypoints": 200}, "preprocessing": {**conf["preprocessing"], "resize_max": 150}}
    kw = dict(model_and_extractor=(model, el.extract_resnet_return), num_workers=workers, lanes=2)
    rep_pil, rep_hip = {}, {}
    a = el.main(conf, el.ImageDataset(tmp_path / "img", conf["preprocessing"], decoder="pil"), tmp_path / "pil", report=rep_pil, **kw)
    b = el.main(conf, el.ImageDataset(tmp_path / "img", conf["preprocessing"]), tmp_path / "hip", decoder="hip", report=rep_hip, **kw)
    _stores_equal(a, b)
    assert rep_hip == {"decoder": "hip", "gpu_decoded": 5, "fallbacks": 0}, rep_hip
    assert rep_pil["decoder"] == "pil" and rep_pil["gpu_decoded"] == 0


@pytest.mark.parametrize("workers", [0, 2])
def test_driver_hip_decoder_falls_back_per_file(tmp_path, synth_sd, workers):
    """A directory with a PNG and a progressive JPEG next to baseline ones: those two go through the CPU decoder (counted), the store equals
    decoder="pil"'s."""
    from sfd2_amd import extract_localization as el
    n_extra = _write_images(str(tmp_path / "img"), extra=True)
    model = _model(synth_sd, "f16c")
    name, conf = next(iter(el.confs.items()))
    conf = {**conf, "model": {**conf["model"], "max_keypoints": 200}}
    kw = dict(model_and_extractor=(model, el.extract_resnet_return), num_workers=workers, lanes=2)
    rep = {}
    a = el.main(conf, el.ImageDataset(tmp_path / "img", conf["preprocessing"], decoder="pil"), tmp_path / "pil", **kw)
    b = el.main(conf, el.ImageDataset(tmp_path / "img", conf["preprocessing"], decoder="hip"), tmp_path / "hip", report=rep, **kw)
    _stores_equal(a, b)
    assert rep["fallbacks"] == n_extra and rep["gpu_decoded"] == 6, rep


def test_pipelined_hip_decoder_repeats_saturated_images_in_strict_mode(tmp_path):
    """test_gpu_pipeline's saturation case with device-decoded files: SFD2_PREC_F16C, exponents zero, weights x 2^10, every image saturates;
    the pipelined loop repeats each image synchronously from the slot's device image, and the store equals the serial loop's."""
    from PIL import Image
    from sfd2_amd import extract_localization as el
    sd = synth.make_state_dict(0, gain_log2=10)
    model = _model(sd, "f16c", auto_range=0, range_fallback=1)
    root = tmp_path / "img"
    os.makedirs(root)
    for i in range(4):
        Image.fromarray((synth.make_image(96, 128, 500 + i).transpose(1, 2, 0) * 255).astype(np.uint8)).save(root / f"{i}.jpg", "JPEG", quality=92)
    name, conf = next(iter(el.confs.items()))
    conf = {**conf, "model": {**conf["model"], "max_keypoints": 100}}
    ds = el.ImageDataset(root, conf["preprocessing"], decoder="hip")
    a = el.main(conf, ds, tmp_path / "s", model_and_extractor=(model, el.extract_resnet_return), num_workers=0)
    n_serial = model.context.range_status(reset=True)["fallbacks"]
    rep = {}
    b = el.main(conf, ds, tmp_path / "p", model_and_extractor=(model, el.extract_resnet_return), num_workers=2, report=rep)
    st = model.context.range_status()
    assert n_serial == 4 and st["fallbacks"] == 8, (n_serial, st)
    assert rep["gpu_decoded"] == 4, rep
    _stores_equal(b, a)


def test_corrupted_scans_decode_like_pil(tmp_path):
    """Seeded bit flips inside the entropy-coded data: load() + the driver's decode under "hip" gives what "pil" gives -- the same pixels
    or the same ValueError (a decode the device refuses goes to the CPU decoder)."""
    from sfd2_amd import extract_localization as el
    from sfd2_amd import jpeg
    ctx_model = _model(synth.make_state_dict(0), "f16c")
    src = _encode(_content(96, 64, "smooth", 3), quality=85)
    info = jpeg.parse(src)
    rs = np.random.RandomState(1)
    root = tmp_path / "img"
    os.makedirs(root)
    for t in range(24):
        d = bytearray(src)
        for _ in range(1 + t % 3):
            p = rs.randint(info.scan_begin, info.scan_end)
            d[p] ^= 1 << rs.randint(8)
        with open(root / f"c{t:02d}.jpg", "wb") as f:
            f.write(bytes(d))
    hip = el.ImageDataset(root, {}, decoder="hip")
    pil = el.ImageDataset(root, {}, decoder="pil")
    for i in range(len(hip)):
        try:
            want = pil.load(i)["image"]
        except ValueError:
            want = None
        try:
            item = hip.load(i)
            if item.get("jpeg") is not None:
                img = el.device_image(ctx_model, item)
                got = img[:, :, :3].cpu().numpy() if img is not None else el.cpu_decode(item["path"])
            else:
                got = item["image"]
        except ValueError:
            got = None
        assert (want is None) == (got is None), hip.paths[i]
        if want is not None:
            assert np.array_equal(want, got), hip.paths[i]
