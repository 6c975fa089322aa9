"""Option 'sparse_da0' (extract path, with 'sparse_da3'): convDa.0 is computed on the 4 x 4 blocks around the selected key points' corners only
(sparse_da0_kernel) and stored into the dense map at the pixels' true positions.  The kernel issues, per output element, the MFMAs of the dense
kernel that runs the layer at the same map size, in its order (conv3x3_rf on small maps: taps row by row; conv3x3_pp on large ones: column by
column), so every output of sfd2_extract must equal the dense path's bit for bit: the assertions below are torch.equal, with option 2 forcing
the kernel on at sizes the plan would leave dense and option 0 as the dense reference.  Both tap orders are covered: the small cases against
conv3x3_rf, 544x1024 and 1200x1600 against conv3x3_pp.

The sparse descriptor head exists only where 16 x top_k <= the 1/4-resolution map (plan_pass): at 96x128 (a 24 x 32 map) that is top_k <= 48, so
the larger capacities of the list run the dense layers on both sides there (equality still has to hold); the cases at 192x256 and 512x640 carry the
counts above one tile, and option 'cu_limit' gives a block several tiles so that the pipeline crosses tile boundaries as it does at 1600x1200.
Which cases ran the kernel is asserted from the layer table, not assumed."""
import ctypes
import functools

import numpy as np
import pytest

from sfd2_amd import _lib, synth

pytestmark = pytest.mark.gpu

DENSE, PLAN, FORCED = 0, 1, 2


def _d4(n):
    d2 = lambda v: (v - 1) // 2 + 1
    return d2(d2(n))


def _model(sd, prec, da0, **opts):
    from sfd2_amd.model import ResSegNetV2
    m = ResSegNetV2(outdim=128, require_stability=True, precision=prec).eval()
    m.load_state_dict(sd)
    m.cuda(0)
    m.context.set_option("sparse_da0", da0)
    for k, v in opts.items():
        m.context.set_option(k, v)
    return m


@functools.lru_cache(maxsize=None)
def _models(prec):
    """(dense, forced) contexts of one precision: made once, shared by the cases (a context costs a weight upload and the self-check)."""
    sd = synth.make_state_dict(0)
    return _model(sd, prec, DENSE), _model(sd, prec, FORCED)


def _extract(m, img, topk, conf_th=0.001):
    from sfd2_amd.extractor import extract_resnet_return
    return extract_resnet_return(m, img[None], conf_th=conf_th, topK=topk, scales=[1.0])


def _da0_kernel(m, img, topk, conf_th=0.001):
    """The kernel label of the layer table's convDa.0 row for one extract of this geometry."""
    m.context.set_profiling(2)
    try:
        _extract(m, img, topk, conf_th)
        rows = {r["name"]: r["kernel"] for r in m.context.layer_timings()}
    finally:
        m.context.set_profiling(0)
    return rows.get("convDa.0")


def _assert_equal(a, b, what):
    import torch
    for k in ("keypoints", "scores", "descriptors"):
        assert torch.equal(torch.from_numpy(np.ascontiguousarray(a[k])), torch.from_numpy(np.ascontiguousarray(b[k]))), (what, k)


def _corner(kp, h, w):
    """sd_corner (sfd2_internal.h) in the kernel's fp32 arithmetic: the top-left pixel of each key point's 2 x 2 bilinear block."""
    f = np.float32
    hc, wc = _d4(h), _d4(w)
    kx, ky = kp[:, 0].astype(f), kp[:, 1].astype(f)
    gx = kx / f(w / 2.0) - f(1.0)
    gy = ky / f(h / 2.0) - f(1.0)
    ix = ((gx + f(1.0)) * f(wc) - f(1.0)) / f(2.0)
    iy = ((gy + f(1.0)) * f(hc) - f(1.0)) / f(2.0)
    return np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)


# ------------------------------------------------------------------------------------------ equality with the dense path
SMALL = [(96, 128), (100, 132)]        # 100x132: a 25 x 33 map -- the width no multiple of 4 or 16, partial last rows
TOPKS = [1, 7, 8, 9, 100, 1024]        # below a tile, a tile exactly, one over; 100 / 1024: beyond the sparse head's range at these sizes


@pytest.mark.parametrize("prec", ["f16c", "f16"])
@pytest.mark.parametrize("h,w", SMALL)
@pytest.mark.parametrize("topk", TOPKS)
def test_sparse_da0_equals_dense_small(prec, h, w, topk):
    dense, forced = _models(prec)
    img = synth.make_image(h, w, 40 + topk % 7)
    a, b = _extract(dense, img, topk), _extract(forced, img, topk)
    n = len(a["keypoints"])
    assert n == topk if topk <= 9 else n > 9, n
    _assert_equal(a, b, (prec, h, w, topk))
    sparse_head = 16 * topk <= _d4(h) * _d4(w)
    assert _da0_kernel(forced, img, topk) == ("sparse_da0_kernel" if sparse_head else _da0_kernel(dense, img, topk))
    assert "sparse" not in _da0_kernel(dense, img, topk)


@pytest.mark.parametrize("prec", ["f16c", "f16"])
@pytest.mark.parametrize("h,w,topk,cu_limit", [(192, 256, 100, 0), (192, 256, 100, 3), (512, 640, 1024, 0), (512, 640, 1024, 5), (196, 260, 57, 2), (544, 1024, 1000, 0), (544, 1024, 1000, 7)])
def test_sparse_da0_equals_dense_many_tiles(prec, h, w, topk, cu_limit):
    """Counts of many tiles; with 'cu_limit' a block runs several tiles back to back (13 tiles on 3 blocks, 128 on 5: uneven shares, the ring and
    the patch pipeline cross tile boundaries; 57 key points: a last tile with one live cell).  544x1024: the smallest kind of map whose dense
    layer runs on conv3x3_pp (272 conv3x3_rf tiles are two rounds on 256 CUs), so the kernel's column-major tap order is the one compared."""
    dense, forced = _models(prec)
    img = synth.make_image(h, w, 50 + cu_limit)
    try:
        for m in (dense, forced):
            m.context.set_option("cu_limit", cu_limit)
        a, b = _extract(dense, img, topk), _extract(forced, img, topk)
        print(f"{prec} {h}x{w} top-{topk} cu_limit {cu_limit}: {len(a['keypoints'])} key points")
        assert len(a["keypoints"]) > 16 * max(cu_limit, 1)       # more than two tiles per block where the blocks are limited
        _assert_equal(a, b, (prec, h, w, topk, cu_limit))
        assert _da0_kernel(forced, img, topk) == "sparse_da0_kernel"
        assert _da0_kernel(dense, img, topk) == ("conv3x3_pp" if h == 544 else "conv3x3_rf<1>")
    finally:
        for m in (dense, forced):
            m.context.set_option("cu_limit", 0)


@pytest.mark.parametrize("prec", ["f16c", "f16"])
def test_sparse_da0_count_zero_and_below_capacity(prec):
    dense, forced = _models(prec)
    img = synth.make_image(96, 128, 44)
    n_all = len(_extract(dense, img, 4096)["keypoints"])
    assert 16 < n_all
    # a threshold nothing passes: the count is 0, every block of the launch returns at once
    a, b = _extract(dense, img, 40, conf_th=1e6), _extract(forced, img, 40, conf_th=1e6)
    assert len(a["keypoints"]) == 0 and len(b["keypoints"]) == 0 and b["descriptors"].shape == (0, 128)
    assert _da0_kernel(forced, img, 40, conf_th=1e6) == "sparse_da0_kernel"
    # a threshold between the scores: fewer key points than the capacity of 40 (cells and tiles beyond the count do nothing)
    sc = _extract(dense, img, 40)["scores"]
    th = float(0.5 * (sc[10] + sc[11]))
    assert sc[10] > th > sc[11]
    a, b = _extract(dense, img, 40, conf_th=th), _extract(forced, img, 40, conf_th=th)
    assert len(a["keypoints"]) == 11
    _assert_equal(a, b, (prec, "count 11 of 40"))
    _assert_equal(_extract(forced, img, 40), _extract(dense, img, 40), (prec, "after a call with fewer key points"))


# ------------------------------------------------------------------------------------------ borders
def _frame_image(h, w, seed):
    """synth.make_image with the contrast kept in a frame of twelve pixels and flattened inside: the detector's strongest responses then sit
    along the outermost rows and columns the selection admits."""
    img = synth.make_image(h, w, seed)
    flat = np.full_like(img, 0.5) + 0.05 * (img - 0.5)
    out = flat.copy()
    for sl in ((slice(None), slice(0, 12), slice(None)), (slice(None), slice(h - 12, h), slice(None)),
               (slice(None), slice(None), slice(0, 12)), (slice(None), slice(None), slice(w - 12, w))):
        out[sl] = img[sl]
    return out.astype(np.float32)


@pytest.mark.parametrize("prec", ["f16c", "f16"])
def test_sparse_da0_blocks_over_the_map_border(prec):
    """Key points whose blocks stick out of the map on each of its four sides.  The selection drops key points closer than four pixels to the image
    border (run_selection: border = 4), so a key point's x lies in [4, W - 5] and sd_corner returns x0 in [0, W4 - 2] -- x0 = -1 and x0 = W4 - 1
    cannot come out of sfd2_extract.  The extremes that do occur are asserted: x0 = 0 / y0 = 0 (the block's first column / row and the patch's
    first two are outside the map) and x0 = W4 - 2 / y0 = H4 - 2 (the block's last column / row and the patch's last two are outside)."""
    h, w, topk = 192, 256, 150
    dense, forced = _models(prec)
    # the image: the first of a few seeds whose key points ON THE DENSE PATH show all four kinds (each kind is a band of two pixel rows or columns)
    for seed in range(61, 73):
        img = _frame_image(h, w, seed)
        a = _extract(dense, img, topk)
        x0, y0 = _corner(a["keypoints"], h, w)
        kinds = {"x0 = 0": int((x0 == 0).sum()), "y0 = 0": int((y0 == 0).sum()), "x0 = W4 - 2": int((x0 == _d4(w) - 2).sum()), "y0 = H4 - 2": int((y0 == _d4(h) - 2).sum())}
        if all(v >= 1 for v in kinds.values()):
            break
    b = _extract(forced, img, topk)
    print(f"{prec} border image (seed {seed}): {len(x0)} key points, {kinds}; x0 in [{x0.min()}, {x0.max()}], y0 in [{y0.min()}, {y0.max()}]")
    assert x0.min() >= 0 and y0.min() >= 0 and x0.max() <= _d4(w) - 2 and y0.max() <= _d4(h) - 2
    assert all(v >= 1 for v in kinds.values()), kinds
    _assert_equal(a, b, (prec, "border"))
    assert _da0_kernel(forced, img, topk) == "sparse_da0_kernel"


# ------------------------------------------------------------------------------------------ stale map
@pytest.mark.parametrize("prec", ["f16c", "f16"])
def test_sparse_da0_alternating_images_eager_and_graphs(prec):
    """Two images alternately on ONE context: the map keeps the other image's blocks between calls, none of which may be read.  Eager through
    sfd2_extract, then through sfd2_extract_match with option 'graphs' (first sight eager, second captured, two replays).  (No entry point
    writes a tensor's buffer from outside, so the alternation is what makes the map stale.)"""
    import torch
    h, w, K = 192, 256, 100
    dense, forced = _models(prec)
    imgs = [synth.make_image(h, w, 70), _frame_image(h, w, 71)]
    want = [_extract(dense, im, K) for im in imgs]
    assert not np.array_equal(want[0]["keypoints"], want[1]["keypoints"])
    for rnd in range(2):
        for i in (0, 1):
            _assert_equal(_extract(forced, imgs[i], K), want[i], (prec, "eager", rnd, i))
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    kp = torch.zeros((K, 2), device="cuda"); sc = torch.zeros((K,), device="cuda"); de = torch.zeros((K, 128), device="cuda")

    def unit(m, i):
        for t in (kp, sc, de):
            t.zero_()
        torch.cuda.synchronize()
        ctx = m.context
        _lib.check(ctx.lib.sfd2_extract_match(ctx.h, dev[i].data_ptr(), h, w, 0.001, K, 0, kp.data_ptr(), sc.data_ptr(), de.data_ptr(),
                                              None, 0, 128, None, None, None))
        ctx.sync()
        return kp.clone(), sc.clone(), de.clone()

    ref = [unit(dense, 0), unit(dense, 1)]
    for i in (0, 1):      # the device-resident form of the same extract: the rows of the count equal the host form's
        n = len(want[i]["keypoints"])
        assert torch.equal(ref[i][0][:n].cpu().double(), torch.from_numpy(want[i]["keypoints"]))
        assert torch.equal(ref[i][2][:n].cpu().double(), torch.from_numpy(want[i]["descriptors"]))
    forced.context.set_option("graphs", 1)
    try:
        for rnd in range(4):      # 0 eager, 1 captures, 2-3 replay
            for i in (0, 1):
                got = unit(forced, i)
                for g, r in zip(got, ref[i]):
                    assert torch.equal(g, r), (prec, "graphs", rnd, i)
    finally:
        forced.context.set_option("graphs", 0)
    _assert_equal(_extract(forced, imgs[0], K), want[0], (prec, "eager after graphs"))


# ------------------------------------------------------------------------------------------ plan
def test_sparse_da0_plan_and_debug_readback(synth_sd):
    """Option 1 (the default): dense at 480x640 / top-4096, the sparse kernel at 1200x1600, dense again with compensated head branches; the
    partly written map is not handed out by debug_activation, and det (which runs the dense layer) makes it readable again."""
    m = _model(synth_sd, "f16c", PLAN)
    assert m.context.get_option("sparse_da0") == 1
    assert "sparse" not in _da0_kernel(m, synth.make_image(480, 640, 3), 4096)
    big = synth.make_image(1200, 1600, 4)
    m.context.set_option("sparse_da0", DENSE)
    want = _extract(m, big, 4096)
    assert _da0_kernel(m, big, 4096) == "conv3x3_pp"
    m.context.set_option("sparse_da0", PLAN)
    _assert_equal(_extract(m, big, 4096), want, "1200x1600 top-4096: two tiles per block, against conv3x3_pp")
    assert _da0_kernel(m, big, 4096) == "sparse_da0_kernel"
    with pytest.raises(RuntimeError, match="not materialised"):
        m.context.debug_activation("convDa.0")
    small = np.ascontiguousarray(big[:, :192, :256])
    m.context.set_option("alias", 0)          # one buffer per activation: the other tensors are readable, this one still is not
    m.context.set_option("sparse_da0", FORCED)
    _extract(m, small, 40)
    with pytest.raises(RuntimeError, match="not materialised"):
        m.context.debug_activation("convDa.0")
    assert m.context.debug_activation("conv4.2").shape == (256, 48, 64)
    m.context.set_option("alias", 1)
    m.context.set_option("sparse_da0", PLAN)
    import oracle.oracle as orc
    m.det(orc.norm_rgb(small)[None])
    assert m.context.debug_activation("convDa.0").shape == (256, 48, 64)
    m.context.set_option("comp_heads", 1)
    assert "sparse" not in _da0_kernel(m, big, 4096)
    # the replicas of the pipelined driver copy the option
    m.context.set_option("comp_heads", 0)
    m.context.set_option("sparse_da0", DENSE)
    assert m.replica().context.get_option("sparse_da0") == 0
