"""GPU parity tests (pytest -m gpu): every call goes through the C-ABI of libsfd2hip.so and is
compared with the CPU oracle on the same seeded inputs, with the committed reference goldens,
and -- at BASELINE.json's full sizes -- directly (the oracle needs seconds) plus through
size-independent properties.

Tolerances (fp16 MFMA operands, fp32 accumulate; measured worst cases in DESIGN.md):
  * integer / index / compare-only stages (heat map, NMS, threshold, border, sort, top-K,
    mutual check given identical similarities): BIT-EXACT
  * conv-stack activations: |err| <= 1.5e-2 * max|layer|   (fp16 rounding through 22 layers)
  * detector score: |err| <= 8e-2 * score + 1e-4           (exp() of logits known to ~6e-2)
  * descriptors (dense and sampled): |err| <= 3e-3 abs on unit vectors; norms 1 +- 1e-5
  * key points end-to-end: set IoU >= 0.95 vs the fp32 oracle (selection is a cascade of
    discontinuities: exactness is claimed per stage, not across the fp16 conv stack)
  * matcher: fp16 operands: similarities within 1e-3, matches identical wherever the
    top-1/top-2 gap exceeds 1e-3; hi+lo split mode ('f16x2'): within 1e-6 / identical.
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402  (tests may use the oracle; the product never does)
from sfd2_amd import _lib, synth  # noqa: E402


def _gpu_ok():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def model(synth_sd):
    if not _gpu_ok():
        pytest.fail("no MI355X visible: GPU tests cannot run (there is no CPU fallback)")
    from sfd2_amd.model import ResSegNetV2
    m = ResSegNetV2(outdim=128, require_stability=True, precision="f16").eval()
    m.load_state_dict(synth_sd)
    m.cuda(0)
    return m


@pytest.fixture(scope="module")
def ctx(model):
    return model.context


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _kp_index(kp):
    # exact coordinates (pyramid levels map back to fractional positions); first occurrence wins
    out = {}
    for i, (x, y) in enumerate(kp):
        out.setdefault((float(x), float(y)), i)
    return out


def _compare_extract(got, want, min_iou, desc_tol):
    a, b = _kp_index(got["keypoints"]), _kp_index(want["keypoints"])
    common = sorted(set(a) & set(b))
    iou = len(common) / max(1, len(set(a) | set(b)))
    assert iou >= min_iou, iou
    ia = np.array([a[k] for k in common]); ib = np.array([b[k] for k in common])
    gs, ws = got["scores"][ia], want["scores"][ib]
    bad = np.abs(gs - ws) > 8e-2 * ws + 1e-4
    # score = detector score x stability in {0.1, 0.5, 1.0}: an fp16-level arg-max flip of the 3-class
    # stability head changes a key point's score by exactly one of these ratios -- rare, and the
    # only admissible cause of a large score difference
    assert bad.mean() <= 0.01, bad.mean()
    ratio = gs[bad] / ws[bad]
    flips = np.array([0.1, 0.2, 0.5, 2.0, 5.0, 10.0])
    assert all(np.min(np.abs(r / flips - 1.0)) < 0.09 for r in ratio), ratio
    dd = np.abs(got["descriptors"][ia] - np.asarray(want["descriptors"], dtype=np.float64)[ib]).max()
    assert dd <= desc_tol, dd
    return iou


# ------------------------------------------------------------------ conv stack / det
@pytest.mark.parametrize("h,w,seed", [(64, 96, 11), (100, 130, 12), (37, 53, 13)])
def test_det_vs_oracle(model, ctx, synth_sd, h, w, seed):
    img = synth.make_image(h, w, seed)
    x = orc.norm_rgb(img)
    taps = {}
    o_score, o_stab, o_desc = orc.det(synth_sd, x, taps)
    score, stab, desc = model.det(x[None])
    assert score.shape == (1, 1) + o_score.shape and desc.shape == (1,) + o_desc.shape and stab.shape == (1, 1, h, w)
    for name, want in taps.items():
        got = ctx.debug_activation(name)
        assert got.shape == want.shape, name
        err = np.abs(got - want).max()
        assert err <= 1.5e-2 * np.abs(want).max(), (name, err)
    assert (np.abs(score[0, 0] - o_score) <= 8e-2 * o_score + 1e-4).all()
    assert np.abs(desc[0] - o_desc).max() <= 3e-3
    np.testing.assert_allclose(np.linalg.norm(desc[0], axis=0), 1.0, atol=1e-5)
    assert (stab[0, 0] != o_stab).mean() < 0.01          # 3-class arg-max flips only at near-ties
    assert set(np.unique(stab)) <= {np.float32(0.1), np.float32(0.5), np.float32(1.0)}


@pytest.mark.parametrize("tag", ["64x96", "100x130"])
def test_det_vs_reference_golden(model, golden_dir, tag):
    g = _load(golden_dir, f"det_{tag}.npz")
    img = synth.make_image(int(g["h"]), int(g["w"]), int(g["seed"]))
    score, stab, desc = model.det(orc.norm_rgb(img)[None])
    assert (np.abs(score[0, 0] - g["score"]) <= 8e-2 * g["score"] + 1e-4).all()
    assert np.abs(desc[0] - g["desc"]).max() <= 3e-3
    assert (stab[0, 0] != g["stability"]).mean() < 0.01


def test_det_torch_cuda_tensors(model, synth_sd):
    import torch
    x = torch.from_numpy(orc.norm_rgb(synth.make_image(64, 96, 11)))[None].cuda()
    score, stab, desc = model.det(x)
    assert score.is_cuda and desc.is_cuda and stab.is_cuda
    s2, st2, d2 = model.det(x.cpu().numpy())
    np.testing.assert_array_equal(score.cpu().numpy(), s2)
    np.testing.assert_array_equal(desc.cpu().numpy(), d2)
    np.testing.assert_array_equal(stab.cpu().numpy(), st2)


# ------------------------------------------------------------------ exact stages
def _heat_hip(ctx, score, sta, h, w):
    score = np.ascontiguousarray(score, dtype=np.float32)
    out = np.empty((h, w), dtype=np.float32)
    sp = None
    hc = wc = 0
    if sta is not None:
        sta = np.ascontiguousarray(sta, dtype=np.float32)
        sp, hc, wc = sta.ctypes.data, sta.shape[1], sta.shape[2]
    _lib.check(ctx.lib.sfd2_heatmap(ctx.h, score.ctypes.data, score.shape[0], score.shape[1], sp, hc, wc, h, w, out.ctypes.data))
    return out


@pytest.mark.parametrize("h,w,hs,ws,hc,wc", [(64, 96, 64, 96, 16, 24), (100, 130, 104, 136, 25, 33),
                                              (1063, 1600, 1064, 1600, 266, 400), (1200, 1600, 1200, 1600, 300, 400)])
def test_heatmap_bit_exact(ctx, h, w, hs, ws, hc, wc):
    rs = np.random.RandomState(h + w)
    score = rs.random_sample((hs, ws)).astype(np.float32)
    sta = rs.standard_normal((3, hc, wc)).astype(np.float32)
    want = orc.heatmap(score, orc.cls_to_value(orc.resize_bilinear(sta, h, w)), h, w)
    np.testing.assert_array_equal(_heat_hip(ctx, score, sta, h, w), want)
    want_ns = orc.heatmap(score, None, h, w)
    np.testing.assert_array_equal(_heat_hip(ctx, score, None, h, w), want_ns)


def _nms_hip(ctx, m, r=4):
    m = np.ascontiguousarray(m, dtype=np.float32)
    out = np.empty_like(m)
    _lib.check(ctx.lib.sfd2_simple_nms(ctx.h, m.ctypes.data, m.shape[0], m.shape[1], r, out.ctypes.data))
    return out


def _select_hip(ctx, m, conf_th, border, topk):
    m = np.ascontiguousarray(m, dtype=np.float32)
    cap = m.size
    kp = np.empty((cap, 2), dtype=np.float32)
    sc = np.empty((cap,), dtype=np.float32)
    n = ctypes.c_int()
    _lib.check(ctx.lib.sfd2_select_keypoints(ctx.h, m.ctypes.data, m.shape[0], m.shape[1], conf_th, 4, border, topk,
                                             kp.ctypes.data, sc.ctypes.data, cap, ctypes.byref(n)))
    return kp[:n.value], sc[:n.value]


@pytest.mark.parametrize("case", ["rand_61x83", "rand_128x160", "plateau_64x64", "sparse_70x90", "tiny_5x7"])
def test_nms_vs_reference_golden_bit_exact(ctx, golden_dir, case):
    g = _load(golden_dir, "nms.npz")
    out = _nms_hip(ctx, g[case + "/in"])
    idx = np.flatnonzero(out)
    np.testing.assert_array_equal(idx, g[case + "/idx"])
    np.testing.assert_array_equal(out.reshape(-1)[idx], g[case + "/val"])


@pytest.mark.parametrize("h,w,kind", [(33, 65, "rand"), (200, 333, "rand"), (64, 64, "plateau"), (97, 131, "sparse"),
                                       (8, 9, "rand"), (1200, 1600, "rand"), (1063, 1600, "smooth"), (64, 64, "const")])
def test_nms_and_selection_bit_exact(ctx, h, w, kind):
    rs = np.random.RandomState(h * 7 + w)
    m = rs.random_sample((h, w))
    if kind == "plateau":
        m = np.floor(m * 4) / 4
    elif kind == "sparse":
        m = np.where(m > 0.97, rs.random_sample((h, w)), 0)
    elif kind == "smooth":   # heat-map like: peaky, mostly tiny values
        m = m ** 12
    elif kind == "const":
        m = np.full((h, w), 0.25)
    m = m.astype(np.float32)
    want = orc.simple_nms(m, 4)
    np.testing.assert_array_equal(_nms_hip(ctx, m), want)
    for topk in (64, 4096, -1):
        kp_w, sc_w, _ = orc.select_keypoints(want, 0.001, 4, topk)
        kp, sc = _select_hip(ctx, m, 0.001, 4, topk)
        np.testing.assert_array_equal(kp, kp_w)
        np.testing.assert_array_equal(sc, sc_w)
        assert (np.diff(sc) <= 0).all()
        if len(kp):
            assert kp[:, 0].min() >= 4 and kp[:, 0].max() < w - 4 and kp[:, 1].min() >= 4 and kp[:, 1].max() < h - 4


def test_selection_vs_reference_golden_bit_exact(ctx, golden_dir):
    """Reference NMS output (candidates) -> threshold / border / sort / top-K identical to the
    reference's key points and scores (nets/extractor.py:158-183,322-326)."""
    g = _load(golden_dir, "extract_480x640_k1024.npz")
    h, w, topk = int(g["h"]), int(g["w"]), int(g["topk"])
    nms = np.zeros((h * w,), dtype=np.float32)
    nms[g["cand_idx"]] = g["cand_val"]
    # the NMS of an already-suppressed map keeps isolated maxima, so feeding the reference's NMS
    # output through the full stage reproduces the reference's selection
    kp, sc = _select_hip(ctx, nms.reshape(h, w), 0.001, 4, topk)
    np.testing.assert_array_equal(kp, g["keypoints"])
    np.testing.assert_array_equal(sc, g["scores"])


def test_nms_radius_argument(ctx):
    m = np.random.RandomState(1).random_sample((50, 60)).astype(np.float32)
    for r in (0, 1, 2, 3):
        np.testing.assert_array_equal(_nms_hip(ctx, m, r), orc.simple_nms(m, r))
    with pytest.raises(RuntimeError):
        _nms_hip(ctx, m, 5)


def test_sample_descriptors_vs_oracle(ctx):
    rs = np.random.RandomState(5)
    for (hc, wc, nh, nw) in ((25, 33, 100, 130), (300, 400, 1200, 1600), (16, 24, 64, 96)):
        dm = orc.l2norm_channels(rs.standard_normal((128, hc, wc)).astype(np.float32))
        n = 500
        kp = np.stack([rs.randint(0, nw, n), rs.randint(0, nh, n)], axis=1).astype(np.float32)
        kp[:4] = [[0, 0], [nw - 1, nh - 1], [0, nh - 1], [nw - 1, 0]]          # zero-padded border taps
        want = orc.sample_descriptors(dm, kp, nh, nw)
        got = np.empty_like(want)
        _lib.check(ctx.lib.sfd2_sample_descriptors(ctx.h, dm.ctypes.data, hc, wc, nh, nw, kp.ctypes.data, n, got.ctypes.data))
        np.testing.assert_allclose(got, want, atol=2e-6)
        np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("h,w,seed,topk", [(96, 128, 21, 200), (100, 130, 22, -1), (480, 640, 0, 1024)])
def test_extract_vs_oracle_and_golden(model, synth_sd, golden_dir, h, w, seed, topk):
    from sfd2_amd.extractor import extract_resnet_return
    img = synth.make_image(h, w, seed)
    got = extract_resnet_return(model, img[None], conf_th=0.001, topK=topk, scales=[1.0])
    assert got["keypoints"].dtype == np.float64 and got["descriptors"].dtype == np.float64 and got["scores"].dtype == np.float64
    assert got["descriptors"].shape == (len(got["scores"]), 128)
    assert (np.diff(got["scores"]) <= 0).all()
    want = orc.extract_resnet_return(synth_sd, img, conf_th=0.001, topK=topk)
    _compare_extract(got, want, 0.95, 3e-3)
    tag = {(96, 128): "96x128_k200", (100, 130): "100x130_all", (480, 640): "480x640_k1024"}[(h, w)]
    g = _load(golden_dir, f"extract_{tag}.npz")
    ref = {"keypoints": g["keypoints"], "scores": g["scores"].astype(np.float64), "descriptors": g["descriptors"].astype(np.float64)}
    _compare_extract(got, ref, 0.95, 4e-3)   # fixture descriptors are stored as fp16


def test_extract_full_size_1600x1200(model, synth_sd):
    """BASELINE.json configs[1] geometry: direct comparison with the oracle + invariants."""
    from sfd2_amd.extractor import extract_resnet_return
    import torch
    img = synth.make_image(1200, 1600, 5)
    got = extract_resnet_return(model, torch.from_numpy(img)[None].cuda(), conf_th=0.001, topK=4096, scales=[1.0])
    n = len(got["scores"])
    assert n == 4096
    kp = got["keypoints"]
    assert len({(int(x), int(y)) for x, y in kp}) == n
    assert kp[:, 0].min() >= 4 and kp[:, 0].max() < 1600 - 4 and kp[:, 1].min() >= 4 and kp[:, 1].max() < 1200 - 4
    assert (np.diff(got["scores"]) <= 0).all() and got["scores"].min() > 0.001
    np.testing.assert_allclose(np.linalg.norm(got["descriptors"], axis=1), 1.0, atol=1e-5)
    # NMS radius: no two key points within Chebyshev distance 4 unless they tie exactly
    order = np.lexsort((kp[:, 0], kp[:, 1]))
    pts = kp[order]
    for i in range(0, n - 1):
        j = i + 1
        while j < n and pts[j, 1] - pts[i, 1] <= 4:
            if abs(pts[j, 0] - pts[i, 0]) <= 4:
                assert got["scores"][order[i]] == got["scores"][order[j]]
            j += 1
    want = orc.extract_resnet_return(synth_sd, img, conf_th=0.001, topK=4096)
    _compare_extract(got, want, 0.93, 3e-3)


def test_extract_beyond_one_round_of_tiles_2048x1536(model, synth_sd):
    """A 3-megapixel image: the stride-2 convPa.0 has 384 tiles (and conv2b 1 536) for the 256 persistent blocks of
    conv3x3_rf, i.e. its tile loop with the pipeline running across tile boundaries, and conv3x3_pp runs three tiles per
    block.  Same comparison with the oracle as at 1600x1200."""
    from sfd2_amd.extractor import extract_resnet_return
    import torch
    img = synth.make_image(1536, 2048, 15)
    got = extract_resnet_return(model, torch.from_numpy(img)[None].cuda(), conf_th=0.001, topK=4096, scales=[1.0])
    assert len(got["scores"]) == 4096
    want = orc.extract_resnet_return(synth_sd, img, conf_th=0.001, topK=4096)
    _compare_extract(got, want, 0.93, 3e-3)


def test_extract_async_device_outputs_equal_sync(model):
    import torch
    from sfd2_amd.extractor import extract_resnet_return
    ctx = model.context
    img = torch.from_numpy(synth.make_image(240, 320, 3)).cuda()
    sync = extract_resnet_return(model, img[None], conf_th=0.001, topK=512, scales=[1.0])
    kp = torch.zeros((512, 2), device="cuda"); sc = torch.zeros((512,), device="cuda"); de = torch.zeros((512, 128), device="cuda")
    n = ctypes.c_int()
    torch.cuda.synchronize()
    _lib.check(ctx.lib.sfd2_extract(ctx.h, img.data_ptr(), 1, 240, 320, 0.001, 512, _lib.FLAG_ASYNC, kp.data_ptr(),
                                    sc.data_ptr(), de.data_ptr(), 1, 512, ctypes.byref(n)))
    assert n.value == -1
    ctx.sync()
    _lib.check(ctx.lib.sfd2_extract_count(ctx.h, ctypes.byref(n)))
    k = n.value
    assert k == len(sync["scores"])
    np.testing.assert_array_equal(kp[:k].cpu().numpy().astype(np.float64), sync["keypoints"])
    np.testing.assert_array_equal(sc[:k].cpu().numpy().astype(np.float64), sync["scores"])
    np.testing.assert_array_equal(de[:k].cpu().numpy().astype(np.float64), sync["descriptors"])


def test_no_stability_and_empty_result(synth_sd):
    from sfd2_amd.extractor import extract_resnet_return
    from sfd2_amd.model import ResSegNetV2
    m = ResSegNetV2(outdim=128, require_stability=False, precision="f16").eval()
    m.load_state_dict(synth_sd)
    m.cuda(0)
    img = synth.make_image(96, 128, 21)
    got = extract_resnet_return(m, img[None], conf_th=0.001, topK=100, scales=[1.0])
    want = orc.extract_resnet_return(synth_sd, img, conf_th=0.001, topK=100, use_stability=False)
    _compare_extract(got, want, 0.9, 3e-3)
    score, stab, desc = m.det(orc.norm_rgb(img)[None])
    assert stab is None
    none = extract_resnet_return(m, img[None], conf_th=2.0, topK=100, scales=[1.0])   # nothing above threshold
    assert none["keypoints"].shape == (0, 2) and none["descriptors"].shape == (0, 128) and none["scores"].shape == (0,)


# ------------------------------------------------------------------ matchers
HLOC_CONFS = {
    "NNM": dict(do_mutual_check=True),
    "ONN": dict(do_mutual_check=False),
    "NNR": dict(do_mutual_check=True, distance_threshold=0.9),
    "RATIO": dict(do_mutual_check=True, ratio_threshold=0.8),
    "RATIO_DIST": dict(do_mutual_check=False, ratio_threshold=0.9, distance_threshold=0.7),
}


def _hloc(d0, d1, conf, sim_mode):
    from sfd2_amd.matchers.nearest_neighbor import NearestNeighbor
    p = NearestNeighbor({**conf, "sim_mode": sim_mode})({"descriptors0": d0.T[None].copy(), "descriptors1": d1.T[None].copy()})
    return p["matches0"][0], p["matching_scores0"][0]


def _gaps(d0, d1):
    sim = d0.astype(np.float64) @ d1.astype(np.float64).T
    r = np.sort(sim, axis=1)
    c = np.sort(sim, axis=0)
    return r[:, -1] - r[:, -2], c[-1] - c[-2], sim


@pytest.mark.parametrize("tag", ["a", "b"])
def test_matchers_vs_reference_golden(golden_dir, tag):
    from sfd2_amd.matcher import Matcher, confs as mconfs
    g = _load(golden_dir, "matchers.npz")
    d0, d1 = g[f"{tag}/d0"], g[f"{tag}/d1"]
    for name, conf in HLOC_CONFS.items():
        gm, gs = g[f"{tag}/hloc/{name}/matches0"], g[f"{tag}/hloc/{name}/scores0"]
        m, s = _hloc(d0, d1, conf, "f16x2")
        assert (m != gm).mean() <= 0.003, name            # threshold tests on ~1e-7-different sums
        np.testing.assert_allclose(s[m == gm], gs[m == gm], atol=2e-6)
        m, s = _hloc(d0, d1, conf, "f16")
        assert (m != gm).mean() <= 0.02, name
        np.testing.assert_allclose(s[m == gm], gs[m == gm], atol=1e-3)
    for name in ("NNM", "NNR"):
        gm, gs = g[f"{tag}/itloc/{name}/matches0"], g[f"{tag}/itloc/{name}/scores0"]
        for sim_mode, tol_m, tol_s in (("f16x2", 0.003, 2e-6), ("f16", 0.02, 1e-3)):
            mc = {"output": name, "model": {**mconfs[name]["model"], "sim_mode": sim_mode}}
            p = Matcher(mc).eval().cuda()({"descriptors0": d0.astype(np.float64), "descriptors1": d1.astype(np.float64)})
            assert p["matches0"].dtype == np.int64 and p["matching_scores0"].dtype == np.float64
            assert (p["matches0"] != gm).mean() <= tol_m, (name, sim_mode)
            np.testing.assert_allclose(p["matching_scores0"], gs, atol=tol_s)


@pytest.mark.parametrize("n0,n1", [(4096, 4096), (1000, 37), (33, 1025), (1, 3), (5, 1), (128, 128), (300, 9001), (700, 33)])
def test_matcher_vs_oracle_sizes(n0, n1):
    d0 = synth.make_descriptors(n0, seed=n0 + 7)
    d1 = synth.make_descriptors(n1, seed=n1 + 8)
    k = min(n0, n1) // 2
    if k:
        rs = np.random.RandomState(9)
        src, dst = rs.permutation(n0)[:k], rs.permutation(n1)[:k]
        noisy = d0[src] + (0.02 + 0.1 * rs.random_sample((k, 1))).astype(np.float32) * rs.standard_normal((k, 128)).astype(np.float32)
        d1[dst] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
    rg, cg, sim = _gaps(d0, d1) if n1 > 1 and n0 > 1 else (np.ones(n0), np.ones(n1), d0.astype(np.float64) @ d1.astype(np.float64).T)
    for name, conf in (("NNM", HLOC_CONFS["NNM"]), ("ONN", HLOC_CONFS["ONN"])):
        want = orc.hloc_nearest_neighbor(d0, d1, **conf)
        for sim_mode, gap, tol in (("f16", 1e-3, 1e-3), ("f16x2", 1e-5, 2e-6)):
            m, s = _hloc(d0, d1, conf, sim_mode)
            # rows whose own arg-max and whose partner's arg-max are unambiguous at this precision
            safe = rg > gap
            if conf["do_mutual_check"]:
                j = np.argmax(sim, axis=1)
                safe &= cg[j] > gap
            np.testing.assert_array_equal(m[safe], want["matches0"][safe])
            same = m == want["matches0"]
            np.testing.assert_allclose(s[same], want["matching_scores0"][same], atol=tol)
            if conf["do_mutual_check"]:      # mutual matches are a partial bijection
                mm = m[m >= 0]
                assert len(np.unique(mm)) == len(mm)


@pytest.mark.parametrize("name", ["NNM", "ONN"])
def test_matcher_exact_ties_take_the_first_index(name):
    """Duplicated descriptors give bit-identical similarities: torch's argmax / topk take the FIRST maximum
    (hloc/matchers/nearest_neighbor.py:8,19-24), in both directions, and so must the single-GEMM kernel (id bits of the
    reverse keys in index order, lowest claiming candidate wins).  Rows are checked where the tie is the only ambiguity."""
    rs = np.random.RandomState(31)
    n0, n1 = 700, 900
    d0 = synth.make_descriptors(n0, seed=41)
    d1 = synth.make_descriptors(n1, seed=42)
    src = rs.permutation(300)[:120]
    d1[:120] = d0[src]                                   # exact partners: similarity |fp16(d)|^2 on both sides
    d1[500:560] = d1[:60]                                # duplicated candidates: the lower index must win
    dup_q = np.arange(60, 100)
    d0[400 + np.arange(40)] = d0[src[dup_q]]             # duplicated queries (all above 300): the lower index must win
    near = np.array([[4, 8], [37, 41], [70, 100], [200, 203]])      # ... and within one 32-row MFMA tile / one wave / one block
    d0[near[:, 1]] = d0[near[:, 0]]
    d1[700:704] = d0[near[:, 0]]
    conf = HLOC_CONFS[name]
    want = orc.hloc_nearest_neighbor(d0, d1, **conf)["matches0"]
    m, _ = _hloc(d0, d1, conf, "f16")
    rows = np.concatenate([src, 400 + np.arange(40), near.ravel()])
    np.testing.assert_array_equal(m[rows], want[rows])
    # the construction does what it is meant to (the oracle is the judge of the rows, these only guard the test itself)
    assert (want[src] == np.arange(120)).mean() > 0.9    # first of the duplicated candidates
    dq = want[400 + np.arange(40)]
    assert ((dq == -1).mean() > 0.9) if conf["do_mutual_check"] else ((dq == dup_q).mean() > 0.9)


def test_matcher_near_ties_are_bounded():
    """Near ties: the mutual modes carry an 8-bit query id in the low mantissa bits of the column maxima, so two
    similarities closer than 2^-15 relative compare equal and the lower index wins -- torch compares all 24 bits.  Where the two
    differ, the pair this library reports is a mutual nearest neighbour UP TO that truncation: never a pair whose similarity is
    more than 2^-14 (relative) below the row's and the column's true maximum.  Descriptors are fp16-representable, so the only
    differences left are summation order (1e-7) and the truncation."""
    rs = np.random.RandomState(77)
    n0, n1 = 1500, 1800
    d0 = synth.make_descriptors(n0, seed=51).astype(np.float16).astype(np.float32)
    d1 = synth.make_descriptors(n1, seed=52).astype(np.float16).astype(np.float32)
    d1[:600] = d0[rs.permutation(n0)[:600]]                      # partners
    base = rs.permutation(600)[:300]
    dup = 600 + np.arange(300)
    d1[dup] = d1[base]                                           # near-duplicates of partners: one element one fp16 step away
    k = rs.randint(0, 128, size=300)
    step = np.spacing(np.abs(d1[dup, k]).astype(np.float16)).astype(np.float32)
    d1[dup, k] += np.where(rs.rand(300) < 0.5, step, -step)
    conf = HLOC_CONFS["NNM"]
    want = orc.hloc_nearest_neighbor(d0, d1, **conf)["matches0"]
    got, _ = _hloc(d0, d1, conf, "f16")
    sim = d0.astype(np.float64) @ d1.astype(np.float64).T
    rmax, cmax = sim.max(axis=1), sim.max(axis=0)
    diff = np.nonzero(got != want)[0]
    assert len(diff) <= 0.15 * n0, len(diff)      # (300 planted near-duplicates: each can flip a row either way)
    tol = 2.0 ** -14
    for i in diff:
        if got[i] >= 0:       # a reported pair must be mutual up to the truncation
            j = got[i]
            assert sim[i, j] >= rmax[i] - tol * abs(rmax[i]) and sim[i, j] >= cmax[j] - tol * abs(cmax[j]), (i, j)
        if want[i] >= 0:      # a dropped pair must have lost against a near-equal
            j = want[i]
            assert got[i] >= 0 or np.sort(sim[:, j])[-2] >= cmax[j] - tol * abs(cmax[j]) or np.sort(sim[i])[-2] >= rmax[i] - tol * abs(rmax[i]), (i, j)
    # rows without a near-tie are identical
    r2 = np.sort(sim, axis=1)[:, -2]
    clear = (rmax - r2) > 1e-3
    cl_c = (cmax - np.sort(sim, axis=0)[-2]) > 1e-3
    rows = np.nonzero(clear & ((want < 0) | cl_c[np.maximum(want, 0)]))[0]
    assert (got[rows] == want[rows]).mean() > 0.995


def test_matcher_batch_equals_single_and_handles_empty():
    from sfd2_amd.matcher import Matcher, confs as mconfs
    mt = Matcher(mconfs["NNM"])
    d0 = synth.make_descriptors(700, seed=1)
    dbs = [synth.make_descriptors(n, seed=10 + i) for i, n in enumerate((512, 100, 0, 900, 33))]
    m, s = mt.match_batch(d0, dbs)
    assert m.shape == (5, 700)
    for i, d1 in enumerate(dbs):
        if len(d1) == 0:
            assert (m[i] == -1).all()
            continue
        p = mt({"descriptors0": d0, "descriptors1": d1})
        np.testing.assert_array_equal(m[i], p["matches0"])
        np.testing.assert_allclose(s[i], p["matching_scores0"], atol=0)


def test_hloc_plugin_with_cuda_tensors():
    import torch
    from sfd2_amd import matchers
    from sfd2_amd.base_model import dynamic_load
    Model = dynamic_load(matchers, "nearest_neighbor")
    model = Model({"do_mutual_check": True, "distance_threshold": 0.9}).eval().to("cuda")
    d0 = torch.from_numpy(synth.make_descriptors(600, seed=3).T.copy())[None].cuda()
    d1 = torch.from_numpy(synth.make_descriptors(500, seed=4).T.copy())[None].cuda()
    pred = model({"descriptors0": d0, "descriptors1": d1})
    assert pred["matches0"].is_cuda and pred["matches0"].dtype == torch.int64 and pred["matches0"].shape == (1, 600)
    assert pred["matching_scores0"].dtype == torch.float32
    cpu = model({"descriptors0": d0.cpu(), "descriptors1": d1.cpu()})
    assert torch.equal(pred["matches0"].cpu(), cpu["matches0"]) and torch.equal(pred["matching_scores0"].cpu(), cpu["matching_scores0"])
    from sfd2_amd.match_features import cast_for_storage
    m16, s16 = cast_for_storage(cpu["matches0"][0].numpy(), cpu["matching_scores0"][0].numpy())
    assert m16.dtype == np.int16 and s16.dtype == np.float16


# ------------------------------------------------------------------ strict fp32 mode
# precision='f32': the conv stack runs in exact fp32 on the f32-input MFMA.  It differs from the
# fp32 reference only by summation order, so the tolerances are fp32 round-off and the key-point
# LIST (not just the set) reproduces the reference's up to swaps of near-equal scores.
@pytest.fixture(scope="module")
def model_f32(synth_sd):
    if not _gpu_ok():
        pytest.fail("no MI355X visible")
    from sfd2_amd.model import ResSegNetV2
    m = ResSegNetV2(outdim=128, require_stability=True, precision="f32").eval()
    m.load_state_dict(synth_sd)
    m.cuda(0)
    return m


@pytest.mark.parametrize("h,w,seed", [(64, 96, 11), (100, 130, 12), (37, 53, 13)])
def test_strict_det_vs_oracle(model_f32, synth_sd, h, w, seed):
    img = synth.make_image(h, w, seed)
    x = orc.norm_rgb(img)
    taps = {}
    o_score, o_stab, o_desc = orc.det(synth_sd, x, taps)
    score, stab, desc = model_f32.det(x[None])
    ctx = model_f32.context
    for name, want in taps.items():
        got = ctx.debug_activation(name)
        np.testing.assert_allclose(got, want, atol=1e-4, rtol=1e-4, err_msg=name)
    np.testing.assert_allclose(score[0, 0], o_score, atol=1e-6, rtol=2e-4)
    np.testing.assert_allclose(desc[0], o_desc, atol=2e-5)
    assert (stab[0, 0] != o_stab).mean() <= 5e-4


def _compare_strict(got, want, desc_tol):
    mine = _kp_index(got["keypoints"])
    rank = np.array([mine.get((float(x), float(y)), -1) for x, y in want["keypoints"]])
    found = rank >= 0
    assert abs(len(got["scores"]) - len(want["scores"])) <= 2
    assert found.mean() >= 0.995, found.mean()
    assert np.abs(rank[found] - np.flatnonzero(found)).max() <= 3          # order, up to near-ties
    np.testing.assert_allclose(got["scores"][rank[found]], np.asarray(want["scores"], dtype=np.float64)[found], atol=1e-5, rtol=2e-4)
    dd = np.abs(got["descriptors"][rank[found]] - np.asarray(want["descriptors"], dtype=np.float64)[found]).max()
    # what the tolerance above actually admitted: written next to the other measured values of the run
    line = (f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}: {int((~found).sum())} of {len(found)} reference key points missing, "
            f"max rank shift {int(np.abs(rank[found] - np.flatnonzero(found)).max())}, "
            f"{int((rank[found] != np.flatnonzero(found)).sum())} at another rank, descriptors {dd:.2e}")
    print(line)
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(d):
        with open(os.path.join(d, "strict_parity_measured.txt"), "a") as f:
            f.write(line + "\n")
    assert dd <= desc_tol, dd


@pytest.mark.parametrize("h,w,seed,topk", [(96, 128, 21, 200), (100, 130, 22, -1), (480, 640, 0, 1024)])
def test_strict_extract_vs_oracle_and_reference_golden(model_f32, synth_sd, golden_dir, h, w, seed, topk):
    from sfd2_amd.extractor import extract_resnet_return
    img = synth.make_image(h, w, seed)
    got = extract_resnet_return(model_f32, img[None], conf_th=0.001, topK=topk, scales=[1.0])
    want = orc.extract_resnet_return(synth_sd, img, conf_th=0.001, topK=topk)
    _compare_strict(got, want, 2e-5)
    tag = {(96, 128): "96x128_k200", (100, 130): "100x130_all", (480, 640): "480x640_k1024"}[(h, w)]
    g = _load(golden_dir, f"extract_{tag}.npz")
    ref = {"keypoints": g["keypoints"], "scores": g["scores"], "descriptors": g["descriptors"].astype(np.float64)}
    _compare_strict(got, ref, 2e-3)    # the fixture stores the reference's descriptors as fp16


# ------------------------------------------------------------------ scale pyramid + uint8 ingest
MS_CASES = [("96x128_k150", 96, 128, 21, 150, [1.0, 0.5]), ("100x130_all", 100, 130, 22, -1, [1.2, 1.0, 0.6])]


@pytest.mark.parametrize("tag,h,w,seed,topk,scales", MS_CASES)
def test_strict_multiscale_vs_oracle_and_reference_golden(model_f32, synth_sd, golden_dir, tag, h, w, seed, topk, scales):
    from sfd2_amd.extractor import extract_resnet_return
    img = synth.make_image(h, w, seed)
    got = extract_resnet_return(model_f32, img[None], conf_th=0.001, topK=topk, scales=scales)
    want = orc.extract_resnet_return(synth_sd, img, conf_th=0.001, topK=topk, scales=tuple(scales))
    if topk > 0:
        assert (np.diff(got["scores"]) <= 0).all() and len(got["scores"]) == topk
        _compare_strict(got, want, 2e-5)
    else:   # concatenation in scale order, each level sorted: compare level by level (same lengths up to near-threshold points)
        assert abs(len(got["scores"]) - len(want["scores"])) <= 2
        _compare_strict_unordered(got, want, 2e-5)
    g = _load(golden_dir, f"extract_ms_{tag}.npz")
    ref = {"keypoints": g["keypoints"], "scores": g["scores"], "descriptors": g["descriptors"].astype(np.float64)}
    (_compare_strict if topk > 0 else _compare_strict_unordered)(got, ref, 2e-3)


def _compare_strict_unordered(got, want, desc_tol):
    # two pyramid levels can map key points onto the same coordinates: match with multiplicity, in order
    mine = {}
    for i, (x, y) in enumerate(got["keypoints"]):
        mine.setdefault((float(x), float(y)), []).append(i)
    rank = np.array([(mine.get((float(x), float(y))) or [-1]).pop(0) for x, y in want["keypoints"]])
    found = rank >= 0
    assert found.mean() >= 0.99, found.mean()
    assert np.abs(rank[found] - np.flatnonzero(found)).max() <= 4
    np.testing.assert_allclose(got["scores"][rank[found]], np.asarray(want["scores"], dtype=np.float64)[found], atol=1e-5, rtol=2e-4)
    dd = np.abs(got["descriptors"][rank[found]] - np.asarray(want["descriptors"], dtype=np.float64)[found]).max()
    assert dd <= desc_tol, dd


@pytest.mark.parametrize("tag,h,w,seed,topk,scales", MS_CASES)
def test_multiscale_f16_vs_oracle(model, synth_sd, tag, h, w, seed, topk, scales):
    from sfd2_amd.extractor import extract_resnet_return
    img = synth.make_image(h, w, seed)
    got = extract_resnet_return(model, img[None], conf_th=0.001, topK=topk, scales=scales)
    want = orc.extract_resnet_return(synth_sd, img, conf_th=0.001, topK=topk, scales=tuple(scales))
    _compare_extract(got, want, 0.9, 3e-3)
    np.testing.assert_allclose(np.linalg.norm(got["descriptors"], axis=1), 1.0, atol=1e-5)


def test_multiscale_single_level_equals_single_scale(model):
    """scales=[1.0] through the pyramid entry point == sfd2_extract, bit for bit."""
    ctx = model.context
    img = synth.make_image(240, 320, 3)
    from sfd2_amd.extractor import extract_resnet_return
    one = extract_resnet_return(model, img[None], conf_th=0.001, topK=512, scales=[1.0])
    kp = np.empty((512, 2), np.float32); sc = np.empty((512,), np.float32); de = np.empty((512, 128), np.float32)
    n = ctypes.c_int()
    sarr = (ctypes.c_double * 1)(1.0)
    _lib.check(ctx.lib.sfd2_extract_multiscale(ctx.h, img.ctypes.data, 0, 240, 320, sarr, 1, 0.001, 512, 0, kp.ctypes.data,
                                               sc.ctypes.data, de.ctypes.data, 0, 512, ctypes.byref(n)))
    k = n.value
    assert k == len(one["scores"])
    np.testing.assert_array_equal(kp[:k].astype(np.float64), one["keypoints"])
    np.testing.assert_array_equal(sc[:k].astype(np.float64), one["scores"])
    np.testing.assert_array_equal(de[:k].astype(np.float64), one["descriptors"])


@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_uint8_hwc_ingest_equals_float_path(model, model_f32, precision):
    """extract_localization.py:165-186: uint8 HWC (RGB or cv2 BGR) -> astype(float32) / 255. -> CHW on the device
    must equal the same conversion done on the host, bit for bit, in both precisions and through the pyramid."""
    import torch
    from sfd2_amd.extractor import extract_resnet_return
    m = model if precision == "f16" else model_f32
    rs = np.random.RandomState(7)
    base = (synth.make_image(120, 168, 9).transpose(1, 2, 0) * 255.0 + rs.uniform(-0.5, 0.5, (120, 168, 3)))
    u8 = np.clip(np.rint(base), 0, 255).astype(np.uint8)
    f = (u8.astype(np.float32).transpose(2, 0, 1) / 255.).astype(np.float32)
    want = extract_resnet_return(m, f[None], conf_th=0.001, topK=300, scales=[1.0])
    for arr, kw in [(u8, {}), (np.ascontiguousarray(u8[:, :, ::-1]), {"bgr": True}), (torch.from_numpy(u8).cuda(), {})]:
        got = extract_resnet_return(m, arr, conf_th=0.001, topK=300, scales=[1.0], **kw)
        for k in ("keypoints", "scores", "descriptors"):
            np.testing.assert_array_equal(got[k], want[k])
    want = extract_resnet_return(m, f[None], conf_th=0.001, topK=300, scales=[1.0, 0.75])
    got = extract_resnet_return(m, u8, conf_th=0.001, topK=300, scales=[1.0, 0.75])
    for k in ("keypoints", "scores", "descriptors"):
        np.testing.assert_array_equal(got[k], want[k])


def test_strict_full_size_vs_oracle(model_f32, synth_sd):
    from sfd2_amd.extractor import extract_resnet_return
    img = synth.make_image(1200, 1600, 5)
    got = extract_resnet_return(model_f32, img[None], conf_th=0.001, topK=4096, scales=[1.0])
    want = orc.extract_resnet_return(synth_sd, img, conf_th=0.001, topK=4096)
    _compare_strict(got, want, 2e-5)
    print("strict 1600x1200 timings:", model_f32.context.timings())


# ------------------------------------------------------------------ extract.py variant (greedy NMS) and feature_matching
@pytest.mark.parametrize("h,w,density", [(60, 80, 0.2), (97, 131, 1.0), (300, 400, 0.05), (64, 64, 1.0)])
def test_nms_fast_vs_oracle_bit_exact(ctx, h, w, density):
    rs = np.random.RandomState(h + w)
    heat = rs.random_sample((h, w)).astype(np.float32) + 0.01
    if (h, w) == (64, 64):      # monotone ramp: the longest dependency chain of the greedy order
        heat = (np.arange(h * w, dtype=np.float32).reshape(h, w) + 1) / (h * w)
    heat = np.where(rs.random_sample((h, w)) < density, heat, 0).astype(np.float32)
    th = 0.005
    ys, xs = np.where(heat >= th)
    keep = orc.nms_fast(xs.astype(np.float32), ys.astype(np.float32), heat[ys, xs], h, w, 4)
    want = np.zeros_like(heat)
    want[ys[keep], xs[keep]] = heat[ys[keep], xs[keep]]
    got = np.empty_like(heat)
    _lib.check(ctx.lib.sfd2_nms_fast(ctx.h, heat.ctypes.data, h, w, th, 4, got.ctypes.data))
    np.testing.assert_array_equal(got, want)


def test_extract_py_api_vs_reference_golden_and_oracle(model, model_f32, synth_sd, golden_dir):
    from sfd2_amd.extract import extract_spp_return, nms_fast
    g = _load(golden_dir, "extract_spp_96x128.npz")
    c = g["nf/corners"]
    out, inds = nms_fast(c, int(g["nf/h"]), int(g["nf/w"]), 4)
    np.testing.assert_array_equal(inds, g["nf/inds"])
    np.testing.assert_array_equal(out, g["nf/out"])
    h, w, th = int(g["h"]), int(g["w"]), float(g["conf_th"])
    x = orc.norm_rgb(synth.make_image(h, w, int(g["seed"])))
    want = orc.extract_spp_feats_singlescale(synth_sd, x, th)
    for m, tol_pts, tol_desc, min_found in ((model_f32, 1e-5, 2e-5, 0.99), (model, 8e-2, 3e-3, 0.93)):
        pts, desc, scores, desc_full, heat = extract_spp_return(m, x[None], conf_th=th)
        assert pts.dtype == np.float64 and desc.dtype == np.float32 and desc_full.shape == want[3].shape and heat.shape == (h, w)
        for ref_pts, ref_desc, dt in ((want[0], want[1], tol_desc), (g["pts"], g["desc"].astype(np.float32), max(tol_desc, 2e-3))):
            mine = {(int(a), int(b)): i for i, (a, b, _) in enumerate(pts)}
            rank = np.array([mine.get((int(a), int(b)), -1) for a, b, _ in ref_pts])
            ok = rank >= 0
            assert ok.mean() >= min_found, ok.mean()
            rel = np.abs(pts[rank[ok], 2] - ref_pts[ok, 2]) / ref_pts[ok, 2]
            assert np.mean(rel > tol_pts + 1e-4) <= 0.02          # fp16 mode: rare stability-class flips
            assert np.abs(desc[rank[ok]] - ref_desc[ok]).max() <= dt
        np.testing.assert_allclose(desc_full, want[3], atol=max(tol_desc, 2e-5))
    with pytest.raises(NotImplementedError):
        extract_spp_return(model, "an/image/path.jpg")       # decoding stays with the caller


def test_feature_matching_mask_and_remap():
    """it_loc/localize_cv2.py:511-560: only db key points with a 3D point take part; indices map back."""
    from sfd2_amd.localize import feature_matching
    from sfd2_amd.matcher import Matcher, confs as mconfs
    mt = Matcher({"output": "NNM", "model": {**mconfs["NNM"]["model"], "sim_mode": "f16x2"}}).eval().cuda()
    q = synth.make_descriptors(400, seed=5).astype(np.float64)
    db = synth.make_descriptors(600, seed=6).astype(np.float64)
    rs = np.random.RandomState(2)
    db[rs.permutation(600)[:200]] = q[rs.permutation(400)[:200]]      # exact duplicates -> certain matches
    ids = np.where(rs.random_sample(600) < 0.6, rs.randint(0, 10000, 600), -1)
    got = feature_matching(q, db, mt, db_3D_ids=ids)
    valid = np.flatnonzero(ids != -1)
    want = orc.itloc_matcher(q, db[valid], "nnm")["matches0"]
    want = np.where(want >= 0, valid[np.maximum(want, 0)], -1)
    np.testing.assert_array_equal(got, want)
    assert (ids[got[got >= 0]] != -1).all()
    assert (feature_matching(q, db, mt, db_3D_ids=np.full(600, -1)) == -1).all()      # <= 3 valid: early out
    plain = feature_matching(q, db, mt)
    np.testing.assert_array_equal(plain, orc.itloc_matcher(q, db, "nnm")["matches0"])


@pytest.mark.parametrize("mode", ["NNM", "NNR"])
def test_feature_matching_batch_device_mask_and_remap(mode):
    """One query against K database images, masks and remaps on the device:
    equals the per-image feature_matching loop and the oracle on gathered descriptors."""
    from sfd2_amd.localize import feature_matching, feature_matching_batch
    from sfd2_amd.matcher import Matcher, confs as mconfs
    mt = Matcher({"output": mode, "model": {**mconfs[mode]["model"], "sim_mode": "f16x2"}}).eval().cuda()
    rs = np.random.RandomState(11)
    q = synth.make_descriptors(500, seed=15).astype(np.float64)
    dbs, ids = [], []
    for i, n in enumerate([700, 64, 333, 10, 1200]):
        d = synth.make_descriptors(n, seed=20 + i).astype(np.float64)
        take = rs.permutation(n)[:n // 3]
        d[take] = q[rs.permutation(500)[:len(take)]] + rs.normal(0, 0.01, (len(take), 128))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        dbs.append(d)
        ids.append(np.where(rs.random_sample(n) < 0.5, rs.randint(0, 100000, n), -1))
    ids[3][:] = -1
    ids[3][:3] = 5                                       # exactly 3 valid -> early out, all -1
    ids.append(None); dbs.append(dbs[0])                 # an unmasked image rides in the same batch
    got = feature_matching_batch(q, dbs, mt, ids)
    assert len(got) == len(dbs)
    for i, (d, pid) in enumerate(zip(dbs, ids)):
        np.testing.assert_array_equal(got[i], feature_matching(q, d, mt, db_3D_ids=pid), err_msg=str(i))
        if pid is None:
            want = orc.itloc_matcher(q, d, mode.lower())["matches0"]
        else:
            valid = np.flatnonzero(pid != -1)
            if len(valid) <= 3:
                want = np.full(500, -1)
            else:
                w = orc.itloc_matcher(q, d[valid], mode.lower())["matches0"]
                want = np.where(w >= 0, valid[np.maximum(w, 0)], -1)
        np.testing.assert_array_equal(got[i], want, err_msg=str(i))
    assert (got[3] == -1).all()


def test_match_batch_row_selection_rejects_bad_indices(ctx):
    d = synth.make_descriptors(32, seed=1)
    rows = np.array([0, 5, 32], dtype=np.int32)
    q = _lib.DescSet(d.ctypes.data, 32, _lib.DT_F32, _lib.LAYOUT_ND, 0, None, 0, 0)
    db = (_lib.DescSet * 1)(_lib.DescSet(d.ctypes.data, 32, _lib.DT_F32, _lib.LAYOUT_ND, 0, rows.ctypes.data, 3, 0))
    conf = _lib.MatchConf(1, 1, 0.0, 0.0, 0)
    m = np.empty((1, 32), np.int64); s = np.empty((1, 32), np.float32)
    rc = ctx.lib.sfd2_match_batch(ctx.h, ctypes.byref(q), db, 1, 128, ctypes.byref(conf), m.ctypes.data, s.ctypes.data, 0, 0)
    assert rc != 0 and b"out of range" in ctx.lib.sfd2_last_error()


def test_pipeline_mains_write_reference_layout(tmp_path, synth_sd):
    """extract_localization.main -> feature store -> match_features.main, uint8 images in, the reference's
    group / dataset names and dtypes out; stored matches equal a direct NearestNeighbor call."""
    from sfd2_amd import extract_localization as el, match_features as mf, feature_io as fio
    from sfd2_amd.matchers.nearest_neighbor import NearestNeighbor
    name, conf = next(iter(el.confs.items()))
    conf = {**conf, "model": {**conf["model"], "max_keypoints": 256}}
    imgs = []
    for i, nm in enumerate(["db/a.jpg", "db/b.jpg", "query/c.jpg"]):
        u8 = (synth.make_image(96, 128, 40 + i).transpose(1, 2, 0) * 255).astype(np.uint8)
        imgs.append({"name": nm, "image": u8, "original_size": (256, 192)})      # features live at 2x the network size
    path = el.main(conf, imgs, tmp_path, state_dict=synth_sd)
    st = fio.open_store(path, "r")
    assert list(st.keys()) == ["db/a.jpg", "db/b.jpg", "query/c.jpg"]
    g = st["db/a.jpg"]
    n = g["scores"].shape[0]
    assert g["keypoints"].shape == (n, 2) and g["descriptors"].shape == (128, n) and n > 50
    assert g["keypoints"].dtype == np.float64 and g["descriptors"].dtype == np.float64 and g["scores"].dtype == np.float64
    np.testing.assert_array_equal(g["image_size"].__array__(), [256, 192])
    kp = g["keypoints"].__array__()
    assert np.allclose((kp + .5) / 2 - .5, np.rint((kp + .5) / 2 - .5))          # (kp + .5) * scale - .5 with scale 2
    pairs = ["query/c.jpg db/a.jpg", "db/a.jpg query/c.jpg", "query/c.jpg db/b.jpg"]
    mpath = mf.main(mf.confs["NNM"], pairs, "feats-" + name, tmp_path)
    ms = fio.open_store(mpath, "r")
    assert list(ms.keys()) == ["query-c.jpg_db-a.jpg", "query-c.jpg_db-b.jpg"]           # the reversed duplicate is skipped
    m = ms["query-c.jpg_db-a.jpg"]
    assert m["matches0"].dtype == np.int16 and m["matching_scores0"].dtype == np.float16
    nn = NearestNeighbor(mf.confs["NNM"]["model"]).eval().to("cuda")
    pred = nn({"descriptors0": st["query/c.jpg"]["descriptors"].__array__().astype(np.float32)[None],
               "descriptors1": st["db/a.jpg"]["descriptors"].__array__().astype(np.float32)[None]})
    np.testing.assert_array_equal(m["matches0"][()], np.asarray(pred["matches0"][0]).astype(np.int16))
    assert (m["matches0"][()] >= 0).sum() > 0


@pytest.mark.parametrize("h,w,seed", [(64, 96, 11), (100, 130, 12), (37, 53, 13), (480, 640, 2), (8, 8, 3), (9, 17, 4), (16, 250, 5)])
def test_fused_resblock_vs_oracle_and_unfused(model, ctx, synth_sd, h, w, seed):
    """resblock_kernel (conv1 + grouped conv + conv3 + residual in one kernel, the throughput path's ResBlock)
    forced onto the parity entry point: its block outputs against the oracle's fp32 activations and against the
    three-kernel path, and the heads computed from them."""
    img = synth.make_image(h, w, seed)
    x = orc.norm_rgb(img)
    taps = {}
    o_score, o_stab, o_desc = orc.det(synth_sd, x, taps)
    score_u, stab_u, desc_u = model.det(x[None])
    unfused = {k: ctx.debug_activation(k) for k in ("conv4.0", "conv4.1", "conv4.2")}
    ctx.set_option("fuse_det", 1)      # the throughput path's fused kernels at the parity entry point
    try:
        score_f, stab_f, desc_f = model.det(x[None])
        fused = {k: ctx.debug_activation(k) for k in ("conv4.0", "conv4.1", "conv4.2")}
    finally:
        ctx.set_option("fuse_det", 0)
    for k in fused:
        want = taps[k]
        assert fused[k].shape == want.shape
        err = np.abs(fused[k] - want).max()
        assert err <= 1.5e-2 * np.abs(want).max(), (k, err)
        # same fp16 operands and K order as the three-kernel path: equal up to fp16 rounding of the intermediates
        assert np.abs(fused[k] - unfused[k]).max() <= 4e-3 * np.abs(want).max(), k
    # score = soft-max of logits the fp16 stack knows to ~8e-2 at this size (profiles/r02_error_budget.txt, column
    # "logits"): 8 % relative for all but a handful of the 307 200 pixels at 480 x 640, 15 % for every pixel
    d = np.abs(score_f[0, 0] - o_score)
    assert (d <= 8e-2 * o_score + 1e-4).mean() >= 0.9999 and (d <= 15e-2 * o_score + 1e-4).all()
    assert np.abs(desc_f[0] - o_desc).max() <= 3e-3
    assert (stab_f[0, 0] != o_stab).mean() < 0.01


def test_hipgraph_capture_replay_matches_eager(model):
    """BASELINE configs[4]: one extract + match step captured on the context's stream and replayed as a hipGraph gives the
    eager step's outputs bit for bit (device-resident inputs / outputs, SFD2_FLAG_ASYNC: the calls are pure stream work)."""
    import torch
    hip = ctypes.CDLL("libamdhip64.so")
    ctx = model.context
    lib = ctx.lib
    H, W, K, KDB = 240, 320, 512, 3
    img = torch.from_numpy(synth.make_image(H, W, 31)).cuda()
    db = [torch.from_numpy(synth.make_descriptors(400 + 50 * i, seed=70 + i)).to(torch.float16).cuda().contiguous() for i in range(KDB)]
    dbs = (_lib.DescSet * KDB)(*[_lib.DescSet(d.data_ptr(), d.shape[0], _lib.DT_F16, _lib.LAYOUT_ND, 1) for d in db])
    mconf = _lib.MatchConf(_lib.MATCH_HLOC, 1, 0.0, 0.0, _lib.SIM_F16)
    kp = torch.zeros((K, 2), device="cuda"); sc = torch.zeros((K,), device="cuda"); de = torch.zeros((K, 128), device="cuda")
    mt = torch.full((KDB, K), -7, dtype=torch.int64, device="cuda"); ms = torch.zeros((KDB, K), device="cuda")
    q = _lib.DescSet(de.data_ptr(), K, _lib.DT_F32, _lib.LAYOUT_ND, 1)
    n = ctypes.c_int()

    def step():
        _lib.check(lib.sfd2_extract(ctx.h, img.data_ptr(), 1, H, W, 0.001, K, _lib.FLAG_ASYNC, kp.data_ptr(), sc.data_ptr(),
                                    de.data_ptr(), 1, K, ctypes.byref(n)))
        _lib.check(lib.sfd2_match_batch(ctx.h, ctypes.byref(q), dbs, KDB, 128, ctypes.byref(mconf), mt.data_ptr(), ms.data_ptr(),
                                        1, _lib.FLAG_ASYNC))

    torch.cuda.synchronize()
    step(); step()
    ctx.sync()
    want = (kp.clone(), sc.clone(), de.clone(), mt.clone(), ms.clone())
    assert (want[3] >= 0).sum() > 0
    stream = ctypes.c_void_p(lib.sfd2_get_stream(ctx.h))
    graph, gexec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 2) == 0      # hipStreamCaptureModeRelaxed
    try:
        step()
    finally:
        rc = hip.hipStreamEndCapture(stream, ctypes.byref(graph))
    assert rc == 0 and graph.value
    assert hip.hipGraphInstantiate(ctypes.byref(gexec), graph, None, None, 0) == 0
    for t in (kp, sc, de, ms):
        t.zero_()
    mt.fill_(-7)
    torch.cuda.synchronize()
    assert hip.hipGraphLaunch(gexec, stream) == 0
    assert hip.hipGraphLaunch(gexec, stream) == 0
    ctx.sync()
    for got, exp in zip((kp, sc, de, mt, ms), want):
        assert torch.equal(got, exp)
    hip.hipGraphExecDestroy(gexec)
    hip.hipGraphDestroy(graph)
    step()        # eager calls keep working after the capture
    ctx.sync()
    assert torch.equal(mt, want[3])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_itloc_label_matcher_vs_reference_golden(golden_dir, tag):
    """Matcher mode 'nnml' (it_loc/matcher.py:239-297): every per-label and rest-set mutual NN on the
    device, grouping on the host as in the reference."""
    from sfd2_amd.matcher import Matcher
    g = _load(golden_dir, "matchers.npz")
    mt = Matcher({"output": "NNML", "model": {"name": "nnml", "sim_mode": "f16x2"}}).eval().cuda()
    pred = mt({"descriptors0": g[f"{tag}/d0"].astype(np.float64), "descriptors1": g[f"{tag}/d1"].astype(np.float64),
               "labels0": g[f"{tag}/labels0"], "labels1": g[f"{tag}/labels1"]})
    np.testing.assert_array_equal(pred["matches0"], g[f"{tag}/itloc/NNML/matches0"])
    np.testing.assert_allclose(pred["matching_scores0"], g[f"{tag}/itloc/NNML/scores0"], atol=2e-6)


@pytest.mark.parametrize("tag", ["96x128_k120", "96x128_k180", "100x130_k5000"])
def test_strict_extract_mask_branch_vs_reference_golden(model_f32, synth_sd, golden_dir, tag):
    """extract_resnet_return(mask=...) (nets/extractor.py:240-319): every candidate from the device,
    the labelled-first selection on the host as in the reference."""
    from sfd2_amd.extractor import extract_resnet_return
    g = _load(golden_dir, f"extract_mask_{tag}.npz")
    img = synth.make_image(int(g["h"]), int(g["w"]), int(g["seed"]))
    got = extract_resnet_return(model_f32, img[None], conf_th=0.001, mask=g["mask"], topK=int(g["topk"]), scales=[1.0])
    want = orc.extract_resnet_return(synth_sd, img, conf_th=0.001, topK=int(g["topk"]), mask=g["mask"])
    assert got["labels"].dtype == np.int32 and len(got["labels"]) == len(got["scores"])
    for ref in (want, {"keypoints": g["keypoints"], "scores": g["scores"], "descriptors": g["descriptors"].astype(np.float64),
                       "labels": g["labels"]}):
        assert abs(len(got["scores"]) - len(ref["scores"])) <= 2
        mine = {(float(x), float(y)): i for i, (x, y) in enumerate(got["keypoints"])}
        rank = np.array([mine.get((float(x), float(y)), -1) for x, y in ref["keypoints"]])
        found = rank >= 0
        assert found.mean() >= 0.99
        np.testing.assert_array_equal(got["labels"][rank[found]], np.asarray(ref["labels"])[found])
        assert np.abs(rank[found] - np.flatnonzero(found)).max() <= 3


def test_throughput_path_equals_layerwise_path_random_sizes(synth_sd):
    """The throughput path of sfd2_extract (fused stem, fused ResBlocks, aliased activation arena, persistent kernels)
    against a context with option "fuse" = 0 (one kernel per layer, private buffers) on seeded random image
    sizes, odd ones included: same key-point set up to near-threshold points, scores and descriptors within fp16
    rounding of the intermediates."""
    from sfd2_amd.model import ResSegNetV2
    from sfd2_amd.extractor import extract_resnet_return

    def make(no_fuse):
        m = ResSegNetV2(outdim=128, require_stability=True, precision="f16").eval()
        m.load_state_dict(synth_sd)
        m.cuda(0)
        if no_fuse:
            m.context.set_option("fuse", 0)
        return m

    fused, plain = make(False), make(True)
    rs = np.random.RandomState(123)
    sizes = [(int(rs.randint(8, 260)), int(rs.randint(8, 330))) for _ in range(10)] + [(8, 8), (33, 31), (240, 320)]
    ratios = []
    for h, w in sizes:
        img = synth.make_image(h, w, 1000 + h * 7 + w)
        a = extract_resnet_return(fused, img[None], conf_th=0.001, topK=300, scales=[1.0])
        b = extract_resnet_return(plain, img[None], conf_th=0.001, topK=300, scales=[1.0])
        assert np.isfinite(a["descriptors"]).all() and np.isfinite(a["scores"]).all(), (h, w)
        ka = {(x, y): i for i, (x, y) in enumerate(map(tuple, a["keypoints"]))}
        kb = {(x, y): i for i, (x, y) in enumerate(map(tuple, b["keypoints"]))}
        common = sorted(set(ka) & set(kb))
        union = len(set(ka) | set(kb))
        # one 3-class stability arg-max flip at a near-tie rescales a 4x4 block of the heat map by 2x-10x and moves the
        # NMS winners around it, so a single size may lose a cluster of key points; the typical size must not
        ratios.append(1.0 if union == 0 else len(common) / union)
        assert ratios[-1] >= 0.90, (h, w, len(common), union)
        if common:
            ia = np.array([ka[k] for k in common]); ib = np.array([kb[k] for k in common])
            sa, sb = a["scores"][ia], b["scores"][ib]
            ok = np.abs(sa - sb) <= 2e-2 * sb + 1e-5
            assert ok.mean() >= 0.98, (h, w, ok.mean())          # the rest: 3-class stability flips at near-ties
            assert np.abs(a["descriptors"][ia] - b["descriptors"][ib]).max() <= 2e-3, (h, w)
    assert sum(r >= 0.97 for r in ratios) >= len(ratios) - 1, ratios
