"""NMS and top-K selection at the places the parity suite's inputs never reach (pytest -m gpu): values that decide a
pixel's fate from exactly 5 * radius away across every tile seam of both nms4 tile heights and of the generic-radius
kernel, equal scores straddling the top-K cut, boundary bins of more than 256 keys, cuts on bin edges and inside the two
clamped bins, the candidate capacity and one past it, cap_out below the number selected, and calls of different kinds
back to back on one context.

Every test calls sfd2_simple_nms / sfd2_select_keypoints on host maps and compares with the C oracle (orc_simple_nms,
orc_select_keypoints: score descending, then pixel index ascending) by assert_array_equal: no tolerance anywhere.
tests/test_nms_ref_host.py shows without a GPU that these inputs can fail: a halo one pixel short changes every seam
chain, the const / plateau maps put more than 256 keys into one bin, and the shape lists reach the tile they name.
The case definitions up to the first fixture need no GPU and no library."""
import ctypes
import functools
import time

import numpy as np
import pytest

import nms_ref as nr
from oracle import oracle as orc
from sfd2_amd import _lib

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------ cases (CPU side)
# tile 24 x 88: one tile, one row / column more, one less / exactly / one more than two tiles, a two-column last tile
SMALL_TILE_SHAPES = [(h, w) for h in (24, 25, 47, 48, 49, 73) for w in (88, 89, 175, 176, 177, 90)] + [(200, 300)]
# launch_nms4_select takes the 96-row tile when that leaves the busiest CU fewer region rows: more than 512 small tiles
# and at most 256 big ones, which tall narrow maps reach at ~0.5 Mpx.  (nr.nms4_tile restates the rule; the host test
# asserts it for these lists.)  H = 12384 = 129 * 96 with W = 88 is the map of whole tiles only: at W = 88 the launcher
# keeps the small tile up to H = 12288, so (6240, 88) -- also whole tiles, 65 * 96 -- runs as a tall small-tile map.
BIG_TILE_SHAPES = [(6145, 90), (12384, 88), (6241, 177), (6147, 89)]
TALL_SMALL_TILE_SHAPES = [(6240, 88)]
SEAM_KINDS = ("seam_zero", "seam_noisy", "corner_zero", "corner_noisy")
BIG_TILE_KINDS = SEAM_KINDS + ("rampnoise", "plateau", "const", "sparse", "rand", "sparse_plateau")
GENERIC_SHAPES = [(70, 140), (120, 160)]        # generic-radius kernel: tile 32 x 64
TIE_MAPS = [("const", 64, 64), ("const", 136, 136), ("plateau", 64, 64), ("plateau", 200, 333)]
CONF_TH, BORDER = 0.001, 4


@functools.lru_cache(maxsize=None)
def seams(h, w, tile_h, tile_w, radius, corners_first=False):
    zero, noisy, anchors = nr.seam_chains(h, w, tile_h, tile_w, radius, corners_first=corners_first)
    zero.setflags(write=False)
    noisy.setflags(write=False)
    return zero, noisy, anchors


@functools.lru_cache(maxsize=None)
def reference(kind, h, w, radius=4, conf_th=CONF_TH):
    """(map, oracle NMS, oracle key points, scores) with every candidate selected; computed once, read-only."""
    if kind in SEAM_KINDS:   # chains across the seams of the tiling this map runs with: seam sides first, or crossings first
        tile = (32, 64) if radius < 4 else ((96, 88) if nr.nms4_tile(h, w) == "big" else (24, 88))
        m = seams(h, w, tile[0], tile[1], radius, kind.startswith("corner"))[0 if kind.endswith("zero") else 1]
    else:
        m = nr.family(kind, h, w)
    want = orc.simple_nms(m, radius)
    kp, sc, _ = orc.select_keypoints(want, conf_th, BORDER, -1)
    for a in (want, kp, sc):
        a.setflags(write=False)
    return m, want, kp, sc


def bin_edge_ks(sc, n_bins=5):
    """top_k values that put the cut on the lower edge of an occupied histogram bin, one above and one below it, for
    n_bins occupied bins spread over the (descending) scores: need == bin count, need == 1, need == bin count - 1."""
    bins = nr.key_bin(sc)
    occupied = np.unique(bins)[::-1]
    pick = occupied[np.linspace(1, len(occupied) - 2, n_bins).astype(int)]
    ks = []
    for b in pick:
        cum = int((bins >= b).sum())
        ks += [cum - 1, cum, cum + 1]
    return ks


def clamp_ks(sc):
    """top_k values with the cut inside bin 4095 (scores >= 16), on its edge, between the clamped bins, on the edge of
    bin 0 (scores < 2^-12) and inside it."""
    bins = nr.key_bin(sc)
    n, top, low = len(sc), int((bins == nr.HIST_BINS - 1).sum()), int((bins == 0).sum())
    assert top >= 4 and low >= 4 and n - top - low >= 4, (n, top, low)
    return [1, top // 2, top - 1, top, top + 1, (top + n - low) // 2, n - low - 1, n - low, n - low + 1, n - low // 2, n - 1]


# ------------------------------------------------------------------------------------------ GPU side
def _gpu_ok():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def ctx():
    if not _gpu_ok():
        pytest.fail("no MI355X visible: GPU tests cannot run (there is no CPU fallback)")
    c = _lib.Context(0)
    yield c
    c.close()


def _nms(ctx, m, radius=4):
    m = np.ascontiguousarray(m, dtype=np.float32)
    out = np.empty_like(m)
    _lib.check(ctx.lib.sfd2_simple_nms(ctx.h, m.ctypes.data, m.shape[0], m.shape[1], radius, out.ctypes.data))
    return out


def _select(ctx, m, top_k, radius=4, conf_th=CONF_TH, border=BORDER, cap_out=None):
    m = np.ascontiguousarray(m, dtype=np.float32)
    cap = m.size if cap_out is None else cap_out
    kp = np.empty((max(cap, 1), 2), dtype=np.float32)
    sc = np.empty((max(cap, 1),), dtype=np.float32)
    n = ctypes.c_int(-1)
    _lib.check(ctx.lib.sfd2_select_keypoints(ctx.h, m.ctypes.data, m.shape[0], m.shape[1], conf_th, radius, border, top_k,
                                             kp.ctypes.data, sc.ctypes.data, cap, ctypes.byref(n)))
    return kp[:n.value], sc[:n.value]


def _check_selection(ctx, m, kp_all, sc_all, top_k, radius=4, conf_th=CONF_TH):
    """The oracle's selection is the first top_k rows of its full ordering.  More candidates than the capacity is the
    documented error of the call, not a result."""
    if len(sc_all) > nr.capacity(m.size):
        with pytest.raises(RuntimeError, match="candidate buffer overflow"):
            _select(ctx, m, top_k, radius, conf_th)
        return
    k = len(sc_all) if top_k <= 0 else min(top_k, len(sc_all))
    kp, sc = _select(ctx, m, top_k, radius, conf_th)
    np.testing.assert_array_equal(sc, sc_all[:k])
    np.testing.assert_array_equal(kp, kp_all[:k])


def _check_map(ctx, kind, h, w, top_ks, radius=4):
    m, want, kp_all, sc_all = reference(kind, h, w, radius)
    np.testing.assert_array_equal(_nms(ctx, m, radius), want)
    for top_k in top_ks:
        _check_selection(ctx, m, kp_all, sc_all, top_k, radius)


# ------------------------------------------------------------------------------------------ seams
@pytest.mark.parametrize("h", sorted({s[0] for s in SMALL_TILE_SHAPES}))
def test_small_tile_seams(ctx, h):
    """nms4_select_kernel<64>: chains that cross every seam of the 24 x 88 tiling on a zero and on a noisy background, and two
    dense families with near-ties everywhere; dense NMS and the selection of all / the best 64."""
    for hh, w in SMALL_TILE_SHAPES:
        if hh != h:
            continue
        assert nr.nms4_tile(h, w) == "small"
        for kind in SEAM_KINDS + ("rampnoise", "quant"):
            _check_map(ctx, kind, h, w, (-1, 64))


@pytest.mark.parametrize("kind", BIG_TILE_KINDS)
@pytest.mark.parametrize("h,w", BIG_TILE_SHAPES + TALL_SMALL_TILE_SHAPES)
def test_big_tile(ctx, h, w, kind):
    """nms4_select_kernel<136> on the maps the launcher itself sends there (tall and narrow): seam chains of the 96 x 88
    tiling, plateaus, a constant map, sparse maps, W % 4 != 0.  The plateau and const maps have more candidates than the
    capacity at these sizes: their selection must report the overflow (their dense NMS is compared like the others;
    with top_k = 4096 the boundary ranker still ranks a capacity-sized bin before the error is read: up to 4 s at 1.1 Mpx);
    sparse_plateau is the family with equal scores that fits."""
    assert nr.nms4_tile(h, w) == ("big" if (h, w) in BIG_TILE_SHAPES else "small")
    _check_map(ctx, kind, h, w, (-1, 4096))


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
@pytest.mark.parametrize("h,w", GENERIC_SHAPES)
def test_generic_radius_nms_and_selection(ctx, h, w, radius):
    """nms_select_kernel (tile 32 x 64, halo 5 * radius) with hist_from_cand_kernel and select_threshold_kernel<false>
    behind it: seam chains at pitch = radius (radius 0 has no neighbourhood: rand only) and rand."""
    kinds = ("rand",) if radius == 0 else SEAM_KINDS + ("rand",)
    for kind in kinds:
        _check_map(ctx, kind, h, w, (-1, 1, 100, 5000), radius)


# ------------------------------------------------------------------------------------------ ties, bin edges, clamped bins
@pytest.mark.parametrize("kind,h,w", TIE_MAPS)
def test_ties_at_the_cut(ctx, kind, h, w):
    """Equal scores on both sides of the cut: the boundary ranker must keep the lowest pixel indices (the oracle's
    comparator).  const puts 3 136 / 16 384 keys into one bin: the ranker's multi-tile loop."""
    m, want, kp_all, sc_all = reference(kind, h, w)
    n = len(sc_all)
    if kind == "const":
        assert n == (h - 2 * BORDER) * (w - 2 * BORDER) and np.bincount(nr.key_bin(sc_all)).max() == n
    assert np.bincount(nr.key_bin(sc_all)).max() > 256
    for top_k in (1, 2, 63, 64, 65, 255, 256, 257, 1000, n - 1, n, n + 1):
        _check_selection(ctx, m, kp_all, sc_all, top_k)


def test_top_k_sweep(ctx):
    m, want, kp_all, sc_all = reference("rand", 480, 640)
    n = len(sc_all)
    assert n > 4097
    ks = [1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, n - 1, n, n + 1] + bin_edge_ks(sc_all)
    for top_k in ks:
        _check_selection(ctx, m, kp_all, sc_all, top_k)


def test_cut_in_the_clamped_bins(ctx):
    """Scores below 2^-12 share bin 0 and scores from 16 up share bin 4095; a cut inside either ranks a bin that spans
    octaves."""
    m, want, kp_all, sc_all = reference("wide", 97, 131, conf_th=0.0)
    np.testing.assert_array_equal(_nms(ctx, m), want)
    for top_k in clamp_ks(sc_all):
        _check_selection(ctx, m, kp_all, sc_all, top_k, conf_th=0.0)


# ------------------------------------------------------------------------------------------ capacity
def test_candidates_equal_to_the_capacity(ctx):
    """const 264 x 264 with border 4: 256 * 256 = 65 536 candidates = min(max(65 536, P / 8), P).  All of them come back
    in index order; with top_k = 4096 one block ranks a boundary bin of 65 536 keys (time printed: CHANGELOG)."""
    m, want, kp_all, sc_all = reference("const", 264, 264)
    assert len(sc_all) == 65536 == nr.capacity(m.size)
    _check_selection(ctx, m, kp_all, sc_all, -1)
    _select(ctx, m, 4096)                                   # first call of this size: allocations
    t0 = time.perf_counter()
    kp, sc = _select(ctx, m, 4096)
    dt = time.perf_counter() - t0
    print(f"top_k 4096 of a 65 536-key boundary bin: {dt * 1e3:.1f} ms (upload, NMS, selection, download)")
    np.testing.assert_array_equal(sc, sc_all[:4096])
    np.testing.assert_array_equal(kp, kp_all[:4096])


def test_one_past_the_capacity_is_an_error_and_leaves_the_context_usable(ctx):
    m, want, kp_all, sc_all = reference("const", 265, 265)
    assert len(sc_all) == 257 * 257 and nr.capacity(m.size) == 65536
    for top_k in (-1, 4096):
        with pytest.raises(RuntimeError, match="candidate buffer overflow"):
            _select(ctx, m, top_k)
        m2, _, kp2, sc2 = reference("rand", 200, 333)
        _check_selection(ctx, m2, kp2, sc2, top_k)


@pytest.mark.parametrize("cap_out", [1, 100])
def test_cap_out_below_the_number_selected(ctx, cap_out):
    m, want, kp_all, sc_all = reference("rand", 200, 333)
    assert len(sc_all) > 100
    for top_k in (-1, 4096, 150):
        kp, sc = _select(ctx, m, top_k, cap_out=cap_out)
        np.testing.assert_array_equal(sc, sc_all[:cap_out])
        np.testing.assert_array_equal(kp, kp_all[:cap_out])


# ------------------------------------------------------------------------------------------ context state
def test_back_to_back_calls_on_one_context(ctx):
    """Counters, the histogram and the two ticket words are reused from call to call: a big-tile call, a small-tile call
    and a radius-2 call (unfused threshold search) in turn, each equal to the same call on a fresh context."""
    calls = [("rand", 6145, 90, 4, 4096), ("rampnoise", 73, 177, 4, 64), ("rand", 70, 140, 2, 100),
             ("sparse_plateau", 6241, 177, 4, -1), ("quant", 49, 90, 4, -1), ("seam_noisy", 120, 160, 2, 5000)]
    fresh = []
    for kind, h, w, radius, top_k in calls:
        m = reference(kind, h, w, radius)[0]
        c = _lib.Context(0)
        try:
            fresh.append((_nms(c, m, radius),) + _select(c, m, top_k, radius))
        finally:
            c.close()
    for rnd in range(2):
        for (kind, h, w, radius, top_k), (nms_f, kp_f, sc_f) in zip(calls, fresh):
            m, want, kp_all, sc_all = reference(kind, h, w, radius)
            kp, sc = _select(ctx, m, top_k, radius)
            np.testing.assert_array_equal(sc, sc_f)
            np.testing.assert_array_equal(kp, kp_f)
            if rnd:
                np.testing.assert_array_equal(_nms(ctx, m, radius), nms_f)
            k = len(sc_all) if top_k <= 0 else min(top_k, len(sc_all))
            np.testing.assert_array_equal(sc_f, sc_all[:k])
            np.testing.assert_array_equal(kp_f, kp_all[:k])


# ------------------------------------------------------------------------------------------ arguments
@pytest.mark.parametrize("conf_th", [-1.0, -1e-30, float("nan")])
def test_negative_or_nan_conf_th_is_rejected(ctx, conf_th):
    """Keys are raw float bits: a negative score would sort above every positive one, so the threshold must keep them
    out.  The next call with a valid threshold works."""
    m, want, kp_all, sc_all = reference("rand", 200, 333)
    with pytest.raises(RuntimeError, match="conf_th"):
        _select(ctx, m, 64, conf_th=conf_th)
    _check_selection(ctx, m, kp_all, sc_all, 64)
    kp, sc = _select(ctx, m, -1, conf_th=0.0)               # zero stays valid (the extract-spp path passes it)
    kp0, sc0, _ = orc.select_keypoints(want, 0.0, BORDER, -1)
    np.testing.assert_array_equal(sc, sc0)
    np.testing.assert_array_equal(kp, kp0)
