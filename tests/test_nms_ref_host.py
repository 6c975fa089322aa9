"""tests/nms_ref.py checked on its own, without a GPU and without the library, and the conditions under which the inputs of
tests/test_gpu_selection_edges.py can fail at all: a tiling of the oracle with the full 5 * radius halo reproduces the
untiled result, one pixel less changes the sixth point of EVERY seam chain; const / plateau maps put more than 256 keys
into one histogram bin; the shape lists reach the nms4 tile they are named after."""
import numpy as np
import pytest

import nms_ref as nr
import test_gpu_selection_edges as cases
from oracle import oracle as orc


def test_chain_sixth_point_depends_on_the_first():
    for r in (1, 2, 3, 4):
        for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):
            m = np.zeros((60, 60), dtype=np.float32)
            pts = nr.chain(m, 30 - 10 * dy, 30 - 10 * dx, dy, dx, r)
            assert np.all(np.diff([m[p] for p in pts]) < 0)
            assert max(abs(pts[5][0] - pts[0][0]), abs(pts[5][1] - pts[0][1])) == 5 * r
            full = orc.simple_nms(m, r)
            assert [full[p] > 0 for p in pts] == [True, False, True, False, True, False]
            m[pts[0]] = 0
            cut = orc.simple_nms(m, r)
            assert [cut[p] > 0 for p in pts] == [False, True, False, True, False, True]


def _seam_condition(h, w, tile_h, tile_w, radius):
    return _layout_condition(h, w, tile_h, tile_w, radius, False) + _layout_condition(h, w, tile_h, tile_w, radius, True)


def _layout_condition(h, w, tile_h, tile_w, radius, corners_first):
    zero, noisy, anchors = cases.seams(h, w, tile_h, tile_w, radius, corners_first)
    sixth = {a["sixth"] for a in anchors}
    groups = {c[0] for c in nr._seam_candidates(h, w, tile_h, tile_w, 5 * radius)}
    placed = {a["group"] for a in anchors}
    if corners_first:    # a diagonal chain wherever the map has a crossing with room for one
        assert any(g[0] == "c" for g in placed) == any(g[0] == "c" for g in groups)
    else:                # every seam side on which a chain fits has one
        sides = {g for g in groups if g[0] != "c"}
        assert sides and sides <= placed
    pts = np.argwhere(zero > 0)
    assert len(pts) == 6 * len(anchors)
    for a in anchors:
        (y0, x0), (y5, x5) = a["first"], a["sixth"]
        assert max(abs(y5 - y0), abs(x5 - x0)) == 5 * radius
        assert y5 % tile_h in (0, tile_h - 1) or x5 % tile_w in (0, tile_w - 1)
        lo_y, hi_y, lo_x, hi_x = min(y0, y5), max(y0, y5), min(x0, x5), max(x0, x5)
        near = pts[(pts[:, 0] >= lo_y - 5 * radius - 4) & (pts[:, 0] <= hi_y + 5 * radius + 4) &
                   (pts[:, 1] >= lo_x - 5 * radius - 4) & (pts[:, 1] <= hi_x + 5 * radius + 4)]
        assert len(near) == 6, a
    assert noisy[zero == 0].max() < 0.05 and np.array_equal(noisy[zero > 0], zero[zero > 0])
    for name, m in (("zero", zero), ("noisy", noisy)):
        full = orc.simple_nms(m, radius)
        np.testing.assert_array_equal(nr.tiled_nms(m, tile_h, tile_w, 5 * radius, radius), full)
        short = nr.tiled_nms(m, tile_h, tile_w, 5 * radius - 1, radius)
        diff = {tuple(p) for p in np.argwhere(short != full)}
        assert sixth <= diff, (name, sorted(sixth - diff))
        if name == "zero":
            assert diff == sixth     # exactly one pixel per chain
    return len(anchors)


@pytest.mark.parametrize("h,w,tile_h,tile_w", [(200, 300, 24, 88), (300, 200, 96, 88), (73, 177, 24, 88), (25, 89, 24, 88)])
def test_seam_chains_need_the_full_halo_radius_4(h, w, tile_h, tile_w):
    n = _seam_condition(h, w, tile_h, tile_w, 4)
    assert n >= {(200, 300): 30, (300, 200): 20, (73, 177): 6, (25, 89): 2}[(h, w)]


def test_seam_chains_need_the_full_halo_big_tile_shape():
    h, w = cases.BIG_TILE_SHAPES[2]
    assert _seam_condition(h, w, 96, 88, 4) >= 260     # 65 seams in y, two sides each, two seams in x


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("h,w", cases.GENERIC_SHAPES)
def test_seam_chains_need_the_full_halo_other_radii(h, w, radius):
    _seam_condition(h, w, 32, 64, radius)


def test_random_families_pass_with_a_short_halo():
    """What the seam chains are for: on every random family a 16-px halo already reproduces the radius-4 result on this
    map, so whether a kernel gets the last four halo pixels right is decided by the chains alone."""
    for kind in ("rand", "smooth", "plateau", "sparse", "rampnoise", "quant"):
        m = nr.family(kind, 200, 300)
        np.testing.assert_array_equal(nr.tiled_nms(m, 24, 88, 16, 4), orc.simple_nms(m, 4))


def test_key_bin():
    s = np.float32(2.0) ** np.arange(-30, 12, dtype=np.float32)
    dense = np.sort(np.concatenate([s, np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(np.inf)),
                                    np.random.RandomState(0).uniform(0, 20, 4000).astype(np.float32), [np.float32(0)]]))
    b = nr.key_bin(dense)
    assert (np.diff(b) >= 0).all() and b.min() == 0 and b.max() == 4095
    lo, hi = np.float32(2.0 ** -12), np.float32(16.0)
    assert nr.key_bin(lo) == 0 and nr.key_bin(np.nextafter(lo, np.float32(0))) == 0
    assert nr.key_bin(np.float32(2.0 ** -12 * (1 + 2.0 ** -8))) == 1          # one bin = 2^15 float32 values = 1/256 octave
    assert nr.key_bin(np.nextafter(hi, np.float32(0))) == 4095 and nr.key_bin(hi) == 4095 and nr.key_bin(np.float32(1e30)) == 4095
    assert nr.key_bin(np.float32(16.0 * (1 - 2.0 ** -8))) == 4094
    assert nr.key_bin(np.float32(1.0)) == 12 * 256 and nr.key_bin(np.float32(0.25)) == 10 * 256


@pytest.mark.parametrize("kind,h,w", cases.TIE_MAPS)
def test_tie_maps_fill_one_bin_beyond_a_ranker_tile(kind, h, w):
    m, want, kp, sc = cases.reference(kind, h, w)
    counts = np.bincount(nr.key_bin(sc), minlength=nr.HIST_BINS)
    assert counts.max() > 256
    assert len(sc) <= nr.capacity(h * w)
    if kind == "const":
        assert counts.max() == len(sc) == {64: 3136, 136: 16384}[h]
    # equal scores straddle every cut the test makes inside that bin, and the oracle orders them by index
    idx = kp[:, 1].astype(np.int64) * w + kp[:, 0].astype(np.int64)
    same = sc[1:] == sc[:-1]
    assert same.sum() > 256 and (np.diff(idx)[same] > 0).all() and (np.diff(sc) <= 0).all()


def test_sweep_and_clamp_cuts():
    m, want, kp, sc = cases.reference("rand", 480, 640)
    bins = nr.key_bin(sc)
    ks = cases.bin_edge_ks(sc)
    assert len(set(ks)) >= 13 and min(ks) >= 1 and max(ks) <= len(sc)
    edges = [k for k in ks if k < len(sc) and bins[k - 1] != bins[k]]          # the k-th best is the last of its bin
    assert len(edges) >= 5
    m, want, kp, sc = cases.reference("wide", 97, 131, conf_th=0.0)
    bins = nr.key_bin(sc)
    ks = cases.clamp_ks(sc)
    assert sc.min() < 2.0 ** -12 and sc.max() >= 16
    assert any(bins[k - 1] == 4095 and bins[k] == 4095 for k in ks)      # cut inside the top bin ...
    assert any(bins[k - 1] == 0 and bins[k] == 0 for k in ks)            # ... inside bin 0 ...
    assert any(0 < bins[k - 1] < 4095 and 0 < bins[k] < 4095 for k in ks)   # ... and in between


def test_capacity_cases():
    assert nr.capacity(264 * 264) == 65536 == len(cases.reference("const", 264, 264)[3])
    assert nr.capacity(265 * 265) == 65536 < len(cases.reference("const", 265, 265)[3]) == 66049
    assert nr.capacity(4096) == 4096 and nr.capacity(1600 * 1200) == 240000
    # big-tile maps: plateau and const exceed the capacity (their selection is the overflow error), the others fit
    h, w = cases.BIG_TILE_SHAPES[0]
    over = {k for k in cases.BIG_TILE_KINDS if len(cases.reference(k, h, w)[3]) > nr.capacity(h * w)}
    assert over == {"plateau", "const"}


def test_shape_lists_reach_their_tile():
    assert len(cases.BIG_TILE_SHAPES) >= 4 and len(cases.SMALL_TILE_SHAPES) == 37
    for h, w in cases.BIG_TILE_SHAPES:
        assert nr.nms4_tile(h, w) == "big", (h, w)
    for h, w in cases.SMALL_TILE_SHAPES + cases.TALL_SMALL_TILE_SHAPES:
        assert nr.nms4_tile(h, w) == "small", (h, w)
    assert {w % 4 for _, w in cases.BIG_TILE_SHAPES} == {0, 1, 2}          # the aligned and the scalar load path
    assert any(h % 96 == 0 and w % 88 == 0 for h, w in cases.BIG_TILE_SHAPES)
    # the flagship sizes, as the launcher's comment states them
    assert nr.nms4_tile(1200, 1600) == "big" and nr.nms4_tile(480, 640) == "small"
