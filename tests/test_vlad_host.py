"""The VLAD global descriptors, the parts that need no GPU: the caps on the banded share that tests/test_gpu_vlad.py relies on (with the
restatement tests/vlad_ref.py alone), what the generators of tests/test_gpu_vlad_edges.py claim, the retrieval scene's property, the command line, the vocabulary file, the header against the
binding, and the compiled kernels' metadata."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import vlad_ref as vr
from sfd2_amd import _lib, build, global_features, vlad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_family_has_exact_chains_and_its_designed_ties():
    for n, k in ((257, 1), (257, 2), (300, 17), (1000, 64), (257, 256)):
        x, c = vr.exact_family(11, n, k)
        assert vr.chains_exact(x, c)                                   # the rounding bound is 0: no banded row
        s = np.sort(vr.scores64(x, c), axis=1)
        a32, s32 = vr.assign32(x, c)
        np.testing.assert_array_equal(s32.astype(np.float64), s[:, -1])   # the restated fp32 chain gives the exact score's bits
        np.testing.assert_array_equal(a32, np.argmax(vr.scores64(x, c), axis=1))
        if k >= 2:
            ties = int((s[:, -1] == s[:, -2]).sum())
            print(f"exact n = {n} K = {k}: rows whose two best scores are equal {ties}")
            assert ties >= (n if k == 2 else n // 5)                   # every row of k = 2; the rows 0, 5, 10, .. otherwise
    x, o, c = vr.aggregate_case(13, 17, "exact")
    assert vr.chains_exact(x, c)


def test_float_family_banded_share_is_capped():
    worst = 0.0
    for n, k in ((1000, 2), (1000, 17), (1000, 64), (1000, 100), (1000, 256)):
        x, c = vr.float_family(12, n, k)
        share = float(vr.banded(x, c).mean())
        worst = max(worst, share)
        assert share <= 0.01, (n, k, share)
    for k in vr.AGG_KS:
        x, o, c = vr.aggregate_case(13, k)
        share = float(vr.banded(x, c).mean())
        worst = max(worst, share)
        assert share <= 0.01, (k, share)
        if k >= 3:
            assert not (np.argmax(vr.scores64(x, c), axis=1) == k - 2).any()       # the centroid no row chooses
    print(f"largest banded share of a float case: {worst:.5f}")


@functools.lru_cache(maxsize=None)
def _separated(i):
    seed, n, k = vr.KMEANS_SEPARATED[i]
    x, start = vr.separated(seed, n, k)
    return x, start, vr.kmeans_ref(x, start, 20)


@pytest.mark.parametrize("i", range(len(vr.KMEANS_SEPARATED)))
def test_separated_kmeans_has_no_banded_row_and_converges(i):
    x, start, its = _separated(i)
    assert its[-1][2] == 0 and 2 <= len(its) < 20                      # stops on moved == 0 before max_iters
    assert its[0][2] == len(x)
    c = start
    for cen, counts, moved, a in its:
        assert not vr.banded(x, c).any()
        np.testing.assert_array_equal(a, np.argmax(vr.scores64(x, c), axis=1))
        assert counts.sum() == len(x)
        c = cen
    print(f"separated case {i}: moved per iteration {[it[2] for it in its]}")


def test_duplicated_start_row_keeps_its_value():
    seed, n, k = vr.KMEANS_SEPARATED[0]
    x, start = vr.separated(seed, n, k)
    start[5] = start[2]
    its = vr.kmeans_ref(x, start, 1)                                   # the tie rule gives every row of the two to centroid 2
    assert its[-1][1][5] == 0 and (its[-1][0][5] == start[5]).all() and its[-1][1][2] > 0
    # (over further iterations the start row itself, which IS centroid 5, scores 0.5 against it and less against its cluster's mean: it returns)
    its = vr.kmeans_ref(x, start, 20)
    assert its[-1][2] == 0 and len(its) < 20 and its[-1][1][5] <= 1


# ------------------------------------------------------------------------------------ the generators of tests/test_gpu_vlad_edges.py
def _exact_bits(x, c):
    """The fp64 scores of a case whose chains are exact: they ARE the fp32 scores."""
    assert vr.chains_exact(x, c)
    s = vr.scores64(x, c)
    assert (s.astype(np.float32).astype(np.float64) == s).all()
    return s


@pytest.mark.parametrize("k", vr.EDGE_KS)
def test_edge_k_cases_cover_every_centroid_and_stay_under_the_band_cap(k):
    n = max(vr.EDGE_NS)
    x, c = vr.covering_family("exact", 20 + k, n, k)
    s = _exact_bits(x, c)
    assert sorted(set(np.argmax(s, axis=1).tolist())) == list(range(k))            # every column of every accumulator tile wins a row
    np.testing.assert_array_equal(np.argmax(s, axis=1)[:k], np.arange(k))
    x, c = vr.exact_family(20 + k, n, k)
    s = _exact_bits(x, c)
    assert (np.argmax(s, axis=1)[::5] == 0).all() and (s[::5, 0] == s[::5, 1]).all()
    x, c = vr.covering_family("float", 20 + k, n, k)
    share_cover = float(vr.banded(x, c).mean())
    assert sorted(set(np.argmax(vr.scores64(x, c), axis=1)[~vr.banded(x, c)].tolist())) == list(range(k))
    x, c = vr.float_family(20 + k, 1000, k)
    share = float(vr.banded(x, c).mean())
    print(f"K = {k}: banded share of the covering float case {share_cover:.5f}, of the float case at n = 1000 {share:.5f}")
    assert share_cover <= 0.01 and share <= 0.01


@pytest.mark.parametrize("k", vr.LANE_TIE_KS)
def test_lane_tie_family_ties_inside_a_lane(k):
    n = 257
    x, c, rows, want = vr.lane_tie_family(30 + k, n, k)
    s = _exact_bits(x, c)
    lanes = vr.lane_tie_lanes(k)
    assert 15 in lanes and len(set(lanes)) == 2 and len(rows) >= 2 * (n // 8)
    for lc in lanes:
        group = list(range(lc, k, 16))
        assert len(group) >= 2 and all((c[j] == c[lc]).all() for j in group)
        r = rows[want == lc]
        assert len(r) >= n // 8
        assert (s[r][:, group] == s[r][:, [lc]]).all() and (s[r].max(1) == s[r, lc]).all()      # the whole lane ties at the row's best score
    np.testing.assert_array_equal(np.argmax(s, axis=1)[rows], want)
    print(f"lane ties K = {k}: lanes {lanes}, {len(rows)} designed rows of {n}")


def test_all_equal_families_tie_as_many_ways_as_stated():
    for k in (16, 17, 256):
        x, c, want = vr.all_equal_family(257, k)
        s = _exact_bits(x, c)
        assert (s == s[:, :1]).all() and (want == 0).all() and (np.argmax(s, axis=1) == 0).all()
    x, c, want = vr.all_equal_family(257, 96, group=16)
    s = _exact_bits(x, c)
    np.testing.assert_array_equal(np.argmax(s, axis=1), want)
    assert sorted(set(want.tolist())) == [0, 16, 32, 48, 64, 80]
    for i in range(len(x)):
        assert (s[i, want[i]:want[i] + 16] == s[i].max()).all() and int((s[i] == s[i].max()).sum()) == 16


def test_negative_family_scores_below_zero():
    lo, hi = 0.0, -np.inf
    for k in sorted(set(vr.NEGATIVE_KS) | {35, 48, 49, 65, 96, 97, 129, 192}):
        x, c = vr.negative_family(40 + k, 257, k)
        s = _exact_bits(x, c)
        assert (s < 0).all()
        lo, hi = min(lo, float(s.max(1).min())), max(hi, float(s.max(1).max()))
    print(f"negative family: the largest score of a row lies in [{lo:.3f}, {hi:.3f}]")
    assert hi < -3.5                                                  # far below the 0 a zero centroid row scores


@functools.lru_cache(maxsize=None)
def _large():
    x, c = vr.exact_family(50, max(vr.LARGE_NS), 17)
    return x, c


def test_large_cases_have_exact_chains():
    x, c = _large()
    s = _exact_bits(x, c)
    assert (np.argmax(s, axis=1)[::5] == 0).all() and (s[::5, 0] == s[::5, 1]).all()
    for n in vr.LARGE_NS:
        tiles = (n + 63) // 64
        assert tiles > 1024 and n - 64 * (tiles - 1) == 1             # a block takes a further tile, and the last tile has one live row
    x, c, rows, want = vr.lane_tie_family(51, vr.LARGE_NS[0], 35)
    s = _exact_bits(x, c)
    np.testing.assert_array_equal(np.argmax(s, axis=1)[rows], want)
    assert len(rows) >= 2 * (len(x) // 8) and (rows >= 65536).any()


def _check_kmeans_case(x, start, its):
    assert its[-1][2] == 0 and 2 <= len(its) < 20 and its[0][2] == len(x)
    c = start
    for cen, counts, moved, a in its:
        assert not vr.banded(x, c).any()
        np.testing.assert_array_equal(a, np.argmax(vr.scores64(x, c), axis=1))
        assert counts.sum() == len(x)
        c = cen


def test_large_kmeans_case_has_no_banded_row_and_converges():
    seed, n, k = vr.KMEANS_LARGE
    x, start = vr.separated(seed, n, k)
    its = vr.kmeans_ref(x, start, 20)
    _check_kmeans_case(x, start, its)
    moved = [it[2] for it in its]
    print(f"large k-means case: moved per iteration {moved}")
    assert len(its) >= 3 and 0 < moved[1] < n                         # the second iteration's count is a partial one
    assert (n + vr.CHUNK - 1) // vr.CHUNK == 17


@pytest.mark.parametrize("i", range(len(vr.KMEANS_WIDE)))
def test_wide_kmeans_cases_have_no_banded_row_and_converge(i):
    seed, n, k, empty = vr.KMEANS_WIDE[i]
    x, start, _ = vr.kmeans_wide_case(i)
    its = vr.kmeans_ref(x, start, 20)
    _check_kmeans_case(x, start, its)
    print(f"wide k-means case K = {k}, n = {n}: moved per iteration {[it[2] for it in its]}")
    assert n > vr.CHUNK
    if k == 1:
        assert [it[2] for it in its] == [n, 0]
    if empty is None:
        assert (its[0][1] > 0).all()                                  # every cluster has rows
    else:
        assert n > 2 * vr.CHUNK
        for cen, counts, moved, a in its:
            assert counts[empty] == 0 and cen[empty].tobytes() == start[empty].tobytes()
        assert (np.delete(its[-1][1], empty) > 0).all()


@pytest.mark.parametrize("k", vr.AGG_SEAM_KS)
def test_aggregate_seam_cases_change_centroid_on_the_tile_seam(k):
    for family in ("exact", "float"):
        x, o, c, a, b = vr.aggregate_seam_case(60 + k, k, family)
        if family == "exact":
            _exact_bits(x, c)
        share = float(vr.banded(x, c).mean()) if family == "float" else 0.0
        assert share <= 0.01
        want = np.argmax(vr.scores64(x, c), axis=1)
        assert o.tolist() == [0, 31, 95, 128, 128, 193, 194] and a == k - 1 and (a & 1) != (b & 1)
        assert (want[31:63] == a).all() and (want[63:95] == b).all()


@functools.lru_cache(maxsize=None)
def _scene():
    scene = vr.make_scene()
    centroids, iters = vr.scene_vocabulary(scene)
    db, q = vr.scene_descriptors(scene, centroids)
    return scene, centroids, iters, db, q


def test_scene_restatement_retrieves_the_most_overlapping_image():
    scene, centroids, iters, db, q = _scene()
    sim = q.astype(np.float64) @ db.astype(np.float64).T
    top = np.argsort(-sim, axis=1, kind="stable")[:, :vr.SCENE_TOP]
    best = vr.most_overlapping(scene)
    hits = [best[i] in top[i] for i in range(len(best))]
    print(f"scene: k-means iterations {iters}, queries whose most-overlapping image is in the top {vr.SCENE_TOP}: {sum(hits)} of {len(hits)}")
    assert all(hits)
    assert np.isfinite(db).all() and np.allclose((db.astype(np.float64) ** 2).sum(1), 1.0, atol=1e-5)


def test_normalisations_of_the_restatement():
    v = np.zeros((3, vr.DIM), dtype=np.float32)
    v[0, :4] = (3, -4, 0, 0)
    v[2, 7] = -2
    w = vr.normalise64(v, "intra").reshape(3, vr.DIM)
    np.testing.assert_allclose(w[0, :2], np.array([0.6, -0.8]) / np.sqrt(2))
    assert (w[1] == 0).all() and w[2, 7] == -1 / np.sqrt(2)
    w = vr.normalise64(v, "ssr").reshape(3, vr.DIM)
    np.testing.assert_allclose(w[0, :2] / w[2, 7], np.array([np.sqrt(3), -2]) / -np.sqrt(2))
    np.testing.assert_allclose(vr.normalise64(v, "none").reshape(3, vr.DIM)[0, :2], np.array([3, -4]) / np.sqrt(29))
    for norm in ("intra", "ssr", "none"):
        assert (vr.normalise64(np.zeros((2, vr.DIM), np.float32), norm) == 0).all()    # never NaN
    assert vr.within_one_ulp(np.float32(0.1), 0.1) and not vr.within_one_ulp(np.float32(0.1) + 2 * np.spacing(np.float32(0.1)), 0.1)
    assert not vr.within_one_ulp(np.float32(1e-30), 0.0)


def test_command_line_lists_the_options():
    out = subprocess.run([sys.executable, "-m", "sfd2_amd.global_features", "--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    for opt in ("--features", "--output", "--vocabulary", "--train", "--train_prefix", "--train_list", "--prefix", "--image_list", "--k",
                "--max_iters", "--max_train", "--seed", "--norm"):
        assert opt in out, opt
    a = global_features.make_parser().parse_args(["--features", "f.h5", "--output", "g.h5", "--vocabulary", "v.npz"])
    assert (a.train, a.k, a.max_iters, a.max_train, a.seed, a.norm) == (False, 64, 20, 1 << 20, 0, "intra")
    import inspect
    assert list(inspect.signature(global_features.main).parameters) == [
        "features", "output", "vocabulary", "train", "train_prefix", "train_list", "prefix", "image_list", "k", "max_iters", "max_train", "seed", "norm"]
    assert set(vars(a)) == set(inspect.signature(global_features.main).parameters)
    assert "256 MiB" in global_features.__doc__ and global_features.BATCH_BYTES == 256 << 20


def test_vocabulary_round_trips(tmp_path):
    c = np.random.RandomState(0).standard_normal((17, vlad.DIM)).astype(np.float32)
    p = tmp_path / "voc.npz"
    vlad.save_vocabulary(p, c, norm="ssr", seed=7, iters_run=12)
    with np.load(p) as z:
        assert sorted(z.files) == ["centroids", "iters_run", "k", "norm", "seed"]
    v = vlad.load_vocabulary(p)
    assert v["centroids"].tobytes() == c.tobytes() and (v["k"], v["norm"], v["seed"], v["iters_run"]) == (17, "ssr", 7, 12)
    with pytest.raises(ValueError):
        vlad.save_vocabulary(p, c[:, :7])
    with pytest.raises(ValueError):
        vlad.save_vocabulary(p, c, norm="l3")


def test_array_checks_need_no_gpu():
    with pytest.raises(ValueError):
        vlad.assign(np.zeros((4, 64), np.float32), np.zeros((2, vlad.DIM), np.float32))
    with pytest.raises(ValueError):
        vlad.aggregate(np.zeros((4, vlad.DIM), np.float32), [0, 3], np.zeros((2, vlad.DIM), np.float32))
    with pytest.raises(ValueError):
        vlad.aggregate(np.zeros((4, vlad.DIM), np.float32), [0, 4], np.zeros((2, vlad.DIM), np.float32), norm="l3")
    with pytest.raises(ValueError):
        vlad.kmeans(np.zeros((4, vlad.DIM), np.float32), 5)
    with pytest.raises(ValueError):
        vlad.kmeans(np.zeros((400, vlad.DIM), np.float32), vlad.MAX_K + 1)


def test_header_and_binding_agree_on_vlad():
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1))  # noqa: E731
    for name in ("sfd2_vlad_assign", "sfd2_vlad_aggregate", "sfd2_vlad_kmeans"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in _lib.EXPORTS
    assert val("SFD2_VLAD_DIM") == _lib.VLAD_DIM == vlad.DIM == vr.DIM == 128
    assert val("SFD2_VLAD_MAX_K") == _lib.VLAD_MAX_K == vlad.MAX_K == 256
    assert val("SFD2_VLAD_CHUNK") == _lib.VLAD_CHUNK == vlad.CHUNK == vr.CHUNK == 4096
    assert (val("SFD2_VLAD_NORM_INTRA"), val("SFD2_VLAD_NORM_SSR"), val("SFD2_VLAD_NORM_NONE")) == (0, 1, 2)
    assert vlad.NORMS == {"intra": 0, "ssr": 1, "none": 2}
    assert "vlad_kernels.hip" in build.SOURCES and "api_vlad.hip" in build.SOURCES
    assert ctypes.sizeof(ctypes.c_int64) == 8


def test_vlad_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "vlad.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "vlad_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*vlad_\S*_kernel\S*)", meta)
    assert len(kernels) == 3 + 8                                    # half norms, aggregate, update; the assignment at 8 accumulator counts
    assert sum("vlad_assign_kernel" in k for k in kernels) == 8
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta) == ["0"] * len(kernels)
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta) == ["0"] * len(kernels)
    assert re.findall(r"\.sgpr_spill_count:\s+(\d+)", meta) == ["0"] * len(kernels)
    assert re.findall(r"\.wavefront_size:\s+(\d+)", meta) == ["64"] * len(kernels)
    assert re.findall(r"\.group_segment_fixed_size:\s+(\d+)", meta) == ["0"] * len(kernels)      # all LDS is dynamic: sized by k at the launch
    assert len(re.findall(r"v_mfma_f32_16x16x4_f32", meta)) >= 8 * 8        # the assignment runs on the f32-input MFMA
