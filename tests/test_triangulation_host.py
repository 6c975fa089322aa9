"""The SfM map, the parts that need no GPU: sfd2_amd.colmap_io against a model the reference's read_write_model.py wrote
(tests/golden/tri_model, tests/golden/gen_tri_goldens.py), no CPU fallback in sfd2_amd.triangulation, the numpy restatement of
tests/tri_ref.py against the scene's ground truth (it is the yardstick of tests/test_gpu_triangulation.py), the designed inputs of
tests/test_gpu_triangulation_edges.py held to their band caps and class counts by the restatement alone, and the new kernels'
resource metadata and instruction vocabulary."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import tri_ref as tr
from sfd2_amd import build, colmap_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "golden", "tri_model")


def test_read_model_matches_expected_values():
    g = np.load(os.path.join(MODEL, "expected.npz"))
    cameras, images, points3D = colmap_io.read_model(MODEL)
    assert sorted(cameras) == list(g["cam/ids"])
    at = 0
    for k, cid in enumerate(g["cam/ids"]):
        c = cameras[int(cid)]
        n = int(g["cam/nparams"][k])
        assert (c.id, c.model, c.width, c.height) == (cid, str(g["cam/models"][k]), g["cam/wh"][k, 0], g["cam/wh"][k, 1])
        assert c.params.dtype == np.float64 and np.array_equal(c.params, g["cam/params"][at:at + n])
        assert c["model"] == c.model and c.get("width") == c.width       # the mapping sfd2_amd.pose takes
        at += n
    assert "RADIAL" in g["cam/models"]
    assert sorted(images) == list(g["img/ids"])
    for k, iid in enumerate(g["img/ids"]):
        im = images[int(iid)]
        lo, hi = g["img/offsets"][k], g["img/offsets"][k + 1]
        assert (im.id, im.camera_id, im.name) == (iid, g["img/camera_id"][k], str(g["img/names"][k]))
        assert np.array_equal(im.qvec, g["img/qvec"][k]) and np.array_equal(im.tvec, g["img/tvec"][k])
        assert im.xys.shape == (hi - lo, 2) and np.array_equal(im.xys, g["img/xys"][lo:hi])
        assert np.array_equal(im.point3D_ids, g["img/point3D_ids"][lo:hi])
    assert sorted(points3D) == list(g["pt/ids"]) and len(points3D) > 100
    for k, pid in enumerate(g["pt/ids"]):
        p = points3D[int(pid)]
        lo, hi = g["pt/offsets"][k], g["pt/offsets"][k + 1]
        assert p.id == pid and np.array_equal(p.xyz, g["pt/xyz"][k]) and np.array_equal(p.rgb, g["pt/rgb"][k]) and p.error == g["pt/error"][k]
        assert np.array_equal(p.image_ids, g["pt/image_ids"][lo:hi]) and np.array_equal(p.point2D_idxs, g["pt/point2D_idxs"][lo:hi])


def test_write_model_is_byte_exact(tmp_path):
    cameras, images, points3D = colmap_io.read_model(MODEL)
    colmap_io.write_model(cameras, images, points3D, tmp_path / "out")
    for f in ("cameras.bin", "images.bin", "points3D.bin"):
        assert (tmp_path / "out" / f).read_bytes() == open(os.path.join(MODEL, f), "rb").read(), f


def test_camera_goes_into_pose_unchanged():
    from sfd2_amd import pose
    cameras = colmap_io.read_cameras_binary(os.path.join(MODEL, "cameras.bin"))
    for c in cameras.values():
        if c.model == "RADIAL":
            with pytest.raises(ValueError, match="RADIAL"):
                pose.camera_model(c)
        else:
            mid, params = pose.camera_model(c)
            assert mid == colmap_io.CAMERA_MODEL_IDS[c.model][0] and np.array_equal(params[:len(c.params)], c.params)


def test_unknown_model_and_truncation_raise(tmp_path):
    raw = bytearray(open(os.path.join(MODEL, "cameras.bin"), "rb").read())
    raw[12:16] = (77).to_bytes(4, "little")                 # the first camera's model id
    bad = tmp_path / "cameras.bin"
    bad.write_bytes(bytes(raw))
    with pytest.raises(ValueError, match="unknown model id 77"):
        colmap_io.read_cameras_binary(bad)
    cameras = colmap_io.read_cameras_binary(os.path.join(MODEL, "cameras.bin"))
    first = next(iter(cameras.values()))
    with pytest.raises(ValueError, match="unknown model"):
        colmap_io.write_cameras_binary({1: colmap_io.Camera(1, "NO_SUCH_MODEL", 10, 10, [1.0])}, tmp_path / "c.bin")
    with pytest.raises(ValueError, match="takes"):
        colmap_io.write_cameras_binary({1: colmap_io.Camera(1, first.model, 10, 10, [1.0] * 11)}, tmp_path / "c.bin")
    for f, reader in (("cameras.bin", colmap_io.read_cameras_binary), ("images.bin", colmap_io.read_images_binary),
                      ("points3D.bin", colmap_io.read_points3D_binary)):
        data = open(os.path.join(MODEL, f), "rb").read()
        for cut in (4, len(data) // 2, len(data) - 3):
            p = tmp_path / ("cut_" + f)
            p.write_bytes(data[:cut])
            with pytest.raises(ValueError, match="truncated"):
                reader(p)
        p.write_bytes(data + b"\x00")
        with pytest.raises(ValueError, match="after the last record"):
            reader(p)


def test_triangulation_raises_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from sfd2_amd import triangulation as T
    sc = tr.make_scene(seed=1, n_images=4, n_points=60, n_clutter=10, n_joiners=0, n_weak_pairs=0)
    with pytest.raises(RuntimeError):
        T.verify_pairs(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"])
    with pytest.raises(RuntimeError):
        T.build_tracks(10, np.array([[0, 1], [1, 2]]))
    ids, views = T.make_views(sc["cameras"], sc["images"])
    with pytest.raises(RuntimeError):
        T.triangulate(views, len(ids), [0, 2], [0], [0, 1], np.zeros((2, 2), np.float32))
    with pytest.raises(RuntimeError):
        T.triangulate_model(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"])
    with pytest.raises(TypeError, match="unknown options"):
        T.triangulate_model(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], no_such_option=1)


def test_tracks_restatement_definition():
    rs = np.random.RandomState(0)
    n = 300
    e = rs.randint(0, n, (120, 2))
    labels, off, nodes = tr.tracks_ref(n, e)
    for u, v in e:
        assert labels[u] == labels[v]
    for t in range(len(off) - 1):
        seg = nodes[off[t]:off[t + 1]]
        assert len(seg) >= 2 and (np.diff(seg) > 0).all() and (labels[seg] == seg[0]).all()
    assert (np.diff(nodes[off[:-1]]) > 0).all()
    assert off[-1] == sum(1 for v in range(n) if (labels == labels[v]).sum() >= 2)


@functools.lru_cache(maxsize=None)
def _restated():
    sc = tr.make_scene(0, n_queries=6)
    L = tr.Layout(sc["cameras"], sc["images"], sc["keypoints"])
    ver = tr.verify_ref(L, sc["pair_matches"])
    _, t_off, t_nodes = tr.tracks_ref(int(L.off[-1]), tr.edges_of(L, sc["pair_matches"], ver[0], ver[1]))
    return sc, L, ver, t_off, t_nodes, tr.triangulate_ref(L, t_off, t_nodes)


def test_restatement_recovers_ground_truth():
    """Guards the yardstick: on the scene of the GPU tests the restatement keeps the true matches and drops the false ones, drops the
    thinned pairs, finds nearly every true point without mixing, and stays inside the band caps the GPU tests rely on."""
    sc, L, (m, off, counts, banded, sure), t_off, t_nodes, tri = _restated()
    truth = np.concatenate(sc["match_truth"])
    weak = np.zeros(len(truth), bool)
    for p in sc["weak_pairs"]:
        weak[off[p]:off[p + 1]] = True
        assert counts[p] < 15 and (m[off[p]:off[p + 1]] == -1).all()
    kept = m[:, 0] >= 0
    assert kept[truth & ~weak].mean() >= 0.98
    assert kept[~truth].mean() <= 0.15
    assert banded.mean() <= 0.01 and all(s is not None for s in sure)
    recall, mixing, err = tr.truth_figures(sc, L, t_off, t_nodes, tri)
    print(f"restatement: recall {recall:.4f}, mixing {mixing:.4f}, median |xyz error| / depth {err:.5f}, banded tracks {tri['banded'].mean():.4f}, "
          f"points per pass {(tri['n_obs'] > 0).sum(0)}")
    assert recall >= 0.95 and mixing <= 0.02 and err <= 0.005
    assert tri["banded"].mean() <= 0.02
    assert (tri["n_obs"][:, 1] > 0).sum() >= 1              # a component of two true points yields both


def test_restatement_map_supports_the_localisation_bound():
    """The end-to-end GPU test localises held-out cameras against the map within 0.1 deg and 0.5 % of the median depth
    (tests/test_gpu_pose.py's rule).  A map built from 1 px observations supports that: the restatement's map, each query's true
    correspondences, the Cauchy refinement of tests/pose_ref.py started at the true pose."""
    import pose_ref as pr
    sc, L, _, t_off, t_nodes, tri = _restated()
    truth = np.concatenate([sc["kp_truth"][i] for i in L.ids])
    where = {}
    for t in range(len(t_off) - 1):
        for p in range(tr.MAX_POINTS):
            if tri["n_obs"][t, p] >= 3:
                g = set(truth[t_nodes[t_off[t]:t_off[t + 1]][tri["obs_point"][t_off[t]:t_off[t + 1]] == p]].tolist())
                if len(g) == 1 and min(g) >= 0:
                    where[g.pop()] = tri["xyz"][t, p]
    assert len(sc["queries"]) == 6
    for q in sc["queries"]:
        sel = np.array([g in where for g in q["point_idx"]])
        X = np.array([where[g] for g in q["point_idx"][sel]])
        assert len(X) >= 100
        qv, tv = pr.refine_cauchy(q["camera"], q["qvec"], q["tvec"], q["xy"][sel], X, np.ones(len(X), bool))
        depth = np.median(X @ pr.qvec2rotmat(q["qvec"]).T[:, 2] + q["tvec"][2])
        rot, pos = np.degrees(pr.rot_angle(qv, q["qvec"])), np.linalg.norm(pr.centre(qv, tv) - pr.centre(q["qvec"], q["tvec"])) / depth
        print(f"query: {len(X)} correspondences, rotation {rot:.4f} deg, centre {100 * pos:.4f} % of the median depth")
        assert rot <= 0.05 and pos <= 0.0025                 # half the bound the GPU test asserts


# ---------------------------------------------------------------------------------------------------------------- designed inputs
@pytest.mark.parametrize("name", sorted(tr.LONG_SCENES))
def test_long_track_scenes_meet_their_classes(name):
    """The committed seeds keep the restatement inside the band cap and give the GPU test its classes of unbanded tracks."""
    sc, tri = tr.track_scene(name), tr.long_ref(name)
    got = tr.track_classes(sc, tri)
    print(f"{name}: {got}, lengths {np.diff(sc['t_off']).tolist()}, points per pass {(tri['n_obs'] > 0).sum(0).tolist()}")
    assert got["banded"] <= tr.LONG_BAND_CAP * got["tracks"]
    for k, least in tr.LONG_CLASSES[name].items():
        assert got[k] >= least, (k, got[k])
    assert (np.diff(sc["t_nodes"]) > 0)[np.setdiff1d(np.arange(len(sc["t_nodes"]) - 1), sc["t_off"][1:-1] - 1)].all()   # nodes ascend inside a track
    # an outlier is an outlier: no point of the restatement holds one
    assert (tri["obs_point"][sc["truth"] < 0] == -1).all()


def test_rule_tracks_take_their_designed_paths(monkeypatch):
    """The hand-built tracks of the one-per-image rule: nothing banded, and the restatement does with them what they were built for."""
    made = []
    refine = tr._Track.refine
    monkeypatch.setattr(tr._Track, "refine", lambda self, p, X, iters=200: (made.append((self.n, p)), refine(self, p, X, iters))[1])
    tr.rule_ref.cache_clear()
    rt, plain, off, nodes, tri, loff, lnodes, late = tr.rule_ref()
    tr.rule_ref.cache_clear()                                 # (computed under the patch: not for the other tests)
    assert not tri["banded"].any() and not late["banded"].any()
    for name in ("dup_mid", "dup_first"):
        t = plain.index(name)
        seg = tri["obs_point"][off[t]:off[t + 1]]
        lower, higher = rt["at"][name]["lower"], rt["at"][name]["higher"]
        a, b = rt["t_nodes"][rt["t_off"][rt["names"].index(name)]:][[lower, higher]]
        assert rt["L"].node_view[a] == rt["L"].node_view[b] and np.concatenate(rt["L"].kp)[a].tobytes() == np.concatenate(rt["L"].kp)[b].tobytes()
        assert seg[lower] == 0 and seg[higher] == -1 and (np.delete(seg, higher) == 0).all() and list(tri["n_obs"][t]) == [9, 0, 0, 0]
    for name in ("narrow", "narrow_far", "narrow_far_long"):
        t = plain.index(name)
        assert (tri["n_obs"][t] == 0).all() and (tri["obs_point"][off[t]:off[t + 1]] == -1).all()
    # 'narrow' never makes a point; 'narrow_far' and 'narrow_far_long' make one (of the five observations at the end) and drop it
    assert (4, 0) not in made and (5, 0) in made and made.count((75, 0)) == 1
    assert tri["n_obs"][plain.index("plain"), 0] == 9
    t = plain.index("plain_long")                             # its point's observations all lie past index 64
    assert tri["n_obs"][t, 0] == 9 and (tri["obs_point"][off[t]:off[t + 1]][:70] == -1).all() and (tri["obs_point"][off[t] + 70:off[t + 1]] == 0).all()
    at, seg = rt["at"]["late"], late["obs_point"]
    assert seg[at["a_near"]] == 0 and seg[at["a_far"]] != 0 and seg[at["b_near"]] == 0 and seg[at["b_far"]] != 0
    assert seg[at["c_held"]] == 0 and seg[at["c_other"]] != 0 and late["n_obs"][0, 0] == 9
    # b joins in the completion only: with a filter bound that leaves it out the point has 8 observations
    only = tr.triangulate_ref(rt["L"], loff, lnodes, create_max_angle_error=tr.RULE_LATE["create_max_angle_error"], filter_max_reproj_error=1.2)
    assert only["n_obs"][0, 0] == 8 and only["obs_point"][at["b_near"]] == -1


@pytest.mark.parametrize("g", tr.GRID, ids=lambda g: "-".join(str(v) for v in g))
def test_option_grid_stays_inside_the_band_cap(g):
    tri = tr.grid_ref(g)
    print(f"grid {g}: {int(tri['banded'].sum())} of {len(tri['banded'])} tracks banded, points per pass {(tri['n_obs'] > 0).sum(0).tolist()}")
    assert tri["banded"].mean() <= tr.GRID_BAND_CAP
    assert (tri["n_obs"][:, 0] > 0).sum() >= 6


@pytest.mark.parametrize("seed", tr.SEEDS)
def test_seed_and_label_cases_stay_inside_the_band_cap(seed):
    sc, off, nodes = tr.short_tracks()
    assert ((np.diff(off) >= 12) & (np.diff(off) <= 64)).sum() >= 6
    for label in tr.LABELS:
        tri = tr.seed_ref(seed, label)
        print(f"seed {seed} label {label}: {int(tri['banded'].sum())} of {len(tri['banded'])} tracks banded")
        assert tri["banded"].mean() <= tr.GRID_BAND_CAP, label


def test_seed_and_label_cases_depend_on_all_64_bits():
    """The committed values make the draws matter: restated with the seed or the labels cut to 32 bits, unbanded tracks take other
    observations, so a device that truncates either cannot pass tests/test_gpu_triangulation_edges.py."""
    sc, off, nodes = tr.short_tracks()
    for seed, label, kw in ((1, tr.LABELS[2], dict(label_mask=0xFFFFFFFF)), (tr.SEEDS[2], tr.LABELS[2], dict(label_mask=0xFFFFFFFF)),
                            (tr.SEEDS[2], tr.LABELS[0], dict(seed_mask=0xFFFFFFFF)), (tr.SEEDS[3], tr.LABELS[1], dict(seed_mask=0xFFFFFFFF))):
        tri, cut = tr.seed_ref(seed, label), tr.seed_ref(seed, label, **kw)
        clear = np.repeat(~tri["banded"], np.diff(off))
        changed = int((cut["obs_point"] != tri["obs_point"])[clear].sum())
        print(f"seed {seed} label {label} {kw}: {changed} observations of unbanded tracks change")
        assert changed > 0


def test_seam_pairs_are_what_they_claim():
    sp = tr.seam_scene()
    L = sp["L"]
    m, off, counts, banded, _ = tr.verify_ref(L, sp["pair_matches"], min_num_inliers=0)
    assert not banded.any()
    assert sorted(int(n) for n in np.diff(off)[:8]) == [0, 1, 255, 256, 257, 512, 513, 700]
    for p, (name, (i, j, rows), truth) in enumerate(zip(sp["names"], sp["pair_matches"], sp["truth"])):
        kept = m[off[p]:off[p + 1], 0] >= 0
        assert np.array_equal(kept, truth) and counts[p] == truth.sum(), name
        if len(rows) > 1 and name.startswith("n"):
            assert not truth[[r for r in (0, 255, 256, 511, 512, len(rows) - 1) if r < len(rows)]].any(), name
    by = dict(zip(sp["names"], range(len(sp["names"]))))
    assert not sp["truth"][by["self"]].any() and sp["pair_matches"][by["self"]][0] == sp["pair_matches"][by["self"]][1]
    i, j, _ = sp["pair_matches"][by["reversed_last_block"]]
    assert i > j and sp["truth"][by["reversed_last_block"]][:512].all() and not sp["truth"][by["reversed_last_block"]][512:].all()
    for name, n in (("exactly_min", tr.SEAM_MIN_INLIERS), ("one_short", tr.SEAM_MIN_INLIERS - 1)):
        t = sp["truth"][by[name]]
        assert t.sum() == n and t[:256].any() and t[256:512].any() and t[512:].any()
    dropped = tr.verify_ref(L, sp["pair_matches"], min_num_inliers=tr.SEAM_MIN_INLIERS)
    assert (dropped[0][off[by["exactly_min"]]:off[by["exactly_min"] + 1], 0] >= 0).sum() == tr.SEAM_MIN_INLIERS
    assert (dropped[0][off[by["one_short"]]:off[by["one_short"] + 1]] == -1).all() and np.array_equal(dropped[2], counts)
    # empty images at the front, in the middle and at the end; their non-empty neighbours are matched at key points 0 and n - 1
    assert [len(sp["keypoints"][i]) for i in tr.SEAM_EMPTY] == [0, 0, 0] and tr.SEAM_EMPTY == (min(sp["images"]), 6, max(sp["images"]))
    used = {i: set() for i in sp["images"]}
    for i, j, rows in sp["pair_matches"]:
        used[i] |= set(rows[:, 0].tolist())
        used[j] |= set(rows[:, 1].tolist())
    for i in (2, 5, 7, 9):
        assert {0, len(sp["keypoints"][i]) - 1} <= used[i], i
    assert {sp["cameras"][sp["images"][i].camera_id]["model"] for i in sp["images"] if len(sp["keypoints"][i])} == set(tr.MODELS)
    i, j, rows = sp["pair_matches"][by["corners"]]
    corner = {(0.0, 0.0), (639.0, 0.0), (0.0, 479.0), (639.0, 479.0)}
    assert corner <= {tuple(k) for k in sp["keypoints"][i][rows[:, 0]].tolist()} and corner <= {tuple(k) for k in sp["keypoints"][j][rows[:, 1]].tolist()}
    assert {sp["cameras"][sp["images"][v].camera_id]["model"] for v in (i, j)} == {"SIMPLE_RADIAL", "OPENCV"}


def test_tri_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "tri.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "tri_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*tri_\w+_kernel\S*)", meta)
    assert len(kernels) >= 10 and any("tri_track_kernel" in k for k in kernels)
    seg = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    assert seg and all(int(v) == 0 for v in seg)
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))


def test_new_sources_keep_to_vector_stores():
    """No scalar store to memory, scalar atomic or scalar data-cache write-back / discard in the new sources, in any spelling."""
    words = ["s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic",
             "s_dcache_" + "wb", "s_dcache_" + "discard"]
    for rel in ("sfd2_amd/csrc/tri_kernels.hip", "sfd2_amd/csrc/api_triangulate.hip", "sfd2_amd/triangulation.py", "sfd2_amd/colmap_io.py",
                "tools/triangulate_bench.py"):
        text = open(os.path.join(ROOT, rel)).read().lower()
        for w in words:
            assert w not in text, (rel, w)
