"""The round-based mapper on the MI355X (sfd2_amd.reconstruction) against the numpy restatement and the scenes
of tests/mapper_ref.py.

restrict / visible / assemble are integer work and copies: compared byte for byte.  The filter's obs_keep and point_live are compared
exactly (no comparison of the scenes lies within 1e-9 of a threshold, tests/test_mapper_host.py); point_error and point_angle to
100 x the floor between the restatement's two formulations, measured on the machine the test runs on, ceiling 1e-9 relative (on the
CPU the floor is 3.8e-14 on 'long_tracks' and 2.5e-13 on 'busy_views', so the tolerances are 3.8e-12 and 2.5e-11).

End to end the yardstick is the project's own pieces started from the truth: triangulation.triangulate_model with the true poses, then
bundle_adjustment.bundle_adjust (Cauchy, 1 px, 100 steps: the mapper's final adjustment) with the mapper's initial pair constant.  Both
models are aligned to the true camera centres by a similarity transform.  Required: all 12 images, >= 0.9 x the yardstick's points,
mean reprojection error <= 1.5 x, largest rotation and centre error <= 3 x the yardstick's (the yardstick holds two true poses; the
mapper's gauge comes from one relative pose and the alignment).  Measured on the MI355X: point_error to 4.2e-14 / 3.1e-13 and
point_angle to 2.3e-16 / 3.5e-15 ('long_tracks' / 'busy_views'; tolerances 3.1e-12 / 2.5e-11); end to end 12 of 12 images in 3 rounds,
points 1.00 x, mean reprojection error 0.99 x, rotation 2.4 x, centre 1.00 x the yardstick's.  With both images of the initial pair
constant in every adjustment (option fix_initial_pair) the rotation figure was 7.6 x: the pair's relative pose is 0.65 degrees off and
nothing could correct it, which is why the second image is held only while the pair stands alone."""

import numpy as np
import pytest

import mapper_ref as mr
import tri_ref as tr

pytestmark = pytest.mark.gpu

SCENES = ("long_tracks", "busy_views")
REGS = ("none", "one", "all", "every_other")


def _RC():
    from sfd2_amd import reconstruction
    return reconstruction


def _flags():
    from sfd2_amd import _lib
    return {None: 0, "lane": _lib.MAPPER_FLAG_TRACK_LANE, "wave": _lib.MAPPER_FLAG_TRACK_WAVE}


def _views(tuples):
    from sfd2_amd import _lib
    from sfd2_amd.pose import camera_model
    arr = (_lib.TriView * len(tuples))()
    for i, (cam, q, t) in enumerate(tuples):
        arr[i].model, params = camera_model(cam)
        for k in range(8):
            arr[i].params[k] = params[k]
        for k in range(4):
            arr[i].qvec[k] = q[k]
        for k in range(3):
            arr[i].tvec[k] = t[k]
    return arr


def _same(a, b, keys):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


# ---------------------------------------------------------------------------------------------------------------- restrict
RESTRICT_KEYS = ("sub_track", "sub_offsets", "sub_obs", "sub_view", "sub_xy")


@pytest.mark.parametrize("name", SCENES)
def test_restrict_matches_the_restatement_under_every_mapping(name):
    sc = mr.table_scene(name)
    for reg in REGS:
        want = mr.restrict_ref(sc["off"], sc["obs_view"], sc["obs_xy"], sc["registered"][reg])
        for flag in _flags().values():
            got = _RC().restrict_tracks(sc["off"], sc["obs_view"], sc["obs_xy"], sc["registered"][reg], flags=flag)
            _same(got, want, RESTRICT_KEYS)
        if reg in ("none", "one"):
            assert len(want["sub_track"]) == 0 and want["sub_offsets"].tolist() == [0]
        if reg == "all":
            assert want["sub_obs"].tolist() == list(range(len(sc["obs_view"])))
    if name == "long_tracks":                                 # the tracks of 2 .. 300 observations all lose some and keep two views
        want = mr.restrict_ref(sc["off"], sc["obs_view"], sc["obs_xy"], sc["registered"]["every_other"])
        kept = np.diff(want["sub_offsets"])
        assert 0 < len(kept) and (kept < np.diff(sc["off"])[want["sub_track"]]).any() and kept.max() > 64


def test_restrict_drops_a_track_seen_by_one_registered_view_only():
    off = np.array([0, 3, 5, 5, 9, 79], np.int64)             # the last track: 70 observations, a wave's
    ov = np.concatenate([[0, 1, 2, 1, 1, 0, 2, 2, 3], np.r_[np.full(35, 1), np.full(35, 4)]]).astype(np.int32)
    xy = np.arange(2 * len(ov), dtype=np.float32).reshape(-1, 2)
    for reg, tracks in (([0, 1, 0, 0, 0], []), ([0, 0, 1, 0, 0], []), ([1, 0, 1, 0, 0], [0, 3]), ([0, 1, 0, 0, 1], [4]), ([0, 1, 0, 1, 0], []), ([1, 1, 1, 1, 1], [0, 3, 4])):
        want = mr.restrict_ref(off, ov, xy, reg)
        assert want["sub_track"].tolist() == tracks
        for flag in _flags().values():
            _same(_RC().restrict_tracks(off, ov, xy, reg, flags=flag), want, RESTRICT_KEYS)
    empty = _RC().restrict_tracks(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), [1, 1])
    assert len(empty["sub_track"]) == 0 and empty["sub_offsets"].tolist() == [0]


# ---------------------------------------------------------------------------------------------------------------- visible / assemble
@pytest.mark.parametrize("name", SCENES)
def test_visible_counts_match_the_restatement(name):
    sc = mr.table_scene(name)
    assert sorted(set(np.bincount(sc["point_track"], minlength=len(sc["off"]) - 1).tolist())) == [0, 1, 2, 3, 4]      # tracks with 0 to 4 points
    for reg in REGS:
        want = mr.visible_ref(sc["off"], sc["obs_view"], sc["registered"][reg], sc["point_track"], sc["point_live"])
        got = _RC().visible_counts(sc["off"], sc["obs_view"], sc["registered"][reg], sc["point_track"], sc["point_live"])
        assert got.dtype == np.int64 and got.tolist() == want.tolist(), reg
        assert (got[sc["registered"][reg]] == 0).all()
    assert mr.visible_ref(sc["off"], sc["obs_view"], sc["registered"]["none"], sc["point_track"], sc["point_live"]).sum() > 0
    dead = _RC().visible_counts(sc["off"], sc["obs_view"], sc["registered"]["none"], sc["point_track"], np.zeros(len(sc["point_track"]), bool))
    none = _RC().visible_counts(sc["off"], sc["obs_view"], sc["registered"]["none"], np.zeros(0, np.int32), np.zeros(0, bool))
    assert dead.sum() == 0 and none.sum() == 0 and len(none) == sc["n_views"]


ASSEMBLE_KEYS = ("offsets", "points2D", "points3D", "src_obs", "src_point")


@pytest.mark.parametrize("name", SCENES)
def test_assembled_problems_are_the_restatements_bytes(name):
    sc = mr.table_scene(name)
    cand = [0, 150, 299, 150, 7] if name == "long_tracks" else [6, 0, 1, 2, 3, 4, 5, 8, 6]       # a repeated view; busy_views' view 0 has no observation
    args = (sc["off"], sc["obs_view"], sc["obs_xy"], sc["n_views"], sc["point_track"], sc["point_live"], sc["point_xyz"])
    counts = mr.visible_ref(sc["off"], sc["obs_view"], sc["registered"]["none"], sc["point_track"], sc["point_live"])
    want = mr.assemble_ref(*args, cand)
    assert want["offsets"][-1] == counts[cand].sum() > 0                          # the capacity rule: the sum of the visible counts
    got = _RC().assemble_problems(*args, cand, int(counts[cand].sum()))
    _same(got, want, ASSEMBLE_KEYS)
    assert (np.diff(want["src_obs"]) == 0).any()                                  # an observation with two live points: same 2D, different 3D
    if name == "busy_views":
        assert np.diff(want["offsets"])[1] == 0 and np.diff(want["offsets"]).max() > 1000      # a candidate with nothing, one beyond four blocks
    again = _RC().assemble_problems(*args, cand, int(counts[cand].sum()) + 5)     # spare capacity changes nothing
    _same(again, want, ASSEMBLE_KEYS)
    zero = _RC().assemble_problems(*args, [], 0)
    assert zero["offsets"].tolist() == [0] and len(zero["src_obs"]) == 0
    with pytest.raises(RuntimeError, match=f"{int(want['offsets'][-1])} correspondences for a capacity of 3"):
        _RC().assemble_problems(*args, cand, 3)


def test_bad_arguments_name_the_first_offending_index():
    RC, sc = _RC(), mr.table_scene("busy_views")
    ov = sc["obs_view"].copy()
    ov[[41, 500]] = sc["n_views"]
    off = sc["off"].copy()
    off[9] = off[8] - 1
    pt = sc["point_track"].copy()
    pt[30] = pt[29] - 1
    far = sc["point_track"].copy()
    far[-1] = len(sc["off"]) - 1
    reg, live = sc["registered"]["every_other"], sc["point_live"]
    with pytest.raises(RuntimeError, match="sfd2_mapper_restrict: observation 41: view index out of range"):
        RC.restrict_tracks(sc["off"], ov, sc["obs_xy"], reg)
    with pytest.raises(RuntimeError, match="sfd2_mapper_restrict: track 8: track_offsets decrease"):
        RC.restrict_tracks(off, sc["obs_view"], sc["obs_xy"], reg)
    with pytest.raises(RuntimeError, match="sfd2_mapper_visible: observation 41: view index out of range"):
        RC.visible_counts(sc["off"], ov, reg, sc["point_track"], live)
    with pytest.raises(RuntimeError, match="sfd2_mapper_visible: point 30: point_track must be ascending"):
        RC.visible_counts(sc["off"], sc["obs_view"], reg, pt, live)
    with pytest.raises(RuntimeError, match=f"sfd2_mapper_visible: point {len(far) - 1}: track index out of range"):
        RC.visible_counts(sc["off"], sc["obs_view"], reg, far, live)
    five = np.zeros(5, np.int32)
    with pytest.raises(RuntimeError, match="sfd2_mapper_visible: point 4: more than SFD2_TRI_MAX_POINTS"):
        RC.visible_counts(sc["off"], sc["obs_view"], reg, five, np.ones(5, bool))
    args = (sc["off"], sc["obs_view"], sc["obs_xy"], sc["n_views"], sc["point_track"], live, sc["point_xyz"])
    with pytest.raises(RuntimeError, match="sfd2_mapper_assemble: candidate 1: view index out of range"):
        RC.assemble_problems(*args, [3, sc["n_views"], -1], 10)
    with pytest.raises(RuntimeError, match="sfd2_mapper_assemble: point 30: point_track must be ascending"):
        RC.assemble_problems(sc["off"], sc["obs_view"], sc["obs_xy"], sc["n_views"], pt, live, sc["point_xyz"], [3], 10)
    views = _views(sc["views"])
    with pytest.raises(RuntimeError, match="sfd2_mapper_filter: observation 41: view index out of range"):
        RC.filter_points(views, sc["n_views"], sc["fxyz"], sc["off"], ov, sc["fxy"])
    with pytest.raises(RuntimeError, match="sfd2_mapper_filter: point 8: point_offsets decrease"):
        RC.filter_points(views, sc["n_views"], sc["fxyz"], np.concatenate([off[:-1], sc["off"][-1:]]), sc["obs_view"], sc["fxy"])
    bad = sc["fxyz"].copy()
    bad[17, 1] = np.nan
    with pytest.raises(RuntimeError, match="sfd2_mapper_filter: point 17: non-finite"):
        RC.filter_points(views, sc["n_views"], bad, sc["off"], sc["obs_view"], sc["fxy"])
    with pytest.raises(RuntimeError, match="unknown flags"):
        RC.restrict_tracks(sc["off"], sc["obs_view"], sc["obs_xy"], reg, flags=3)


# ---------------------------------------------------------------------------------------------------------------- filter
@pytest.mark.parametrize("name", SCENES)
def test_filter_matches_the_restatement_under_every_mapping(name):
    sc, refs, second = mr.table_scene(name), mr.filter_refs(name), mr.filter_second(name)
    views = _views(sc["views"])
    for mapping, flag in _flags().items():
        want = refs[mapping]
        assert not want["banded"].any()
        tol = min(100 * mr.filter_floor(want, second), 1e-9)
        got = _RC().filter_points(views, sc["n_views"], sc["fxyz"], sc["off"], sc["obs_view"], sc["fxy"], 4.0, 1.5, flags=flag)
        assert (got["obs_keep"] == want["obs_keep"]).all() and (got["point_live"] == want["point_live"]).all(), mapping
        assert (np.isnan(got["point_angle"]) == np.isnan(want["point_angle"])).all()
        worst = {}
        for k in ("point_error", "point_angle"):
            ok = np.isfinite(want[k]) & (want[k] != 0)
            worst[k] = float((np.abs(got[k][ok] - want[k][ok]) / np.abs(want[k][ok])).max())
            assert (got[k][~ok & np.isfinite(want[k])] == 0).all()
        print(name, mapping, "tolerance %.2g" % tol, {k: "%.2g" % v for k, v in worst.items()})
        assert max(worst.values()) <= tol, (name, mapping, worst, tol)
        again = _RC().filter_points(views, sc["n_views"], sc["fxyz"], sc["off"], sc["obs_view"], sc["fxy"], 4.0, 1.5, flags=flag)
        _same(again, got, ("obs_keep", "point_live", "point_error", "point_angle"))
    assert not want["obs_keep"][sc["off"][5]] and want["depth"][sc["off"][12]] < 0 and not got["point_live"][12]     # 60 px off; behind a camera


# ---------------------------------------------------------------------------------------------------------------- end to end
def _scene():
    return mr.br.cached(("mapper_gpu_scene",), tr.make_scene)


def _mapped():
    def make():
        sc, rep = _scene(), {}
        ims, pts = _RC().reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], report=rep)
        return ims, pts, rep
    return mr.br.cached(("mapper_gpu_run",), make)


def test_reconstruction_from_matches_alone_against_the_pieces_started_from_the_truth():
    from sfd2_amd import bundle_adjustment as B, triangulation as T
    sc = _scene()
    ims, pts, rep = _mapped()
    assert sorted(ims) == list(range(1, 13)) and rep["final"]["n_registered"] == 12
    y_ims, y_pts = T.triangulate_model(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"])
    y_ims, y_pts, _ = B.bundle_adjust(sc["cameras"], y_ims, y_pts, constant_images=list(rep["initial_pair"]), max_iterations=100, loss="cauchy",
                                      loss_scale=1.0)
    got, want = mr.model_errors(ims, pts, sc["images"]), mr.model_errors(y_ims, y_pts, sc["images"])
    ratios = {"points": got["points"] / want["points"], "mean_reproj": got["mean_reproj"] / want["mean_reproj"],
              "rotation": got["rotation"] / want["rotation"], "centre": got["centre"] / want["centre"]}
    print("mapper", got, "yardstick", want, "ratios", {k: round(v, 3) for k, v in ratios.items()}, "rounds", len(rep["rounds"]))
    assert ratios["points"] >= 0.9 and ratios["mean_reproj"] <= 1.5 and ratios["rotation"] <= 3.0 and ratios["centre"] <= 3.0, ratios
    for pid, p in pts.items():
        assert all(ims[int(i)].point3D_ids[int(k)] == pid for i, k in zip(p.image_ids, p.point2D_idxs))


def _write_inputs(sc, root):
    """A model that only carries the intrinsics, the pair list (with a repeated pair and one naming an unknown image) and the two stores."""
    from sfd2_amd import colmap_io, feature_io
    from sfd2_amd.match_features import names_to_pair
    ref = root / "ref"
    blank = {i: colmap_io.Image(i, np.array([1.0, 0, 0, 0]), np.zeros(3), im.camera_id, im.name, np.zeros((0, 2)), np.zeros(0, np.int64))
             for i, im in sc["images"].items()}
    colmap_io.write_model(sc["cameras"], blank, {}, ref)
    name = {i: im.name for i, im in sc["images"].items()}
    lines = [f"{name[a]} {name[b]}" for a, b in sc["pairs"]]
    lines += [lines[0], f"{name[1]} nowhere/else.jpg"]
    (root / "pairs.txt").write_text("\n".join(lines) + "\n")
    feats = feature_io.open_store(str(root / "feats.h5"), "a")
    for i, kp in sc["keypoints"].items():
        feature_io.write_features(feats, name[i], {"keypoints": kp.astype(np.float64), "scores": np.ones(len(kp)), "image_size": np.array([640, 480])})
    feats.close()
    store = feature_io.open_store(str(root / "matches.h5"), "a")
    for i0, i1, m in sc["pair_matches"]:
        m0 = np.full(len(sc["keypoints"][i0]), -1, dtype=np.int64)
        m0[m[:, 0]] = m[:, 1]
        feature_io.write_matches(store, names_to_pair(name[i0], name[i1]), m0, np.ones(len(m0), dtype=np.float32))
    store.close()
    return ref, root / "pairs.txt", root / "feats.h5", root / "matches.h5"


def test_main_writes_a_model_the_readers_load_and_two_runs_write_equal_bytes(tmp_path):
    from sfd2_amd import colmap_io, triangulation as T
    from sfd2_amd.covis import MapIndex
    RC, sc = _RC(), _scene()
    ref, pairs, feats, matches = _write_inputs(sc, tmp_path)
    stats = RC.main(tmp_path / "sfm", tmp_path / "images", pairs, feats, matches, reference_sfm_model=ref)
    model = tmp_path / "sfm" / "models" / "0"
    assert not (tmp_path / "sfm" / "database.db").exists()
    cameras, images, points3D = colmap_io.read_model(model)
    assert len(images) == 12 == stats["num_reg_images"] == stats["num_input_images"] and len(points3D) == stats["num_sparse_points"] > 500
    assert len(MapIndex(images, points3D).point_ids) == len(points3D)
    lines = (tmp_path / "sfm" / "stats.txt").read_text().splitlines()
    assert [ln.split(": ")[0] for ln in lines] == list(RC.STAT_KEYS) and len(lines) == 7
    st = {ln.split(": ")[0]: float(ln.split(": ")[1]) for ln in lines}
    assert st["num_observations"] == sum(len(p.image_ids) for p in points3D.values()) and 0 < st["mean_reproj_error"] < 4
    # the same inputs through reconstruct(): the second run writes the bytes of the first
    cams2, imgs2 = RC.read_images(pairs, feats, reference_sfm_model=ref)
    kps, pm = T.read_inputs(imgs2, pairs, feats, matches)
    ims, pts = RC.reconstruct(cams2, imgs2, kps, pm)
    colmap_io.write_model(cams2, ims, pts, tmp_path / "direct")
    for f in ("cameras.bin", "images.bin", "points3D.bin"):
        assert (model / f).read_bytes() == (tmp_path / "direct" / f).read_bytes(), f
    # and it is the model of the in-memory scene: the stores carry the same key points and matches
    base = _mapped()
    assert len(pts) == len(base[1]) and all(ims[i].qvec.tobytes() == base[0][i].qvec.tobytes() for i in ims)


def test_skip_geometric_verification_on_verified_matches_registers_every_image():
    from sfd2_amd import two_view
    sc = _scene()
    m, off, _, _ = two_view.verify_pairs_two_view(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], 4.0, 15)
    verified = [(a, b, m[off[p]:off[p + 1]][m[off[p]:off[p + 1], 0] >= 0]) for p, (a, b, _) in enumerate(sc["pair_matches"])]
    rep = {}
    ims, pts = _RC().reconstruct(sc["cameras"], sc["images"], sc["keypoints"], verified, skip_geometric_verification=True, report=rep)
    assert len(ims) == 12 and len(pts) > 500 and rep["n_eligible_pairs"] <= 50
