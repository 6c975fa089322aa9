"""Pose-free geometric verification on the MI355X: sfd2_amd.two_view.verify_pairs_two_view against its restatement
(tests/two_view_ref.py per pair, plus the rules of the wrapper) and the command sfd2_amd.geometric_verification on a temporary store."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import tri_ref
import two_view_ref as tv

pytestmark = pytest.mark.gpu

MIN_INLIERS = 15
_cache = {}


def _scene():
    """Four images, about 60 key points each, a tenth of the matches wrong; plus a pair of an image with itself, a pair with
    pre-rejected rows and a pair thinned below MIN_INLIERS."""
    if "sc" not in _cache:
        sc = tri_ref.make_scene(seed=5, n_images=4, n_points=60, n_clutter=12, window=3, n_joiners=0, n_weak_pairs=1, p_visible=0.9,
                                noise_px=0.5, spacing=1.5)
        pm = list(sc["pair_matches"])
        i0, i1, m = pm[0]
        pre = m.copy()
        pre[::7] = -1
        pm[0] = (i0, i1, pre)
        pm.append((2, 2, np.stack([np.arange(20), np.arange(20)], 1).astype(np.int32)))
        sc["pm"] = pm
        _cache["sc"] = sc
    return _cache["sc"]


def _restated(sc):
    """(matches, counts, banded) by the rules of verify_pairs_two_view over relative_pose_ref."""
    rows, counts, banded = [], [], []
    for i0, i1, m in sc["pm"]:
        out = np.full_like(m, -1)
        live = np.flatnonzero((m[:, 0] >= 0) & (m[:, 1] >= 0))
        if i0 == i1:
            live = live[:0]
        k0 = sc["keypoints"][i0].astype(np.float64) + 0.5
        k1 = sc["keypoints"][i1].astype(np.float64) + 0.5
        r = tv.relative_pose_ref(k0[m[live, 0]], k1[m[live, 1]], sc["cameras"][sc["images"][i0].camera_id],
                                 sc["cameras"][sc["images"][i1].camera_id], 4.0, MIN_INLIERS)
        if r["success"] and r["num_inliers"] >= MIN_INLIERS:
            out[live[r["inliers"]]] = m[live[r["inliers"]]]
        rows.append(out)
        counts.append(r["num_inliers"])
        banded.append(r["banded"])
    return rows, counts, banded


def test_verify_pairs_two_view_against_its_restatement():
    from sfd2_amd import triangulation, two_view
    sc = _scene()
    m, off, counts, results = two_view.verify_pairs_two_view(sc["cameras"], sc["images"], sc["keypoints"], sc["pm"], 4.0, MIN_INLIERS)
    rows, ref_counts, banded = _restated(sc)
    assert len(off) == len(sc["pm"]) + 1 and off[-1] == len(m) == sum(len(p[2]) for p in sc["pm"]) and len(results) == len(sc["pm"])
    compared = 0
    for p in range(len(sc["pm"])):
        if banded[p]:
            continue
        compared += 1
        assert counts[p] == ref_counts[p], p
        assert np.array_equal(m[off[p]:off[p + 1]], rows[p]), p
    print(f"{compared} of {len(sc['pm'])} pairs compared")
    assert compared >= len(sc["pm"]) - 1
    assert (m[off[-2]:off[-1]] == -1).all() and counts[-1] == 0                      # the pair of an image with itself
    assert (m[off[0]:off[1]][::7] == -1).all()                                        # rows that came in rejected
    weak = sc["weak_pairs"][0]
    assert (m[off[weak]:off[weak + 1]] == -1).all() and counts[weak] < MIN_INLIERS    # the thinned pair
    assert sum(int((m[off[p]:off[p + 1], 0] >= 0).sum()) >= MIN_INLIERS for p in range(len(sc["pm"]))) >= 3
    # the survivors are all true matches, and the result feeds build_tracks as verify_pairs' does
    ids = sorted(sc["images"])
    kp_off, _ = triangulation.keypoint_table(ids, sc["keypoints"])
    index = {iid: k for k, iid in enumerate(ids)}
    pv = np.array([[index[a], index[b]] for a, b, _ in sc["pm"]])
    n_per = np.diff(off)
    live = m[:, 0] >= 0
    edges = np.stack([np.repeat(kp_off[pv[:, 0]], n_per) + m[:, 0], np.repeat(kp_off[pv[:, 1]], n_per) + m[:, 1]], 1)[live]
    labels, t_off, t_nodes = triangulation.build_tracks(int(kp_off[-1]), edges)
    assert len(t_off) - 1 > 20 and len(labels) == kp_off[-1]


def test_index_beyond_the_key_points_raises():
    from sfd2_amd import two_view
    sc = _scene()
    i0, i1, m = sc["pm"][1]
    bad = m.copy()
    bad[0, 1] = len(sc["keypoints"][i1])
    with pytest.raises(ValueError, match="beyond"):
        two_view.verify_pairs_two_view(sc["cameras"], sc["images"], sc["keypoints"], [(i0, i1, bad)])


def _write_inputs(sc, root):
    from sfd2_amd import colmap_io, feature_io
    from sfd2_amd.match_features import names_to_pair
    ref = root / "ref"
    empty = {i: colmap_io.Image(i, im.qvec, im.tvec, im.camera_id, im.name, np.zeros((0, 2)), np.zeros(0, np.int64)) for i, im in sc["images"].items()}
    colmap_io.write_model(sc["cameras"], empty, {}, ref)
    name = {i: im.name for i, im in sc["images"].items()}
    (root / "pairs.txt").write_text("\n".join(f"{name[a]} {name[b]}" for a, b in sc["pairs"]) + "\n")
    feats = feature_io.open_store(str(root / "feats.h5"), "a")
    for i, kp in sc["keypoints"].items():
        feature_io.write_features(feats, name[i], {"keypoints": kp.astype(np.float64), "scores": np.ones(len(kp)), "image_size": np.array([640, 480])})
    feats.close()
    store = feature_io.open_store(str(root / "matches.h5"), "a")
    for i0, i1, m in sc["pair_matches"]:
        m0 = np.full(len(sc["keypoints"][i0]), -1, dtype=np.int64)
        m0[m[:, 0]] = m[:, 1]
        feature_io.write_matches(store, names_to_pair(name[i0], name[i1]), m0, np.where(m0 >= 0, 0.9, 0.0).astype(np.float32))
    store.close()
    return ref, root / "pairs.txt", root / "feats.h5", root / "matches.h5"


def _groups(path):
    from sfd2_amd import feature_io
    st = feature_io.open_store(str(path), "r")
    out = {k: {d: np.asarray(st[k][d].__array__()) for d in st[k].keys()} for k in st.keys()}
    st.close()
    return out


def test_command_on_a_temporary_store(tmp_path):
    from sfd2_amd import geometric_verification as gv, two_view
    from sfd2_amd.match_features import names_to_pair
    sc = _scene()
    ref, pairs, feats, matches = _write_inputs(sc, tmp_path)
    res = gv.main(pairs, feats, matches, tmp_path / "verified.h5", reference_sfm_model=ref, relative_poses=tmp_path / "rel.txt")
    src, dst = _groups(matches), _groups(tmp_path / "verified.h5")
    assert set(src) == set(dst) and len(dst) == len(sc["pairs"])
    name = {i: im.name for i, im in sc["images"].items()}
    dropped = 0
    for (i0, i1, m) in sc["pair_matches"]:
        g0, g1 = src[names_to_pair(name[i0], name[i1])], dst[names_to_pair(name[i0], name[i1])]
        assert set(g0) == set(g1) and g1["matches0"].dtype == g0["matches0"].dtype
        assert np.array_equal(g0["matching_scores0"], g1["matching_scores0"])
        changed = g0["matches0"] != g1["matches0"]
        assert (g1["matches0"][changed] == -1).all()
        dropped += int(changed.sum())
        # the values are those of relative_pose_batch on the pair's matches
        k0, k1 = sc["keypoints"][i0].astype(np.float64) + 0.5, sc["keypoints"][i1].astype(np.float64) + 0.5
        r = two_view.relative_pose(k0[m[:, 0]], k1[m[:, 1]], sc["cameras"][sc["images"][i0].camera_id], sc["cameras"][sc["images"][i1].camera_id])
        got = res[name[i0], name[i1]]
        assert np.array_equal(r["qvec"], got["qvec"]) and np.array_equal(r["tvec"], got["tvec"]) and r["num_inliers"] == got["num_inliers"]
    assert dropped > 0
    lines = (tmp_path / "rel.txt").read_text().splitlines()
    assert len(lines) == len(sc["pairs"])
    for ln, (a, b) in zip(lines, sc["pairs"]):
        f = ln.split()
        r = res[name[a], name[b]]
        assert f[:2] == [name[a], name[b]] and len(f) == 12 and int(f[2]) == int(r["success"]) and int(f[3]) == r["num_inliers"]
        assert np.array_equal(np.array(f[4:11], float), np.concatenate([r["qvec"], r["tvec"]]))
        assert float(f[11]) == r["tri_angle_deg"] or (np.isnan(float(f[11])) and np.isnan(r["tri_angle_deg"]))
    # the command line writes the same files
    subprocess.run([sys.executable, "-m", "sfd2_amd.geometric_verification", "--pairs", str(pairs), "--features", str(feats), "--matches",
                    str(matches), "--output", str(tmp_path / "cli.h5"), "--reference_sfm_model", str(ref), "--relative_poses",
                    str(tmp_path / "cli.txt")], check=True, timeout=120, cwd=str(Path(__file__).resolve().parent.parent))
    assert (tmp_path / "cli.txt").read_text() == (tmp_path / "rel.txt").read_text()
    cli = _groups(tmp_path / "cli.h5")
    assert set(cli) == set(dst) and all(np.array_equal(cli[k][d], dst[k][d]) for k in dst for d in dst[k])
