"""Fundamental matrix on the MI355X (sfd2_amd.two_view.fundamental_matrix*, verify_pairs_fundamental) against the restatement of
tests/fundamental_ref.py: the RANSAC table, the option runs, the stride seams, the solver probes, degenerate inputs (trials, count and
mask equal; F within fundamental_ref.F_TOL), properties that need no restatement, and the two commands end to end on a scene whose
cameras the caller does not know."""
import numpy as np
import pytest

import fundamental_ref as fr
import mapper_ref as mr
import tri_ref as tr

pytestmark = pytest.mark.gpu


def _tv():
    from sfd2_amd import two_view
    return two_view


def _run_table(name, cases, refs, **conf):
    """One batch against its restatement; returns the device results."""
    res = _tv().fundamental_matrix_batch(cases, **conf)
    left, worst = 0, [0.0]
    for r, ref in zip(res, refs):
        if ref["banded"]:
            left += 1
            continue
        fr.compare(r, ref, worst)
    print(f"{name}: {left} of {len(cases)} left out, worst distance of the matrices {worst[0]:.3g} (tolerance {fr.F_TOL:.3g})")
    assert left <= len(cases) // 10
    return res


# ---------------------------------------------------------------------------------------------------------------- against the restatement
def test_ransac_table_against_the_restatement():
    """n = 7, 8, 12, 40, 80, 300 x outliers 0 / 0.25 / 0.5 / 0.7 x thresholds 4 and 1 px, 0.5 px noise."""
    res = _run_table("RANSAC table", fr.ransac_cases(), fr.ransac_refs())
    for (n, _, _, _), r, ref in zip(fr.RANSAC_CASES, res, fr.ransac_refs()):
        if n in (7, 8):
            assert not ref["banded"]
    assert {r["num_trials"] for r in res} >= {256, 512, 10000}


def test_option_runs_against_the_restatement():
    p0, p1, th = fr.option_case()
    left, worst, trials = 0, [0.0], set()
    for conf in fr.OPTION_RUNS:
        ref = fr.option_ref(**conf)
        r = _tv().fundamental_matrix(p0, p1, th, **conf)
        trials.add(r["num_trials"])
        if ref["banded"]:
            left += 1
            continue
        fr.compare(r, ref, worst)
    print(f"option runs: {left} of {len(fr.OPTION_RUNS)} left out, worst {worst[0]:.3g}, trial counts {sorted(trials)}")
    assert left <= len(fr.OPTION_RUNS) // 10 and trials >= {1, 255, 256, 257, 300, 600}
    # a seed is 64 bits without a sign
    a, b = _tv().fundamental_matrix(p0, p1, th, seed=-1), _tv().fundamental_matrix(p0, p1, th, seed=2 ** 64 - 1)
    assert np.array_equal(a["F"], b["F"]) and np.array_equal(a["inliers"], b["inliers"])


def test_stride_seams_in_one_batch():
    """n = 255, 256, 257, 511, 513, 1025 between pairs of 0, 6 and 7 correspondences."""
    res = _run_table("stride seams", fr.size_cases(), fr.size_refs())
    for (p0, _, _), r in zip(fr.size_cases(), res):
        assert len(r["inliers"]) == len(p0)
        if len(p0) < 7:
            assert not r["success"] and r["num_trials"] == 0 and not r["F"].any() and not r["inliers"].any()


@pytest.mark.parametrize("family", fr.PROBE_FAMILIES)
def test_solver_probes(family):
    """One trial on 8 or 9 correspondences: what the device returns for the sample is what the restatement returns, and in the exact
    families the generating matrix holds every point wherever the restatement says the sample yields it."""
    ps, refs = fr.probes(family), fr.probe_refs(family)
    res = _run_table("probes " + family, [(p0, p1, th) for p0, p1, _, _, th in ps], refs, **fr.PROBE_CONF)
    assert all(r["num_trials"] == 1 for r in res)
    if family != "near_planar":
        found = sum(bool(r["inliers"].all()) and np.linalg.norm(r["F"] - _signed(fr.true_F(R, t))) < 1e-6 for r, (_, _, R, t, _) in zip(res, ps))
        print(f"{family}: the generating matrix found in {found} of {len(ps)}")
        assert found >= fr.probe_disagreement(family)[1] - len(ps) // 10


def _signed(F):
    F = F / np.linalg.norm(F)
    return F if F.reshape(-1)[int(np.argmax(np.abs(F)))] > 0 else -F


@pytest.mark.parametrize("name", sorted(fr.DEGENERATE))
def test_degenerate_inputs_give_no_result(name):
    p0, p1 = fr.degenerate(name)
    ref = fr.degenerate_ref(name)
    r = _tv().fundamental_matrix(p0, p1, 4.0, **fr.DEGENERATE[name])
    assert not ref["success"] and ref["num_inliers"] == 0
    assert (r["success"], r["num_inliers"], r["num_trials"]) == (False, 0, ref["num_trials"])
    assert not r["F"].any() and not r["inliers"].any() and len(r["inliers"]) == len(p0)


# ---------------------------------------------------------------------------------------------------------------- properties
def _sampson_px(F, p0, p1):
    return fr.sampson_f64(F, p0, p1)


def _check_properties(r, p0, p1, th):
    assert r["num_inliers"] == int(r["inliers"].sum())
    if not r["F"].any():
        assert r["num_inliers"] == 0 and not r["success"]
        return
    F = r["F"]
    assert abs(np.linalg.norm(F) - 1) < 1e-12 and abs(np.linalg.det(F)) <= 1e-12
    assert F.reshape(-1)[int(np.argmax(np.abs(F)))] > 0
    assert r["num_inliers"] >= 7


def test_properties_of_the_table_results():
    """Rank, norm, sign and count on every table result.  The mask is the best RANSAC matrix's and the returned F is refined over it, so
    a point near the threshold may sit on the other side under the returned F: how many entries it reproduces is recorded here, and
    asserted in the next test where no point is near the threshold."""
    cases = fr.ransac_cases() + fr.size_cases()
    res = _tv().fundamental_matrix_batch(cases)
    agree = total = 0
    for (p0, p1, th), r in zip(cases, res):
        _check_properties(r, p0, p1, th)
        if r["F"].any():
            e = _sampson_px(r["F"], p0, p1)
            clear = np.abs(e - th * th) > 1e-3 * th * th
            total += int(clear.sum())
            agree += int(((e <= th * th) == r["inliers"])[clear].sum())
    print(f"mask entries that the returned F reproduces: {agree} of {total}")       # recorded: the mask is the best RANSAC matrix's


def test_mask_is_the_threshold_on_the_returned_matrix_when_every_point_is_an_inlier():
    """Without outliers and with a generous threshold the refined F and the best RANSAC matrix hold the same points: every mask entry
    agrees with e <= th^2 recomputed from the returned F, outside the band."""
    for seed, n in ((801, 40), (802, 300), (803, 1025)):
        _, _, p0, p1, _ = fr.scene(seed, n, 0.0, 0.5)
        r = _tv().fundamental_matrix(p0, p1, 4.0)
        e = _sampson_px(r["F"], p0, p1)
        clear = np.abs(e - 16.0) > fr.BAND * 16.0
        assert r["success"] and ((e <= 16.0) == r["inliers"])[clear].all() and r["num_inliers"] == n
        _check_properties(r, p0, p1, 4.0)


def test_bit_identical_alone_in_the_batch_and_twice():
    cases = fr.size_cases()[:8] + fr.ransac_cases()[20:28]
    T = _tv()
    a, b = T.fundamental_matrix_batch(cases), T.fundamental_matrix_batch(cases)
    rev = T.fundamental_matrix_batch(cases[::-1])[::-1]
    alone = [T.fundamental_matrix_batch([c])[0] for c in cases]
    for other in (b, rev, alone):
        for x, y in zip(a, other):
            assert x["F"].tobytes() == y["F"].tobytes() and np.array_equal(x["inliers"], y["inliers"])
            assert (x["success"], x["num_inliers"], x["num_trials"]) == (y["success"], y["num_inliers"], y["num_trials"])


def test_three_hundred_small_pairs_in_one_call():
    cases = fr.many_cases()
    res = _tv().fundamental_matrix_batch(cases, **fr.MANY_CONF)
    left, worst = 0, [0.0]
    for i, (r, (p0, p1, th)) in enumerate(zip(res, cases)):
        assert len(r["inliers"]) == len(p0)
        _check_properties(r, p0, p1, th)
        if i % 3 == 0:                                      # a third of them against the restatement
            ref = fr.many_ref(i)
            if ref["banded"]:
                left += 1
                continue
            fr.compare(r, ref, worst)
    print(f"300 pairs: {left} of {len(cases) // 3} compared ones left out, worst {worst[0]:.3g}")
    assert left <= len(cases) // 30


def test_errors():
    import ctypes
    from sfd2_amd import _lib
    p = np.random.RandomState(0).uniform(0, 400, (10, 2))
    bad = p.copy()
    bad[3, 1] = np.nan
    ctx = _lib.default_context(0)
    pb = _lib.FundamentalProblem()
    pb.n, pb.points2D_0, pb.points2D_1, pb.max_error_px = 10, bad.ctypes.data, p.ctypes.data, 4.0
    conf = _lib.TwoViewConf(0.25, 0, 100, 0.999, 0, 15, 0)
    res = (_lib.FundamentalResult * 1)()
    mask = np.zeros(10, np.uint8)
    assert ctx.lib.sfd2_fundamental_batch(ctx.h, ctypes.byref(pb), 1, ctypes.byref(conf), res, mask.ctypes.data, 0) == -1
    assert b"non-finite" in ctx.lib.sfd2_last_error()
    pb.points2D_0 = p.ctypes.data
    assert ctx.lib.sfd2_fundamental_batch(ctx.h, ctypes.byref(pb), 1, ctypes.byref(conf), res, mask.ctypes.data, 1) == -1
    with pytest.raises(RuntimeError, match="max_error_px"):
        _tv().fundamental_matrix(p, p + 1, 0.0)
    with pytest.raises(RuntimeError, match="trial limits"):
        _tv().fundamental_matrix(p, p + 1, max_num_trials=0)


# ---------------------------------------------------------------------------------------------------------------- end to end
def _scene():
    return mr.br.cached(("fundamental_gpu_scene",), tr.make_scene)


def _true_rows(sc, a, b, m):
    ga, gb = sc["kp_truth"][a][m[:, 0]], sc["kp_truth"][b][m[:, 1]]
    return (ga >= 0) & (ga == gb)


def test_verification_without_cameras_keeps_what_the_true_cameras_keep():
    """verify_pairs_fundamental keeps at least 0.95 x the true matches verify_pairs_two_view keeps with the true cameras on the same
    pairs.  The share of planted false matches among the survivors is recorded, not bounded: F cannot reject a false match on its
    epipolar line.  Measured on an MI355X: see DESIGN.md 16."""
    T, sc = _tv(), _scene()
    mf, off, cf, rf = T.verify_pairs_fundamental(sc["keypoints"], sc["pair_matches"], 4.0, 15)
    me, off_e, ce, _ = T.verify_pairs_two_view(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], 4.0, 15)
    assert np.array_equal(off, off_e) and len(rf) == len(sc["pair_matches"])
    kept = {"F": [0, 0], "E": [0, 0]}                       # true, false
    for p, (a, b, m) in enumerate(sc["pair_matches"]):
        true = _true_rows(sc, a, b, np.asarray(m))
        for key, mm in (("F", mf), ("E", me)):
            on = mm[off[p]:off[p + 1], 0] >= 0
            assert np.array_equal(mm[off[p]:off[p + 1]][on], np.asarray(m)[on])
            kept[key][0] += int((on & true).sum())
            kept[key][1] += int((on & ~true).sum())
    print(f"true matches kept: F {kept['F'][0]}, E at the true cameras {kept['E'][0]}; false matches among the survivors: "
          f"F {kept['F'][1] / max(sum(kept['F']), 1):.4f}, E {kept['E'][1] / max(sum(kept['E']), 1):.4f}")
    assert kept["F"][0] >= 0.95 * kept["E"][0]
    # the rules of verify_pairs_two_view: negative rows stay rejected, a pair of an image with itself loses everything
    a, b, m = max(sc["pair_matches"], key=lambda pm: len(pm[2]))
    m2 = np.asarray(m).copy()
    m2[::3] = -1
    out, o2, _, _ = T.verify_pairs_fundamental(sc["keypoints"], [(a, b, m2), (a, a, np.asarray(m)[:, [0, 0]])], 4.0, 15)
    assert (out[o2[0]:o2[1]][::3] == -1).all() and (out[o2[0]:o2[1]][:, 0] >= 0).sum() >= 15 and (out[o2[1]:] == -1).all()


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


def test_command_without_intrinsics_writes_a_store_triangulation_reads(tmp_path):
    from sfd2_amd import geometric_verification as gv, triangulation as T
    sc = _scene()
    ref, pairs, feats, matches = _write_inputs(sc, tmp_path)
    res = gv.main(pairs, feats, matches, tmp_path / "verified.h5", model="fundamental", fundamental_matrices=tmp_path / "F.txt")
    name = {i: im.name for i, im in sc["images"].items()}
    assert len(res) == len(sc["pairs"])
    lines = (tmp_path / "F.txt").read_text().splitlines()
    assert len(lines) == len(sc["pairs"])
    for ln, (a, b) in zip(lines, sc["pairs"]):
        f = ln.split()
        r = res[name[a], name[b]]
        assert f[:2] == [name[a], name[b]] and len(f) == 13 and int(f[2]) == int(r["success"]) and int(f[3]) == r["num_inliers"]
        assert np.array_equal(np.array(f[4:], float), r["F"].reshape(-1))
    # the pair's values are fundamental_matrix's on the pair's matches
    a, b, m = sc["pair_matches"][0]
    k0, k1 = sc["keypoints"][a].astype(np.float64) + 0.5, sc["keypoints"][b].astype(np.float64) + 0.5
    assert np.array_equal(_tv().fundamental_matrix(k0[m[:, 0]], k1[m[:, 1]])["F"], res[name[a], name[b]]["F"])
    with pytest.raises(ValueError, match="relative_poses"):
        gv.main(pairs, feats, matches, tmp_path / "x.h5", model="fundamental", relative_poses=tmp_path / "rel.txt")
    stats = T.main(tmp_path / "sfm", ref, tmp_path / "images", pairs, feats, tmp_path / "verified.h5", skip_geometric_verification=True)
    plain = T.main(tmp_path / "sfm_plain", ref, tmp_path / "images", pairs, feats, matches)
    print("triangulation on the store verified without cameras:", stats, "with its own verification:", plain)
    assert stats["num_reg_images"] == 12 and stats["num_sparse_points"] >= 0.9 * plain["num_sparse_points"]


def _registered(call):
    try:
        return len(call()[0])
    except RuntimeError as e:               # no initial pair
        print("reconstruct:", e)
        return 0


def test_reconstruct_at_the_prior_cameras():
    """verification="fundamental" registers at least as many of the 12 images as the default path on the same input, both at COLMAP's
    prior cameras (f = 1.2 max(w, h))."""
    from sfd2_amd import reconstruction as RC
    sc = _scene()
    cams = {i: RC.prior_camera(i, c.width, c.height) for i, c in sc["cameras"].items()}
    n_f = _registered(lambda: RC.reconstruct(cams, sc["images"], sc["keypoints"], sc["pair_matches"], verification="fundamental"))
    n_e = _registered(lambda: RC.reconstruct(cams, sc["images"], sc["keypoints"], sc["pair_matches"]))
    print(f"registered at the prior cameras: fundamental {n_f}, essential {n_e} of 12")
    assert n_f >= n_e


def test_default_reconstruction_is_untouched(tmp_path):
    """reconstruct() with the default keyword writes the bytes of reconstruct(verification="essential"), and never calls the new stage."""
    from sfd2_amd import colmap_io, reconstruction as RC
    sc = _scene()

    class Stages(RC.DeviceStages):
        def fundamental(self, *a, **k):
            raise AssertionError("the default path verified with a fundamental matrix")
    a = RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], stages=Stages())
    b = RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], verification="essential")
    colmap_io.write_model(sc["cameras"], a[0], a[1], tmp_path / "a")
    colmap_io.write_model(sc["cameras"], b[0], b[1], tmp_path / "b")
    for f in ("cameras.bin", "images.bin", "points3D.bin"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    assert len(a[0]) == 12
