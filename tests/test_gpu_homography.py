"""Homography and the E / F / H decision on the MI355X (sfd2_amd.two_view.homography*, verify_pairs_homography, two_view_geometry_batch,
verify_pairs_geometry) against the restatement of tests/homography_ref.py: the RANSAC table, the option runs, the stride seams, the
solver probes, degenerate inputs (trials, count and mask equal; H within homography_ref.H_TOL), batch independence, the decision on
five synthetic pairs, and the two commands end to end on a scene with a planar and a rotation-only pair."""
import numpy as np
import pytest

import homography_ref as hr
import mapper_ref as mr
import pose_ref as pr
import tri_ref as tr

pytestmark = pytest.mark.gpu


def _tv():
    from sfd2_amd import two_view
    return two_view


def _run_table(name, cases, refs, **conf):
    """One batch against its restatement; returns the device results."""
    res = _tv().homography_batch(cases, **conf)
    left, worst = 0, [0.0]
    for r, ref in zip(res, refs):
        if ref["banded"]:
            left += 1
            continue
        hr.compare(r, ref, worst)
    print(f"{name}: {left} of {len(cases)} left out, worst distance of the matrices {worst[0]:.3g} (tolerance {hr.H_TOL:.3g})")
    assert left <= len(cases) // 10
    return res


# ---------------------------------------------------------------------------------------------------------------- against the restatement
def test_ransac_table_against_the_restatement():
    """n = 4, 5, 8, 40, 80, 300 x outliers 0 / 0.25 / 0.5 / 0.7 x thresholds 4 and 1 px, 0.5 px noise."""
    res = _run_table("RANSAC table", hr.ransac_cases(), hr.ransac_refs())
    for (n, _, _, _), ref in zip(hr.RANSAC_CASES, hr.ransac_refs()):
        if n in (4, 5):
            assert not ref["banded"]
    assert {r["num_trials"] for r in res} >= {256, 512, 2560, 5295}


def test_option_runs_against_the_restatement():
    p0, p1, th = hr.option_case()
    left, worst, trials = 0, [0.0], set()
    for conf in hr.OPTION_RUNS:
        ref = hr.option_ref(**conf)
        r = _tv().homography(p0, p1, th, **conf)
        trials.add(r["num_trials"])
        if ref["banded"]:
            left += 1
            continue
        hr.compare(r, ref, worst)
    print(f"option runs: {left} of {len(hr.OPTION_RUNS)} left out, worst {worst[0]:.3g}, trial counts {sorted(trials)}")
    assert left <= len(hr.OPTION_RUNS) // 10 and trials >= {1, 255, 256, 257, 512, 600}
    # a seed is 64 bits without a sign
    a, b = _tv().homography(p0, p1, th, seed=-1), _tv().homography(p0, p1, th, seed=2 ** 64 - 1)
    assert a["H"].tobytes() == b["H"].tobytes() and np.array_equal(a["inliers"], b["inliers"]) and a["num_trials"] == b["num_trials"]


def test_stride_seams_in_one_batch():
    """n = 255, 256, 257, 511, 513, 1025 between pairs of 0, 3 and 4 correspondences."""
    res = _run_table("stride seams", hr.size_cases(), hr.size_refs())
    for (p0, _, _), r in zip(hr.size_cases(), res):
        assert len(r["inliers"]) == len(p0)
        if len(p0) < 4:
            assert not r["success"] and r["num_trials"] == 0 and not r["H"].any() and not r["inliers"].any()


def _signed(H):
    H = H / np.linalg.norm(H)
    return H if H.reshape(-1)[int(np.argmax(np.abs(H)))] > 0 else -H


@pytest.mark.parametrize("family", hr.PROBE_FAMILIES)
def test_solver_probes(family):
    """One trial on 5 or 6 exact correspondences: what the device returns for the sample is what the restatement returns, and the
    generating matrix holds every point wherever the restatement says the sample yields it."""
    ps, refs = hr.probes(family), hr.probe_refs(family)
    res = _run_table("probes " + family, [(p0, p1, th) for p0, p1, _, th in ps], refs, **hr.PROBE_CONF)
    assert all(r["num_trials"] == 1 for r in res)
    found = sum(bool(r["inliers"].all()) and np.linalg.norm(r["H"] - _signed(H)) < 1e-6 for r, (_, _, H, _) in zip(res, ps))
    print(f"{family}: the generating matrix found in {found} of {len(ps)}")
    assert found >= hr.probe_disagreement(family)[1] - len(ps) // 10


@pytest.mark.parametrize("name", sorted(hr.DEGENERATE))
def test_degenerate_inputs_give_no_result(name):
    p0, p1 = hr.degenerate(name)
    ref = hr.degenerate_ref(name)
    r = _tv().homography(p0, p1, 4.0, **hr.DEGENERATE[name])
    assert not ref["success"] and ref["num_inliers"] == 0 and not ref["H"].any() and not ref["inliers"].any()
    assert (r["success"], r["num_inliers"], r["num_trials"]) == (False, 0, ref["num_trials"])
    assert not r["H"].any() and not r["inliers"].any() and len(r["inliers"]) == len(p0)


# ---------------------------------------------------------------------------------------------------------------- properties
def test_properties_and_verify_pairs():
    cases = hr.ransac_cases() + hr.size_cases()
    for (p0, p1, th), r in zip(cases, _tv().homography_batch(cases)):
        assert r["num_inliers"] == int(r["inliers"].sum())
        if not r["H"].any():
            assert r["num_inliers"] == 0 and not r["success"]
            continue
        H = r["H"]
        assert abs(np.linalg.norm(H) - 1) < 1e-12 and H.reshape(-1)[int(np.argmax(np.abs(H)))] > 0 and r["num_inliers"] >= 4
    # verify_pairs_homography on key points as a feature store holds them (float32, without COLMAP's +0.5)
    _, p0, p1, out = hr.scene(990, 200, 0.3, 0.5)
    kp = {0: (p0 - 0.5).astype(np.float32), 1: (p1 - 0.5).astype(np.float32)}
    m = np.stack([np.arange(200), np.arange(200)], 1)
    m2 = m.copy()
    m2[::4] = -1
    res, off, counts, rr = _tv().verify_pairs_homography(kp, [(0, 1, m), (0, 1, m2), (0, 0, m), (0, 1, m[:10])], 4.0, 15)
    assert off.tolist() == [0, 200, 400, 600, 610] and len(rr) == 4
    kept = res[:200, 0] >= 0
    assert counts[0] == kept.sum() >= 0.95 * (~out).sum() and not (kept & out).sum() > 3 and np.array_equal(res[:200][kept], m[kept])
    assert (res[200:400][::4] == -1).all() and (res[200:400, 0] >= 0).sum() >= 15
    assert (res[400:] == -1).all() and counts[2] == 0 and not rr[3]["success"]


def test_bit_identical_alone_in_the_batch_and_twice():
    cases = hr.size_cases()[:8] + hr.ransac_cases()[20:32]
    T = _tv()
    a, b = T.homography_batch(cases), T.homography_batch(cases)
    rev = T.homography_batch(cases[::-1])[::-1]
    alone = [T.homography_batch([c])[0] for c in cases]
    for other in (b, rev, alone):
        for x, y in zip(a, other):
            assert x["H"].tobytes() == y["H"].tobytes() and np.array_equal(x["inliers"], y["inliers"])
            assert (x["success"], x["num_inliers"], x["num_trials"]) == (y["success"], y["num_inliers"], y["num_trials"])


def test_errors():
    import ctypes
    from sfd2_amd import _lib
    p = np.random.RandomState(0).uniform(0, 400, (10, 2))
    bad = p.copy()
    bad[3, 1] = np.nan
    ctx = _lib.default_context(0)
    pb = _lib.HomographyProblem()
    pb.n, pb.points2D_0, pb.points2D_1, pb.max_error_px = 10, bad.ctypes.data, p.ctypes.data, 4.0
    conf = _lib.TwoViewConf(0.25, 0, 100, 0.999, 0, 15, 0)
    res = (_lib.HomographyResult * 1)()
    mask = np.zeros(10, np.uint8)
    assert ctx.lib.sfd2_homography_batch(ctx.h, ctypes.byref(pb), 1, ctypes.byref(conf), res, mask.ctypes.data, 0) == -1
    assert b"sfd2_homography_batch" in ctx.lib.sfd2_last_error() and b"non-finite" in ctx.lib.sfd2_last_error()
    pb.points2D_0 = p.ctypes.data
    assert ctx.lib.sfd2_homography_batch(ctx.h, ctypes.byref(pb), 1, ctypes.byref(conf), res, mask.ctypes.data, 1) == -1
    with pytest.raises(RuntimeError, match="max_error_px"):
        _tv().homography(p, p + 1, 0.0)
    with pytest.raises(RuntimeError, match="trial limits"):
        _tv().homography(p, p + 1, max_num_trials=0)


# ---------------------------------------------------------------------------------------------------------------- the decision
def test_decision_on_five_pairs_with_and_without_cameras():
    """The three device calls give the restatements' counts (none of the fifteen is left out), so the rule gives the expected configs."""
    T = _tv()
    scenes = [hr.decision_scene(name) for name in hr.DECISION_SCENES]
    probs = [(p0, p1) for p0, p1, _, _ in scenes]
    with_cams = T.two_view_geometry_batch(probs, [(c0, c1) for _, _, c0, c1 in scenes])
    without = T.two_view_geometry_batch(probs)
    for name, a, b in zip(hr.DECISION_SCENES, with_cams, without):
        E, F, H = hr.decision_refs(name)
        assert not (E["banded"] or F["banded"] or H["banded"])
        print(name, a["config"], b["config"], a["E"]["num_inliers"], a["F"]["num_inliers"], a["H"]["num_inliers"], a["num_inliers"], b["num_inliers"])
        assert (a["E"]["num_inliers"], a["F"]["num_inliers"], a["H"]["num_inliers"]) == (E["num_inliers"], F["num_inliers"], H["num_inliers"])
        assert a["E"]["success"] == E["success"] and a["E"]["small_baseline"] == E["small_baseline"] and b["E"] is None
        assert (a["config"], b["config"]) == hr.DECISION_EXPECT[name]
        assert b["F"]["F"].tobytes() == a["F"]["F"].tobytes() and b["H"]["H"].tobytes() == a["H"]["H"].tobytes()
        for d in (a, b):
            assert d["num_inliers"] == int(d["inliers"].sum()) and len(d["inliers"]) == hr.DECISION_N
            want = T.decide_two_view_geometry(d["E"], d["F"], d["H"])
            assert want["config"] == d["config"] and want["model"] == d["model"] and np.array_equal(want["inliers"], d["inliers"])
        if name == "random":
            assert a["num_inliers"] == b["num_inliers"] == 0 and a["model"] is None
        else:
            assert a["num_inliers"] >= 285 and b["num_inliers"] >= 285


# ---------------------------------------------------------------------------------------------------------------- end to end
N_PLANE = 300


def _observe(rs, cam, im, X, ids, n_clutter=60, noise_px=1.0):
    """Key points of one image as tri_ref.make_scene makes them: noisy projections of the visible points plus clutter, shuffled."""
    px, z = pr.project(cam, im.qvec, im.tvec, X)
    vis = (z > 0) & (px[:, 0] > 5) & (px[:, 0] < cam["width"] - 5) & (px[:, 1] > 5) & (px[:, 1] < cam["height"] - 5)
    idx = np.nonzero(vis)[0]
    allp = np.concatenate([px[idx] + noise_px * rs.standard_normal((len(idx), 2)),
                           np.stack([rs.uniform(0, cam["width"], n_clutter), rs.uniform(0, cam["height"], n_clutter)], 1)])
    truth = np.concatenate([ids[idx], np.full(n_clutter, -1)])
    perm = rs.permutation(len(allp))
    return (allp[perm] - 0.5).astype(np.float32), truth[perm]


def _match(rs, t0, t1, false_share=0.3):
    """The true matches of two key-point tables and a share of random false ones."""
    where1 = {int(g): k for k, g in enumerate(t1) if g >= 0}
    rows = [(k0, where1[int(g)]) for k0, g in enumerate(t0) if g >= 0 and int(g) in where1]
    used0, used1 = {r[0] for r in rows}, {r[1] for r in rows}
    for _ in range(int(round(false_share * len(rows)))):
        k0, k1 = int(rs.randint(len(t0))), int(rs.randint(len(t1)))
        if k0 in used0 or k1 in used1 or (t0[k0] >= 0 and t0[k0] == t1[k1]):
            continue
        rows.append((k0, k1))
        used0.add(k0)
        used1.add(k1)
    return np.array(sorted(rows), dtype=np.int32)


def _make_scene():
    """tri_ref.make_scene's 12 images, and: image 13 at image 1's centre, turned by 8 degrees (a rotation-only pair 1-13); images 14 and
    15 far from the others in front of a plane of N_PLANE points of their own (a planar pair 14-15)."""
    sc = dict(tr.make_scene())
    rs = np.random.RandomState(77)
    cams, images = sc["cameras"], dict(sc["images"])
    keypoints, truth = dict(sc["keypoints"]), dict(sc["kp_truth"])
    X = np.asarray(sc["X"])
    n_x = len(X)
    im1 = images[1]
    R1 = pr.qvec2rotmat(im1.qvec)
    c1 = -R1.T @ np.asarray(im1.tvec)
    R = hr.tv._exp_so3(np.radians(8.0) * np.array([[0.2, 0.97, 0.1]]))[0] @ R1
    images[13] = tr.Img(13, pr.rotmat2qvec(R), -R @ c1, im1.camera_id, "db/rot.jpg")
    # the rotated image sees the points image 1 sees, from the same centre
    keypoints[13], truth[13] = _observe(rs, cams[im1.camera_id], images[13], X, np.arange(n_x))
    # the plane z = 9 + 0.3 x - 0.2 y around (0, 200, 0)
    P = np.stack([rs.uniform(-4, 4, N_PLANE), 200 + rs.uniform(-3, 3, N_PLANE), np.zeros(N_PLANE)], 1)
    P[:, 2] = 9 + 0.3 * P[:, 0] - 0.2 * (P[:, 1] - 200)
    for iid, c in ((14, np.array([-0.8, 200.0, 0.0])), (15, np.array([0.9, 200.3, 0.2]))):
        q, t = tr._look_at(c, np.array([0.0, 200.0, 9.0]), 0.02 * (iid - 14))
        images[iid] = tr.Img(iid, q, t, 2, f"db/plane{iid}.jpg")
        keypoints[iid], truth[iid] = _observe(rs, cams[2], images[iid], P, n_x + np.arange(N_PLANE))
    extra = [(1, 13, _match(rs, truth[1], truth[13])), (14, 15, _match(rs, truth[14], truth[15]))]
    sc.update(images=images, keypoints=keypoints, kp_truth=truth, pairs=list(sc["pairs"]) + [(1, 13), (14, 15)],
              pair_matches=list(sc["pair_matches"]) + extra)
    return sc


def _scene():
    return mr.br.cached(("homography_gpu_scene",), _make_scene)


def _true_rows(sc, a, b, m):
    ga, gb = sc["kp_truth"][a][m[:, 0]], sc["kp_truth"][b][m[:, 1]]
    return (ga >= 0) & (ga == gb)


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


def test_geometry_command_writes_a_store_triangulation_reads(tmp_path):
    """--model geometry with and without intrinsics: one line per pair in --two_view_geometries, the planar and the rotation-only pair keep
    their true matches (what --model fundamental keeps of them is recorded), and triangulation reads the store."""
    from sfd2_amd import feature_io, geometric_verification as gv, triangulation as T
    from sfd2_amd.match_features import names_to_pair
    sc = _scene()
    ref, pairs, feats, matches = _write_inputs(sc, tmp_path)
    name = {i: im.name for i, im in sc["images"].items()}
    res = gv.main(pairs, feats, matches, tmp_path / "verified.h5", reference_sfm_model=ref, model="geometry", two_view_geometries=tmp_path / "T.txt")
    bare = gv.main(pairs, feats, matches, tmp_path / "bare.h5", model="geometry", two_view_geometries=tmp_path / "T0.txt")
    fund = gv.main(pairs, feats, matches, tmp_path / "fund.h5", model="fundamental")
    lines = (tmp_path / "T.txt").read_text().splitlines()
    assert len(res) == len(bare) == len(lines) == len(sc["pairs"])
    for ln, (a, b) in zip(lines, sc["pairs"]):
        f, r = ln.split(), res[name[a], name[b]]
        assert f == [name[a], name[b], r["config"], str(r["E"]["num_inliers"]), str(r["F"]["num_inliers"]), str(r["H"]["num_inliers"]), str(r["num_inliers"])]
    assert all(ln.split()[3] == "-1" for ln in (tmp_path / "T0.txt").read_text().splitlines())
    configs = [r["config"] for r in res.values()]
    print("configs with intrinsics:", {c: configs.count(c) for c in set(configs)}, "without:",
          {c: [r["config"] for r in bare.values()].count(c) for c in set(r["config"] for r in bare.values())})
    assert res[name[14], name[15]]["config"] == "planar" and res[name[1], name[13]]["config"] == "panoramic"
    assert bare[name[14], name[15]]["config"] == bare[name[1], name[13]]["config"] == "planar_or_panoramic"
    stores = {k: feature_io.open_store(str(tmp_path / f), "r") for k, f in (("geometry", "verified.h5"), ("bare", "bare.h5"), ("fundamental", "fund.h5"))}
    try:
        for a, b, m in sc["pair_matches"][-2:]:
            true = _true_rows(sc, a, b, m)
            kept = {}
            for k, st in stores.items():
                m0 = np.asarray(st[names_to_pair(name[a], name[b])]["matches0"].__array__()).reshape(-1)
                on = m0[m[:, 0]] == m[:, 1]
                kept[k] = (int((on & true).sum()), int((on & ~true).sum()))
            print(f"pair {name[a]} {name[b]}: {int(true.sum())} true and {int((~true).sum())} false matches; kept (true, false):", kept)
            assert kept["geometry"][0] >= 0.95 * true.sum() and kept["bare"][0] >= 0.95 * true.sum()
            assert kept["geometry"][1] <= 0.1 * (~true).sum() + 2 and kept["bare"][1] <= 0.1 * (~true).sum() + 2
    finally:
        for st in stores.values():
            st.close()
    with pytest.raises(ValueError, match="two_view_geometries"):
        gv.main(pairs, feats, matches, tmp_path / "x.h5", model="fundamental", two_view_geometries=tmp_path / "x.txt")
    stats = T.main(tmp_path / "sfm", ref, tmp_path / "images", pairs, feats, tmp_path / "verified.h5", skip_geometric_verification=True)
    print("triangulation on the store verified by the decision:", stats)
    assert stats["num_reg_images"] == 15 and stats["num_sparse_points"] > 0


def test_reconstruct_with_the_decision():
    """verification="geometry" registers the 12 images of the scene; the rotation-only pair, whose 248 matches put it among the
    init_max_pairs pairs that get a relative pose (the test asserts that it would be offered without the bar), is labelled panoramic and
    is not offered as the initial pair."""
    from sfd2_amd import reconstruction as RC
    sc = _scene()
    keep = [p for p, (a, b) in enumerate(sc["pairs"]) if max(a, b) <= 13]
    pm = [sc["pair_matches"][p] for p in keep]
    images = {i: im for i, im in sc["images"].items() if i <= 13}
    rot = next(k for k, (a, b, _) in enumerate(pm) if (a, b) == (1, 13))
    offered = []

    class Stages(RC.DeviceStages):
        def two_view(self, cameras, images_, keypoints, pair_matches, *a, **k):
            offered.extend((x, y) for x, y, _ in pair_matches)
            return super().two_view(cameras, images_, keypoints, pair_matches, *a, **k)
    sizes = sorted((len(m) for _, _, m in pm), reverse=True)
    assert len(pm[rot][2]) >= sizes[min(RC.DEFAULTS["init_max_pairs"], len(sizes)) - 1]
    report = {}
    out_images, _ = RC.reconstruct(sc["cameras"], images, sc["keypoints"], pm, verification="geometry", stages=Stages(), report=report)
    names = {im.name for im in out_images.values()}
    print("registered:", len(names), "initial pair:", report["initial_pair"], "config of the rotation-only pair:", report["two_view_configs"][rot])
    assert names >= {f"db/img{i:03d}.jpg" for i in range(12)}
    assert report["two_view_configs"][rot] == "panoramic" and (1, 13) not in offered and offered
    assert set(report["initial_pair"]) != {1, 13}
    with pytest.raises(ValueError, match="unknown verification"):
        RC.reconstruct(sc["cameras"], images, sc["keypoints"], pm, verification="homography")
