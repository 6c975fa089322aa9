"""Absolute pose on the MI355X (sfd2_amd.pose, sfd2_amd.localize.pose_from_clusters) against synthetic scenes and the fp64
helpers of tests/pose_ref.py."""
import numpy as np
import pytest

import pose_ref as pr

pytestmark = pytest.mark.gpu

MODELS = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "OPENCV"]
THRESH = 12.0


def _pose():
    from sfd2_amd import pose
    return pose


def _check_accuracy(r, q, t, X, x, cam, thresh=THRESH):
    assert r["success"]
    assert np.degrees(pr.rot_angle(r["qvec"], q)) <= 0.1
    depth = np.median(X @ pr.qvec2rotmat(q).T[:, 2] + t[2])
    assert np.linalg.norm(pr.centre(r["qvec"], r["tvec"]) - pr.centre(q, t)) <= 0.005 * depth
    assert r["num_inliers"] == int(r["inliers"].sum())
    e = pr.ransac_error(cam, q, t, x, X)
    truth = e <= thresh
    ambiguous = np.abs(e - thresh) <= 0.1 * thresh
    # The mask is the RANSAC winner's (pycolmap's contract), and LO-RANSAC ranks by inlier count as COLMAP does: a sampled pose that
    # keeps one point a little beyond the band outranks its own local optimisation that drops it.  So a few such points are allowed.
    wrong = int((r["inliers"][~ambiguous] != truth[~ambiguous]).sum())
    assert wrong <= max(1, len(e) // 500), wrong


@pytest.mark.parametrize("model", MODELS)
def test_exact_data(model):
    rs = np.random.RandomState(1)
    cam = pr.camera(model)
    q, t, x, X, _ = pr.scene(rs, cam, 200, offset=(300.0, -150.0, 40.0))
    r = _pose().absolute_pose_estimation(x, X, cam, THRESH)
    assert r["success"] and r["inliers"].all() and r["num_inliers"] == 200
    assert pr.rot_angle(r["qvec"], q) <= 1e-6
    assert np.linalg.norm(r["tvec"] - t) <= 1e-6 * np.linalg.norm(t)
    assert abs(np.linalg.norm(r["qvec"]) - 1) < 1e-12 and r["qvec"][0] >= 0


@pytest.mark.parametrize("n", [50, 500, 5000])
@pytest.mark.parametrize("outliers", [0.0, 0.5, 0.8, 0.9])
def test_noisy_data(n, outliers):
    if n * (1 - outliers) < 20:
        pytest.skip("fewer than 20 inliers")
    rs = np.random.RandomState(int(n + 100 * outliers))
    cam = pr.camera("OPENCV")
    q, t, x, X, _ = pr.scene(rs, cam, n, outliers, noise_px=1.0, offset=(250.0, 80.0, -30.0))
    r = _pose().absolute_pose_estimation(x, X, cam, THRESH)
    _check_accuracy(r, q, t, X, x, cam)


def _problems(k, seed=5):
    rs = np.random.RandomState(seed)
    out, truth = [], []
    for i in range(k):
        cam = pr.camera(MODELS[i % 4])
        n = int(rs.randint(20, 600))
        q, t, x, X, _ = pr.scene(rs, cam, n, rs.uniform(0, 0.7), noise_px=1.0)
        out.append((x, X, cam))
        truth.append((q, t))
    return out, truth


def _same(a, b):
    return (a["success"] == b["success"] and np.array_equal(a["qvec"], b["qvec"]) and np.array_equal(a["tvec"], b["tvec"])
            and a["num_inliers"] == b["num_inliers"] and np.array_equal(a["inliers"], b["inliers"]) and a["num_trials"] == b["num_trials"])


def test_determinism():
    P = _pose()
    probs, _ = _problems(64)
    batch = P.absolute_pose_estimation_batch(probs, THRESH)
    single = [P.absolute_pose_estimation(x, X, cam, THRESH) for x, X, cam in probs]
    rev = P.absolute_pose_estimation_batch(probs[::-1], THRESH)[::-1]
    again = P.absolute_pose_estimation_batch(probs, THRESH)
    for i in range(64):
        assert _same(batch[i], single[i]), i
        assert _same(batch[i], rev[i]), i
        assert _same(batch[i], again[i]), i
    assert all(r["success"] for r in batch)


def test_degenerate_cases():
    P = _pose()
    cam = pr.camera("PINHOLE")
    rs = np.random.RandomState(3)
    q, t, x, X, _ = pr.scene(rs, cam, 30)
    r = P.absolute_pose_estimation(x[:3], X[:3], cam, THRESH)
    assert not r["success"] and np.isfinite(r["qvec"]).all() and np.isfinite(r["tvec"]).all() and r["num_inliers"] == 0
    r = P.absolute_pose_estimation(x[:0], X[:0], cam, THRESH)
    assert not r["success"]
    s = np.arange(40, dtype=np.float64)
    Xl = np.stack([s, 2 * s, np.full_like(s, 30.0)], 1)          # exactly collinear
    xl, _ = pr.project(cam, np.array([1.0, 0, 0, 0]), np.array([0.0, 0, 5.0]), Xl)
    r = P.absolute_pose_estimation(xl, Xl, cam, THRESH)
    assert not r["success"] and np.isfinite(r["qvec"]).all() and np.isfinite(r["tvec"]).all()
    bad = x.copy()
    bad[4, 0] = np.nan
    with pytest.raises(ValueError):
        P.absolute_pose_estimation(bad, X, cam, THRESH)
    with pytest.raises(ValueError):
        P.absolute_pose_estimation(x, X, {"model": "FOV", "width": 640, "height": 480, "params": [1, 2, 3, 4, 5]}, THRESH)


@pytest.mark.parametrize("model", ["PINHOLE", "OPENCV"])
def test_pose_refinement(model):
    rs = np.random.RandomState(11)
    cam = pr.camera(model)
    q, t, x, X, out = pr.scene(rs, cam, 300, 0.3, noise_px=1.0, offset=(120.0, 0.0, 60.0))
    mask = ~out
    ax = rs.standard_normal(3)
    ax *= np.radians(1.0) / np.linalg.norm(ax)
    dq = np.concatenate([[np.cos(np.linalg.norm(ax) / 2)], np.sin(np.linalg.norm(ax) / 2) * ax / np.linalg.norm(ax)])
    q0 = pr.rotmat2qvec(pr.qvec2rotmat(dq) @ pr.qvec2rotmat(q))
    depth = np.median(X @ pr.qvec2rotmat(q).T[:, 2] + t[2])
    dc = rs.standard_normal(3)
    C0 = pr.centre(q, t) + 0.01 * depth * dc / np.linalg.norm(dc)   # the camera centre moved by 1 % of the scene depth
    t0 = -pr.qvec2rotmat(q0) @ C0
    r = _pose().pose_refinement(t0, q0, x, X, mask, cam)
    assert r["success"]
    qr, tr = pr.refine_cauchy(cam, q0, t0, x, X, mask, iters=1000)
    assert pr.rot_angle(r["qvec"], qr) <= 1e-6
    assert np.linalg.norm(r["tvec"] - tr) <= 1e-6 * np.linalg.norm(tr)


def test_scale_50x4096():
    rs = np.random.RandomState(21)
    probs, truth = [], []
    for i in range(50):
        cam = pr.camera(MODELS[i % 4])
        q, t, x, X, _ = pr.scene(rs, cam, 4096, 0.8, noise_px=1.0, offset=(rs.uniform(-500, 500), rs.uniform(-500, 500), 20.0))
        probs.append((x, X, cam))
        truth.append((q, t))
    res = _pose().absolute_pose_estimation_batch(probs, THRESH)
    for (x, X, cam), (q, t), r in zip(probs, truth, res):
        _check_accuracy(r, q, t, X, x, cam)


class _Img:
    def __init__(self, name, qvec, tvec, point3D_ids):
        self.name, self.qvec, self.tvec, self.point3D_ids = name, qvec, tvec, point3D_ids


class _Pt:
    def __init__(self, xyz, image_ids):
        self.xyz, self.image_ids = xyz, image_ids


def test_pose_from_clusters_end_to_end():
    from sfd2_amd import localize
    P = _pose()
    rs = np.random.RandomState(31)
    cam = pr.camera("SIMPLE_RADIAL")
    q, t, x, X, out = pr.scene(rs, cam, 600, 0.4, noise_px=1.0, offset=(200.0, 10.0, 0.0))
    points3D = {1000 + i: _Pt(X[i], np.arange(rs.randint(1, 8))) for i in range(len(X))}
    kpq = x - 0.5                                         # the glue adds the +0.5 back
    clusters = []
    for c in range(6):
        cl = []
        for d in range(3):
            m = 800
            ids = np.full(m, -1, dtype=np.int64)
            sel = rs.choice(len(X), 150 if c >= 2 else 3, replace=False)
            slots = rs.choice(m, len(sel), replace=False)
            ids[slots] = 1000 + sel
            matches0 = np.full(len(kpq), -1, dtype=np.int64)
            matches0[sel] = slots
            cl.append((_Img(f"db{c}_{d}.jpg", np.array([1.0, 0, 0, 0]), np.zeros(3), ids), matches0))
        clusters.append(cl)
    got = localize.pose_from_clusters(kpq, clusters, cam, THRESH, points3D=points3D)
    seq = localize.pose_from_clusters(kpq, clusters, cam, THRESH, points3D=points3D,
                                      estimator=lambda probs: [P.absolute_pose_estimation(*p) for p in probs])
    assert np.array_equal(got[0], seq[0]) and np.array_equal(got[1], seq[1]) and got[2] == seq[2]
    assert got[2] > 0
    assert np.degrees(pr.rot_angle(got[0], q)) <= 0.1
    depth = np.median(X @ pr.qvec2rotmat(q).T[:, 2] + t[2])
    assert np.linalg.norm(pr.centre(got[0], got[1]) - pr.centre(q, t)) <= 0.005 * depth


# =====================================================================================================================
# The solver against its restatement (tests/pose_ref.py: sample3, p3p_ref, lo_ransac_ref).  The caps on what these tests may
# leave out (banded cases, left-out probes) are asserted without a GPU in tests/test_pose_ref_host.py.
# =====================================================================================================================
def _centre_error(r, q, t, X):
    """(rotation error in rad, camera-centre error relative to the median depth)."""
    depth = np.median(X @ pr.qvec2rotmat(q).T[:, 2] + t[2])
    return pr.rot_angle(r["qvec"], q), np.linalg.norm(pr.centre(r["qvec"], r["tvec"]) - pr.centre(q, t)) / depth


@pytest.mark.parametrize("family,level", pr.P3P_FAMILIES)
def test_p3p_probe(family, level):
    """One trial per problem (max_num_trials = 1): the sample is sample3(0, 0, n), whose three points have the family's shape.  All n
    exact points are found, and the generating pose with them, if and only if the P3P returned the true root for that triple;
    a lost root leaves the 3 sampled points."""
    probes = pr.p3p_probes(family, level)
    res = _pose().absolute_pose_estimation_batch(probes["problems"], pr.P3P_ERROR_PX, max_num_trials=1)
    failed = []
    for i, (r, (x, X, cam), (q, t)) in enumerate(zip(res, probes["problems"], probes["truth"])):
        assert r["num_trials"] == 1
        rot, cen = _centre_error(r, q, t, X) if r["success"] else (np.inf, np.inf)
        good = r["success"] and r["num_inliers"] == len(x) and r["inliers"].all() and rot <= 1e-6 and cen <= 1e-6
        if probes["kept"][i] and not good:
            failed.append((i, r["num_inliers"], rot, cen, probes["triple"][i]))
    kept = int(probes["kept"].sum())
    print(f"P3P {family} {level:g}: kept {kept}, left out {len(res) - kept}, failed {len(failed)}")
    assert not failed, failed[:5]


@pytest.mark.parametrize("model", sorted(pr.STRONG_CAMERAS))
def test_strong_distortion_to_the_corners(model):
    cam, q, t, x, X = pr.strong_scene(model)
    assert pr.distortion_monotonic(cam)
    r = _pose().absolute_pose_estimation(x, X, cam, THRESH)
    assert r["success"] and r["inliers"].all() and r["num_inliers"] == len(x)
    assert pr.rot_angle(r["qvec"], q) <= 1e-6
    assert np.linalg.norm(r["tvec"] - t) <= 1e-6 * np.linalg.norm(t)
    rs = np.random.RandomState(52)
    ax = rs.standard_normal(3)
    ax /= np.linalg.norm(ax)
    dq = np.concatenate([[np.cos(np.radians(1.0) / 2)], np.sin(np.radians(1.0) / 2) * ax])
    q0 = pr.rotmat2qvec(pr.qvec2rotmat(dq) @ pr.qvec2rotmat(q))
    depth = np.median(X @ pr.qvec2rotmat(q).T[:, 2] + t[2])
    dc = rs.standard_normal(3)
    t0 = -pr.qvec2rotmat(q0) @ (pr.centre(q, t) + 0.01 * depth * dc / np.linalg.norm(dc))
    mask = np.ones(len(x), bool)
    rr = _pose().pose_refinement(t0, q0, x, X, mask, cam)
    qr, tr = pr.refine_cauchy(cam, q0, t0, x, X, mask, iters=1000)
    assert rr["success"]
    assert pr.rot_angle(rr["qvec"], qr) <= 1e-6
    assert np.linalg.norm(rr["tvec"] - tr) <= 1e-6 * np.linalg.norm(tr)


def test_far_world_coordinates():
    """World coordinates ~5e6 from the origin: judged by the rotation and by the camera centre against the median depth (|t| is
    ~5e6 here, so an error relative to it says nothing)."""
    rs = np.random.RandomState(61)
    exact, noisy = [], []
    for model in MODELS:
        cam = pr.camera(model)
        q, t, x, X, _ = pr.scene(rs, cam, 100, offset=pr.FAR_OFFSET)
        exact.append((x, X, cam, q, t))
        q, t, x, X, _ = pr.scene(rs, cam, 150, 0.5, noise_px=1.0, offset=pr.FAR_OFFSET)
        noisy.append((x, X, cam, q, t))
    res = _pose().absolute_pose_estimation_batch([p[:3] for p in exact + noisy], THRESH)
    for (x, X, cam, q, t), r in zip(exact, res[:4]):
        assert r["success"] and r["inliers"].all() and r["num_inliers"] == 100
        rot, cen = _centre_error(r, q, t, X)
        assert rot <= 1e-6 and cen <= 1e-6, (rot, cen)
    for (x, X, cam, q, t), r in zip(noisy, res[4:]):
        _check_accuracy(r, q, t, X, x, cam)


def _agrees(r, ref):
    """The device result equals the restatement's outside the bands; returns the refined pose's deviation (rad, relative t)."""
    assert r["num_trials"] == ref["num_trials"], (r["num_trials"], ref["num_trials"])
    assert r["success"] == ref["success"]
    assert r["num_inliers"] == ref["num_inliers"], (r["num_inliers"], ref["num_inliers"])
    assert r["num_inliers"] == int(r["inliers"].sum())
    free = ~ref["point_banded"]
    assert np.array_equal(r["inliers"][free], ref["inliers"][free])
    if not ref["success"]:
        return 0.0, 0.0
    dev = (pr.rot_angle(r["qvec"], ref["qvec_refined"]), np.linalg.norm(r["tvec"] - ref["tvec_refined"]) / np.linalg.norm(ref["tvec_refined"]))
    assert dev[0] <= 1e-6 and dev[1] <= 1e-6, dev
    return dev


def test_ransac_equals_restatement():
    """num_trials, num_inliers, the mask and the refined pose of 16 problems (n = 12 / 40 / 80; 1, 4 and 14+ rounds; thresholds 12
    and 3 px; the four camera models) against lo_ransac_ref + refine_cauchy, in one launch."""
    cases, refs = pr.ransac_cases(), pr.ransac_refs()
    res = _pose().absolute_pose_estimation_batch([(x, X, cam, th) for x, X, cam, _, _, th in cases], THRESH, **pr.RANSAC_CONF)
    banded = [i for i, ref in enumerate(refs) if ref["banded"]]
    worst = (0.0, 0.0)
    for i, (r, ref) in enumerate(zip(res, refs)):
        print(f"case {i} {pr.RANSAC_CASES[i]}: trials {r['num_trials']} / {ref['num_trials']}, inliers {r['num_inliers']} / {ref['num_inliers']}"
              f"{' (banded: ' + ref['why'][0] + ')' if ref['banded'] else ''}")
    for i, (r, ref) in enumerate(zip(res, refs)):
        if i in banded:
            continue
        dev = _agrees(r, ref)
        worst = (max(worst[0], dev[0]), max(worst[1], dev[1]))
    print(f"banded share {len(banded)} / {len(refs)}; largest pose deviation {worst[0]:.2e} rad, {worst[1]:.2e} of |t|")
    assert len(banded) <= 0.10 * len(refs)


@pytest.mark.parametrize("run", range(len(pr.OPTION_RUNS)))
def test_options_equal_restatement(run):
    """seed, max_num_trials (not a multiple of the round), min_num_trials, confidence and the min_inlier_ratio limit, each against
    the restatement run with the same options."""
    kind, conf = pr.OPTION_RUNS[run]
    x, X, cam, _, _ = pr.option_problem(kind)
    ref = pr.option_ref(kind, **conf)
    r = _pose().absolute_pose_estimation(x, X, cam, pr.OPTION_THRESH, **conf)
    print(f"{kind} {conf}: trials {r['num_trials']} / {ref['num_trials']}, inliers {r['num_inliers']} / {ref['num_inliers']}, banded {ref['banded']}")
    lo, hi = pr.trial_limits(conf.get("min_inlier_ratio", 0.01), conf.get("min_num_trials", 1000), conf.get("max_num_trials", 100000),
                             conf.get("confidence", 0.9999))
    assert lo <= r["num_trials"] <= hi and (r["num_trials"] % 256 == 0 or r["num_trials"] == hi)
    want = {(("max_num_trials", 300),): 300, (("min_num_trials", 2000),): 2048, (("confidence", 1.0), ("max_num_trials", 600)): 600,
            (("confidence", 0.99), ("min_inlier_ratio", 0.5)): 104}.get(tuple(sorted(conf.items())))
    if want is not None:
        assert r["num_trials"] == want
    if "confidence" in conf and conf["confidence"] < 1 and "min_inlier_ratio" not in conf:     # the formula, on the reported count
        assert r["num_trials"] >= pr.num_trials_needed(r["num_inliers"] / len(x), conf["confidence"])
    assert not ref["banded"], ref["why"]          # (tests/test_pose_ref_host.py asserts it for the committed scenes)
    _agrees(r, ref)


def test_seeds_differ():
    x, X, cam, _, _ = pr.option_problem("half")
    res = [_pose().absolute_pose_estimation(x, X, cam, pr.OPTION_THRESH, seed=s) for s in (1, 2, 3)]
    assert all(r["success"] for r in res)
    assert not _same(res[0], res[1]) and not _same(res[0], res[2]) and not _same(res[1], res[2])
    assert _same(res[0], _pose().absolute_pose_estimation(x, X, cam, pr.OPTION_THRESH, seed=1))
    conf_sweep = [_pose().absolute_pose_estimation(*pr.option_problem("third")[:3], pr.OPTION_THRESH, min_num_trials=0, confidence=c)["num_trials"]
                  for c in (0.5, 0.99, 0.999999)]
    assert conf_sweep[0] < conf_sweep[1] < conf_sweep[2], conf_sweep


def test_option_ranges_and_tiny_problems():
    P = _pose()
    x, X, cam, _, _ = pr.option_problem("half")
    for bad in (dict(confidence=1.5), dict(max_num_trials=0), dict(min_num_trials=-1), dict(max_error_px=0.0), dict(min_inlier_ratio=-0.1)):
        with pytest.raises(RuntimeError):
            P.absolute_pose_estimation(x, X, cam, **{"max_error_px": pr.OPTION_THRESH, **bad})
    r = P.absolute_pose_estimation(x[:3], X[:3], cam, THRESH)
    assert r["num_trials"] == 0 and not r["success"] and r["num_inliers"] == 0 and not r["inliers"].any() and len(r["inliers"]) == 3
    q, t, xe, Xe, _ = pr.scene(np.random.RandomState(71), cam, 4)
    r = P.absolute_pose_estimation(xe, Xe, cam, THRESH)
    assert r["success"] and r["num_inliers"] == 4 and r["inliers"].all()
    rot, cen = _centre_error(r, q, t, Xe)
    assert rot <= 1e-6 and cen <= 1e-6, (rot, cen)
    ref = pr.lo_ransac_ref(xe, Xe, cam, THRESH)
    assert r["num_trials"] == ref["num_trials"] == 1024


def test_pose_refinement_degenerate_masks():
    x, X, cam, q, t = pr.option_problem("half")
    two = np.zeros(len(x), bool)
    two[[3, 17]] = True
    for mask in (np.zeros(len(x), bool), two):
        r = _pose().pose_refinement(t, q, x, X, mask, cam)
        assert not r["success"]
        assert np.isfinite(r["qvec"]).all() and np.isfinite(r["tvec"]).all()


@pytest.mark.parametrize("empty_at", [0, 1])
def test_an_empty_problem_beside_a_full_one(empty_at):
    """k = 2, one problem of n = 0 beside one of n = 8 (an empty array takes a slot of the packed input all the same): the empty one
    fails, the other is what it is alone and what the restatement gives -- estimation and refinement."""
    P = _pose()
    cam = pr.camera("PINHOLE")
    q, t, x, X, _ = pr.scene(np.random.RandomState(72), cam, 8)
    full = 1 - empty_at
    probs = [None, None]
    probs[empty_at], probs[full] = (x[:0], X[:0], cam), (x, X, cam)
    res = P.absolute_pose_estimation_batch(probs, THRESH)
    assert not res[empty_at]["success"] and res[empty_at]["num_inliers"] == 0 and len(res[empty_at]["inliers"]) == 0
    assert np.isfinite(res[empty_at]["qvec"]).all() and np.isfinite(res[empty_at]["tvec"]).all()
    assert _same(res[full], P.absolute_pose_estimation(x, X, cam, THRESH))
    ref = pr.absolute_pose_ref(x, X, cam, THRESH)
    assert not ref["banded"] and ref["success"] and ref["num_inliers"] == 8
    _agrees(res[full], ref)
    mask = np.ones(8, bool)
    probs[empty_at], probs[full] = (t, q, x[:0], X[:0], mask[:0], cam), (t, q, x, X, mask, cam)
    res = P.pose_refinement_batch(probs)
    assert not res[empty_at]["success"]
    alone = P.pose_refinement(t, q, x, X, mask, cam)
    assert res[full]["success"] and np.array_equal(res[full]["qvec"], alone["qvec"]) and np.array_equal(res[full]["tvec"], alone["tvec"])
    qr, tr = pr.refine_cauchy(cam, q, t, x, X, mask, iters=1000)
    assert pr.rot_angle(res[full]["qvec"], qr) <= 1e-6 and np.linalg.norm(res[full]["tvec"] - tr) <= 1e-6 * np.linalg.norm(tr)
