"""The restatement of the pose solver (tests/pose_ref.py: p3p_ref, score_f32, lo_ransac_ref; its sampling is checked with the other
estimators' in tests/test_ransac_ref_host.py) checked on its own,
without a GPU and without the library: against generating poses, closed-form trial counts and its own deliberately broken
variants.  The caps on what the GPU tests of tests/test_gpu_pose.py may leave out are asserted here, on the committed seeds."""
import numpy as np
import pytest

import pose_ref as pr
from test_gpu_pose import _check_accuracy


def test_undistort_is_converged_and_jacobian_is_right():
    rs = np.random.RandomState(0)
    cams = [pr.camera(m) for m in pr.MODELS] + [pr.strong_scene(m)[0] for m in pr.STRONG_CAMERAS]
    for cam in cams:
        assert pr.distortion_monotonic(cam)
        px = np.stack([rs.uniform(0, 640, 500), rs.uniform(0, 480, 500)], 1)
        px[:4] = [[0, 0], [640, 0], [0, 480], [640, 480]]
        uv = pr.undistort(cam, px)
        fx, fy, cx, cy = pr._opencv(cam)[:4]
        ud, vd = pr.distort(cam, uv[:, 0], uv[:, 1])
        assert np.abs(fx * ud + cx - px[:, 0]).max() <= 1e-10 and np.abs(fy * vd + cy - px[:, 1]).max() <= 1e-10
        h = 1e-6
        j = pr.distort_jacobian(cam, uv[:, 0], uv[:, 1])
        au, av = pr.distort(cam, uv[:, 0] + h, uv[:, 1])
        bu, bv = pr.distort(cam, uv[:, 0] - h, uv[:, 1])
        cu, cv = pr.distort(cam, uv[:, 0], uv[:, 1] + h)
        du, dv = pr.distort(cam, uv[:, 0], uv[:, 1] - h)
        for got, want in zip(j, ((au - bu) / (2 * h), (cu - du) / (2 * h), (av - bv) / (2 * h), (cv - dv) / (2 * h))):
            assert np.abs(got - want).max() <= 1e-9
    bad = {"model": "SIMPLE_RADIAL", "width": 640, "height": 480, "params": [400.0, 320.0, 240.0, -0.6]}   # folds inside the image
    assert not pr.distortion_monotonic(bad)


def test_p3p_ref_contains_the_generating_pose():
    rs = np.random.RandomState(0)
    T = 2000
    ys, Xs, truth = [], [], []
    for i in range(T):
        cam = pr.camera(pr.MODELS[i % 4])
        q, t, x, X, _ = pr.scene(rs, cam, 3)
        yb = np.concatenate([pr.undistort(cam, x), np.ones((3, 1))], 1)
        ys.append(yb / np.linalg.norm(yb, axis=1, keepdims=True))
        Xs.append(X)
        truth.append((pr.qvec2rotmat(q), t))
    ys, Xs = np.array(ys), np.array(Xs)
    sol = pr.p3p_ref(ys, Xs)
    assert sol["valid"].any(1).all()
    worst = 0.0
    for i, (R, t) in enumerate(truth):
        ang = [np.arccos(np.clip((np.trace(sol["R"][i, k] @ R.T) - 1) / 2, -1, 1)) if sol["valid"][i, k] else np.inf for k in range(4)]
        k = int(np.argmin(ang))
        # arccos near 1 resolves 1e-8 at best; the Frobenius distance bounds the angle from above
        assert np.linalg.norm(sol["R"][i, k] - R) <= 1e-9, (i, ang)
        worst = max(worst, np.linalg.norm(sol["R"][i, k] - R))
    V = sol["valid"]
    R, t = sol["R"][V], sol["t"][V]
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= 1e-12
    assert np.abs(np.linalg.det(R) - 1).max() <= 1e-12
    ti, _ = np.nonzero(V)
    P = np.einsum("mij,mkj->mki", R, Xs[ti]) + t[:, None, :]
    assert (P[:, :, 2] > 0).all()
    assert np.abs(P / np.linalg.norm(P, axis=2, keepdims=True) - ys[ti]).max() <= 1e-10
    assert set(np.unique(V.sum(1))) >= {1, 2, 4}                    # the multi-solution samples are exercised
    print(f"p3p_ref: worst |R - R_true| {worst:.2e}, solutions per sample {np.bincount(V.sum(1), minlength=5).tolist()}")


def test_p3p_ref_rejects_degenerate_samples():
    y = np.array([[[0.1, 0, 1], [0, 0.1, 1], [-0.1, 0, 1.0]]])
    y /= np.linalg.norm(y, axis=2, keepdims=True)
    Xl = np.array([[[0.0, 0, 5], [1, 2, 5], [2, 4, 5.0]]])          # collinear 3D points
    assert not pr.p3p_ref(y, Xl)["valid"].any()
    yc = np.array([[[0.1, 0, 1], [0.2, 0, 1], [-0.1, 0, 1.0]]])      # coplanar bearings
    yc /= np.linalg.norm(yc, axis=2, keepdims=True)
    assert not pr.p3p_ref(yc, np.array([[[0.0, 0, 5], [1, 0, 6], [0, 1, 7.0]]]))["valid"].any()


def test_score_f32_counts_sums_and_bands():
    X = np.array([[0.0, 0, 4], [1, 0, 4], [0, 1, -4], [0.5, 0.5, 2]])
    xn = np.array([[0.0, 0.0], [0.25 + 0.01, 0.0], [0.0, -0.25], [0.25, 0.25 + 0.02 * (1 + 0.4 * pr.BAND)]])
    cnt, sm, inl, bnd = pr.score_f32((np.eye(3), np.zeros(3)), X, xn, 0.02 ** 2)
    assert inl.tolist() == [True, True, False, False] and cnt == 2       # behind the camera; just outside the threshold
    assert bnd.tolist() == [False, False, False, True]
    assert sm.dtype == np.float32 and abs(float(sm) - 1e-4) <= 1e-9
    cnt2, sm2, _, _ = pr.score_f32((np.tile(np.eye(3), (5, 1, 1)), np.zeros((5, 3))), X, xn, 0.02 ** 2, "tree")
    assert cnt2.tolist() == [2] * 5 and np.allclose(sm2, sm, rtol=1e-6)


def test_lo_ransac_ref_is_accurate_on_every_committed_scene():
    for (x, X, cam, q, t, th), r in zip(pr.ransac_cases(), pr.ransac_refs()):
        _check_accuracy({**r, "qvec": r["qvec_refined"], "tvec": r["tvec_refined"]}, q, t, X, x, cam, th)
    for kind, conf in pr.OPTION_RUNS:
        x, X, cam, q, t = pr.option_problem(kind)
        r = pr.option_ref(kind, **conf)
        if kind != "tenth":                      # 4 inliers of 40 in 104 trials: that run is about the trial limit only
            _check_accuracy({**r, "qvec": r["qvec_refined"], "tvec": r["tvec_refined"]}, q, t, X, x, cam, pr.OPTION_THRESH)
    rs = np.random.RandomState(61)                                      # the scenes of test_far_world_coordinates
    for model in pr.MODELS:
        cam = pr.camera(model)
        for n, outliers, noise in ((100, 0.0, 0.0), (150, 0.5, 1.0)):
            q, t, x, X, _ = pr.scene(rs, cam, n, outliers, noise_px=noise, offset=pr.FAR_OFFSET)
            r = pr.absolute_pose_ref(x, X, cam, pr.THRESH, min_num_trials=0)
            _check_accuracy({**r, "qvec": r["qvec_refined"], "tvec": r["tvec_refined"]}, q, t, X, x, cam)


def test_num_trials_closed_forms():
    # the documented formula, against values worked by hand: log(1e-4) / log(1 - 0.5^3) * 3 = 206.9, .. 0.3: 1009.6, 0.2: 3440.04
    assert pr.num_trials_needed(0.5, 0.9999) == 207 and pr.num_trials_needed(0.3, 0.9999) == 1010 and pr.num_trials_needed(0.2, 0.9999) == 3441
    assert pr.num_trials_needed(1.0, 0.9999) == 1 and pr.num_trials_needed(0.5, 1.0) == np.inf and pr.num_trials_needed(0.0, 0.5) == np.inf
    assert pr.trial_limits(0.5, 1000, 100000, 0.99) == (104, 104)        # log(0.01) / log(0.875) * 3 = 103.5
    assert pr.trial_limits(0.01, 1000, 100000, 0.9999) == (1000, 100000)
    assert pr.trial_limits(0.5000099, 0, 100000, 0.99) == (0, 104)       # floored to 1e-5 steps
    cam = pr.camera("PINHOLE")
    q, t, x, X, _ = pr.scene(np.random.RandomState(2), cam, 30)           # 100 % inliers, exact
    r = pr.lo_ransac_ref(x, X, cam, pr.THRESH, min_num_trials=0)
    assert r["num_trials"] == 256 and r["num_inliers"] == 30 and r["inliers"].all()
    assert pr.lo_ransac_ref(x, X, cam, pr.THRESH)["num_trials"] == 1024   # the default min_num_trials 1000: four rounds
    x, X, cam, _, _ = pr.option_problem("tenth")                          # 10 % inliers: the formula asks for ~27 600
    assert pr.lo_ransac_ref(x, X, cam, pr.THRESH, min_num_trials=0, max_num_trials=700)["num_trials"] == 700
    assert pr.lo_ransac_ref(x, X, cam, pr.THRESH, min_inlier_ratio=0.5, confidence=0.99)["num_trials"] == 104
    assert pr.lo_ransac_ref(x[:3], X[:3], cam, pr.THRESH)["num_trials"] == 0
    got = sorted({r["num_trials"] for r in pr.ransac_refs()})
    assert got[0] == 256 and got[-1] >= 3328 and any(256 < g < 3328 for g in got), got      # 1, several and ~14 rounds


def test_caps_banded_share_and_left_out_probes():
    """The caps of the GPU tests, on the committed seeds: at most 10 % of the RANSAC cases banded, at most 25 % of each P3P
    family left out.  A seed that breaks a cap is replaced; the cap is not."""
    refs = pr.ransac_refs()
    banded = [i for i, r in enumerate(refs) if r["banded"]]
    print(f"banded RANSAC cases: {len(banded)} of {len(refs)} {[refs[i]['why'] for i in banded]}")
    assert len(banded) <= 0.10 * len(refs)
    opt = [pr.option_ref(kind, **conf) for kind, conf in pr.OPTION_RUNS]
    assert not any(r["banded"] for r in opt), [r["why"] for r in opt if r["banded"]]
    assert len({tuple(r["rounds"]) for r in opt[:3]}) == 3           # the three seeds' round histories differ
    for family, level in pr.P3P_FAMILIES:
        kept = pr.p3p_probes(family, level)["kept"]
        print(f"P3P {family} {level:g}: kept {int(kept.sum())}, left out {int((~kept).sum())}")
        assert (~kept).sum() <= 0.25 * len(kept), (family, level)


@pytest.mark.parametrize("mutate", ["drop_root", "mult2", "sum_gt", "no_lo"])
def test_broken_rules_change_the_restatement(mutate):
    """Each rule the GPU comparison is meant to pin shows in the compared quantities (num_trials, num_inliers, the mask) on
    unbanded committed cases: breaking it in the restatement changes them, so a kernel with that fault cannot agree with the
    restatement as written."""
    cases, refs = pr.ransac_cases(), pr.ransac_refs()
    pick = {"drop_root": [1, 5], "mult2": [7, 9], "sum_gt": [13], "no_lo": [1, 11]}[mutate]
    differs = 0
    for i in pick:
        x, X, cam, _, _, th = cases[i]
        m = pr.lo_ransac_ref(x, X, cam, th, mutate=mutate, **pr.RANSAC_CONF)
        r = refs[i]
        free = ~(r["point_banded"] | m["point_banded"])
        differs += (m["num_trials"] != r["num_trials"] or m["num_inliers"] != r["num_inliers"]
                    or not np.array_equal(m["inliers"][free], r["inliers"][free]))
    assert differs == len(pick)
