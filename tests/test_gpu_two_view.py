"""Relative pose on the MI355X (sfd2_amd.two_view) against the restatement of tests/two_view_ref.py: degenerate sizes, the solver
probes, the RANSAC and option cases (count, mask, trials equal; pose within 1e-6 rad), small baselines, determinism and errors."""
import numpy as np
import pytest

import pose_ref as pr
import two_view_ref as tv

pytestmark = pytest.mark.gpu

POSE_TOL = tv.POSE_TOL


def _tv():
    from sfd2_amd import two_view
    return two_view


def _R(r):
    return pr.qvec2rotmat(r["qvec"])


@pytest.mark.parametrize("n", [0, 4])
def test_fewer_than_five(n):
    rs = np.random.RandomState(n)
    cam = pr.camera("PINHOLE")
    r = _tv().relative_pose(rs.uniform(0, 400, (n, 2)), rs.uniform(0, 400, (n, 2)), cam, cam)
    assert not r["success"] and r["num_inliers"] == 0 and r["num_trials"] == 0 and not r["inliers"].any() and len(r["inliers"]) == n
    assert np.isfinite(r["qvec"]).all() and np.isfinite(r["tvec"]).all() and np.isfinite(r["E"]).all()
    assert np.isnan(r["tri_angle_deg"]) and not r["small_baseline"]


def test_five_points():
    cam0, cam1 = pr.camera("SIMPLE_RADIAL"), pr.camera("OPENCV")
    _, _, p0, p1, _ = tv.two_view_scene(np.random.RandomState(7), cam0, cam1, 5)
    r = _tv().relative_pose(p0, p1, cam0, cam1, min_num_inliers=5)
    assert r["num_inliers"] == 5 and r["inliers"].all() and r["success"]
    x0, x1 = tv._hom(pr.undistort(cam0, p0)), tv._hom(pr.undistort(cam1, p1))
    assert np.max(np.abs(np.sum((x1 @ r["E"]) * x0, 1))) <= 1e-12
    assert abs(np.linalg.norm(r["tvec"]) - 1) < 1e-12 and abs(np.linalg.norm(r["qvec"]) - 1) < 1e-12


@pytest.mark.parametrize("family", tv.PROBE_FAMILIES)
def test_solver_probes(family):
    """One round of one trial on n = 6 or 7 exact points: all n inliers and the generating pose within POSE_TOL if and only if the
    restatement says the sample yields it (for planar scenes: one of the two plane-consistent poses).  Measured on an MI355X: every
    family agrees on every probe, 0 or 1 of 256 left out, worst pose difference 3.0e-8 rad."""
    ps = tv.probes(family)
    expect, _ = tv.probe_expect(family)
    res = _tv().relative_pose_batch([(p0, p1, c0, c1) for p0, p1, c0, c1, _, _ in ps], tv.PROBE_ERROR_PX, max_num_trials=1, min_num_inliers=5)
    left_out, worst, missed = 0, 0.0, []
    for i, ((p0, _, _, _, R, t), (e, poses), r) in enumerate(zip(ps, expect, res)):
        assert r["num_trials"] == 1
        found = bool(r["inliers"].all())
        err = min((max(tv.pose_error(_R(r), r["tvec"], Rp, tp)) for Rp, tp in poses), default=np.inf)
        if e is None:
            left_out += 1
        elif e is False:
            if found and max(tv.pose_error(_R(r), r["tvec"], R, t)) <= POSE_TOL:
                missed.append(i)
        elif not (found and r["success"] and err <= POSE_TOL):
            missed.append(i)
        else:
            worst = max(worst, err)
    print(f"{family}: {left_out} of {len(ps)} left out, {len(missed)} disagree with the restatement, worst pose difference {worst:.3g} rad")
    assert left_out <= len(ps) // 4
    assert not missed, missed


_compare = tv.compare       # shared with tests/test_gpu_two_view_edges.py


def test_ransac_cases_against_the_restatement():
    cases, refs = tv.ransac_cases(), tv.ransac_refs()
    res = _tv().relative_pose_batch([(p0, p1, c0, c1, th) for p0, p1, c0, c1, _, _, th in cases])
    banded, worst = 0, [0.0, 0.0]
    for r, ref in zip(res, refs):
        if ref["banded"]:
            banded += 1
            continue
        _compare(r, ref, worst)
    print(f"RANSAC cases: {banded} of {len(cases)} banded, worst rotation / translation difference {worst[0]:.3g} / {worst[1]:.3g} rad")
    assert banded <= len(cases) // 10


def test_option_runs_against_the_restatement():
    p0, p1, c0, c1, _, _, th = tv.option_case()
    banded, worst, trials = 0, [0.0, 0.0], set()
    for conf in tv.OPTION_RUNS:
        ref = tv.option_ref(**conf)
        r = _tv().relative_pose(p0, p1, c0, c1, th, **conf)
        trials.add(ref["num_trials"])
        if ref["banded"]:
            banded += 1
            continue
        _compare(r, ref, worst)
    print(f"option runs: {banded} of {len(tv.OPTION_RUNS)} banded, worst {worst[0]:.3g} / {worst[1]:.3g} rad, trial counts {sorted(trials)}")
    assert banded <= len(tv.OPTION_RUNS) // 10 and len(trials) >= 4


def test_cheirality_tie_goes_to_the_lowest_slot():
    p0, p1, c0, c1, R, t = tv.tie_case()
    r, ref = _tv().relative_pose(p0, p1, c0, c1), tv.relative_pose_ref(p0, p1, c0, c1, 4.0)
    assert not ref["banded"] and r["num_inliers"] == 24
    _compare(r, ref, [0.0, 0.0])
    assert max(tv.pose_error(_R(r), r["tvec"], R, t)) <= POSE_TOL and np.isfinite(r["tri_angles_deg"]).sum() == 12


def test_small_baseline():
    cam = pr.camera("OPENCV")
    _, _, p0, p1, _ = tv.two_view_scene(np.random.RandomState(3), cam, cam, 80, noise_px=0.5, baseline=0.0)
    r = _tv().relative_pose(p0, p1, cam, cam)
    assert r["small_baseline"]
    R, t, p0, p1, _ = tv.two_view_scene(np.random.RandomState(4), cam, cam, 80, noise_px=0.5, baseline=0.1)
    r = _tv().relative_pose(p0, p1, cam, cam)
    assert r["success"] and not r["small_baseline"] and r["tri_angle_deg"] > 1.5
    assert max(tv.pose_error(_R(r), r["tvec"], R, t)) < 0.05


def test_bit_identical_whatever_the_batch():
    cam0, cam1 = pr.camera("OPENCV"), pr.camera("SIMPLE_RADIAL")
    probs = []
    for i, n in enumerate((40, 0, 300, 12)):
        p0 = p1 = np.zeros((0, 2))
        if n:
            _, _, p0, p1, _ = tv.two_view_scene(np.random.RandomState(30 + i), cam0, cam1, n, 0.3, noise_px=0.5)
        probs.append((p0, p1, cam0, cam1))
    T = _tv()
    a, b = T.relative_pose_batch(probs), T.relative_pose_batch(probs)
    rev = T.relative_pose_batch(probs[::-1])[::-1]
    alone = [T.relative_pose_batch([p])[0] for p in probs]
    for other in (b, rev, alone):
        for x, y in zip(a, other):
            for k in ("qvec", "tvec", "E", "inliers", "tri_angles_deg"):
                assert np.array_equal(x[k], y[k], equal_nan=(k == "tri_angles_deg")), k
            assert (x["success"], x["num_inliers"], x["num_trials"]) == (y["success"], y["num_inliers"], y["num_trials"])


def test_errors():
    cam = pr.camera("PINHOLE")
    p = np.random.RandomState(0).uniform(0, 400, (10, 2))
    bad = p.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        _tv().relative_pose(bad, p, cam, cam)
    from sfd2_amd import _lib
    import ctypes
    ctx = _lib.default_context(0)
    pb = _lib.TwoViewProblem()
    pb.n, pb.model0, pb.model1 = 10, 1, 1
    for i, v in enumerate(cam["params"]):
        pb.params0[i] = pb.params1[i] = v
    pb.points2D_0, pb.points2D_1, pb.max_error_px = bad.ctypes.data, p.ctypes.data, 4.0
    conf = _lib.TwoViewConf(0.25, 0, 100, 0.999, 0, 15, 0)
    res = (_lib.TwoViewResult * 1)()
    mask, ang = np.zeros(10, np.uint8), np.zeros(10)
    assert ctx.lib.sfd2_relative_pose_batch(ctx.h, ctypes.byref(pb), 1, ctypes.byref(conf), res, mask.ctypes.data, ang.ctypes.data, 0) == -1
    pb.points2D_0, pb.model1 = p.ctypes.data, 7
    with pytest.raises(RuntimeError, match="camera model 7"):
        _lib.check(ctx.lib.sfd2_relative_pose_batch(ctx.h, ctypes.byref(pb), 1, ctypes.byref(conf), res, mask.ctypes.data, ang.ctypes.data, 0))
    with pytest.raises(ValueError, match="not supported"):
        _tv().relative_pose(p, p, {"model": "FOV", "params": [1, 1, 1, 1, 1]}, cam)
