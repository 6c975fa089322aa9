"""Relative pose on the MI355X at its edges (sfd2_amd.two_view against the restatement of tests/two_view_ref.py): sizes at the seams
of the 256-wide strides, the trial limits around a round, match lists with repeated correspondences (rank-deficient samples), many
small pairs in one call and degenerate pairs.  Every result also goes through _invariants.  The tables are two_view_ref's;
tests/test_two_view_ref_host.py checks on the CPU that they stay within the caps used here."""
import numpy as np
import pytest

import pose_ref as pr
import two_view_ref as tv

pytestmark = pytest.mark.gpu

POSE_TOL = tv.POSE_TOL
_ARRAYS = ("qvec", "tvec", "E", "inliers", "tri_angles_deg")
_SCALARS = ("success", "num_inliers", "num_trials", "small_baseline")


def _tv():
    from sfd2_amd import two_view
    return two_view


def _R(r):
    return pr.qvec2rotmat(r["qvec"])


def _invariants(r, n, conf):
    """What holds for every result: r of a pair of n correspondences run with the options conf."""
    max_trials = conf.get("max_num_trials", tv.DEFAULTS["max_num_trials"])
    min_inliers = conf.get("min_num_inliers", 15)
    inl, ang = r["inliers"], r["tri_angles_deg"]
    assert len(inl) == n and len(ang) == n and inl.dtype == bool
    assert r["num_inliers"] == int(inl.sum())
    fin = np.isfinite(ang)
    assert not (fin & ~inl).any() and np.isnan(ang[~fin]).all()
    assert ((ang[fin] >= 0) & (ang[fin] <= 180)).all()
    if n >= 5:
        assert 1 <= r["num_trials"] <= max_trials
    else:
        assert r["num_trials"] == 0
    if r["num_inliers"] >= 5:
        assert abs(np.linalg.norm(r["qvec"]) - 1) <= 1e-12 and abs(np.linalg.norm(r["tvec"]) - 1) <= 1e-12
        assert np.max(np.abs(r["E"] - tv.skew(r["tvec"][None])[0] @ _R(r))) <= 1e-12
    else:
        assert not r["success"] and r["num_inliers"] == 0 and not inl.any() and not fin.any()
        assert np.array_equal(r["qvec"], [1.0, 0.0, 0.0, 0.0]) and not r["tvec"].any() and not r["E"].any()
    if r["success"]:
        assert r["num_inliers"] >= min_inliers and fin.any()
    assert r["small_baseline"] == bool(fin.any() and np.median(ang[fin]) < 1.5)


def _same_bytes(x, y):
    for k in _ARRAYS:
        assert x[k].dtype == y[k].dtype and x[k].tobytes() == y[k].tobytes(), k
    for k in _SCALARS:
        assert x[k] == y[k], k
    assert x["tri_angle_deg"] == y["tri_angle_deg"] or (np.isnan(x["tri_angle_deg"]) and np.isnan(y["tri_angle_deg"]))


def test_sizes_at_the_stride_seams():
    """n = 255 .. 1025 at 30 and 60 % outliers (and 1025 without outliers, where index 1024 is an inlier) in one call, between pairs
    of 0, 3 and 4 correspondences that keep every offset off a multiple of 256, then every pair alone.  A stride that is skipped, or
    an element dropped at index 256, 512, 768 or 1024, changes the mask and the count (tests/test_two_view_ref_host.py: each of those
    is an inlier of some case), the sums behind the support order or the normal equations behind the pose.  Measured on an MI355X:
    0 of 15 banded, trials 256 (0 and 30 %) and 1536 to 2048 (60 %) as the restatement's, worst rotation / translation difference
    3.0e-8 / 0 rad (pose_error resolves 1.5e-8 rad), every pair alone byte-equal."""
    cases = tv.size_cases()
    probs, where, fill = [], [], (3, 0, 4)
    rs = np.random.RandomState(0)
    cam = pr.camera("PINHOLE")
    for k, (p0, p1, c0, c1, _, _, th) in enumerate(cases):
        m = fill[k % 3]
        probs.append((rs.uniform(0, 400, (m, 2)), rs.uniform(0, 400, (m, 2)), cam, cam, th))
        where.append(len(probs))
        probs.append((p0, p1, c0, c1, th))
    offs = np.concatenate([[0], np.cumsum([len(p[0]) for p in probs])])
    assert all(offs[w] % 256 for w in where)
    T = _tv()
    res = T.relative_pose_batch(probs)
    for p, r in zip(probs, res):
        _invariants(r, len(p[0]), {})
        assert len(p[0]) >= 5 or not r["success"]
    banded, worst, trials = 0, [0.0, 0.0], []
    for k, w in enumerate(where):
        ref = tv.size_ref(k)
        trials.append(res[w]["num_trials"])
        if ref["banded"]:
            banded += 1
            continue
        tv.compare(res[w], ref, worst)
    print(f"size cases: {banded} of {len(cases)} banded, trials {trials}, worst rotation / translation difference "
          f"{worst[0]:.3g} / {worst[1]:.3g} rad")
    assert len(cases) == 15 and banded <= 1
    for p, r in zip(probs, res):
        _same_bytes(T.relative_pose_batch([p])[0], r)


def test_trial_limits():
    """max_num_trials one under, at and over a round, at two rounds and at 1; confidence and min_inlier_ratio at both closed ends;
    min_num_trials between the limits and beyond max_num_trials; seeds with the top bit set.  A round more or less changes
    num_trials; an idle lane's trial that ran in a partial round changes the winner of the three runs of one trial (13 inliers, 32
    with more trials; tests/test_two_view_ref_host.py).  Measured on an MI355X: num_trials as the table says, none banded, worst
    rotation / translation difference 2.1e-8 / 0 rad; seed -1 byte-equal to 2^64 - 1."""
    p0, p1, c0, c1, _, _, th = tv.limit_case()
    T, worst = _tv(), [0.0, 0.0]
    for conf, trials in tv.LIMIT_RUNS:
        ref = tv.limit_ref(**conf)
        r = T.relative_pose(p0, p1, c0, c1, th, **conf)
        _invariants(r, len(p0), conf)
        assert not ref["banded"], conf
        assert r["num_trials"] == trials == ref["num_trials"], (conf, r["num_trials"])
        tv.compare(r, ref, worst)
    by_seed = {s: T.relative_pose(p0, p1, c0, c1, th, seed=s) for s in tv.SEED_RUNS + [-1]}
    _same_bytes(by_seed[-1], by_seed[2 ** 64 - 1])
    for s in tv.SEED_RUNS:
        ref = tv.limit_ref(seed=s)
        _invariants(by_seed[s], len(p0), {})
        assert not ref["banded"], s
        tv.compare(by_seed[s], ref, worst)
    print(f"limit runs: worst rotation / translation difference {worst[0]:.3g} / {worst[1]:.3g} rad")


def test_repeated_correspondences():
    """8 or 12 distinct correspondences 16 or 10 times over: 71 % or 56 % of the samples hold a correspondence twice and must yield
    nothing, and the others must still find every point.  (A matrix from such a sample goes through four of the classes and cannot
    win here; four_classes of test_degenerate_pairs is where taking one shows.)  Measured on an MI355X: 0 of 12 banded, every
    point an inlier after 256 trials, worst rotation / translation difference to the restatement and, for the exact cases, to the
    generating pose 0 rad (below pose_error's resolution of 1.5e-8 rad)."""
    cases = tv.repeat_cases()
    res = _tv().relative_pose_batch([(p0, p1, c0, c1, th) for p0, p1, c0, c1, _, _, th in cases])
    banded, worst, exact = 0, [0.0, 0.0], 0.0
    for k, ((p0, _, _, _, R, t, _), (_, _, _, noise), r) in enumerate(zip(cases, tv.REPEAT_CASES, res)):
        _invariants(r, len(p0), {})
        ref = tv.repeat_ref(k)
        if ref["banded"]:
            banded += 1
            continue
        tv.compare(r, ref, worst)
        assert r["inliers"].all() and r["success"]
        if noise == 0.0:
            e = max(tv.pose_error(_R(r), r["tvec"], R, t))
            exact = max(exact, e)
            assert e <= POSE_TOL
    print(f"repeat cases: {banded} of {len(cases)} banded, worst rotation / translation difference {worst[0]:.3g} / {worst[1]:.3g} rad, "
          f"exact cases to the generating pose {exact:.3g} rad")
    assert banded <= 1


def test_many_small_pairs_in_one_call():
    """300 pairs of 0 to 40 correspondences in one call: more workgroups than CUs, and the per-pair scratch rows far apart.
    With n = 5 each of the sample's solutions fits every point, and with so few points a slot of R and one of R' may tie in the
    cheirality count: the restatement lists those answers ('either') and the pose must be one of them.  Measured on an MI355X: 5 of
    the 258 compared pairs (n <= 12) banded (their refinement had not converged), worst rotation / translation difference
    3.0e-8 / 1.5e-8 rad; 20 pairs run alone are byte-equal."""
    cases = tv.many_cases()
    T = _tv()
    res = T.relative_pose_batch(cases, **tv.MANY_CONF)
    assert len(res) == tv.MANY
    banded, compared, worst = 0, 0, [0.0, 0.0]
    for i, (c, r) in enumerate(zip(cases, res)):
        _invariants(r, len(c[0]), tv.MANY_CONF)
        if len(c[0]) <= 12:
            ref = tv.many_ref(i)
            compared += 1
            if ref["banded"]:
                banded += 1
                continue
            tv.compare(r, ref, worst)
    print(f"many pairs: {banded} of {compared} compared pairs banded, worst rotation / translation difference {worst[0]:.3g} / {worst[1]:.3g} rad")
    assert compared == 258 and banded <= compared // 10
    alone = list(range(2, tv.MANY, 15))
    assert len(alone) == 20 and len({len(cases[i][0]) for i in alone}) == len(tv.MANY_NS)
    for i in alone:
        _same_bytes(T.relative_pose_batch([cases[i]], **tv.MANY_CONF)[0], res[i])


def _run_degenerate(name):
    p0, p1, c0, c1, R, _ = tv.degenerate(name)
    conf = tv.DEGENERATE[name]
    r = _tv().relative_pose(p0, p1, c0, c1, 4.0, **conf)
    _invariants(r, len(p0), conf)
    return r, R


def test_degenerate_pairs():
    """identical and four_classes (every sample rank-deficient; a hypothesis taken from one would hold all 20 or 64 points):
    nothing found after all 512 trials.  all_outliers: as the restatement, no success.
    collinear: the invariants, and the same bytes twice.  rotation_exact and identity, where every [t]x R fits and no solution is
    isolated: either no result (and then no success, so that no caller takes the pair for a baseline), or at least 55 inliers with
    the generating rotation within POSE_TOL and small_baseline set.  Measured on an MI355X: rotation_exact and identity both give
    no result (0 inliers after 512 trials, success False, small_baseline False), as the restatement does; collinear gives no
    result either; all_outliers 13 inliers of 60 after 1024 trials, 4 of them with an angle, success False."""
    for name in ("identical", "four_classes"):
        r, _ = _run_degenerate(name)
        ref = tv.degenerate_ref(name)
        assert not ref["banded"]
        tv.compare(r, ref, [0.0, 0.0])
        assert r["num_trials"] == 512 and r["num_inliers"] == 0 and not r["success"] and not r["small_baseline"], name

    r, _ = _run_degenerate("all_outliers")
    ref = tv.degenerate_ref("all_outliers")
    assert not ref["banded"]
    tv.compare(r, ref, [0.0, 0.0])
    assert r["num_trials"] == 1024 and not r["success"]
    print(f"all_outliers: {r['num_inliers']} inliers, {int(np.isfinite(r['tri_angles_deg']).sum())} finite angles, success {r['success']}")

    r, _ = _run_degenerate("collinear")
    _same_bytes(_run_degenerate("collinear")[0], r)
    print(f"collinear: {r['num_inliers']} inliers, success {r['success']}, {r['num_trials']} trials")

    for name in ("rotation_exact", "identity"):
        r, R = _run_degenerate(name)
        n = len(r["inliers"])
        dr = tv.pose_error(_R(r), np.ones(3), R, np.ones(3))[0]
        print(f"{name}: {r['num_inliers']} of {n} inliers, success {r['success']}, small_baseline {r['small_baseline']}, "
              f"{int(np.isfinite(r['tri_angles_deg']).sum())} finite angles, rotation difference {dr:.3g} rad, {r['num_trials']} trials")
        if r["num_inliers"] == 0:
            assert not r["success"] and not r["small_baseline"]            # outcome 1: no result (the rest is _invariants')
            print(f"{name}: outcome 1, no result")
        else:
            assert r["num_inliers"] >= 55 and dr <= POSE_TOL and r["small_baseline"]      # outcome 2: the rotation, flagged
            print(f"{name}: outcome 2, the rotation with small_baseline")
