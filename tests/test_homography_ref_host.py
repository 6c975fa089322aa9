"""The restatement of the homography estimator (tests/homography_ref.py) on its own, on the CPU: both four-point routes
against generating matrices and against each other, the closed-form trial counts, the chart, the derived band and H tolerance, the
caps on left-out cases, the margins of the decision's scenes, and that breaking a rule changes a compared quantity.  The sampling is checked
at every sample size in tests/test_ransac_ref_host.py."""
import numpy as np

import homography_ref as hr
from sfd2_amd import two_view


def _exact_samples(count, rotation=False):
    rs = np.random.RandomState(13)
    x0s, x1s, Hs = [], [], []
    for _ in range(count):
        H = hr.plane_H(rs, rotation)
        p0 = hr._pixels(rs, 4)
        p1 = hr.apply_H(H, p0)
        c0, c1, s0, s1 = hr.normalisation(p0, p1)
        x0s.append(s0 * (p0 - c0))
        x1s.append(s1 * (p1 - c1))
        Hs.append(hr._unit(hr._T(c1, s1) @ H @ np.linalg.inv(hr._T(c0, s0))))
    return np.stack(x0s), np.stack(x1s), np.stack(Hs)


def test_both_routes_against_the_generating_matrix_and_each_other():
    for rotation in (False, True):
        x0, x1, Ht = _exact_samples(2000, rotation)
        sols = {}
        for solver in (hr.four_point_dlt, hr.four_point_basis):
            H, owner, near = solver(x0, x1)
            assert not near.any() and (owner == np.arange(len(x0))).all()
            worst = float(hr._hdist(H, Ht).max())
            print(f"{solver.__name__}: worst distance to the generating matrix {worst:.3g}")
            assert worst <= 1e-9
            assert max(float(np.sqrt(hr.transfer_f64(H[k], x0[k], x1[k]).max())) for k in range(len(H))) < 1e-10
            sols[solver.__name__] = H
        worst = float(hr._hdist(sols["four_point_dlt"], sols["four_point_basis"]).max())
        print(f"the two routes' solutions differ by at most {worst:.3g}")
        assert worst <= 1e-9


def test_collinear_samples_give_no_hypothesis():
    x = np.array([[[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [0.3, -0.8]]])          # three points of one line in image 0
    y = np.array([[[0.1, 0.0], [1.0, 0.2], [-0.5, 0.7], [0.3, -0.8]]])
    for solver in (hr.four_point_dlt, hr.four_point_basis):
        for a, b in ((x, y), (y, x), (x[:, [3, 0, 1, 2]], y[:, [3, 0, 1, 2]]), (x[:, [0, 3, 1, 2]], y[:, [0, 3, 1, 2]])):
            H, owner, near = solver(a, b)
            assert len(H) == 0 and not near.any()
        H, _, _ = solver(y, y[:, ::-1] * 0.5)
        assert len(H) == 1
        # a repeated point: every triple with both copies has no area
        H, _, _ = solver(y[:, [0, 0, 1, 2]], y[:, [0, 0, 1, 2]])
        assert len(H) == 0
    for name in hr.DEGENERATE:
        r = hr.degenerate_ref(name)
        assert not r["success"] and r["num_inliers"] == 0 and not r["H"].any() and not r["inliers"].any() and not r["banded"]
        assert r["num_trials"] == hr.DEGENERATE[name].get("max_num_trials", 0) * (name == "line")


def test_trial_counts_in_closed_form():
    assert hr.num_trials_needed(0.3, 0.999) == np.ceil(np.log(0.001) / np.log(1 - 0.3 ** 4) * 3) == 2549
    assert hr.num_trials_needed(1.0, 0.999) == 1.0 and hr.num_trials_needed(0.0, 0.999) == np.inf and hr.num_trials_needed(0.5, 1.0) == np.inf
    assert hr.trial_limits(0.25, 0, 10000, 0.999) == (0, 5295)
    assert hr.trial_limits(0.0, 0, 10000, 0.999) == (0, 10000)
    assert hr.trial_limits(0.25, 50000, 1000, 0.999) == (1000, 1000)
    for ref in hr.ransac_refs():
        t, need = ref["num_trials"], hr.num_trials_needed(max(ref["num_inliers"], 1) / len(ref["inliers"]), 0.999)
        assert t % hr.ROUND == 0 or t == 5295
        assert t == 5295 or t >= need


def test_chart_and_its_jacobian():
    rs = np.random.RandomState(5)
    _, _, Ht = _exact_samples(8)
    for H in Ht:
        fix, free, ok = hr.make_chart(H)
        assert ok and len(free) == 8 and fix not in free and abs(H.reshape(-1)[fix]) == np.abs(H).max()
        a, b = rs.uniform(-1, 1, (20, 2)), rs.uniform(-1, 1, (20, 2))
        Hm, g, c = hr.normal_equations(H, free, a, b, np.ones(20))
        assert np.isclose(c, hr.transfer_f64(H, a, b).sum())

        def cost(dd):
            return hr.normal_equations(hr.apply_update(H, free, dd), free, a, b, np.ones(20))[2]
        num = np.array([(cost(1e-6 * e) - cost(-1e-6 * e)) / 2e-6 for e in np.eye(8)])
        assert np.allclose(num, 2 * g, rtol=1e-5, atol=1e-7)
        assert hr.apply_update(H, free, np.ones(8)).reshape(-1)[fix] == H.reshape(-1)[fix]
    # the first wins a tie
    assert hr.make_chart(np.array([[0.5, -1.0, 0], [1.0, 0.2, 0], [0, 0, -1.0]]))[0] == 1
    # the output convention: x1 ~ H x0 in pixels, unit norm, the first largest entry positive
    H = hr.plane_H(rs)
    p0 = hr._pixels(rs, 6)
    p1 = hr.apply_H(H, p0)
    c0, c1, s0, s1 = hr.normalisation(p0, p1)
    P = hr.to_pixels(-hr._T(c1, s1) @ H @ np.linalg.inv(hr._T(c0, s0)), c0, c1, s0, s1)
    assert np.isclose(np.linalg.norm(P), 1.0) and P.reshape(-1)[np.argmax(np.abs(P))] > 0 and np.allclose(hr.apply_H(P, p0), p1, atol=1e-8)


def test_band_and_tolerance_are_derived_and_caps_hold():
    measured = hr.measure_band()
    print(f"largest relative disagreement in squared transfer error over the probe families {measured:.3g}, band {hr.BAND:.3g}")
    assert measured <= hr.MEASURED <= 4 * measured and hr.BAND == 100 * hr.MEASURED
    routes = hr.measure_routes()
    print(f"largest distance between the two routes' pixel matrices {routes:.3g}, tolerance {hr.H_TOL:.3g}")
    assert routes <= hr.H_MEASURED <= 4 * routes and hr.H_TOL == 100 * hr.H_MEASURED and hr.H_TOL <= hr.H_CEILING
    # the caps, for route A against route B: every case neither leaves out agrees in trials, count and mask (or one of the 'either')
    left, total = {}, {}
    for name, a, b in hr.all_ref_pairs():
        total[name] = total.get(name, 0) + 1
        if a["banded"] or b["banded"]:
            left[name] = left.get(name, 0) + 1
            continue
        assert (a["num_trials"], a["num_inliers"], a["success"]) == (b["num_trials"], b["num_inliers"], b["success"]), name
        if a["num_inliers"] >= 4:
            assert any((a["inliers"] == c["inliers"]).all() and np.linalg.norm(a["H"] - c["H"]) <= hr.H_TOL for c in [b] + b["either"]), name
    print("left out per table:", {k: f"{left.get(k, 0)} of {v}" for k, v in total.items()})
    for name, n in total.items():
        assert left.get(name, 0) <= n // 10, name                # a table: at most 1 in 10; a probe family: at most 10 %
    for (n, _, _, _), a, b in zip(hr.RANSAC_CASES, hr.ransac_refs(), hr.ransac_refs(hr.four_point_basis)):
        if n in (4, 5):
            assert not a["banded"] and not b["banded"], (n, a["why"], b["why"])     # reason (b) alone touches these; 'either' answers it
    for f in hr.PROBE_FAMILIES:
        assert hr.probe_disagreement(f)[1] >= hr.PROBES * 9 // 10
    refs = hr.ransac_refs() + [hr.option_ref(**c) for c in hr.OPTION_RUNS]
    # the cases do what they are there for: several rounds, both trial limits, partial rounds
    assert {r["num_trials"] for r in refs} >= {1, 255, 256, 257, 512, 600, 2560, 5295}


def test_decision_scenes_stand_clear_of_the_thresholds():
    """The restatements' counts on the five scenes give the expected configs with and without cameras, and stand at least 5 % of n away
    from both ratio thresholds (0.95 nF for nE, 0.8 nE or 0.8 nF for nH)."""
    margin = 0.05 * hr.DECISION_N
    for name in hr.DECISION_SCENES:
        E, F, H = hr.decision_refs(name)
        assert not (E["banded"] or F["banded"] or H["banded"]), name
        with_cam, without = hr.DECISION_EXPECT[name]
        assert two_view.decide_two_view_geometry(E, F, H)["config"] == with_cam, name
        assert two_view.decide_two_view_geometry(None, F, H)["config"] == without, name
        nE, nF, nH = (r["num_inliers"] for r in (E, F, H))
        print(name, nE, nF, nH, E["success"], E["small_baseline"])
        if name == "random":
            assert max(nE, nF, nH) < 15
            continue
        assert E["success"] and abs(nE - 0.95 * nF) >= margin and abs(nH - 0.8 * nE) >= margin and abs(nH - 0.8 * nF) >= margin, name
        assert E["small_baseline"] == (name == "rotation")


def test_breaking_a_rule_shows():
    """Each rule break changes trials, count, mask or H on one of the committed table cases with 40 or 80 correspondences and up to half
    of them false: the comparison can tell them apart."""
    picks = [k for k, (n, o, _, _) in enumerate(hr.RANSAC_CASES) if n in (40, 80) and o <= 0.5]

    def differs(r, base):
        return (r["num_trials"], r["num_inliers"]) != (base["num_trials"], base["num_inliers"]) or (r["inliers"] != base["inliers"]).any() \
            or np.linalg.norm(r["H"] - base["H"]) > hr.H_TOL
    for brk in (dict(multiplier=2.0), dict(lo=False), dict(smaller_sum=False)):
        hit = []
        for k in picks:
            p0, p1, th = hr.ransac_cases()[k]
            if differs(hr.homography_ref(p0, p1, th, **brk), hr.ransac_refs()[k]):
                hit.append(k)
                break
        assert hit, brk
