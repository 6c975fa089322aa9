"""The restatement of the relative pose solver (tests/two_view_ref.py) on its own, on the CPU: the five-point solver
against generating matrices, the closed-form trial counts, the derived band, the caps on banded and left-out cases, and that
breaking a rule changes a compared quantity on the committed cases.  The sampling is checked
at every sample size in tests/test_ransac_ref_host.py."""
import numpy as np
import pytest

import pose_ref as pr
import two_view_ref as tv


def test_five_point_against_the_generating_matrix():
    rs = np.random.RandomState(11)
    cam = pr.camera("PINHOLE")
    x0s, x1s, Es = [], [], []
    for _ in range(2000):
        R, t, p0, p1, _ = tv.two_view_scene(rs, cam, cam, 5)
        x0s.append(pr.undistort(cam, p0))
        x1s.append(pr.undistort(cam, p1))
        E = tv.skew(t[None])[0] @ R
        Es.append(E / np.linalg.norm(E))
    sol, owner, near, _ = tv.five_point_ref(np.stack(x0s), np.stack(x1s))
    sol = sol / np.linalg.norm(sol, axis=(1, 2))[:, None, None]
    worst, counts = 0.0, np.bincount(owner, minlength=2000)
    for h in range(2000):
        c = sol[owner == h]
        d = np.minimum(np.linalg.norm(c - Es[h], axis=(1, 2)), np.linalg.norm(c + Es[h], axis=(1, 2)))
        worst = max(worst, float(d.min()))
    print(f"worst distance to the generating matrix {worst:.3g}, {counts.mean():.2f} solutions per sample")
    assert worst <= 1e-9 and counts.max() <= 10 and counts.min() >= 1
    # every solution is an essential matrix through the five points
    s = np.linalg.svd(sol, compute_uv=False)
    assert np.max(np.abs(s[:, 0] - s[:, 1])) < 1e-9 and np.max(s[:, 2]) < 1e-9
    assert np.max(np.sqrt(tv.sampson_f64(sol, np.stack(x0s)[owner], np.stack(x1s)[owner]))) < 1e-10


def test_trial_counts_in_closed_form():
    assert tv.num_trials_needed(0.5, 0.999) == np.ceil(np.log(0.001) / np.log(1 - 0.5 ** 5) * 3) == 653
    assert tv.num_trials_needed(1.0, 0.999) == 1.0 and tv.num_trials_needed(0.0, 0.999) == np.inf and tv.num_trials_needed(0.5, 1.0) == np.inf
    assert tv.num_trials_needed(0.5, 0.999, 2.0) == np.ceil(np.log(0.001) / np.log(1 - 0.5 ** 5) * 2)
    assert tv.trial_limits(0.25, 0, 10000, 0.999) == (0, 10000)            # 21211 trials at a quarter of inliers: no limit below 10000
    assert tv.trial_limits(0.6, 0, 10000, 0.999) == (0, 257)               # ceil(3 log(0.001) / log(1 - 0.6^5)) = 257
    assert tv.trial_limits(0.25, 50000, 10000, 0.999) == (10000, 10000)
    # the committed cases stop where the rule says
    for ref in tv.ransac_refs():
        t, need = ref["num_trials"], tv.num_trials_needed(ref["num_inliers"] / len(ref["inliers"]), 0.999)
        assert t % tv.ROUND == 0 or t == 10000
        assert t == 10000 or t >= need


def test_band_is_derived_and_caps_hold():
    measured = tv.measure_band()
    print(f"largest relative disagreement in squared Sampson error over the probe families {measured:.3g}, band {tv.BAND:.3g}")
    assert measured <= tv.MEASURED <= 4 * measured and tv.BAND == 100 * tv.MEASURED
    for family in tv.PROBE_FAMILIES:
        exp, _ = tv.probe_expect(family)
        left = sum(e is None for e, _ in exp)
        print(f"{family}: {left} of {len(exp)} left out, {sum(e is True for e, _ in exp)} true, {sum(e == 'either' for e, _ in exp)} either")
        assert left <= len(exp) // 4
        assert sum(e is True or e == "either" for e, _ in exp) >= len(exp) // 2
    refs = tv.ransac_refs() + [tv.option_ref(**c) for c in tv.OPTION_RUNS]
    banded = sum(r["banded"] for r in refs)
    print(f"{banded} of {len(refs)} RANSAC and option cases banded")
    assert banded <= len(refs) // 10
    # the cases do what they are there for: several rounds, both trial limits, all inlier ratios
    assert {r["num_trials"] for r in refs} >= {256, 257, 300, 512, 768, 1024, 8704}


def _differs(a, b):
    return (a["num_trials"], a["num_inliers"]) != (b["num_trials"], b["num_inliers"]) or not np.array_equal(a["inliers"], b["inliers"]) \
        or max(tv.pose_error(a["R"], a["t"], b["R"], b["t"])) > 1e-6


@pytest.mark.parametrize("rule", ["drop_root", "multiplier", "smaller_sum", "lo", "slots"])
def test_breaking_a_rule_changes_a_compared_quantity(rule):
    broken = {"drop_root": dict(drop_root=True), "multiplier": dict(multiplier=2.0), "smaller_sum": dict(smaller_sum=False),
              "lo": dict(lo=False), "slots": dict(slots=tv.SLOTS[::-1])}[rule]
    changed = 0
    if rule == "slots":         # only a tie between decompositions shows the slot order
        p0, p1, c0, c1, R, t = tv.tie_case()
        good, bad = tv.relative_pose_ref(p0, p1, c0, c1, 4.0), tv.relative_pose_ref(p0, p1, c0, c1, 4.0, **broken)
        assert good["success"] and max(tv.pose_error(good["R"], good["t"], R, t)) < 1e-6 and np.isfinite(good["angles"]).sum() == 12
        assert _differs(good, bad)
        return
    if rule == "drop_root":     # one trial: the sample's last solution is the generating one in some probes, and nothing makes up for it
        for (p0, p1, c0, c1, _, _), (e, _) in list(zip(tv.probes("generic"), tv.probe_expect("generic")[0]))[:24]:
            conf = dict(max_error_px=tv.PROBE_ERROR_PX, min_num_inliers=5, max_num_trials=1)
            changed += e is True and _differs(tv.relative_pose_ref(p0, p1, c0, c1, **conf), tv.relative_pose_ref(p0, p1, c0, c1, **conf, **broken))
        assert changed >= 1
        return
    for (p0, p1, c0, c1, _, _, th), ref in [list(zip(tv.ransac_cases(), tv.ransac_refs()))[k] for k in (2, 4, 7, 9)]:
        changed += _differs(tv.relative_pose_ref(p0, p1, c0, c1, th, **broken), ref)
    assert changed >= 1


def test_edge_tables_stay_within_their_caps():
    """The tables of tests/test_gpu_two_view_edges.py, on the CPU: they build, the restatement bands no more of them than the GPU
    tests allow, and they still are what they are there for (the trial counts, every repeated point an inlier, nothing found on the
    degenerate pairs).  Measured: 0 banded of the size, limit and repeat cases, 5 of the 258 small pairs (the final refinement
    of each had not converged); about 20 s."""
    refs = [tv.size_ref(k) for k in range(len(tv.SIZE_CASES))]
    assert len(refs) == 15 and sum(r["banded"] for r in refs) <= 1
    for (_, n, o), (p0, *_), r in zip(tv.SIZE_CASES, tv.size_cases(), refs):
        assert len(p0) == n and r["success"] and r["num_inliers"] >= 0.9 * (1 - o) * n
        assert r["num_trials"] == 256 if o <= 0.3 else 1536 <= r["num_trials"] <= 2048
    assert {len(c[0]) for c in tv.size_cases()} == {255, 256, 257, 511, 512, 513, 1025}
    # a stride that is skipped, or an element that is dropped at a seam, shows in the compared mask: the element at every seam is an
    # inlier of some case, and where a pair ends in a partial stride that stride holds inliers in some case of that size
    masks = [r["inliers"] for r in refs if not r["banded"]]
    for seam in (256, 512, 768, 1024):
        assert any(len(m) > seam and m[seam] for m in masks), seam
    for n in (255, 257, 511, 513, 1025):
        assert any(m[(n - 1) // 256 * 256:].any() for m in masks if len(m) == n), n

    assert len(tv.LIMIT_RUNS) == 11
    for conf, trials in tv.LIMIT_RUNS:
        r = tv.limit_ref(**conf)
        assert r["num_trials"] == trials and not r["banded"], conf
    for seed in tv.SEED_RUNS:
        assert not tv.limit_ref(seed=seed)["banded"]
    assert tv.limit_ref(seed=-1)["inliers"].tolist() == tv.limit_ref(seed=2 ** 64 - 1)["inliers"].tolist()
    # a partial round that ran its idle trials as well shows in the runs of one trial (the other runs' local optimisation leads
    # every good hypothesis to the same 32 inliers)
    p0, p1, c0, c1, _, _, th = tv.limit_case()
    for conf in (dict(max_num_trials=1), dict(confidence=0.0), dict(min_inlier_ratio=1.0)):
        assert _differs(tv.limit_ref(**conf), tv.relative_pose_ref(p0, p1, c0, c1, th, dead_lanes=True, **conf))

    refs = [tv.repeat_ref(k) for k in range(len(tv.REPEAT_CASES))]
    assert len(refs) == 12 and sum(r["banded"] for r in refs) <= 1
    for (_, classes, copies, noise), (p0, p1, _, _, R, t, _), r in zip(tv.REPEAT_CASES, tv.repeat_cases(), refs):
        assert len(p0) == classes * copies and r["num_inliers"] == classes * copies in (128, 120) and r["success"] and r["num_trials"] == 256
        assert noise > 0 or max(tv.pose_error(r["R"], r["t"], R, t)) <= 1e-6
        # most samples of such a list hold a correspondence twice, and those give no hypothesis
        idx = tv.sample5v(0, np.arange(256), len(p0)) % classes
        twice = np.array([len(set(row)) < 5 for row in idx.tolist()])
        assert 0.45 <= twice.mean() <= 0.8
        x0, x1 = pr.undistort(pr.camera("OPENCV"), p0), pr.undistort(pr.camera("OPENCV"), p1)
        smp = tv.sample5v(0, np.arange(256), len(p0))
        _, owner, _, _ = tv.five_point_ref(x0[smp], x1[smp])
        assert not twice[owner].any() and len(np.unique(owner)) >= 0.8 * (~twice).sum()

    cases = tv.many_cases()
    assert len(cases) == 300 and [len(c[0]) for c in cases[:7]] == list(tv.MANY_NS)
    small = [i for i, c in enumerate(cases) if len(c[0]) <= 12]
    banded = sum(tv.many_ref(i)["banded"] for i in small)
    assert len(small) == 258 and banded <= len(small) // 10
    assert sum(tv.many_ref(i)["success"] for i in small) >= 150

    for name in ("identical", "four_classes", "rotation_exact", "identity"):
        r = tv.degenerate_ref(name)
        assert r["num_inliers"] == 0 and not r["success"] and r["num_trials"] == 512 and not np.isfinite(r["angles"]).any(), name
    r = tv.degenerate_ref("all_outliers")
    assert not r["banded"] and not r["success"] and r["num_trials"] == 1024 and 5 <= r["num_inliers"] < 15
    p0, p1, *_ = tv.degenerate("collinear")
    for p in (p0, p1):                                     # on a line in both images
        assert np.linalg.svd(p - p.mean(0), compute_uv=False)[1] <= 1e-9 * np.linalg.norm(p - p.mean(0))
    assert len(p0) == 40 and tv.degenerate_ref("collinear")["num_trials"] == 512
