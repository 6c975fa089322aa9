"""The restatement of the fundamental-matrix estimator (tests/fundamental_ref.py) on its own, on the CPU: both
seven-point routes against generating matrices and against each other, the closed-form trial counts, the derived band and F tolerance, the caps
on left-out cases, the chart, and that breaking a rule changes a compared quantity on the committed cases.  The sampling is checked
at every sample size in tests/test_ransac_ref_host.py."""
import numpy as np

import fundamental_ref as fr


def _exact_samples(count):
    rs = np.random.RandomState(11)
    x0s, x1s, Fs = [], [], []
    for _ in range(count):
        R, t, p0, p1, _ = fr.tv.two_view_scene(rs, fr.CAM0, fr.CAM1, 7)
        c0, c1, s = fr.normalisation(p0, p1)
        x0s.append(s * (p0 - c0))
        x1s.append(s * (p1 - c1))
        T0i = np.array([[1 / s, 0, c0[0]], [0, 1 / s, c0[1]], [0, 0, 1.0]])
        T1i = np.array([[1 / s, 0, c1[0]], [0, 1 / s, c1[1]], [0, 0, 1.0]])
        Fs.append(fr._unit(T1i.T @ fr.true_F(R, t) @ T0i))
    return np.stack(x0s), np.stack(x1s), np.stack(Fs)


def test_both_routes_against_the_generating_matrix_and_each_other():
    x0, x1, Ft = _exact_samples(2000)
    sols = {}
    for solver in (fr.seven_point_ref, fr.seven_point_gj):
        F, owner, near = solver(x0, x1)
        counts = np.bincount(owner, minlength=len(x0))
        assert set(np.unique(counts)) <= {1, 3}
        worst = max(float(fr._fdist(F[owner == h], Ft[h]).min()) for h in range(len(x0)))
        print(f"{solver.__name__}: worst distance to the generating matrix {worst:.3g}, {counts.mean():.2f} solutions per sample")
        assert worst <= 1e-9
        # every solution is a rank-2 matrix through the seven points
        assert np.max(np.abs(np.linalg.det(F))) < 1e-12
        assert np.max(np.sqrt(fr.sampson_f64(F, x0[owner], x1[owner]))) < 1e-10
        sols[solver.__name__] = (F, owner, near)
    (Fa, oa, na), (Fb, ob, nb) = sols["seven_point_ref"], sols["seven_point_gj"]
    ok = ~(na | nb)
    assert ok.mean() > 0.95 and (np.bincount(oa, minlength=len(x0))[ok] == np.bincount(ob, minlength=len(x0))[ok]).all()
    worst = max(float(max(fr._fdist(f, Fb[ob == h]).min() for f in Fa[oa == h])) for h in np.flatnonzero(ok))
    print(f"the two routes' solutions differ by at most {worst:.3g}")
    assert worst <= 1e-9


def test_degenerate_samples_give_no_hypothesis():
    for name in ("coplanar", "rotation", "line"):
        p0, p1 = fr.degenerate(name)
        c0, c1, s = fr.normalisation(p0, p1)
        idx = fr.sample_kv(0, np.arange(64), len(p0))
        for solver in (fr.seven_point_ref, fr.seven_point_gj):
            F, _, _ = solver((s * (p0 - c0))[idx], (s * (p1 - c1))[idx])
            assert len(F) == 0, (name, solver.__name__)
        r = fr.degenerate_ref(name)
        assert not r["success"] and r["num_inliers"] == 0 and not r["F"].any() and r["num_trials"] == fr.DEGENERATE[name]["max_num_trials"]
    r = fr.degenerate_ref("repeated")
    assert not r["success"] and r["num_trials"] == 0 and not r["F"].any()


def test_trial_counts_in_closed_form():
    assert fr.num_trials_needed(0.5, 0.999) == np.ceil(np.log(0.001) / np.log(1 - 0.5 ** 7) * 3) == 2643
    assert fr.num_trials_needed(1.0, 0.999) == 1.0 and fr.num_trials_needed(0.0, 0.999) == np.inf and fr.num_trials_needed(0.5, 1.0) == np.inf
    assert fr.trial_limits(0.25, 0, 10000, 0.999) == (0, 10000)
    assert fr.trial_limits(0.7, 0, 10000, 0.999) == (0, int(np.ceil(np.log(0.001) / np.log(1 - 0.7 ** 7) * 3)))
    assert fr.trial_limits(0.25, 50000, 10000, 0.999) == (10000, 10000)
    for ref in fr.ransac_refs():
        t, need = ref["num_trials"], fr.num_trials_needed(max(ref["num_inliers"], 1) / len(ref["inliers"]), 0.999)
        assert t % fr.ROUND == 0 or t == 10000
        assert t == 10000 or t >= need


def test_chart_keeps_rank_two_and_its_jacobian_is_the_derivative():
    rs = np.random.RandomState(5)
    x0, x1, Ft = _exact_samples(8)
    for F in Ft:
        ch, ok = fr.make_chart(F)
        assert ok and np.allclose(fr.chart_matrix(ch), F, atol=1e-14)
        d = 1e-3 * rs.standard_normal(7)
        assert abs(np.linalg.det(fr._unit(fr.chart_matrix(fr.apply_update(ch, d))))) < 1e-15
        a, b = rs.uniform(-1, 1, (20, 2)), rs.uniform(-1, 1, (20, 2))
        H, g, c = fr.normal_equations(ch, a, b, np.ones(20))

        def cost(dd):
            return fr.normal_equations(fr.apply_update(ch, dd), a, b, np.ones(20))[2]
        num = np.array([(cost(1e-6 * e) - cost(-1e-6 * e)) / 2e-6 for e in np.eye(7)])
        assert np.allclose(num, 2 * g, rtol=1e-5, atol=1e-9)
    # the first wins a tie: all three pairs of rows span the same area; rows 1 and 2 are (0 1 0 | 1 1 0)
    ch, _ = fr.make_chart(np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 1.0, 0]]))
    assert ch["k"] == 0 and ch["fix"] == 1 and (ch["a"], ch["b"]) == (-1.0, 1.0)


def test_band_and_tolerance_are_derived_and_caps_hold():
    measured = fr.measure_band()
    print(f"largest relative disagreement in squared Sampson error over the exact probe families {measured:.3g}, band {fr.BAND:.3g}")
    assert measured <= fr.MEASURED <= 4 * measured and fr.BAND == 100 * fr.MEASURED
    routes = fr.measure_routes()
    print(f"largest distance between the two routes' pixel matrices {routes:.3g}, tolerance {fr.F_TOL:.3g}")
    assert routes <= fr.F_MEASURED <= 4 * routes and fr.F_TOL == 100 * fr.F_MEASURED and fr.F_TOL <= fr.F_CEILING
    # the caps, for route A against route B: every case neither leaves out agrees in trials, count and mask (or one of the 'either')
    left, total = {}, {}
    for name, a, b in fr.all_ref_pairs():
        total[name] = total.get(name, 0) + 1
        if a["banded"] or b["banded"]:
            left[name] = left.get(name, 0) + 1
            continue
        assert (a["num_trials"], a["num_inliers"], a["success"]) == (b["num_trials"], b["num_inliers"], b["success"]), name
        if a["num_inliers"] >= 7:
            assert any((a["inliers"] == c["inliers"]).all() and np.linalg.norm(a["F"] - c["F"]) <= fr.F_TOL for c in [b] + b["either"]), name
    print("left out per table:", {k: f"{left.get(k, 0)} of {v}" for k, v in total.items()})
    for name, n in total.items():
        assert left.get(name, 0) <= n // 10, name
    for (n, _, _, _), ref in zip(fr.RANSAC_CASES, fr.ransac_refs()):
        if n in (7, 8):
            assert not ref["banded"], (n, ref["why"])          # reason (b) alone may touch these, and it is answered by 'either'
    for f in fr.PROBE_FAMILIES[:3]:
        assert fr.probe_disagreement(f)[1] >= fr.PROBES * 9 // 10
    refs = fr.ransac_refs() + [fr.option_ref(**c) for c in fr.OPTION_RUNS]
    # the cases do what they are there for: several rounds, both trial limits, partial rounds
    assert {r["num_trials"] for r in refs} >= {1, 255, 256, 257, 300, 512, 600, 2816, 10000}


def test_breaking_a_rule_shows():
    """Each rule break changes trials, count, mask or F on one of the committed table cases with 40 or 80 correspondences and up to half
    of them false: the comparison can tell them apart."""
    picks = [k for k, (n, o, _, _) in enumerate(fr.RANSAC_CASES) if n in (40, 80) and o <= 0.5]

    def differs(r, base):
        return (r["num_trials"], r["num_inliers"]) != (base["num_trials"], base["num_inliers"]) or (r["inliers"] != base["inliers"]).any() \
            or np.linalg.norm(r["F"] - base["F"]) > fr.F_TOL
    for brk in (dict(multiplier=2.0), dict(lo=False), dict(drop_root=True), dict(smaller_sum=False)):
        hit = []
        for k in picks:
            p0, p1, th = fr.ransac_cases()[k]
            if differs(fr.fundamental_ref(p0, p1, th, **brk), fr.ransac_refs()[k]):
                hit.append(k)
                break
        assert hit, brk
