"""numpy restatement of the homography estimator for the tests only (never imported by the product), written from the
text and not from the kernel: the sampling on integers, a four-point solver that shares no step with the kernel's (route A: the SVD
null space of the 8 x 9 DLT system, collinearity through numpy's determinants; the kernel is the closed form through projective
bases), each image's own normalisation, the fp64 one-sided transfer error, the LO-RANSAC rounds with their support order and stopping
rule, the 8-parameter chart of the refinement, the final Levenberg-Marquardt and the output convention.  Route B (four_point_basis) is
the closed form of item 3, written from the same text, against which route A is measured on the CPU
(tests/test_homography_ref_host.py).  Also the committed cases the GPU tests (tests/test_gpu_homography.py) and the CPU checks share,
and the scenes of the E / F / H decision."""
import functools

import numpy as np

import fundamental_ref as fr
import pose_ref as pr
import ransac_ref as rr
import two_view_ref as tv

ROUND = rr.ROUND
LO_STEPS, LO_GN, REF_ITERS = 8, 3, 50
COLLINEAR = 1e-12            # a triple product at or below this times the three vectors' norms: no hypothesis
NEAR = pr.NEAR               # a degeneracy measure within this factor of its threshold is too close to call
# BAND, derived (measure_band() below, asserted by tests/test_homography_ref_host.py): over the exact probe families the largest
# relative disagreement in squared transfer error, at points 1 px off their exact place, between four_point_dlt's matrix and the
# generating matrix is MEASURED; the band is 100 x that.  It is used, relative, around the inlier threshold and for "equal" sums.
MEASURED = 7.0e-7
BAND = 100 * MEASURED
# H_TOL, derived (measure_routes(), asserted by the same host test): the largest distance between the unit-norm pixel matrices the whole
# estimator returns with route A and with route B over the committed cases is H_MEASURED; the tolerance is 100 x that (the margin covers
# differences in summation order across up to 50 refinement steps), and may not exceed H_CEILING.
H_MEASURED = 3.0e-10
H_TOL = 100 * H_MEASURED
H_CEILING = 1e-6
EXACT_SUM = 1e-24            # a sum of squared transfer errors (normalised) below this is that of an exact solution (rounding only)
_hom = tv._hom
sample_k = lambda seed, trial, n: rr.sample_k(seed, trial, n, 4)          # noqa: E731
sample_kv = lambda seed, trials, n: rr.sample_kv(seed, trials, n, 4)      # noqa: E731
_unit = fr._unit
_hdist = fr._fdist           # distance of unit-norm matrices up to sign


# ------------------------------------------------------------------------------------------------------------ error and support
def transfer_f64(H, x0, x1):
    """|x1 - pi(H x0)|^2, H [..., 3, 3], x0, x1 [n, 2] -> [..., n]; NaN or inf where the denominator is 0."""
    y = np.einsum("...ij,nj->...ni", np.asarray(H, np.float64), _hom(x0))
    with np.errstate(all="ignore"):
        d = x1 - y[..., :2] / y[..., 2:]
        return np.sum(d * d, -1)


def support(H, x0, x1, th2):
    """(count, sum of the inliers' errors, errors): an inlier has e <= th2; a NaN or infinite e is none."""
    e = transfer_f64(H, x0, x1)
    with np.errstate(invalid="ignore"):
        inl = e <= th2
    return inl.sum(-1), np.where(inl, e, 0.0).sum(-1), e


# ------------------------------------------------------------------------------------------------------------ four-point solvers
def _collinearity(x):
    """x [T, 4, 2]: the smallest |det [pi pj pk]| / (|pi| |pj| |pk|) over the four triples, through numpy's determinant."""
    p = _hom(x)
    nrm = np.linalg.norm(p, axis=-1)
    out = np.full(len(x), np.inf)
    for tri in ((0, 1, 2), (3, 1, 2), (0, 3, 2), (0, 1, 3)):
        t = list(tri)
        out = np.minimum(out, np.abs(np.linalg.det(p[:, t])) / np.prod(nrm[:, t], 1))
    return out


def _wrap(Hs, good, near):
    with np.errstate(all="ignore"):
        Hs = _unit(Hs)
    good = good & np.isfinite(Hs).all((1, 2))
    h = np.flatnonzero(good)
    return Hs[h], h.astype(np.int64), near


def four_point_dlt(x0, x1):
    """Route A.  x0, x1 [T, 4, 2] normalised samples.  Returns (H [K, 3, 3] unit Frobenius norm, owner [K] = row of the sample, near [T] =
    too close to call: a collinearity measure within a factor NEAR of its threshold, on either side).  The matrix is the right singular vector
    of the smallest singular value of the 8 x 9 system of the rows (0, -w' x, y' x), (w' x, 0, -x' x)."""
    T = len(x0)
    a = _hom(x0)
    A = np.zeros((T, 8, 9))
    A[:, 0::2, 3:6] = -a
    A[:, 0::2, 6:9] = x1[:, :, 1:2] * a
    A[:, 1::2, 0:3] = a
    A[:, 1::2, 6:9] = -x1[:, :, 0:1] * a
    with np.errstate(all="ignore"):
        ok = np.isfinite(A).all((1, 2))
        A[~ok] = 0.0
        _, _, Vt = np.linalg.svd(A)
        col = np.minimum(_collinearity(x0), _collinearity(x1))
    good = ok & (col > COLLINEAR)
    return _wrap(Vt[:, 8].reshape(T, 3, 3), good, (col <= NEAR * COLLINEAR) & (col >= COLLINEAR / NEAR))


def _basis(x):
    """Item 3: lambda of [p1 p2 p3] lambda = p4 through cross and triple products; (A [T, 3, 3] with the columns lambda_i p_i, ok, near)."""
    p = _hom(x)
    p1, p2, p3, p4 = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    n1, n2, n3, n4 = (np.linalg.norm(q, axis=1) for q in (p1, p2, p3, p4))
    c23, c31, c12 = np.cross(p2, p3), np.cross(p3, p1), np.cross(p1, p2)
    d = np.sum(p1 * c23, 1)
    t1, t2, t3 = np.sum(p4 * c23, 1), np.sum(p4 * c31, 1), np.sum(p4 * c12, 1)
    with np.errstate(all="ignore"):
        rel = np.stack([np.abs(d) / (n1 * n2 * n3), np.abs(t1) / (n4 * n2 * n3), np.abs(t2) / (n1 * n4 * n3), np.abs(t3) / (n1 * n2 * n4)], 1).min(1)
        A = np.stack([(t1 / d)[:, None] * p1, (t2 / d)[:, None] * p2, (t3 / d)[:, None] * p3], 2)
    return A, rel > COLLINEAR, (rel <= NEAR * COLLINEAR) & (rel >= COLLINEAR / NEAR)


def four_point_basis(x0, x1):
    """Route B, the closed form of item 3: H = B adj(A) at unit Frobenius norm.  Same return as four_point_dlt."""
    A, oka, na = _basis(x0)
    B, okb, nb = _basis(x1)
    a1, a2, a3 = A[:, :, 0], A[:, :, 1], A[:, :, 2]
    with np.errstate(all="ignore"):
        adj = np.stack([np.cross(a2, a3), np.cross(a3, a1), np.cross(a1, a2)], 1)
        Hs = B @ adj
    return _wrap(Hs, oka & okb, na | nb)


# ------------------------------------------------------------------------------------------------------------ the chart
def make_chart(H):
    """The first entry of largest magnitude (row-major) is held constant: (fix, free indices, ok)."""
    h = np.asarray(H, np.float64).reshape(9)
    fix = int(np.argmax(np.abs(h)))
    return fix, [q for q in range(9) if q != fix], bool(np.isfinite(h).all() and abs(h[fix]) > 0)


def normal_equations(H, free, x0, x1, w):
    """Two residuals per point, the x and y transfer differences; the 8 parameters are the free entries of H in order.  x0, x1 [m, 2],
    w [m] weights (0 / 1).  Returns (J^T J, J^T r, r^T r)."""
    on = w > 0
    a, b = _hom(x0[on]), x1[on]
    with np.errstate(all="ignore"):
        y = a @ np.asarray(H).reshape(3, 3).T
        iw = 1.0 / y[:, 2]
        u, v = y[:, 0] * iw, y[:, 1] * iw
        ai = a * iw[:, None]
        z = np.zeros_like(ai)
        Jx = np.concatenate([ai, z, -u[:, None] * ai], 1)[:, free]
        Jy = np.concatenate([z, ai, -v[:, None] * ai], 1)[:, free]
        J = np.concatenate([Jx, Jy], 0)
        r = np.concatenate([u - b[:, 0], v - b[:, 1]])
        return J.T @ J, J.T @ r, float(r @ r)


def apply_update(H, free, d):
    h = np.asarray(H, np.float64).reshape(9).copy()
    h[free] += d
    return h.reshape(3, 3)


# ------------------------------------------------------------------------------------------------------------ LO-RANSAC
num_trials_needed, trial_limits = rr.trial_rule(4)       # COLMAP's ComputeNumTrials and trial limits for sample size 4


def _distinct(Ha, Hb):
    return float(_hdist(Ha, Hb)) > 1e-8


def _lo_step(carried, H, inl, x0, x1):
    """One re-estimation: LO_GN Gauss-Newton steps over the inliers on a new chart of the current best, on the matrix itself."""
    fix, free, ok = make_chart(H)
    for _ in range(LO_GN):
        if not ok:
            return None
        Hm, g, _ = normal_equations(H, free, x0, x1, inl)
        d, ok = rr.damped_solve(Hm, g)
        if ok:
            H = apply_update(H, free, d)
    return (carried, H) if ok else None


# The rounds are ransac_ref.lo_ransac's.  A winner that fits its inliers to rounding is exact whatever their number (n = 5 with a wrong
# match: every sample without it holds its 4), and here alone such fits are carried across rounds and "near" is said of any sample
# of the round (a sample too close to the collinearity threshold may or may not give a hypothesis: reason (c)); an error may be NaN.
MODEL = rr.Model(name="H", sample_size=4, solver=four_point_dlt, support=support, error=transfer_f64, distinct=_distinct,
                 band=BAND, exact_sum=EXACT_SUM, lo_steps=LO_STEPS, lo_start=lambda H: None, lo_step=_lo_step,
                 nan_errors=True, carries_exact=True, near_any_sample=True)


# lo_ransac_ref(x0, x1, th2, **conf): {'H' (None without a hypothesis), 'cnt', 'sum', 'trials', 'banded', 'why', 'either'}; solver: the route.
lo_ransac_ref = functools.partial(rr.lo_ransac, MODEL)


def final_stage(H, mask, x0, x1):
    """Levenberg-Marquardt over the masked correspondences on make_chart(H).  Returns H refined, or None."""
    fix, free, ok = make_chart(H)
    if not ok:
        return None
    w = mask.astype(np.float64)
    H = np.asarray(H, np.float64).reshape(3, 3)
    return rr.levenberg_marquardt(H, lambda M: normal_equations(M, free, x0, x1, w), rr.damped_solve,
                                  lambda M, d: apply_update(M, free, d), REF_ITERS)[0]


def normalisation(p0, p1):
    """(c0, c1, s0, s1): each image's centroid and scale sqrt(2) / mean distance; the scales are None when a set has no extent."""
    c0, c1 = p0.mean(0), p1.mean(0)
    d0, d1 = np.mean(np.linalg.norm(p0 - c0, axis=1)), np.mean(np.linalg.norm(p1 - c1, axis=1))
    if not (np.isfinite(d0) and np.isfinite(d1) and d0 > 0 and d1 > 0):
        return c0, c1, None, None
    return c0, c1, np.sqrt(2.0) / d0, np.sqrt(2.0) / d1


def _T(c, s):
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def to_pixels(H, c0, c1, s0, s1):
    """T1^-1 H T0 at unit Frobenius norm, the first entry of largest magnitude positive."""
    P = np.linalg.inv(_T(c1, s1)) @ H @ _T(c0, s0)
    P = P / np.linalg.norm(P)
    return P if P.reshape(-1)[int(np.argmax(np.abs(P)))] > 0 else -P


def homography_ref(p0, p1, max_error_px=4.0, min_num_inliers=15, solver=four_point_dlt, **conf):
    """The whole estimator on pixels.  Returns {'success', 'H' (pixels), 'num_inliers', 'inliers', 'num_trials', 'banded', 'why',
    'either': [{'H', 'inliers'}] of the other exact fits of as many points, each as right an answer as the first}."""
    p0, p1 = np.asarray(p0, np.float64).reshape(-1, 2), np.asarray(p1, np.float64).reshape(-1, 2)
    n = len(p0)
    out = {"success": False, "H": np.zeros((3, 3)), "num_inliers": 0, "inliers": np.zeros(n, bool), "num_trials": 0, "banded": False,
           "why": [], "either": []}
    if n < 4:
        return out
    c0, c1, s0, s1 = normalisation(p0, p1)
    if s0 is None:
        return out
    x0, x1 = s0 * (p0 - c0), s1 * (p1 - c1)
    th2 = (s1 * max_error_px) ** 2
    r = lo_ransac_ref(x0, x1, th2, solver=solver, **conf)
    out["num_trials"], out["banded"], out["why"] = r["trials"], r["banded"], r["why"]
    if r["cnt"] < 4:
        return out
    with np.errstate(invalid="ignore"):
        mask = transfer_f64(r["H"], x0, x1) <= th2
    H = final_stage(r["H"], mask, x0, x1)
    if H is None:
        return out
    out.update(H=to_pixels(H, c0, c1, s0, s1), num_inliers=r["cnt"], inliers=mask, success=bool(r["cnt"] >= min_num_inliers))
    for Hk in r["either"]:
        with np.errstate(invalid="ignore"):
            mk = transfer_f64(Hk, x0, x1) <= th2
        He = final_stage(Hk, mk, x0, x1)
        if He is not None:
            out["either"].append({"H": to_pixels(He, c0, c1, s0, s1), "inliers": mk})
    return out


def compare(r, ref, worst):
    """A device result (two_view.homography's dict) against homography_ref's: trials, count and mask equal; success; H within H_TOL of
    the restatement's answer or one of its 'either'.  worst [0] keeps the largest difference."""
    assert r["num_trials"] == ref["num_trials"] and r["num_inliers"] == ref["num_inliers"], \
        (r["num_trials"], ref["num_trials"], r["num_inliers"], ref["num_inliers"])
    assert r["success"] == ref["success"]
    if ref["num_inliers"] < 4:
        assert not r["inliers"].any() and not r["H"].any()
        return
    cands = [c for c in [ref] + ref["either"] if (r["inliers"] == c["inliers"]).all()]
    assert cands, "inlier mask"
    d = min(float(np.linalg.norm(r["H"] - c["H"])) for c in cands)
    worst[0] = max(worst[0], d)
    assert d <= H_TOL, d


# ------------------------------------------------------------------------------------------------------------ scenes and cases
_cached = rr.make_cached()
CAM0, CAM1 = fr.CAM0, fr.CAM1


def _K(c):
    return np.array([[c["params"][0], 0, c["params"][2]], [0, c["params"][1], c["params"][3]], [0, 0, 1.0]])


def plane_H(rs, rotation=False):
    """A pixel homography between the two pinhole cameras: K1 (R + t n^T / d) K0^-1 of a tilted plane 6 units away under a rotation of
    1-14 degrees and a baseline of 0.6-1.8 units, or K1 R K0^-1 alone."""
    w = rs.standard_normal(3)
    w *= rs.uniform(0.02, 0.25) / np.linalg.norm(w)
    R = tv._exp_so3(w[None])[0]
    M = R
    if not rotation:
        nrm = np.array([rs.uniform(-0.3, 0.3), rs.uniform(-0.3, 0.3), 1.0])
        t = rs.standard_normal(3) * [1, 1, 0.3]
        t *= rs.uniform(0.6, 1.8) / np.linalg.norm(t)
        M = R + np.outer(t, nrm) / (6.0 * nrm[2])
    H = _K(CAM1) @ M @ np.linalg.inv(_K(CAM0))
    return H / np.linalg.norm(H)


def apply_H(H, p):
    y = _hom(p) @ H.T
    return y[:, :2] / y[:, 2:]


def _pixels(rs, n):
    W, Hh = CAM0["width"], CAM0["height"]
    return np.stack([rs.uniform(0.05 * W, 0.95 * W, n), rs.uniform(0.05 * Hh, 0.95 * Hh, n)], 1)


def scene(seed, n, outlier_ratio=0.0, noise_px=0.0, rotation=False):
    """n correspondences of a plane (or a rotation) between the two cameras, which the estimator never sees: a fraction replaced in
    image 1 by random pixels, Gaussian noise on both images of the rest.  Returns (H, p0, p1, outliers)."""
    rs = np.random.RandomState(seed)
    H = plane_H(rs, rotation)
    p0 = _pixels(rs, n)
    p1 = apply_H(H, p0)
    p0 = p0 + noise_px * rs.standard_normal(p0.shape)
    p1 = p1 + noise_px * rs.standard_normal(p1.shape)
    out = np.zeros(n, dtype=bool)
    no = int(round(outlier_ratio * n))
    if no:
        idx = rs.choice(n, no, replace=False)
        out[idx] = True
        p1[idx] = np.stack([rs.uniform(0, CAM1["width"], no), rs.uniform(0, CAM1["height"], no)], 1)
    return H, p0, p1, out


# the RANSAC table: every n with every outlier ratio, 0.5 px noise, at both thresholds
TABLE_NS = (4, 5, 8, 40, 80, 300)
TABLE_OUTLIERS = (0.0, 0.25, 0.5, 0.7)
TABLE_SEED = 700
RANSAC_CASES = [(n, o, TABLE_SEED + 10 * i + j, th) for i, n in enumerate(TABLE_NS) for j, o in enumerate(TABLE_OUTLIERS) for th in (4.0, 1.0)]


def ransac_cases():
    """[(p0, p1, max_error_px)] of RANSAC_CASES."""
    return _cached("cases", lambda: [scene(seed, n, o, 0.5)[1:3] + (th,) for n, o, seed, th in RANSAC_CASES])


def ransac_refs(solver=four_point_dlt):
    return _cached(("refs", solver.__name__), lambda: [homography_ref(p0, p1, th, solver=solver) for p0, p1, th in ransac_cases()])


OPTION_SCENE = (40, 0.5, 721, 4.0)
OPTION_RUNS = [dict(seed=1), dict(seed=2), dict(seed=3), dict(max_num_trials=1), dict(max_num_trials=255), dict(max_num_trials=256),
               dict(max_num_trials=257), dict(max_num_trials=512), dict(min_num_trials=5000, max_num_trials=600), dict(confidence=0.0),
               dict(confidence=1.0, max_num_trials=600), dict(min_inlier_ratio=0.0, max_num_trials=600), dict(min_inlier_ratio=1.0),
               dict(seed=2 ** 64 - 1), dict(seed=2 ** 63)]


def option_case():
    n, o, seed, th = OPTION_SCENE
    return _cached("option", lambda: scene(seed, n, o, 0.5)[1:3] + (th,))


def option_ref(solver=four_point_dlt, **conf):
    p0, p1, th = option_case()
    return _cached(("option_ref", solver.__name__, tuple(sorted(conf.items()))), lambda: homography_ref(p0, p1, th, solver=solver, **conf))


# the correspondences are walked in strides of 256: one under, at and over one and two strides, over four
SIZE_NS = (255, 256, 257, 511, 513, 1025)
SIZE_FILL = (0, 3, 4)        # pairs of these sizes stand between the size cases in the batch


def size_cases():
    """[(p0, p1, max_error_px)]: SIZE_NS with 30 % outliers and 0.5 px noise, each followed by pairs of 0, 3 and 4 correspondences."""
    def make():
        out = []
        for i, n in enumerate(SIZE_NS):
            out.append(scene(800 + i, n, 0.3, 0.5)[1:3] + (4.0,))
            for j, m in enumerate(SIZE_FILL):
                out.append((scene(850 + 3 * i + j, m, 0.0, 0.5)[1:3] if m else (np.zeros((0, 2)), np.zeros((0, 2)))) + (4.0,))
        return out
    return _cached("size_cases", make)


def size_refs(solver=four_point_dlt):
    return _cached(("size_refs", solver.__name__), lambda: [homography_ref(p0, p1, th, solver=solver) for p0, p1, th in size_cases()])


# Solver probes: one trial (max_num_trials = 1, the sample is sample_k(0, 0, n)) on n = 5 or 6 exact correspondences
PROBE_FAMILIES = ["plane", "rotation", "identical", "edge_on", "far", "collinear_1e-1", "collinear_1e-2", "collinear_1e-3"]
PROBES = 256
PROBE_ERROR_PX = 0.05
PROBE_CONF = dict(max_num_trials=1, min_num_inliers=4)


def _edge_on_H(rs, p0):
    """A homography whose vanishing line in image 0 passes close by one of the points p0: the denominator of that point is 0.03 ..
    0.1 of the largest one, so its image lies 10 to 30 image widths away (closer than that, the far point alone sets image 1's scale, the
    others collapse into a cluster, and the two routes of this file disagree by up to 0.1 in relative error: measured at 1e-3 .. 1e-2)."""
    c = np.array([CAM0["width"], CAM0["height"]]) / 2.0
    a = rs.uniform(0, 2 * np.pi)
    u = np.array([np.cos(a), np.sin(a)])
    s = (p0 - c) @ u
    eps = 10 ** rs.uniform(-1.5, -1)
    k = (1.0 - eps) / (-s.min())
    H = np.array([[0.7, 0.05, 30.0], [-0.04, 0.72, 20.0], [k * u[0], k * u[1], 1.0 - k * (c @ u)]])
    return H / np.linalg.norm(H)


def probes(family):
    """[(p0, p1, H generating, max_error_px)] of one family, PROBES of them, every correspondence exact."""
    def make():
        rs = np.random.RandomState(4000 + PROBE_FAMILIES.index(family))
        out = []
        for i in range(PROBES):
            n = 5 + (i & 1)
            p0 = _pixels(rs, n)
            H = plane_H(rs, rotation=family == "rotation")
            if family == "identical":
                H = np.eye(3) / np.sqrt(3.0)
            if family == "edge_on":
                H = _edge_on_H(rs, p0)
            if family.startswith("collinear"):          # the sample's third point next to the line through its first two
                i1, i2, i3, _ = sample_k(0, 0, n)
                d = p0[i2] - p0[i1]
                p0[i3] = p0[i1] + rs.uniform(0.3, 0.7) * d + float(family.split("_")[1]) * np.array([-d[1], d[0]])
            p1 = apply_H(H, p0)
            if family == "far":
                T0, T1 = np.eye(3), np.eye(3)
                T0[:2, 2], T1[:2, 2] = -1e4, 1e4
                p0, p1, H = p0 + 1e4, p1 + 1e4, T1 @ H @ T0
                H = H / np.linalg.norm(H)
            out.append((p0, p1, H, PROBE_ERROR_PX))
        return out
    return _cached(("probes", family), make)


def probe_refs(family, solver=four_point_dlt):
    return _cached(("probe_refs", family, solver.__name__),
                   lambda: [homography_ref(p0, p1, th, solver=solver, **PROBE_CONF) for p0, p1, _, th in probes(family)])


def probe_disagreement(family):
    """Per probe whose sample yields the generating matrix: the relative disagreement in squared transfer error, at points 1 px off
    their exact place, between four_point_dlt's matrix and the generating one (normalised coordinates); and how many samples yield it."""
    dis, found = [], 0
    for p0, p1, Ht, _ in probes(family):
        c0, c1, s0, s1 = normalisation(p0, p1)
        x0, x1 = s0 * (p0 - c0), s1 * (p1 - c1)
        idx = list(sample_k(0, 0, len(p0)))
        Hs, _, near = four_point_dlt(x0[idx][None], x1[idx][None])
        Hn = _unit(_T(c1, s1) @ Ht @ np.linalg.inv(_T(c0, s0)))
        if near[0] or not len(Hs):
            continue
        if _hdist(Hs[0], Hn) < 1e-6:
            found += 1
            y1 = x1 + s1 * np.array([0.6, 0.8])
            a, b = transfer_f64(Hs[0], x0, y1), transfer_f64(Hn, x0, y1)
            dis.append(float(np.max(np.abs(a - b) / b)))
    return dis, found


def measure_band():
    """The largest disagreement of probe_disagreement over the probe families (all exact)."""
    return max(max(probe_disagreement(f)[0]) for f in PROBE_FAMILIES)


# name -> options: inputs without a homography.  `line`: every sample is collinear, no hypothesis in max_num_trials trials; `repeated` and
# the pairs below 4: after 0 trials.  Each: success False, no inliers, H = 0.
DEGENERATE = {"line": dict(max_num_trials=512), "repeated": dict(max_num_trials=512), "n0": {}, "n1": {}, "n3": {}}


def degenerate(name):
    """(p0, p1): line -- 40 exact correspondences of points on one line of image 0; repeated -- one correspondence 20 times; n0, n1, n3 --
    that many correspondences."""
    def make():
        if name == "line":
            rs = np.random.RandomState(904)
            H = plane_H(rs)
            p0 = np.array([100.0, 200.0]) + np.sort(rs.uniform(0, 1, 40))[:, None] * np.array([640.0, 256.0])
            return p0, apply_H(H, p0)
        if name == "repeated":
            _, p0, p1, _ = scene(903, 1)                         # on a grid of 1/8 px: every sum of 20 is exact, the mean distance is 0
            return np.tile(np.round(p0 * 8) / 8, (20, 1)), np.tile(np.round(p1 * 8) / 8, (20, 1))
        m = int(name[1:])
        return scene(905, m)[1:3] if m else (np.zeros((0, 2)), np.zeros((0, 2)))
    return _cached(("degenerate", name), make)


def degenerate_ref(name):
    p0, p1 = degenerate(name)
    return _cached(("degenerate_ref", name), lambda: homography_ref(p0, p1, 4.0, **DEGENERATE[name]))


def all_ref_pairs():
    """[(name, route A result, route B result)] over every committed case that has a restatement."""
    out = [("table", a, b) for a, b in zip(ransac_refs(), ransac_refs(four_point_basis))]
    out += [("option", option_ref(**c), option_ref(four_point_basis, **c)) for c in OPTION_RUNS]
    out += [("size", a, b) for a, b in zip(size_refs(), size_refs(four_point_basis))]
    for f in PROBE_FAMILIES:
        out += [("probe " + f, a, b) for a, b in zip(probe_refs(f), probe_refs(f, four_point_basis))]
    return out


def measure_routes():
    """The largest distance between the pixel matrices of the two routes over the cases neither route leaves out (each against the
    other's answer or one of its 'either')."""
    worst = 0.0
    for _, a, b in all_ref_pairs():
        if a["banded"] or b["banded"] or a["num_inliers"] < 4:
            continue
        worst = max(worst, min(float(np.linalg.norm(a["H"] - c["H"])) for c in [b] + b["either"]))
    return worst


# ------------------------------------------------------------------------------------------------------------ the decision's scenes
DECISION_N = 300
DECISION_SCENES = ["general", "plane", "rotation", "half_plane", "random"]
# with cameras, without
DECISION_EXPECT = {"general": ("calibrated", "uncalibrated"), "plane": ("planar", "planar_or_panoramic"),
                   "rotation": ("panoramic", "planar_or_panoramic"), "half_plane": ("calibrated", "uncalibrated"),
                   "random": ("degenerate", "degenerate")}


# the random scene's cameras: wide images, where a chance inlier of any model is rare (in 640 x 480 the epipolar band of 4 px holds 2 %
# of the random pixels, and F collects 27 of 300)
BIG0 = {"model": "PINHOLE", "width": 4096, "height": 3072, "params": [3200.0, 3200.0, 2048.0, 1536.0]}
BIG1 = {"model": "PINHOLE", "width": 4096, "height": 3072, "params": [3000.0, 3050.0, 2048.0, 1536.0]}


def decision_scene(name):
    """(p0, p1, camera 0, camera 1) of DECISION_N matches with 0.5 px noise and no false ones: the rule's first test is nE >= 0.95 nF, and
    with nE = nF = n its margin is 5 % of n, the one the host test asks for; every false match takes from it."""
    def make():
        k = DECISION_SCENES.index(name)
        if name == "general":
            return fr.scene(1100 + k, DECISION_N, 0.0, 0.5)[2:4] + (CAM0, CAM1)
        if name == "plane":
            return fr.scene(1100 + k, DECISION_N, 0.0, 0.5, planar=True)[2:4] + (CAM0, CAM1)
        if name == "rotation":
            return fr.scene(1100 + k, DECISION_N, 0.0, 0.5, baseline=0.0)[2:4] + (CAM0, CAM1)
        rs = np.random.RandomState(1100 + k)
        if name == "half_plane":                              # one pose: half of the points on a plane, the other half anywhere
            px = _pixels(rs, DECISION_N)
            xn = pr.undistort(CAM0, px)
            d = 1.0 / rs.uniform(1.0 / 20, 1.0 / 2, DECISION_N)
            nrm = np.array([0.2, -0.1, 1.0])
            half = np.arange(DECISION_N) % 2 == 0
            d[half] = (6.0 * nrm[2] / (_hom(xn) @ nrm))[half]
            X = _hom(xn) * d[:, None]
            R = tv._exp_so3(np.array([[0.05, -0.12, 0.03]]))[0]
            t = np.array([1.0, 0.2, 0.1])
            p0, _ = pr.project(CAM0, [1.0, 0, 0, 0], np.zeros(3), X)
            p1, z1 = pr.project(CAM1, pr.rotmat2qvec(R), t, X)
            assert (z1 > 0).all()
            p0, p1 = p0 + 0.5 * rs.standard_normal(p0.shape), p1 + 0.5 * rs.standard_normal(p1.shape)
            return p0, p1, CAM0, CAM1
        return tuple(np.stack([rs.uniform(0, c["width"], DECISION_N), rs.uniform(0, c["height"], DECISION_N)], 1) for c in (BIG0, BIG1)) + (BIG0, BIG1)
    return _cached(("decision", name), make)


def decision_refs(name):
    """The three restatements' results on a decision scene: (E of two_view_ref with two_view.relative_pose's 'small_baseline' -- the median
    angle over the inliers with a finite one below 1.5 degrees --, F of fundamental_ref, H of this file)."""
    def make():
        p0, p1, c0, c1 = decision_scene(name)
        E = tv.relative_pose_ref(p0, p1, c0, c1)
        fin = E["angles"][E["inliers"] & np.isfinite(E["angles"])]
        E["small_baseline"] = bool(fin.size and np.median(fin) < 1.5)
        return E, fr.fundamental_ref(p0, p1), homography_ref(p0, p1)
    return _cached(("decision_refs", name), make)
