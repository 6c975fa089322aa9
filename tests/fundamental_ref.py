"""numpy restatement of the fundamental-matrix estimator for the tests only (never imported by the product), written
from the text and not from the kernel: the sampling on integers, a seven-point solver that shares no step with the kernel's (route A:
SVD null space, the cubic through four determinant evaluations, numpy.roots; the kernel reduces by Gauss-Jordan with full pivoting
and brackets the roots between the derivative's critical points), the common normalisation, the fp64 Sampson error, the LO-RANSAC
rounds with their support order and stopping rule, the rank-2 chart of the refinement (which follows the text exactly: the end point of
a Gauss-Newton run depends on the chart), the final Levenberg-Marquardt and the output convention.  Route B (seven_point_gj) is a
second solver written from the same text -- Gauss-Jordan, modified Gram-Schmidt, the bracketing root finder -- against which route A
is measured on the CPU (tests/test_fundamental_ref_host.py).  Also the committed cases the GPU tests (tests/test_gpu_fundamental.py)
and the CPU checks share."""
import functools

import numpy as np

import pose_ref as pr
import ransac_ref as rr
import two_view_ref as tv

ROUND = rr.ROUND
LO_STEPS, LO_GN, REF_ITERS, POLISH = 8, 3, 50, 3
RANK_MIN = 1e-12             # route A: sigma_7 / sigma_1 of the 7 x 9 system at or below which a sample gives no hypothesis
PIVOT_MIN = 1e-12            # route B (and the kernel): a pivot at or below this times max|A|
LEAD_MIN = 1e-12             # the cubic's leading coefficient at or below this times its largest coefficient
NEAR = pr.NEAR               # a degeneracy measure within this factor of its threshold is too close to call
ROOT_SEP = 1e-3              # two solutions of one sample closer than this (unit-norm matrices, up to sign) are too close to call
# BAND, derived (measure_band() below, asserted by tests/test_fundamental_ref_host.py): over the probe families the largest relative
# disagreement in squared Sampson error, at points 1 px off their exact place, between seven_point_ref's matrix and the generating
# matrix is MEASURED; the band is 100 x that.  It is used, relative, around the inlier threshold and for "equal" sums.
MEASURED = 2.5e-9
BAND = 100 * MEASURED
# F_TOL, derived (measure_routes(), asserted by the same host test): the largest distance between the unit-norm pixel matrices the
# whole estimator returns with route A and with route B over the committed cases is F_MEASURED; the tolerance is 100 x that (the margin
# covers differences in summation order across up to 50 refinement steps, DESIGN.md 15's margin), and may not exceed F_CEILING.
F_MEASURED = 6.0e-9
F_TOL = 100 * F_MEASURED
F_CEILING = 1e-6
EXACT_SUM = 1e-24            # a sum of squared Sampson errors (normalised) below this is that of an exact solution (rounding only)
mix64 = rr.mix64
_hom = tv._hom
sampson_f64 = tv.sampson_f64
support = tv.support


# the sampling on integers is ransac_ref's (one scheme for every sample size), at sample size 7 unless told otherwise
sample_k = lambda seed, trial, n, k=7: rr.sample_k(seed, trial, n, k)            # noqa: E731
sample_kv = lambda seed, trials, n, k=7: rr.sample_kv(seed, trials, n, k)        # noqa: E731


# ------------------------------------------------------------------------------------------------------------ seven-point, route A
def _unit(F):
    return F / np.sqrt(np.sum(F * F, (-1, -2)))[..., None, None]


def _fdist(a, b):
    """Distance of unit-norm matrices up to sign."""
    a, b = _unit(a), _unit(b)
    return np.minimum(np.linalg.norm(a - b, axis=(-1, -2)), np.linalg.norm(a + b, axis=(-1, -2)))


def _system(x0, x1):
    H = len(x0)
    return (_hom(x1)[:, :, :, None] * _hom(x0)[:, :, None, :]).reshape(H, 7, 9)


def _finish(Y, W, coef, good, near, x, drop_root=False):
    """x [H, 3]: the real roots of every sample's cubic in ascending order, NaN where there is none.  POLISH Newton steps each, the
    matrices at unit norm; near also where two solutions are closer than ROOT_SEP."""
    c3, c2, c1, c0 = (coef[:, k, None] for k in range(4))
    with np.errstate(all="ignore"):
        for _ in range(POLISH):
            xn = x - (((c3 * x + c2) * x + c1) * x + c0) / ((3 * c3 * x + 2 * c2) * x + c1)
            x = np.where(np.isfinite(xn), xn, x)
        cand = _unit(x[:, :, None, None] * Y[:, None] + W[:, None])             # [H, 3, 3, 3]
    have = good[:, None] & np.isfinite(cand).all((2, 3))
    if drop_root:                                                               # every sample loses its last solution
        last = (np.cumsum(have[:, ::-1], 1)[:, ::-1] == 1) & have
        have &= ~last
    for i in range(3):
        for j in range(i + 1, 3):
            with np.errstate(all="ignore"):
                close = _fdist(cand[:, i], cand[:, j]) < ROOT_SEP
            near |= have[:, i] & have[:, j] & close
    h, k = np.nonzero(have)
    return cand[h, k], h.astype(np.int64), near


def seven_point_ref(x0, x1, drop_root=False):
    """x0, x1 [H, 7, 2] normalised samples.  Returns (F [K, 3, 3] unit Frobenius norm, owner [K] = row of the sample, a sample's matrices
    in ascending order of the root; near [H] = too close to call: the rank measure or the leading coefficient within NEAR of its
    threshold, a complex pair within ROOT_SEP of the real axis, two solutions closer than ROOT_SEP).  Route: SVD null space, Y the
    basis vector of the larger |det|, the cubic det(x Y + W) through its values at -1, 0, 1, 2, and numpy.roots' method (LAPACK's
    eigenvalues of the companion matrix) on all samples at once."""
    H = len(x0)
    _, S, Vt = np.linalg.svd(_system(x0, x1))
    rank = S[:, 6] / S[:, 0]
    N0, N1 = Vt[:, 7].reshape(H, 3, 3), Vt[:, 8].reshape(H, 3, 3)
    swap = np.abs(np.linalg.det(N1)) > np.abs(np.linalg.det(N0))
    Y, W = np.where(swap[:, None, None], N1, N0), np.where(swap[:, None, None], N0, N1)
    xs = np.array([-1.0, 0.0, 1.0, 2.0])
    dets = np.stack([np.linalg.det(x * Y + W) for x in xs], 1)
    coef = np.linalg.solve(np.vander(xs, 4), dets.T).T            # c3 c2 c1 c0
    cmax = np.abs(coef).max(1)
    with np.errstate(all="ignore"):
        lead = np.abs(coef[:, 0]) / cmax
    good = (rank > RANK_MIN) & np.isfinite(coef).all(1) & (lead > LEAD_MIN)
    near = ~good | (rank <= NEAR * RANK_MIN) | (lead <= NEAR * LEAD_MIN)

    comp = np.zeros((H, 3, 3))
    with np.errstate(all="ignore"):
        comp[:, 0] = -coef[:, 1:] / coef[:, :1]
    comp[:, 1, 0] = comp[:, 2, 1] = 1.0
    comp[~good] = np.eye(3)
    ev = np.linalg.eigvals(comp)
    real = ev.imag == 0
    mag = np.maximum(1.0, np.abs(ev).max(1))
    near |= np.any(~real & (np.abs(ev.imag) < ROOT_SEP * mag[:, None]), 1)
    x = np.sort(np.where(real, ev.real, np.nan), 1)                # NaN last
    return _finish(Y, W, coef, good, near, x, drop_root)


# ------------------------------------------------------------------------------------------------------------ seven-point, route B
def _det3(a, b, c):
    return np.sum(a * np.cross(b, c), -1)


def seven_point_gj(x0, x1, drop_root=False):
    """Route B, from the text: Gauss-Jordan with full pivoting (the first largest entry in row-major order; no hypothesis when a pivot
    is <= PIVOT_MIN max|A|), the null space from the two columns left over, modified Gram-Schmidt, the cubic from the rows' mixed
    determinants, the real roots between -B, the derivative's critical points and B (B: Cauchy's bound) by Newton steps safeguarded
    by bisection.  Same return as seven_point_ref."""
    H = len(x0)
    A = _system(x0, x1).copy()
    amax = np.abs(A).max((1, 2))
    ar = np.arange(H)
    rowfree, colfree = np.ones((H, 7), bool), np.ones((H, 9), bool)
    pcol = np.zeros((H, 7), np.int64)
    minpiv = np.full(H, np.inf)
    with np.errstate(all="ignore"):
        for _ in range(7):
            M = np.where(rowfree[:, :, None] & colfree[:, None, :], np.abs(A), -1.0).reshape(H, 63)
            idx = np.argmax(M, 1)
            r, c = idx // 9, idx % 9
            minpiv = np.minimum(minpiv, M[ar, idx] / amax)
            rowfree[ar, r], colfree[ar, c], pcol[ar, r] = False, False, c
            prow = A[ar, r, :] / A[ar, r, c][:, None]
            A[ar, r, :] = prow
            f = A[ar, :, c].copy()
            f[ar, r] = 0.0
            A -= f[:, :, None] * prow[:, None, :]
        fc = np.argsort(~colfree, 1, kind="stable")[:, :2]        # the two free columns, ascending
        u, v = np.zeros((H, 9)), np.zeros((H, 9))
        u[ar, fc[:, 0]] = 1.0
        v[ar, fc[:, 1]] = 1.0
        for r in range(7):
            u[ar, pcol[:, r]] = -A[ar, r, fc[:, 0]]
            v[ar, pcol[:, r]] = -A[ar, r, fc[:, 1]]
        u /= np.linalg.norm(u, axis=1)[:, None]
        v -= np.sum(u * v, 1)[:, None] * u
        v /= np.linalg.norm(v, axis=1)[:, None]
        U, V = u.reshape(H, 3, 3), v.reshape(H, 3, 3)
        swap = np.abs(np.linalg.det(V)) > np.abs(np.linalg.det(U))
        Y, W = np.where(swap[:, None, None], V, U), np.where(swap[:, None, None], U, V)
        c3 = _det3(Y[:, 0], Y[:, 1], Y[:, 2])
        c2 = _det3(W[:, 0], Y[:, 1], Y[:, 2]) + _det3(Y[:, 0], W[:, 1], Y[:, 2]) + _det3(Y[:, 0], Y[:, 1], W[:, 2])
        c1 = _det3(Y[:, 0], W[:, 1], W[:, 2]) + _det3(W[:, 0], Y[:, 1], W[:, 2]) + _det3(W[:, 0], W[:, 1], Y[:, 2])
        c0 = _det3(W[:, 0], W[:, 1], W[:, 2])
        coef = np.stack([c3, c2, c1, c0], 1)
        lead = np.abs(c3) / np.abs(coef).max(1)
    good = (minpiv > PIVOT_MIN) & np.isfinite(coef).all(1) & (lead > LEAD_MIN)
    near = ~good | (minpiv <= NEAR * PIVOT_MIN) | (lead <= NEAR * LEAD_MIN)

    k3, k2, k1, k0 = c3, c2, c1, c0
    p = lambda x: ((k3 * x + k2) * x + k1) * x + k0               # noqa: E731
    dp = lambda x: (3 * k3 * x + 2 * k2) * x + k1                  # noqa: E731
    with np.errstate(all="ignore"):
        B = 1.0 + np.maximum(np.maximum(np.abs(k2), np.abs(k1)), np.abs(k0)) / np.abs(k3)
        disc = k2 * k2 - 3 * k3 * k1
        q = -(k2 + np.where(k2 < 0, -1.0, 1.0) * np.sqrt(np.where(disc > 0, disc, 0.0)))
        ra = q / (3 * k3)
        rb = np.where(q != 0, k1 / q, ra)
        xa, xb = np.minimum(ra, rb), np.maximum(ra, rb)
        three = (disc > 0) & np.isfinite(xa) & np.isfinite(xb) & (xa > -B) & (xb < B)
        near |= three & ((np.abs(p(xa)) < ROOT_SEP * np.abs(k3)) | (np.abs(p(xb)) < ROOT_SEP * np.abs(k3)))     # a double root, near enough
        x = np.full((H, 3), np.nan)
        for piece in range(3):
            lo = np.where(three, (-B, xa, xb)[piece], -B)
            hi = np.where(three, (xa, xb, B)[piece], B)
            flo, fhi = p(lo), p(hi)
            run = good & (three | (piece == 0)) & ((flo < 0) != (fhi < 0))
            xc = 0.5 * (lo + hi)
            for _ in range(100):
                if not run.any():
                    break
                fx = p(xc)
                run &= fx != 0
                left = run & ((fx < 0) == (flo < 0))
                right = run & ~left
                lo, flo, hi = np.where(left, xc, lo), np.where(left, fx, flo), np.where(right, xc, hi)
                xn = xc - fx / dp(xc)
                xn = np.where((xn > lo) & (xn < hi), xn, 0.5 * (lo + hi))
                step = np.abs(xn - xc)
                xc = np.where(run, xn, xc)
                run &= ~((step <= 4e-16 * np.abs(xc)) | ~(hi > lo))
            x[:, piece] = np.where(good & (three | (piece == 0)) & ((p(np.where(three, (-B, xa, xb)[piece], -B)) < 0) != (fhi < 0)), xc, np.nan)
    return _finish(Y, W, coef, good, near, np.sort(x, 1), drop_root)


# ------------------------------------------------------------------------------------------------------------ the rank-2 chart
def make_chart(F):
    """Dependent row k: the row whose two others i < j have the largest |r_i x r_j|^2 (the first on a tie); r_k = a r_i + b r_j by
    the 2 x 2 normal equations; of the six entries f = (r_i, r_j) the first of largest magnitude is held constant."""
    cr = [np.sum(np.cross(F[1], F[2]) ** 2), np.sum(np.cross(F[0], F[2]) ** 2), np.sum(np.cross(F[0], F[1]) ** 2)]
    k = int(np.argmax(cr))
    i, j = [r for r in range(3) if r != k]
    f = np.concatenate([F[i], F[j]]).astype(np.float64)
    m11, m12, m22 = f[:3] @ f[:3], f[:3] @ f[3:], f[3:] @ f[3:]
    b1, b2 = f[:3] @ F[k], f[3:] @ F[k]
    with np.errstate(all="ignore"):
        det = m11 * m22 - m12 * m12
        a, b = (b1 * m22 - b2 * m12) / det, (m11 * b2 - m12 * b1) / det
    fix = int(np.argmax(np.abs(f)))
    ch = {"k": k, "i": i, "j": j, "fix": fix, "free": [q for q in range(6) if q != fix], "f": f, "a": float(a), "b": float(b)}
    return ch, bool(np.isfinite(a) and np.isfinite(b) and np.abs(f[fix]) > 0)


def chart_matrix(ch):
    F = np.zeros((3, 3))
    F[ch["i"]], F[ch["j"]] = ch["f"][:3], ch["f"][3:]
    F[ch["k"]] = ch["a"] * ch["f"][:3] + ch["b"] * ch["f"][3:]
    return F


def normal_equations(ch, x0, x1, w):
    """The residual is C / sqrt(den) of the Sampson error; the 7 parameters are the five free entries of f in order, a, b.  x0, x1 [m, 2],
    w [m] weights (0 / 1).  Returns (J^T J, J^T r, r^T r)."""
    F = chart_matrix(ch)
    a, b = _hom(x0), _hom(x1)
    Fx, Ftx = a @ F.T, b @ F
    C = np.sum(Fx * b, -1)
    with np.errstate(all="ignore"):
        s = np.sqrt(Fx[:, 0] ** 2 + Fx[:, 1] ** 2 + Ftx[:, 0] ** 2 + Ftx[:, 1] ** 2)
        r = C / s
        ex, fx = Fx.copy(), Ftx.copy()
        ex[:, 2] = 0
        fx[:, 2] = 0
        g = (b[:, :, None] * a[:, None, :]) / s[:, None, None] - (C / s ** 3)[:, None, None] * (ex[:, :, None] * a[:, None, :] + b[:, :, None] * fx[:, None, :])
    gi, gj, gk = g[:, ch["i"]], g[:, ch["j"]], g[:, ch["k"]]
    J6 = np.concatenate([gi + ch["a"] * gk, gj + ch["b"] * gk], 1)
    J = np.concatenate([J6[:, ch["free"]], (gk @ ch["f"][:3])[:, None], (gk @ ch["f"][3:])[:, None]], 1)
    on = w > 0
    J, r = J[on], r[on]
    return J.T @ J, J.T @ r, float(r @ r)


def apply_update(ch, d):
    out = dict(ch, f=ch["f"].copy())
    out["f"][ch["free"]] += d[:5]
    out["a"], out["b"] = ch["a"] + d[5], ch["b"] + d[6]
    return out


# ------------------------------------------------------------------------------------------------------------ LO-RANSAC
num_trials_needed, trial_limits = rr.trial_rule(7)       # COLMAP's ComputeNumTrials and trial limits for sample size 7


def _distinct(Fa, Fb):
    return float(_fdist(Fa, Fb)) > 1e-8


def _lo_step(carried, F, inl, x0, x1):
    """One re-estimation: LO_GN Gauss-Newton steps over the inliers on a new chart of the current best."""
    ch, ok = make_chart(F)
    for _ in range(LO_GN):
        if not ok:
            return None
        H, g, _ = normal_equations(ch, x0, x1, inl)
        d, ok = rr.damped_solve(H, g)
        if ok:
            ch = apply_update(ch, d)
    return (carried, chart_matrix(ch)) if ok else None


# The rounds are ransac_ref.lo_ransac's.  A winner that fits its inliers to rounding is exact whatever their number (n = 8 with a wrong
# match: every sample without it holds its 7); the local optimisation carries nothing from step to step.
MODEL = rr.Model(name="F", sample_size=7, solver=seven_point_ref, support=support, error=sampson_f64, distinct=_distinct, band=BAND,
                 exact_sum=EXACT_SUM, lo_steps=LO_STEPS, lo_start=lambda F: None, lo_step=_lo_step, rule_breaks=("drop_root",))


# lo_ransac_ref(x0, x1, th2, **conf): {'F' (None without a hypothesis), 'cnt', 'sum', 'trials', 'banded', 'why', 'either'}; solver: the route.
lo_ransac_ref = functools.partial(rr.lo_ransac, MODEL)


def final_stage(F, mask, x0, x1):
    """Levenberg-Marquardt over the masked correspondences on make_chart(F).  Returns (F refined, left = the length of the Gauss-Newton
    step that remains)."""
    ch, ok = make_chart(F)
    if not ok:
        return None, np.inf
    w = mask.astype(np.float64)
    ch, H, g = rr.levenberg_marquardt(ch, lambda c: normal_equations(c, x0, x1, w), rr.damped_solve, apply_update, REF_ITERS)
    d, ok = rr.damped_solve(H, g)
    scale = np.sqrt(np.sum(ch["f"] ** 2) + ch["a"] ** 2 + ch["b"] ** 2)
    return chart_matrix(ch), (float(np.linalg.norm(d)) / scale if ok else np.inf)


def normalisation(p0, p1):
    """(c0, c1, s): the centroids and the common scale sqrt(2) / mean of the two mean distances; s is None when there is none."""
    c0, c1 = p0.mean(0), p1.mean(0)
    d0, d1 = np.mean(np.linalg.norm(p0 - c0, axis=1)), np.mean(np.linalg.norm(p1 - c1, axis=1))
    if not (np.isfinite(d0) and np.isfinite(d1) and d0 > 0 and d1 > 0):
        return c0, c1, None
    return c0, c1, np.sqrt(2.0) / (0.5 * (d0 + d1))


def to_pixels(F, c0, c1, s):
    """T1^T F T0 at unit Frobenius norm, the first entry of largest magnitude positive."""
    T0 = np.array([[s, 0, -s * c0[0]], [0, s, -s * c0[1]], [0, 0, 1.0]])
    T1 = np.array([[s, 0, -s * c1[0]], [0, s, -s * c1[1]], [0, 0, 1.0]])
    P = T1.T @ F @ T0
    P = P / np.linalg.norm(P)
    return P if P.reshape(-1)[int(np.argmax(np.abs(P)))] > 0 else -P


def fundamental_ref(p0, p1, max_error_px=4.0, min_num_inliers=15, solver=seven_point_ref, **conf):
    """The whole estimator on pixels.  Returns {'success', 'F' (pixels), 'num_inliers', 'inliers', 'num_trials', 'banded', 'why',
    'either': [{'F', 'inliers'}] of the other exact fits of as many points, each as right an answer as the first}."""
    p0, p1 = np.asarray(p0, np.float64).reshape(-1, 2), np.asarray(p1, np.float64).reshape(-1, 2)
    n = len(p0)
    out = {"success": False, "F": np.zeros((3, 3)), "num_inliers": 0, "inliers": np.zeros(n, bool), "num_trials": 0, "banded": False,
           "why": [], "either": []}
    if n < 7:
        return out
    c0, c1, s = normalisation(p0, p1)
    if s is None:
        return out
    x0, x1 = s * (p0 - c0), s * (p1 - c1)
    th2 = (s * max_error_px) ** 2
    r = lo_ransac_ref(x0, x1, th2, solver=solver, **conf)
    out["num_trials"], out["banded"], out["why"] = r["trials"], r["banded"], r["why"]
    if r["cnt"] < 7:
        return out
    mask = sampson_f64(r["F"], x0, x1) <= th2
    F, left = final_stage(r["F"], mask, x0, x1)
    if F is None:
        return out
    out.update(F=to_pixels(F, c0, c1, s), num_inliers=r["cnt"], inliers=mask, success=bool(r["cnt"] >= min_num_inliers))
    for Fk in r["either"]:
        mk = sampson_f64(Fk, x0, x1) <= th2
        Fe, le = final_stage(Fk, mk, x0, x1)
        left = max(left, le)
        if Fe is not None:
            out["either"].append({"F": to_pixels(Fe, c0, c1, s), "inliers": mk})
    out["left"] = left
    return out


def compare(r, ref, worst):
    """A device result (two_view.fundamental_matrix's dict) against fundamental_ref's: trials, count and mask equal; success; F within
    F_TOL of the restatement's answer or one of its 'either'.  worst [0] keeps the largest difference."""
    assert r["num_trials"] == ref["num_trials"] and r["num_inliers"] == ref["num_inliers"], \
        (r["num_trials"], ref["num_trials"], r["num_inliers"], ref["num_inliers"])
    assert r["success"] == ref["success"]
    if ref["num_inliers"] < 7:
        assert not r["inliers"].any() and not r["F"].any()
        return
    cands = [c for c in [ref] + ref["either"] if (r["inliers"] == c["inliers"]).all()]
    assert cands, "inlier mask"
    d = min(float(np.linalg.norm(r["F"] - c["F"])) for c in cands)
    worst[0] = max(worst[0], d)
    assert d <= F_TOL, d


# ------------------------------------------------------------------------------------------------------------ scenes and cases
_cached = rr.make_cached()


CAM0 = {"model": "PINHOLE", "width": 1024, "height": 768, "params": [800.0, 800.0, 512.0, 384.0]}
CAM1 = {"model": "PINHOLE", "width": 640, "height": 480, "params": [600.0, 610.0, 320.0, 240.0]}


def true_F(R, t, cam0=CAM0, cam1=CAM1):
    K = lambda c: np.array([[c["params"][0], 0, c["params"][2]], [0, c["params"][1], c["params"][3]], [0, 0, 1.0]])     # noqa: E731
    F = np.linalg.inv(K(cam1)).T @ tv.skew(np.asarray(t, float)[None])[0] @ R @ np.linalg.inv(K(cam0))
    return F / np.linalg.norm(F)


def scene(seed, n, outlier_ratio=0.0, noise_px=0.0, **kw):
    """two_view_ref.two_view_scene between the two pinhole cameras above (which the estimator never sees): (R, t, p0, p1, outliers)."""
    return tv.two_view_scene(np.random.RandomState(seed), CAM0, CAM1, n, outlier_ratio, noise_px, **kw)


# the RANSAC table: every n with every outlier ratio, 0.5 px noise; the threshold alternates so that both occur with every n and ratio
TABLE_NS = (7, 8, 12, 40, 80, 300)
TABLE_OUTLIERS = (0.0, 0.25, 0.5, 0.7)
TABLE_SEED = 500
RANSAC_CASES = [(n, o, TABLE_SEED + 10 * i + j, th) for i, n in enumerate(TABLE_NS) for j, o in enumerate(TABLE_OUTLIERS) for th in (4.0, 1.0)]


def ransac_cases():
    """[(p0, p1, max_error_px)] of RANSAC_CASES."""
    return _cached("cases", lambda: [scene(seed, n, o, 0.5)[2:4] + (th,) for n, o, seed, th in RANSAC_CASES])


def ransac_refs(solver=seven_point_ref):
    return _cached(("refs", solver.__name__), lambda: [fundamental_ref(p0, p1, th, solver=solver) for p0, p1, th in ransac_cases()])


OPTION_SCENE = (40, 0.5, 521, 4.0)
OPTION_RUNS = [dict(seed=1), dict(seed=2), dict(seed=3), dict(max_num_trials=255), dict(max_num_trials=256), dict(max_num_trials=257),
               dict(max_num_trials=1), dict(max_num_trials=300), dict(min_num_trials=5000, max_num_trials=600), dict(confidence=0.0),
               dict(confidence=1.0, max_num_trials=600), dict(min_inlier_ratio=0.0, max_num_trials=600), dict(min_inlier_ratio=1.0),
               dict(seed=2 ** 64 - 1), dict(seed=2 ** 63)]


def option_case():
    n, o, seed, th = OPTION_SCENE
    return _cached("option", lambda: scene(seed, n, o, 0.5)[2:4] + (th,))


def option_ref(solver=seven_point_ref, **conf):
    p0, p1, th = option_case()
    return _cached(("option_ref", solver.__name__, tuple(sorted(conf.items()))), lambda: fundamental_ref(p0, p1, th, solver=solver, **conf))


# the correspondences are walked in strides of 256: one under, at and over one and two strides, over four
SIZE_NS = (255, 256, 257, 511, 513, 1025)
SIZE_FILL = (0, 6, 7)        # pairs of these sizes stand between the size cases in the batch


def size_cases():
    """[(p0, p1, max_error_px)]: SIZE_NS with 30 % outliers and 0.5 px noise, each followed by pairs of 0, 6 and 7 correspondences."""
    def make():
        out = []
        for i, n in enumerate(SIZE_NS):
            out.append(scene(600 + i, n, 0.3, 0.5)[2:4] + (4.0,))
            for j, m in enumerate(SIZE_FILL):
                out.append((scene(650 + 3 * i + j, m, 0.0, 0.5)[2:4] if m else (np.zeros((0, 2)), np.zeros((0, 2)))) + (4.0,))
        return out
    return _cached("size_cases", make)


def size_refs(solver=seven_point_ref):
    return _cached(("size_refs", solver.__name__), lambda: [fundamental_ref(p0, p1, th, solver=solver) for p0, p1, th in size_cases()])


# Solver probes: one trial (max_num_trials = 1, the sample is sample_k(0, 0, n)) on n = 8 or 9 correspondences
PROBE_FAMILIES = ["generic", "forward", "baseline_1e-2", "near_planar"]
PROBES = 256
# 0.05 px.  The exact families: every point is exact, the generating matrix holds all n.  near_planar (0.5 px noise on points within 1 %
# of their depth of a plane): at this threshold a matrix holds little more than its own sample, so that the probe compares what the
# solver returns for a nearly degenerate sample, not a refinement over 8 or 9 nearly coplanar points, whose end point is ill-conditioned
# (measured with a 1 px threshold: the two routes of this file end up to 2.7e-7 apart).
PROBE_ERROR_PX = 0.05
PROBE_CONF = dict(max_num_trials=1, min_num_inliers=7)


def _near_planar_scene(rs, n):
    """Points within 1 % of their depth of a tilted plane through (0, 0, 6), 0.5 px noise: (R, t, p0, p1)."""
    W, H = CAM0["width"], CAM0["height"]
    px = np.stack([rs.uniform(0.05 * W, 0.95 * W, n), rs.uniform(0.05 * H, 0.95 * H, n)], 1)
    xn = pr.undistort(CAM0, px)
    nrm = np.array([rs.uniform(-0.3, 0.3), rs.uniform(-0.3, 0.3), 1.0])
    d = 6.0 * nrm[2] / (_hom(xn) @ nrm) * (1.0 + rs.uniform(-0.01, 0.01, n))
    X = _hom(xn) * d[:, None]
    w = rs.standard_normal(3)
    w *= rs.uniform(0.02, 0.25) / np.linalg.norm(w)
    R = tv._exp_so3(w[None])[0]
    t = rs.standard_normal(3) * [1, 1, 0.3]
    t *= rs.uniform(0.1, 0.3) * np.median(d) / np.linalg.norm(t)
    p0, _ = pr.project(CAM0, [1.0, 0, 0, 0], np.zeros(3), X)
    p1, z1 = pr.project(CAM1, pr.rotmat2qvec(R), t, X)
    assert (z1 > 0).all()
    return R, t / np.linalg.norm(t), p0 + 0.5 * rs.standard_normal(p0.shape), p1 + 0.5 * rs.standard_normal(p1.shape)


def probes(family):
    """[(p0, p1, R, t, max_error_px)] of one family, PROBES of them."""
    def make():
        rs = np.random.RandomState(2000 + PROBE_FAMILIES.index(family))
        out = []
        for i in range(PROBES):
            n = 8 + (i & 1)
            if family == "near_planar":
                R, t, p0, p1 = _near_planar_scene(rs, n)
                out.append((p0, p1, R, t, PROBE_ERROR_PX))
                continue
            kw = {"forward": True} if family == "forward" else {"baseline": 1e-2} if family.startswith("baseline") else {}
            R, t, p0, p1, _ = tv.two_view_scene(rs, CAM0, CAM1, n, **kw)
            out.append((p0, p1, R, t, PROBE_ERROR_PX))
        return out
    return _cached(("probes", family), make)


def probe_refs(family, solver=seven_point_ref):
    return _cached(("probe_refs", family, solver.__name__),
                   lambda: [fundamental_ref(p0, p1, th, solver=solver, **PROBE_CONF) for p0, p1, _, _, th in probes(family)])


def probe_disagreement(family):
    """Per probe of an exact family whose sample yields the generating matrix: the relative disagreement in squared Sampson error, at
    points 1 px off their exact place, between seven_point_ref's matrix and the generating one (normalised coordinates); and how many
    samples yield it."""
    dis, found = [], 0
    for p0, p1, R, t, _ in probes(family):
        c0, c1, s = normalisation(p0, p1)
        x0, x1 = s * (p0 - c0), s * (p1 - c1)
        idx = list(sample_k(0, 0, len(p0)))
        Fs, _, near = seven_point_ref(x0[idx][None], x1[idx][None])
        T0i = np.array([[1 / s, 0, c0[0]], [0, 1 / s, c0[1]], [0, 0, 1.0]])
        T1i = np.array([[1 / s, 0, c1[0]], [0, 1 / s, c1[1]], [0, 0, 1.0]])
        Ft = _unit(T1i.T @ true_F(R, t) @ T0i)
        if near[0] or not len(Fs):
            continue
        k = int(np.argmin(_fdist(Fs, Ft)))
        if _fdist(Fs[k], Ft) < 1e-6:
            found += 1
            y1 = x1 + s * np.array([0.6, 0.8])
            a, b = sampson_f64(Fs[k], x0, y1), sampson_f64(Ft, x0, y1)
            dis.append(float(np.max(np.abs(a - b) / b)))
    return dis, found


def measure_band():
    """The largest disagreement of probe_disagreement over the exact families."""
    return max(max(probe_disagreement(f)[0]) for f in PROBE_FAMILIES if f != "near_planar")


def all_ref_pairs():
    """[(name, route A result, route B result)] over every committed case that has a restatement."""
    out = [("table", a, b) for a, b in zip(ransac_refs(), ransac_refs(seven_point_gj))]
    out += [("option", option_ref(**c), option_ref(seven_point_gj, **c)) for c in OPTION_RUNS]
    out += [("size", a, b) for a, b in zip(size_refs(), size_refs(seven_point_gj))]
    for f in PROBE_FAMILIES:
        out += [("probe " + f, a, b) for a, b in zip(probe_refs(f), probe_refs(f, seven_point_gj))]
    return out


def measure_routes():
    """The largest distance between the pixel matrices of the two routes over the cases neither route leaves out (each against the
    other's answer or one of its 'either')."""
    worst = 0.0
    for _, a, b in all_ref_pairs():
        if a["banded"] or b["banded"] or a["num_inliers"] < 7:
            continue
        worst = max(worst, min(float(np.linalg.norm(a["F"] - c["F"])) for c in [b] + b["either"]))
    return worst


# 300 small pairs for one call: pair i has MANY_NS[i % 7] correspondences (a quarter outliers from n = 9 on, 0.5 px noise)
MANY = 300
MANY_NS = (0, 3, 6, 7, 9, 12, 40)
MANY_CONF = dict(max_num_trials=64, min_num_inliers=7)


def many_cases():
    def make():
        out = []
        for i in range(MANY):
            n = MANY_NS[i % len(MANY_NS)]
            out.append((scene(3000 + i, n, 0.25 if n >= 9 else 0.0, 0.5)[2:4] if n else (np.zeros((0, 2)), np.zeros((0, 2)))) + (4.0,))
        return out
    return _cached("many_cases", make)


def many_ref(i):
    p0, p1, th = many_cases()[i]
    return _cached(("many_ref", i), lambda: fundamental_ref(p0, p1, th, **MANY_CONF))


# name -> options: inputs without a fundamental matrix of their own.  Each gives no result after max_num_trials trials (`repeated`: after
# 0 trials, its point sets have no extent): success False, no inliers, F = 0.
DEGENERATE = {"coplanar": dict(max_num_trials=512), "rotation": dict(max_num_trials=512), "repeated": dict(max_num_trials=512),
              "line": dict(max_num_trials=512)}


def degenerate(name):
    """(p0, p1): coplanar -- 60 exact correspondences of points on one plane; rotation -- 60 exact correspondences under a rotation
    alone; repeated -- one correspondence 40 times; line -- 40 exact correspondences of points on one line in space."""
    def make():
        if name == "coplanar":
            return scene(701, 60, planar=True)[2:4]
        if name == "rotation":
            return scene(702, 60, baseline=0.0)[2:4]
        if name == "repeated":
            _, _, p0, p1, _ = scene(703, 1)                      # on a grid of 1/8 px: every sum of 40 is exact, the mean distance is 0
            return np.tile(np.round(p0 * 8) / 8, (40, 1)), np.tile(np.round(p1 * 8) / 8, (40, 1))
        if name == "line":
            rs = np.random.RandomState(704)
            X = np.array([-1.0, 0.4, 6.0]) + np.sort(rs.uniform(-1, 1, 40))[:, None] * np.array([1.5, 0.5, 2.0])
            R = tv._exp_so3(np.array([[0.03, -0.1, 0.02]]))[0]
            p0, _ = pr.project(CAM0, [1.0, 0, 0, 0], np.zeros(3), X)
            p1, z1 = pr.project(CAM1, pr.rotmat2qvec(R), np.array([0.9, -0.1, 0.1]), X)
            assert (z1 > 0).all()
            return p0, p1
        raise KeyError(name)
    return _cached(("degenerate", name), make)


def degenerate_ref(name):
    p0, p1 = degenerate(name)
    return _cached(("degenerate_ref", name), lambda: fundamental_ref(p0, p1, 4.0, **DEGENERATE[name]))
