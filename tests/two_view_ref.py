"""numpy restatement of the relative pose solver for the two-view tests only (never imported by the product), written
from the text and not from the kernel: the sampling on integers, a five-point solver that shares no step with the kernel's (SVD null
space in its own chart, LU, the action matrix of multiplication by y and LAPACK's eigenvectors, where the kernel reduces by Gauss-Jordan, picks
its chart, and runs its own QR iteration and inverse iteration on the action matrix of x), the fp64 Sampson error,
the LO-RANSAC rounds with their support order and stopping rule, the final refinement, the cheirality choice and the triangulation
angles; and the committed cases the GPU tests (tests/test_gpu_two_view.py, tests/test_gpu_two_view_edges.py) and the CPU checks
(tests/test_two_view_ref_host.py) share.  Everything is batched over hypotheses so that a round of 256 trials is a handful of numpy calls."""
import functools

import numpy as np

import pose_ref as pr
import ransac_ref as rr

ROUND = rr.ROUND
POLISH, LO_STEPS, LO_GN, REF_ITERS = 3, 8, 3, 50
RANK_MIN = 1e-12             # sigma_5 / sigma_1 of the 5 x 9 system at or below which a sample gives no hypothesis
NEAR = pr.NEAR               # a degeneracy measure within this factor of its threshold is too close to call
ROOT_SEP = pr.ROOT_SEP       # two solutions of one sample closer than this (unit-norm matrices, up to sign) are too close to call
# BAND, derived (measure_band() below, asserted by tests/test_two_view_ref_host.py): over the probe families the largest relative
# disagreement in squared Sampson error, at points 1 px off their exact place, between five_point_ref's best matrix and the
# generating matrix is MEASURED; the band is 100 x that.  It is used, relative, around the inlier threshold and for "equal" sums.
MEASURED = 1.1e-7
BAND = 100 * MEASURED
EXACT_SUM = 1e-24            # a sum of squared Sampson errors below this is that of an exact solution (rounding only)
# The final refinement ends after REF_ITERS steps or when lambda runs away, converged or not.  Where it has not, its end point
# depends on which steps rounding let pass (`cost <= cost before` in a flat valley), and two implementations end apart by about the
# step that remains: a case whose remaining Gauss-Newton step is longer than a hundredth of the pose tolerance is too close to call.
REFINE_LEFT = 1e-8
mix64 = rr.mix64
# the sampling on integers is ransac_ref's, at sample size 5
sample5 = lambda seed, trial, n: rr.sample_k(seed, trial, n, 5)          # noqa: E731
sample5v = lambda seed, trials, n: rr.sample_kv(seed, trials, n, 5)      # noqa: E731


# ------------------------------------------------------------------------------------------------------------ small algebra
def _hom(x):
    return np.concatenate([x, np.ones(x.shape[:-1] + (1,))], -1)


def skew(v):
    z = np.zeros(v.shape[:-1])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def sampson_f64(E, x0, x1):
    """Squared Sampson error of x1^T E x0: E [..., 3, 3]; x0, x1 [n, 2] (shared) or [..., n, 2] -> [..., n]."""
    a, b = _hom(np.asarray(x0, dtype=np.float64)), _hom(np.asarray(x1, dtype=np.float64))
    Ex = np.einsum("...ij,...nj->...ni", E, a)
    Etx = np.einsum("...ji,...nj->...ni", E, b)
    C = np.sum(Ex * b, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return C * C / (Ex[..., 0] ** 2 + Ex[..., 1] ** 2 + Etx[..., 0] ** 2 + Etx[..., 1] ** 2)


def support(E, x0, x1, th2):
    """(count, sum in point order, inlier mask, errors) of E [..., 3, 3] over the shared points."""
    e = sampson_f64(E, x0, x1)
    inl = e <= th2
    s = np.cumsum(np.where(inl, e, 0.0), -1)[..., -1] if e.shape[-1] else np.zeros(e.shape[:-1])
    return inl.sum(-1), s, inl, e


def decompose(E):
    """E [H, 3, 3] -> (R, t) with [t]x R = +-E: E scaled to |E|_F^2 = 2, C its cofactor matrix, t the longest column of C normalised
    (the first on a tie), R = C - [t]x E, projected onto SO(3)."""
    E = E * np.sqrt(2.0 / np.sum(E * E, (-1, -2)))[:, None, None]
    C = np.stack([np.cross(E[:, 1], E[:, 2]), np.cross(E[:, 2], E[:, 0]), np.cross(E[:, 0], E[:, 1])], 1)
    j = np.argmax(np.sum(C * C, 1), 1)
    t = C[np.arange(len(E)), :, j]
    t = t / np.linalg.norm(t, axis=1)[:, None]
    R = C - skew(t) @ E
    U, _, Vt = np.linalg.svd(R)
    d = np.sign(np.linalg.det(U @ Vt))
    U[:, :, 2] *= d[:, None]
    return U @ Vt, t


def _tangent(t):
    e = np.eye(3)[np.argmin(np.abs(t), 1)]
    b1 = np.cross(t, e)
    b1 /= np.linalg.norm(b1, axis=1)[:, None]
    return b1, np.cross(t, b1)


def _exp_so3(w):
    th = np.linalg.norm(w, axis=1)
    K = skew(w)
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1 - th ** 2 / 6, np.sin(ths) / ths)
    b = np.where(small, 0.5 - th ** 2 / 24, (1 - np.cos(ths)) / ths ** 2)
    return np.eye(3) + a[:, None, None] * K + b[:, None, None] * (K @ K)


def normal_equations(R, t, a, b, w=None):
    """R [H, 3, 3], t [H, 3]; a, b [H, m, 2] correspondences, w [H, m] weights (0 / 1).  The residual is C / sqrt(den) of the Sampson
    error; the 5 parameters are R <- Exp(w) R and t <- normalise(t + a b1 + b b2) on t's tangent plane.  Returns (J^T J, J^T r, r^T r)."""
    b1, b2 = _tangent(t)
    E = skew(t) @ R
    D = np.stack([skew(t) @ skew(np.broadcast_to(np.eye(3)[k], t.shape)) @ R for k in range(3)] + [skew(b1) @ R, skew(b2) @ R], 1)
    x0, x1 = _hom(a), _hom(b)
    Ex = np.einsum("hij,hmj->hmi", E, x0)
    Etx = np.einsum("hji,hmj->hmi", E, x1)
    C = np.sum(Ex * x1, -1)
    den = Ex[..., 0] ** 2 + Ex[..., 1] ** 2 + Etx[..., 0] ** 2 + Etx[..., 1] ** 2
    s = np.sqrt(den)
    r = C / s
    ex, fx = Ex.copy(), Etx.copy()
    ex[..., 2] = 0
    fx[..., 2] = 0
    g = (x1[..., :, None] * x0[..., None, :]) / s[..., None, None] - (C / s ** 3)[..., None, None] * (
        ex[..., :, None] * x0[..., None, :] + x1[..., :, None] * fx[..., None, :])
    J = np.einsum("hmij,hkij->hmk", g, D)
    if w is not None:
        J, r = J * w[..., None], r * w
    return np.einsum("hmk,hml->hkl", J, J), np.einsum("hmk,hm->hk", J, r), np.sum(r * r, -1)


def solve5(H, g, lam=0.0):
    """d [H, 5] of (H + lam diag H + 1e-15 max diag H) d = -g, and which systems were positive definite and finite."""
    dg = np.einsum("hii->hi", H)
    A = H + np.einsum("hi,ij->hij", lam * dg + 1e-15 * dg.max(1)[:, None], np.eye(5))
    ok = np.isfinite(A).all((1, 2)) & np.isfinite(g).all(1) & (dg.max(1) > 0)
    A = np.where(ok[:, None, None], A, np.eye(5))
    ok &= np.linalg.eigvalsh(A)[:, 0] > 0
    A = np.where(ok[:, None, None], A, np.eye(5))
    d = -np.linalg.solve(A, np.where(ok[:, None], g, 0.0)[..., None])[..., 0]
    return d, ok & np.isfinite(d).all(1)


def apply_update(R, t, d):
    b1, b2 = _tangent(t)
    tn = t + d[:, 3:4] * b1 + d[:, 4:5] * b2
    return _exp_so3(d[:, :3]) @ R, tn / np.linalg.norm(tn, axis=1)[:, None]


def gauss_newton(R, t, a, b, steps, w=None):
    """steps Gauss-Newton steps; ok[h] False as soon as a system fails (the pose is then left where it was)."""
    ok = np.ones(len(R), dtype=bool)
    for _ in range(steps):
        H, g, _ = normal_equations(R, t, a, b, w)
        d, good = solve5(H, g)
        ok &= good
        Rn, tn = apply_update(R, t, np.where(ok[:, None], d, 0.0))
        R, t = np.where(ok[:, None, None], Rn, R), np.where(ok[:, None], tn, t)
    return R, t, ok


# ------------------------------------------------------------------------------------------------------------ five-point (fp64)
_C3 = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
_B2 = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_L1 = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_ADD = lambda p, q: (p[0] + q[0], p[1] + q[1], p[2] + q[2])     # noqa: E731
_T2 = np.array([[_B2.index(_ADD(p, q)) for q in _L1] for p in _L1])
_T3 = np.array([[(_C3 + _B2).index(_ADD(p, q)) for q in _L1] for p in _B2])


def _mul_ll(a, b):
    out = np.zeros(a.shape[:-1] + (10,))
    for i in range(4):
        for j in range(4):
            out[..., _T2[i, j]] += a[..., i] * b[..., j]
    return out


def _mul_ql(q, l):
    out = np.zeros(q.shape[:-1] + (20,))
    for i in range(10):
        for j in range(4):
            out[..., _T3[i, j]] += q[..., i] * l[..., j]
    return out


def five_point_ref(x0, x1, drop_root=False, polish=POLISH):
    """x0, x1 [H, 5, 2] normalised samples.  Returns (E [K, 3, 3] unit Frobenius norm, owner [K] = row of the sample, near [H] = the
    sample is too close to call: rank measure within NEAR of RANK_MIN, an ill-conditioned elimination, or two solutions closer than
    ROOT_SEP; rank [H] = sigma_5 / sigma_1).  Route: SVD null space, the ten cubic constraints over (x^3 .. z^3 | x^2 xy xz y^2 yz z^2
    x y z 1), the action matrix of multiplication by y on the quotient ring (the kernel's is by x, in another basis of the null space and another
    chart), its real eigenvectors from LAPACK; then `polish` Gauss-Newton steps
    on the sample's five residuals.  drop_root: the rule break of the host test (every sample loses its last solution)."""
    H = len(x0)
    A = (_hom(x1)[:, :, :, None] * _hom(x0)[:, :, None, :]).reshape(H, 5, 9)
    _, S, Vt = np.linalg.svd(A)
    rank = S[:, 4] / S[:, 0]
    N = Vt[:, 5:9].reshape(H, 4, 3, 3)                    # X Y Z W
    El = np.moveaxis(N, 1, -1)                            # [H, 3, 3, 4]: the linear polynomial of every entry
    EEt = {}
    for i in range(3):
        for j in range(i, 3):
            EEt[i, j] = EEt[j, i] = sum(_mul_ll(El[:, i, k], El[:, j, k]) for k in range(3))
    tr = 0.5 * (EEt[0, 0] + EEt[1, 1] + EEt[2, 2])
    rows = []
    for i in range(3):
        for j in range(3):
            rows.append(sum(_mul_ql(EEt[i, k] - (tr if i == k else 0.0), El[:, k, j]) for k in range(3)))
    rows.append(_mul_ql(_mul_ll(El[:, 1, 1], El[:, 2, 2]) - _mul_ll(El[:, 1, 2], El[:, 2, 1]), El[:, 0, 0])
                + _mul_ql(_mul_ll(El[:, 1, 2], El[:, 2, 0]) - _mul_ll(El[:, 1, 0], El[:, 2, 2]), El[:, 0, 1])
                + _mul_ql(_mul_ll(El[:, 1, 0], El[:, 2, 1]) - _mul_ll(El[:, 1, 1], El[:, 2, 0]), El[:, 0, 2]))
    M = np.stack(rows, 1)                                 # [H, 10, 20]
    good = (rank > RANK_MIN) & np.isfinite(M).all((1, 2))
    cond = np.full(H, np.inf)
    cond[good] = np.linalg.cond(M[good][:, :, :10])
    good &= cond < 1e15
    near = ~good | (rank <= NEAR * RANK_MIN) | (cond >= 1e12 / NEAR)
    Es, owner = [], []
    if good.any():
        gi = np.flatnonzero(good)
        B = np.linalg.solve(M[gi][:, :, :10], M[gi][:, :, 10:])
        Ax = np.zeros((len(gi), 10, 10))
        Ax[:, :6] = -B[:, [1, 3, 4, 6, 7, 8]]            # y x^2 = x^2y, y xy = xy^2, y xz = xyz, y y^2 = y^3, y yz = y^2z, y z^2 = yz^2
        Ax[:, 6, 1] = Ax[:, 7, 3] = Ax[:, 8, 4] = Ax[:, 9, 7] = 1.0   # y x = xy, y y = y^2, y z = yz, y 1 = y
        w, V = np.linalg.eig(Ax)
        for r, h in enumerate(gi):
            real = np.flatnonzero(np.isreal(w[r]))
            v = np.real(V[r][:, real])
            with np.errstate(divide="ignore", invalid="ignore"):
                xyz = v[6:9] / v[9]
            cand = np.einsum("ks,kij->sij", np.concatenate([xyz, np.ones((1, xyz.shape[1]))]), N[h])
            cand = cand / np.sqrt(np.sum(cand * cand, (1, 2)))[:, None, None]
            cand = cand[np.isfinite(cand).all((1, 2))]
            if drop_root:
                cand = cand[:-1]
            Es.append(cand)
            owner += [h] * len(cand)
    Es = np.concatenate(Es) if Es else np.zeros((0, 3, 3))
    owner = np.asarray(owner, dtype=np.int64)
    if len(Es) and polish:
        R, t = decompose(Es)
        R, t, ok = gauss_newton(R, t, x0[owner], x1[owner], polish)
        Ep = skew(t) @ R
        use = ok & np.isfinite(Ep).all((1, 2))
        Es = np.where(use[:, None, None], Ep / np.sqrt(2.0), Es)
    for h in np.unique(owner):
        c = Es[owner == h] / np.sqrt(np.sum(Es[owner == h] ** 2, (1, 2)))[:, None, None]
        for i in range(len(c)):
            for j in range(i + 1, len(c)):
                if min(np.linalg.norm(c[i] - c[j]), np.linalg.norm(c[i] + c[j])) < ROOT_SEP:
                    near[h] = True
    return Es, owner, near, rank


# ------------------------------------------------------------------------------------------------------------ LO-RANSAC
num_trials_needed, trial_limits = rr.trial_rule(5)       # COLMAP's ComputeNumTrials and trial limits for sample size 5
DEFAULTS = dict(min_inlier_ratio=0.25, min_num_trials=0, max_num_trials=10000, confidence=0.999, seed=0)


def _distinct(Ea, Eb):
    """Two contenders are distinct when their unit-norm matrices differ, up to sign, by more than 1e-8: the same sample drawn in
    another order, or a re-estimation that has converged, is the same hypothesis and may win either way."""
    a, b = Ea / np.linalg.norm(Ea), Eb / np.linalg.norm(Eb)
    return min(np.linalg.norm(a - b), np.linalg.norm(a + b)) > 1e-8


def _lo_step(pose, E, inl, x0, x1):
    """One re-estimation: LO_GN Gauss-Newton steps over the inliers from the pose carried so far."""
    R, t, ok = gauss_newton(pose[0], pose[1], x0[None], x1[None], LO_GN, inl[None])
    return ((R, t), (skew(t) @ R)[0]) if ok[0] else None


# The rounds are ransac_ref.lo_ransac's.  E decomposes once when a hypothesis wins and carries (R, t) through the LO_STEPS; a winner is
# exact only when it holds all n points (a sample's other solutions hold its five and little else).
MODEL = rr.Model(name="E", sample_size=5, solver=five_point_ref, support=support, error=sampson_f64, distinct=_distinct, band=BAND,
                 exact_sum=EXACT_SUM, lo_steps=LO_STEPS, lo_start=lambda E: decompose(E[None]), lo_step=_lo_step,
                 rule_breaks=("drop_root", "dead_lanes"), exact_needs_all=True)


# lo_ransac_ref(x0, x1, th2, **conf): {'E' (None without a hypothesis), 'cnt', 'sum', 'trials', 'banded', 'why', 'either'}.
lo_ransac_ref = functools.partial(rr.lo_ransac, MODEL)


# ------------------------------------------------------------------------------------------------------------ final stage
def triangulate(R, t, x0, x1):
    """Midpoint triangulation under x1 = R x0 + t: the ray parameters (l0, l1) [n] and the angle in degrees [n] at the midpoint
    between the rays to the two centres."""
    d0, d1, w = _hom(x0), _hom(x1) @ R, -R.T @ t
    aa, bb, cc, p, q = np.sum(d0 * d0, 1), np.sum(d0 * d1, 1), np.sum(d1 * d1, 1), d0 @ w, d1 @ w
    with np.errstate(divide="ignore", invalid="ignore"):
        den = aa * cc - bb * bb
        l0, l1 = (cc * p - bb * q) / den, (bb * p - aa * q) / den
        X = 0.5 * (l0[:, None] * d0 + w + l1[:, None] * d1)
        u, v = -X, w - X
        cs = np.sum(u * v, 1) / np.sqrt(np.sum(u * u, 1) * np.sum(v * v, 1))
        return l0, l1, np.degrees(np.arccos(np.clip(cs, -1, 1)))


SLOTS = ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0))       # (R or R' = (2 t t^T - I) R, sign of t)


def final_stage(E, mask, x0, x1, slots=SLOTS):
    """Levenberg-Marquardt over the masked correspondences from decompose(E), then the first slot with the most masked points in
    front of both cameras.  Returns (R, t, angles [n] with NaN outside, chosen, other = the same four of the slot -E would have
    led to, None when that is the same slot; left = the length of the Gauss-Newton step that remains at the returned pose)."""
    w = mask.astype(np.float64)[None]

    def system(pose):                                      # a batch of one
        H, g, c = normal_equations(pose[0], pose[1], x0[None], x1[None], w)
        return H, g, c[0]

    def solve(H, g, lam):
        d, ok = solve5(H, g, lam)
        return d, ok[0]
    (R, t), H, g = rr.levenberg_marquardt(decompose(E[None]), system, solve, lambda pose, d: apply_update(pose[0], pose[1], d), REF_ITERS)
    d, ok = solve5(H, g)
    left = float(np.linalg.norm(d[0])) if ok[0] else np.inf
    R, t = R[0], t[0]
    Rs = (R, (2.0 * np.outer(t, t) - np.eye(3)) @ R)
    counts, cand = [], []
    for r, s in slots:
        l0, l1, deg = triangulate(Rs[r], s * t, x0, x1)
        front = mask & (l0 > 0) & (l1 > 0)
        counts.append(int(front.sum()))
        cand.append((Rs[r], s * t, np.where(front, deg, np.nan)))
    k = int(np.argmax(counts))                             # the first of the largest
    # E and -E are one hypothesis, and which of the two a solver returns is its own affair; decompose(-E) gives R' where
    # decompose(E) gives R, so under -E the slots come in the order 2, 3, 0, 1.  When a slot of R and one of R' tie for the most
    # points in front (a handful of points, a wrong hypothesis) the text does not say which wins: the other one is returned too.
    flipped = sorted(range(len(slots)), key=lambda j: (slots[j][0] == slots[0][0], j))
    o = max(flipped, key=lambda j: (counts[j], -flipped.index(j)))
    other = None if o == k else (cand[o][0], cand[o][1], cand[o][2], counts[o] > 0)
    return cand[k][0], cand[k][1], cand[k][2], counts[k] > 0, other, left


def threshold2(cam0, cam1, max_error_px):
    return (max_error_px / (0.5 * (pr.mean_focal(cam0) + pr.mean_focal(cam1)))) ** 2


def relative_pose_ref(p0, p1, cam0, cam1, max_error_px=4.0, min_num_inliers=15, slots=SLOTS, **conf):
    """The whole estimator on pixels.  Returns {'success', 'R', 't', 'num_inliers', 'inliers', 'num_trials', 'angles', 'banded', 'either':
    [{'R', 't', 'angles', 'success'}] of the other exact fits of every point and of a cheirality tie that the sign of E decides
    (final_stage), each as right an answer as the first}."""
    x0, x1 = pr.undistort(cam0, p0), pr.undistort(cam1, p1)
    th2 = threshold2(cam0, cam1, max_error_px)
    n = len(x0)
    out = {"success": False, "R": np.eye(3), "t": np.zeros(3), "num_inliers": 0, "inliers": np.zeros(n, bool), "num_trials": 0,
           "angles": np.full(n, np.nan), "banded": False, "either": []}
    if n < 5:
        return out
    r = lo_ransac_ref(x0, x1, th2, **conf)
    out["num_trials"], out["banded"], out["why"] = r["trials"], r["banded"], r["why"]
    if r["cnt"] < 5:
        return out
    mask = sampson_f64(r["E"], x0, x1) <= th2
    R, t, ang, chosen, other, left = final_stage(r["E"], mask, x0, x1, slots)
    out.update(R=R, t=t, num_inliers=r["cnt"], inliers=mask, angles=ang, success=bool(chosen and r["cnt"] >= min_num_inliers))
    others = [other]
    for Ek in r["either"]:                                 # exact fits of every point, as E is: the same mask
        fs = final_stage(Ek, mask, x0, x1, slots)
        others += [fs[:4], fs[4]]
        left = max(left, fs[5])
    if not left <= REFINE_LEFT:
        out["banded"] = True
        out["why"] = out["why"] + ["refinement"]
    for Rk, tk, angk, chk in [o for o in others if o is not None]:
        out["either"].append({"R": Rk, "t": tk, "angles": angk, "success": bool(chk and r["cnt"] >= min_num_inliers)})
    return out


# ------------------------------------------------------------------------------------------------------------ scenes and cases
_cached = rr.make_cached()


def two_view_scene(rs, cam0, cam1, n, outlier_ratio=0.0, noise_px=0.0, baseline=None, px0=None, forward=False, planar=False):
    """A relative pose (R, t with |t| = 1 reported; the scene's baseline is `baseline` times the median depth, default 10-30 %) and n
    correspondences: points 2-20 units in front of camera 0 inside its image (or at the pixels px0), projected into both, a
    fraction of them replaced in image 1 by random pixels, Gaussian noise on both images of the rest.  Returns (R, t, p0, p1, outliers)."""
    W, H = cam0["width"], cam0["height"]
    px = np.stack([rs.uniform(0.05 * W, 0.95 * W, n), rs.uniform(0.05 * H, 0.95 * H, n)], 1) if px0 is None else np.asarray(px0, float)
    xn = pr.undistort(cam0, px)
    d = 1.0 / rs.uniform(1.0 / 20, 1.0 / 2, n)
    if planar:                                             # depths of a tilted plane through (0, 0, 6)
        nrm = np.array([rs.uniform(-0.3, 0.3), rs.uniform(-0.3, 0.3), 1.0])
        d = 6.0 * nrm[2] / (_hom(xn) @ nrm)
    X = _hom(xn) * d[:, None]
    w = rs.standard_normal(3)
    w *= rs.uniform(0.02, 0.25) / np.linalg.norm(w)
    R = _exp_so3(w[None])[0]
    tdir = np.array([0.05 * rs.standard_normal(), 0.05 * rs.standard_normal(), 1.0]) if forward else rs.standard_normal(3) * [1, 1, 0.3]
    tdir /= np.linalg.norm(tdir)
    scale = (rs.uniform(0.1, 0.3) if baseline is None else baseline) * np.median(d)
    Y = X @ R.T + scale * tdir
    q = pr.rotmat2qvec(R)
    p0, _ = pr.project(cam0, [1.0, 0, 0, 0], np.zeros(3), X)
    p1, z1 = pr.project(cam1, q, scale * tdir, X)
    assert (z1 > 0).all()
    p0 = p0 + noise_px * rs.standard_normal(p0.shape)
    p1 = p1 + noise_px * rs.standard_normal(p1.shape)
    out = np.zeros(n, dtype=bool)
    no = int(round(outlier_ratio * n))
    if no:
        idx = rs.choice(n, no, replace=False)
        out[idx] = True
        p1[idx] = np.stack([rs.uniform(0, cam1["width"], no), rs.uniform(0, cam1["height"], no)], 1)
    return pr.qvec2rotmat(q), tdir, p0, p1, out


def pose_error(R, t, Rt, tt):
    """(rotation angle, angle between the translation directions) in radians."""
    c = np.clip((np.trace(R @ Rt.T) - 1) / 2, -1, 1)
    nn = np.linalg.norm(t) * np.linalg.norm(tt)
    return float(np.arccos(c)), float(np.arccos(np.clip(np.dot(t, tt) / nn, -1, 1))) if nn > 0 else float("inf")


# (n, outlier ratio, model 0, model 1, scene seed, max_error_px): 0.5 px noise
RANSAC_CASES = [(12, 0.0, "SIMPLE_PINHOLE", "SIMPLE_PINHOLE", 1, 4.0), (12, 0.25, "PINHOLE", "OPENCV", 2, 1.0),
                (40, 0.0, "SIMPLE_RADIAL", "SIMPLE_RADIAL", 3, 1.0), (40, 0.25, "OPENCV", "OPENCV", 4, 4.0),
                (40, 0.5, "PINHOLE", "SIMPLE_RADIAL", 5, 4.0), (40, 0.7, "OPENCV", "PINHOLE", 6, 4.0),
                (80, 0.25, "SIMPLE_PINHOLE", "OPENCV", 7, 1.0), (80, 0.5, "OPENCV", "OPENCV", 8, 4.0),
                (300, 0.0, "PINHOLE", "PINHOLE", 9, 4.0), (300, 0.25, "OPENCV", "SIMPLE_RADIAL", 10, 1.0),
                (300, 0.5, "SIMPLE_RADIAL", "OPENCV", 11, 4.0), (80, 0.7, "OPENCV", "OPENCV", 12, 1.0)]
OPTION_RUNS = [dict(seed=1), dict(seed=2), dict(seed=3), dict(max_num_trials=300), dict(min_num_trials=700),
               dict(confidence=0.5), dict(confidence=0.999999, max_num_trials=2000), dict(min_inlier_ratio=0.6)]
OPTION_SCENE = (40, 0.5, "OPENCV", "PINHOLE", 21, 4.0)


def _case(n, o, m0, m1, seed, th):
    cam0, cam1 = pr.camera(m0), pr.camera(m1)
    R, t, p0, p1, _ = two_view_scene(np.random.RandomState(seed), cam0, cam1, n, o, noise_px=0.5)
    return p0, p1, cam0, cam1, R, t, th


def ransac_cases():
    """[(p0, p1, cam0, cam1, R, t, max_error_px)] of RANSAC_CASES."""
    return _cached("cases", lambda: [_case(*c) for c in RANSAC_CASES])


def ransac_refs():
    return _cached("refs", lambda: [relative_pose_ref(p0, p1, c0, c1, th) for p0, p1, c0, c1, _, _, th in ransac_cases()])


def option_case():
    return _cached("option", lambda: _case(*OPTION_SCENE))


def option_ref(**conf):
    p0, p1, c0, c1, _, _, th = option_case()
    return _cached(("option_ref", tuple(sorted(conf.items()))), lambda: relative_pose_ref(p0, p1, c0, c1, th, **conf))


def tie_case():
    """(p0, p1, cam, cam, R, t): 12 exact points in front of both cameras under (R, t) and 12 under (R, -t).  All 24 satisfy the same
    essential matrix; decompositions (R, t) and (R, -t) each put 12 in front, so the choice is the tie rule's: the lowest slot."""
    def make():
        rs = np.random.RandomState(77)
        cam = pr.camera("PINHOLE")
        R = _exp_so3(np.array([[0.05, -0.12, 0.03]]))[0]
        t = np.array([0.8, 0.1, 0.05])
        t /= np.linalg.norm(t)
        X = np.stack([rs.uniform(-1.5, 1.5, 24), rs.uniform(-1, 1, 24), rs.uniform(4, 9, 24)], 1)
        sg = np.where(np.arange(24) < 12, 1.0, -1.0)
        Y = X @ R.T + sg[:, None] * t
        f = np.array(cam["params"][:2])
        c = np.array(cam["params"][2:])
        return X[:, :2] / X[:, 2:] * f + c, Y[:, :2] / Y[:, 2:] * f + c, cam, cam, R, t
    return _cached("tie", make)


# Solver probes: n (6 or 7) exact correspondences; with max_num_trials = 1 the one sample is sample5(0, 0, n), and the solver finds
# all n points and the generating pose if and only if its five-point solver returns the generating matrix for that sample.
PROBE_FAMILIES = ["generic", "planar", "forward", "baseline_1e-1", "baseline_1e-2", "baseline_1e-3", "strong_SIMPLE_RADIAL",
                  "strong_OPENCV", "mixed"]
PROBES = 256
PROBE_ERROR_PX = 0.05


def probes(family):
    """[(p0, p1, cam0, cam1, R, t)] of one family, PROBES of them."""
    def make():
        rs = np.random.RandomState(1000 + PROBE_FAMILIES.index(family))
        out = []
        for i in range(PROBES):
            n = 6 + (i & 1)
            kw, cam0, cam1 = {}, pr.camera("PINHOLE"), pr.camera("PINHOLE")
            if family == "planar":
                kw["planar"] = True
            elif family == "forward":
                kw["forward"] = True
            elif family.startswith("baseline"):
                kw["baseline"] = float(family.split("_")[1])
            elif family.startswith("strong"):
                m = family.split("_", 1)[1]
                cam0 = cam1 = {"model": m, "width": 640, "height": 480, "params": list(pr.STRONG_CAMERAS[m])}
                W, H = 640.0, 480.0
                corners = np.array([[0, 0], [W, 0], [0, H], [W, H]])
                kw["px0"] = np.concatenate([corners, np.stack([rs.uniform(0, W, n - 4), rs.uniform(0, H, n - 4)], 1)])[rs.permutation(n)]
                kw["baseline"] = 0.05
            elif family == "mixed":
                cam0, cam1 = pr.camera("SIMPLE_RADIAL"), pr.camera("OPENCV")
            R, t, p0, p1, _ = two_view_scene(rs, cam0, cam1, n, **kw)
            out.append((p0, p1, cam0, cam1, R, t))
        return out
    return _cached(("probes", family), make)


def probe_expect(family):
    """Per probe (expectation, poses): True -- the sample yields the generating matrix, which holds every point and wins, poses =
    [the generating pose]; 'either' -- a second exact solution holds every point as well (all points on one plane: the two-fold
    ambiguity of a planar scene, which only the sums' rounding separates), poses = the final poses of the exact solutions; False --
    the sample does not yield the generating matrix; None -- too close to call (near a degeneracy, two solutions within ROOT_SEP, an
    error within the band of the threshold).  Also the relative disagreement in squared Sampson error at points 1 px off, for
    measure_band()."""
    def make():
        ps = probes(family)
        xs = [(pr.undistort(c0, p0), pr.undistort(c1, p1)) for p0, p1, c0, c1, _, _ in ps]
        idx = [np.asarray(sample5(0, 0, len(x0))) for x0, _ in xs]
        Es, owner, near, _ = five_point_ref(np.stack([x0[i] for (x0, _), i in zip(xs, idx)]), np.stack([x1[i] for (_, x1), i in zip(xs, idx)]))
        exp, dis = [], []
        for h, ((p0, p1, cam0, cam1, R, t), (x0, x1)) in enumerate(zip(ps, xs)):
            th2 = threshold2(cam0, cam1, PROBE_ERROR_PX)
            Eh = Es[owner == h]
            Et = skew(t[None])[0] @ R
            Et /= np.linalg.norm(Et)
            if not len(Eh):
                exp.append((None if near[h] else False, []))
                continue
            Eh = Eh / np.linalg.norm(Eh, axis=(1, 2))[:, None, None]
            dist = np.minimum(np.linalg.norm(Eh - Et, axis=(1, 2)), np.linalg.norm(Eh + Et, axis=(1, 2)))
            k = int(np.argmin(dist))
            cnt, sm, _, err = support(Eh, x0, x1, th2)
            exact = np.flatnonzero((cnt == len(x0)) & (sm < EXACT_SUM))
            if near[h] or bool(np.any(np.abs(err - th2) <= BAND * th2)):
                exp.append((None, []))
            elif not (dist[k] < 1e-6 and k in exact):
                exp.append((False, []))
            elif len(exact) == 1:
                exp.append((True, [(R, t)]))
            else:
                poses = [final_stage(Eh[e], np.ones(len(x0), bool), x0, x1)[:2] for e in exact]
                exp.append(("either", poses))
            if dist[k] < 1e-6:
                f = 0.5 * (pr.mean_focal(cam0) + pr.mean_focal(cam1))
                y1 = x1 + np.array([0.6, 0.8]) / f
                a, b = sampson_f64(Eh[k], x0, y1), sampson_f64(Et, x0, y1)
                dis.append(float(np.max(np.abs(a - b) / b)))
        return exp, dis
    return _cached(("expect", family), make)


def measure_band():
    """The largest disagreement of probe_expect over the families whose samples are well conditioned."""
    return max(max(probe_expect(f)[1]) for f in PROBE_FAMILIES)


# ------------------------------------------------------------------------------------------------------------ comparison
POSE_TOL = 1e-6        # radians: DESIGN.md 9's pose tolerance


def compare(r, ref, worst):
    """A device result (two_view.relative_pose's dict) against relative_pose_ref's: trials, count and mask equal; then success, the
    pose within POSE_TOL, the same angles finite and within 1e-4 degrees, against the restatement's answer or one of its 'either'.
    worst [rotation, translation] keeps the largest differences."""
    assert r["num_trials"] == ref["num_trials"] and r["num_inliers"] == ref["num_inliers"], \
        (r["num_trials"], ref["num_trials"], r["num_inliers"], ref["num_inliers"])
    assert (r["inliers"] == ref["inliers"]).all()
    if ref["num_inliers"] < 5:
        assert r["success"] == ref["success"]
        return
    cands = [ref] + ref.get("either", [])
    errs = [pose_error(pr.qvec2rotmat(r["qvec"]), r["tvec"], c["R"], c["t"]) for c in cands]
    k = int(np.argmin([max(e) for e in errs]))
    c, (dr, dt) = cands[k], errs[k]
    assert dr <= POSE_TOL and dt <= POSE_TOL, errs
    worst[0], worst[1] = max(worst[0], dr), max(worst[1], dt)
    assert r["success"] == c["success"], (r["success"], c["success"])
    both = np.isfinite(c["angles"])
    assert (np.isfinite(r["tri_angles_deg"]) == both).all()
    assert np.allclose(r["tri_angles_deg"][both], c["angles"][both], rtol=0, atol=1e-4)


# ------------------------------------------------------------------------------------------------------------ edge cases
# (tests/test_gpu_two_view_edges.py; tests/test_two_view_ref_host.py keeps them honest on the CPU)
_MODELS = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "OPENCV")
# the correspondences are walked in strides of 256: one under, at and over one, two and four strides; (index i, n, outlier ratio)
SIZE_CASES = [(i, n, o) for i, n in enumerate((255, 256, 257, 511, 512, 513, 1025)) for o in (0.3, 0.6)]
SIZE_CASES.append((7, 1025, 0.0))       # index 1024 is an outlier in both cases above: here the fifth stride's one element is an inlier


def size_cases():
    """[(p0, p1, cam0, cam1, R, t, max_error_px)] of SIZE_CASES: scene seed 100 + i, camera models i and i + 1 of the four, 0.5 px noise."""
    def make():
        out = []
        for i, n, o in SIZE_CASES:
            cam0, cam1 = pr.camera(_MODELS[i % 4]), pr.camera(_MODELS[(i + 1) % 4])
            R, t, p0, p1, _ = two_view_scene(np.random.RandomState(100 + i), cam0, cam1, n, o, noise_px=0.5)
            out.append((p0, p1, cam0, cam1, R, t, 4.0))
        return out
    return _cached("size_cases", make)


def size_ref(k):
    p0, p1, c0, c1, _, _, th = size_cases()[k]
    return _cached(("size_ref", k), lambda: relative_pose_ref(p0, p1, c0, c1, th))


# (options, the num_trials they must give) on LIMIT_SCENE: the trial limit one under, at and over a round and at two rounds, a single
# trial, the closed ends of confidence and min_inlier_ratio, min_num_trials between and beyond the limits
LIMIT_SCENE = (60, 0.5, "OPENCV", "OPENCV", 21, 4.0)
LIMIT_RUNS = [(dict(max_num_trials=255), 255), (dict(max_num_trials=256), 256), (dict(max_num_trials=257), 257),
              (dict(max_num_trials=512), 512), (dict(max_num_trials=1), 1), (dict(confidence=0.0), 1),
              (dict(confidence=1.0, max_num_trials=600), 600), (dict(min_inlier_ratio=0.0, max_num_trials=600), 512),
              (dict(min_inlier_ratio=1.0), 1), (dict(min_num_trials=513, max_num_trials=5000), 768),
              (dict(min_num_trials=5000, max_num_trials=600), 600)]
SEED_RUNS = [2 ** 64 - 1, 2 ** 63]      # a seed is 64 bits without a sign: -1 through the Python wrapper is the first of these


def limit_case():
    return _cached("limit", lambda: _case(*LIMIT_SCENE))


def limit_ref(**conf):
    p0, p1, c0, c1, _, _, th = limit_case()
    return _cached(("limit_ref", tuple(sorted(conf.items()))), lambda: relative_pose_ref(p0, p1, c0, c1, th, **conf))


# (scene seed, classes, copies, noise px): `classes` distinct correspondences without outliers, the whole list `copies` times over, as
# a match list with repeated key points.  A sample with a repeated correspondence is rank-deficient and yields nothing: 1 -
# prod_k (1 - k (copies - 1) / (n - k)) of all samples, 0.71 (8 x 16) and 0.56 (12 x 10).
REPEAT_CASES = [(s, c, k, nz) for s in range(4) for c, k, nz in ((8, 16, 0.0), (8, 16, 0.5), (12, 10, 0.5))]


def repeat_cases():
    """[(p0, p1, cam, cam, R, t, max_error_px)] of REPEAT_CASES (OPENCV)."""
    def make():
        out, cam = [], pr.camera("OPENCV")
        for s, c, k, nz in REPEAT_CASES:
            R, t, p0, p1, _ = two_view_scene(np.random.RandomState(200 + s), cam, cam, c, 0.0, noise_px=nz)
            out.append((np.tile(p0, (k, 1)), np.tile(p1, (k, 1)), cam, cam, R, t, 4.0))
        return out
    return _cached("repeat_cases", make)


def repeat_ref(k):
    p0, p1, c0, c1, _, _, th = repeat_cases()[k]
    return _cached(("repeat_ref", k), lambda: relative_pose_ref(p0, p1, c0, c1, th))


# 300 small pairs for one call: (n, scene seed) of pair i
MANY = 300
MANY_NS = (0, 3, 5, 6, 9, 12, 40)
MANY_CONF = dict(max_num_trials=64, min_num_inliers=5)
MANY_SEED = 3000


def many_cases():
    """[(p0, p1, cam0, cam1, max_error_px)]: pair i has MANY_NS[i % 7] correspondences (a quarter outliers from n = 9 on, 0.5 px
    noise), camera models i and i + 1 of the four."""
    def make():
        out = []
        for i in range(MANY):
            n = MANY_NS[i % len(MANY_NS)]
            cam0, cam1 = pr.camera(_MODELS[i % 4]), pr.camera(_MODELS[(i + 1) % 4])
            p0 = p1 = np.zeros((0, 2))
            if n:
                _, _, p0, p1, _ = two_view_scene(np.random.RandomState(MANY_SEED + i), cam0, cam1, n, 0.25 if n >= 9 else 0.0, noise_px=0.5)
            out.append((p0, p1, cam0, cam1, 4.0))
        return out
    return _cached("many_cases", make)


def many_ref(i):
    p0, p1, c0, c1, th = many_cases()[i]
    return _cached(("many_ref", i), lambda: relative_pose_ref(p0, p1, c0, c1, th, **MANY_CONF))


# name -> options; degenerate() gives the pair
DEGENERATE = {"identical": dict(max_num_trials=512), "four_classes": dict(max_num_trials=512), "all_outliers": dict(max_num_trials=1024),
              "rotation_exact": dict(max_num_trials=512), "identity": dict(max_num_trials=512), "collinear": dict(max_num_trials=512)}


def degenerate(name):
    """(p0, p1, cam, cam, R, t) of a DEGENERATE case (R, t the generating pose, None where there is none).  identical: one
    correspondence 20 times (every sample is rank-deficient).  four_classes: four correspondences 16 times each (every sample holds one
    twice, and a matrix through its four others would hold all 64).  all_outliers: 60 pixels of image 0 against uniformly random pixels of
    image 1.  rotation_exact: 60 exact correspondences under a rotation alone (every [t]x R fits: no isolated solution).  identity:
    the same 60 pixels in both images.  collinear: 40 exact correspondences of points on one line in space (a line in both images;
    their essential matrix is not unique)."""
    def make():
        cam = pr.camera("OPENCV")
        if name == "identical":
            _, _, p0, p1, _ = two_view_scene(np.random.RandomState(6), cam, cam, 1)
            return np.tile(p0, (20, 1)), np.tile(p1, (20, 1)), cam, cam, None, None
        if name == "four_classes":
            _, _, p0, p1, _ = two_view_scene(np.random.RandomState(9), cam, cam, 4, noise_px=0.5)
            return np.tile(p0, (16, 1)), np.tile(p1, (16, 1)), cam, cam, None, None
        if name == "all_outliers":
            _, _, p0, p1, _ = two_view_scene(np.random.RandomState(7), cam, cam, 60, 1.0, noise_px=0.5)
            return p0, p1, cam, cam, None, None
        if name in ("rotation_exact", "identity"):
            R, _, p0, p1, _ = two_view_scene(np.random.RandomState(5), cam, cam, 60, 0.0, noise_px=0.0, baseline=0.0)
            return (p0, p1, cam, cam, R, None) if name == "rotation_exact" else (p0, p0.copy(), cam, cam, np.eye(3), None)
        if name == "collinear":
            cam = pr.camera("PINHOLE")
            rs = np.random.RandomState(8)
            X = np.array([-1.0, 0.4, 6.0]) + np.sort(rs.uniform(-1, 1, 40))[:, None] * np.array([1.5, 0.5, 2.0])
            R = _exp_so3(np.array([[0.03, -0.1, 0.02]]))[0]
            t = np.array([0.9, -0.1, 0.1])
            p0, _ = pr.project(cam, [1.0, 0, 0, 0], np.zeros(3), X)
            p1, z1 = pr.project(cam, pr.rotmat2qvec(R), t, X)
            assert (z1 > 0).all()
            return p0, p1, cam, cam, R, t / np.linalg.norm(t)
        raise KeyError(name)
    return _cached(("degenerate", name), make)


def degenerate_ref(name):
    p0, p1, c0, c1, _, _ = degenerate(name)
    return _cached(("degenerate_ref", name), lambda: relative_pose_ref(p0, p1, c0, c1, 4.0, **DEGENERATE[name]))
