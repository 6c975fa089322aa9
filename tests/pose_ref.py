"""numpy helpers for the pose tests only (never imported by the product): COLMAP's camera models, a synthetic scene generator,
the Cauchy-IRLS refinement the device result is compared against, and (second half) a restatement of the whole solver -- sampling,
an independent fp64 P3P, the fp32 inlier test, the LO-RANSAC rounds and their stopping rule -- with the committed cases the GPU
tests of tests/test_gpu_pose.py and the CPU checks of tests/test_pose_ref_host.py share."""
import numpy as np

import ransac_ref as rr

PARAMS = {   # COLMAP parameter order
    "SIMPLE_PINHOLE": [800.0, 320.0, 240.0],
    "PINHOLE": [810.0, 790.0, 321.0, 239.0],
    "SIMPLE_RADIAL": [800.0, 320.0, 240.0, -0.08],
    "OPENCV": [805.0, 795.0, 318.0, 242.0, -0.1, 0.02, 0.001, -0.0015],
}


def camera(model, width=640, height=480):
    return {"model": model, "width": width, "height": height, "params": list(PARAMS[model])}


def _opencv(cam):
    m, p = cam["model"], np.asarray(cam["params"], dtype=np.float64)
    if m == "SIMPLE_PINHOLE":
        return p[0], p[0], p[1], p[2], 0, 0, 0, 0
    if m == "PINHOLE":
        return p[0], p[1], p[2], p[3], 0, 0, 0, 0
    if m == "SIMPLE_RADIAL":
        return p[0], p[0], p[1], p[2], p[3], 0, 0, 0
    if m == "OPENCV":
        return tuple(p)
    raise ValueError(m)


def distort(cam, u, v):
    fx, fy, cx, cy, k1, k2, p1, p2 = _opencv(cam)
    r2 = u * u + v * v
    rad = k1 * r2 + k2 * r2 * r2
    return u + u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u), v + v * rad + 2 * p2 * u * v + p1 * (r2 + 2 * v * v)


def mean_focal(cam):
    fx, fy = _opencv(cam)[:2]
    return 0.5 * (fx + fy)


def qvec2rotmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rotmat2qvec(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.copysign(np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
    q = np.array([w, x, y, z])
    return q / np.linalg.norm(q)


def project(cam, qvec, tvec, X):
    """Pixels [n, 2] and depths [n] of world points X [n, 3]."""
    P = X @ qvec2rotmat(qvec).T + tvec
    u, v = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    ud, vd = distort(cam, u, v)
    fx, fy, cx, cy = _opencv(cam)[:4]
    return np.stack([fx * ud + cx, fy * vd + cy], 1), P[:, 2]


def rot_angle(q1, q2):
    R = qvec2rotmat(q1) @ qvec2rotmat(q2).T
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


def centre(qvec, tvec):
    return -qvec2rotmat(qvec).T @ np.asarray(tvec)


def random_pose(rs):
    q = rs.standard_normal(4)
    q /= np.linalg.norm(q)
    q *= np.sign(q[0])
    return q, rs.uniform(-2, 2, 3)


def scene(rs, cam, n, outlier_ratio=0.0, noise_px=0.0, offset=(0.0, 0.0, 0.0)):
    """A pose, n correspondences whose 3D points lie 1-60 units in front (uniform in inverse depth) of the camera inside the image (world coordinates
    shifted by `offset`), a fraction outlier_ratio of them with their 2D point replaced by a random pixel, Gaussian noise on the
    rest.  Returns (qvec, tvec, points2D, points3D, outlier labels)."""
    q, t = random_pose(rs)
    R = qvec2rotmat(q)
    W, H = cam["width"], cam["height"]
    fx, fy, cx, cy = _opencv(cam)[:4]
    px = np.stack([rs.uniform(0.05 * W, 0.95 * W, n), rs.uniform(0.05 * H, 0.95 * H, n)], 1)
    xn = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy], 1)   # treat as undistorted rays (the distortion is mild)
    d = 1.0 / rs.uniform(1.0 / 60, 1.0, n)
    Pc = np.concatenate([xn, np.ones((n, 1))], 1) * d[:, None]
    X = (Pc - t) @ R + np.asarray(offset)
    t = t - R @ np.asarray(offset)
    x, _ = project(cam, q, t, X)
    x = x + noise_px * rs.standard_normal(x.shape)
    out = np.zeros(n, dtype=bool)
    no = int(round(outlier_ratio * n))
    if no:
        idx = rs.choice(n, no, replace=False)
        out[idx] = True
        x[idx] = np.stack([rs.uniform(0, W, no), rs.uniform(0, H, no)], 1)
    return q, t, x, X, out


def reproj_error(cam, qvec, tvec, x, X):
    p, z = project(cam, qvec, tvec, X)
    e = np.linalg.norm(p - x, axis=1)
    e[z <= 0] = np.inf
    return e


def distort_jacobian(cam, u, v):
    """d distort / d (u, v), analytic: (j00, j01, j10, j11) = (dud/du, dud/dv, dvd/du, dvd/dv)."""
    fx, fy, cx, cy, k1, k2, p1, p2 = _opencv(cam)
    r2 = u * u + v * v
    rad = k1 * r2 + k2 * r2 * r2
    dr = k1 + 2 * k2 * r2                                   # d rad / d r2; d r2 / du = 2 u
    return (1 + rad + 2 * u * u * dr + 2 * p1 * v + 6 * p2 * u, 2 * u * v * dr + 2 * p1 * u + 2 * p2 * v,
            2 * u * v * dr + 2 * p2 * v + 2 * p1 * u, 1 + rad + 2 * v * v * dr + 2 * p2 * u + 6 * p1 * v)


def undistort(cam, px):
    """Pixels [n, 2] -> normalised image coordinates: Newton on the distortion with the analytic Jacobian (COLMAP's ImageToWorld),
    run until the step is below 1e-15 of the coordinate; raises if a point does not reach |distort(u, v) - (xd, yd)| <= 1e-14."""
    px = np.asarray(px, dtype=np.float64).reshape(-1, 2)
    fx, fy, cx, cy = _opencv(cam)[:4]
    xd, yd = (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy
    u, v = xd.copy(), yd.copy()
    for _ in range(100):
        fu, fv = distort(cam, u, v)
        j00, j01, j10, j11 = distort_jacobian(cam, u, v)
        ru, rv = fu - xd, fv - yd
        det = j00 * j11 - j01 * j10
        du, dv = (j11 * ru - j01 * rv) / det, (j00 * rv - j10 * ru) / det
        u, v = u - du, v - dv
        if np.all(np.hypot(du, dv) <= 1e-15 * (1 + np.hypot(u, v))):
            break
    fu, fv = distort(cam, u, v)
    worst = float(np.max(np.hypot(fu - xd, fv - yd), initial=0.0))
    if not worst <= 1e-14:
        raise ArithmeticError(f"undistortion did not converge: residual {worst:.3e}")
    return np.stack([u, v], 1)


def distortion_monotonic(cam, steps=64):
    """True when the distortion is invertible over the whole image: along the ray from the principal point to the pre-image of
    every border pixel the Jacobian keeps a positive determinant and positive diagonal (so the Newton iteration has one answer)."""
    W, H = cam["width"], cam["height"]
    s = np.linspace(0, 1, 33)
    border = np.concatenate([np.stack([s * W, 0 * s], 1), np.stack([s * W, 0 * s + H], 1), np.stack([0 * s, s * H], 1),
                             np.stack([0 * s + W, s * H], 1)])
    try:
        uv = undistort(cam, border)
    except ArithmeticError:
        return False
    for f in np.linspace(0.0, 1.05, steps):
        j00, j01, j10, j11 = distort_jacobian(cam, f * uv[:, 0], f * uv[:, 1])
        if not (np.all(j00 * j11 - j01 * j10 > 0) and np.all(j00 > 0) and np.all(j11 > 0)):
            return False
    return True


def ransac_error(cam, qvec, tvec, x, X):
    """The reprojection error RANSAC thresholds (COLMAP: in normalised coordinates, scaled by the mean focal length); inf behind
    the camera."""
    P = X @ qvec2rotmat(qvec).T + tvec
    e = np.linalg.norm(P[:, :2] / P[:, 2:3] - undistort(cam, x), axis=1) * mean_focal(cam)
    e[P[:, 2] <= 0] = np.inf
    return e


def refine_cauchy(cam, qvec, tvec, x, X, mask, iters=500):
    """Minimises sum log(1 + |pi(R X + t) - x|^2) (Cauchy, 1 px scale) over the masked points by IRLS / Gauss-Newton with a
    left rotation update (numerical Jacobian), fp64.  Returns (qvec, tvec)."""
    x, X = x[mask], X[mask]
    R, t = qvec2rotmat(qvec), np.asarray(tvec, dtype=np.float64).copy()

    def res(R, t):
        p, _ = project(cam, rotmat2qvec(R), t, X)
        return (p - x).reshape(-1)

    def expm(w):
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        if th < 1e-12:
            return np.eye(3) + K
        return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K

    def upd(R, t, d):
        E = expm(d[:3])
        return E @ R, E @ t + d[3:]

    for _ in range(iters):
        r = res(R, t)
        s = r[0::2] ** 2 + r[1::2] ** 2
        w = np.repeat(1.0 / (1.0 + s), 2)
        J = np.zeros((r.size, 6))
        for k in range(6):
            h = 1e-7
            dp = np.zeros(6)
            dp[k] = h
            dm = -dp
            J[:, k] = (res(*upd(R, t, dp)) - res(*upd(R, t, dm))) / (2 * h)
        A = J.T @ (w[:, None] * J)
        g = J.T @ (w * r)
        d = -np.linalg.solve(A, g)
        R, t = upd(R, t, d)
        if np.linalg.norm(d) < 1e-11:        # the steps shrink geometrically (IRLS); the numerical Jacobian floors them near 1e-12
            break
    q = rotmat2qvec(R)
    return q, t


# =====================================================================================================================
# A restatement of the solver (DESIGN section 9 and the header of pose_kernels.hip, steps 1-5), written from the
# specification and not from the kernel's code.  numpy, fp64 except where the specification says fp32.
# =====================================================================================================================
MODELS = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "OPENCV"]
ROUND = rr.ROUND             # trials per round
LO_STEPS, LO_GN = 8, 3       # re-estimations per improvement, Gauss-Newton steps per re-estimation
COLLINEAR_MIN = 1e-10        # |d12 x d13|^2 / (a12 a13) at or below which a sample gives no pose
COPLANAR_MIN = 1e-12         # |det[y0 y1 y2]| at or below which a sample gives no pose
NEAR = 100.0                 # a degeneracy measure within this factor of its threshold is too close to call
ROOT_SEP = 1e-3              # depth solutions closer than this (relative) are too close to call
# BAND: half-width, relative, of the band around the squared-error threshold inside which the fp32 inlier test may fall either
# way.  The fp32 evaluation is 9 FMAs for R X + t (each 2^-24 relative to sums of a few terms of similar size), a hardware
# reciprocal good to 1 ulp, two subtractions of nearby numbers and their squares: a few 1e-6 relative on the squared error at
# the threshold.  1e-4 is about 40x that, and 4 orders of magnitude below the squared-error scale of 1 px noise at a 12 px
# threshold ((1/12)^2 ~ 7e-3 of the threshold), so a banded point is rare and an unbanded one is decided the same way by any
# correct fp32 evaluation.  The same width is used for "equal" residual sums (fp32 sums of <= a few hundred terms).
BAND = 1e-4

# the sampling on integers is ransac_ref's, at sample size 3: i0 = h0 mod n, i1 = h1 mod (n - 1) skipping i0, i2 = h2 mod (n - 2) skipping both
mix64, _mix64v = rr.mix64, rr._mix64v
sample3 = lambda seed, trial, n: rr.sample_k(seed, trial, n, 3)          # noqa: E731
sample3v = lambda seed, trials, n: rr.sample_kv(seed, trials, n, 3)      # noqa: E731


# ------------------------------------------------------------------------------------------------------------ P3P (fp64)
def _polymul(a, b):
    """Batched polynomial product, coefficients in ascending powers along the last axis."""
    out = np.zeros(a.shape[:-1] + (a.shape[-1] + b.shape[-1] - 1,))
    for i in range(a.shape[-1]):
        out[..., i:i + b.shape[-1]] += a[..., i:i + 1] * b
    return out


def _quartic_roots(q):
    """Roots [T, 4] (complex) of q0 + q1 u + .. + q4 u^4 through the eigenvalues of stacked companion matrices; the reversed
    polynomial is solved instead (roots 1/u) where its leading coefficient is the larger one."""
    q = q / np.max(np.abs(q), axis=1, keepdims=True)
    rev = np.abs(q[:, 0]) > np.abs(q[:, 4])
    c = np.where(rev[:, None], q[:, ::-1], q)
    lead = c[:, 4]
    dead = ~(np.abs(lead) > 1e-300) | ~np.isfinite(c).all(1)
    c = np.where(dead[:, None], np.array([1.0, 0, 0, 0, 1.0]), c)
    C = np.zeros((len(q), 4, 4))
    C[:, 1, 0] = C[:, 2, 1] = C[:, 3, 2] = 1.0
    C[:, :, 3] = -c[:, :4] / c[:, 4:5]
    r = np.linalg.eigvals(C)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(rev[:, None], 1.0 / r, r)
    r[dead] = np.nan
    return r


def _depth_residual(s, y, a):
    """r_ij = |s_i y_i - s_j y_j|^2 - a_ij for (ij) = (12, 13, 23) [M, 3], from the difference vectors (less cancellation than
    the expanded cosine form when the triangle is small against its depth)."""
    P = s[:, :, None] * y
    d = np.stack([P[:, 0] - P[:, 1], P[:, 0] - P[:, 2], P[:, 1] - P[:, 2]], 1)
    return np.einsum("mij,mij->mi", d, d) - a


def _frame(p0, p1, p2):
    """Orthonormal frames [M, 3, 3] (columns e1, e2, e3) of triangles: e1 along p0 -> p1, e3 the normal."""
    e1 = p1 - p0
    e1 = e1 / np.linalg.norm(e1, axis=1, keepdims=True)
    e3 = np.cross(p1 - p0, p2 - p0)
    e3 = e3 / np.linalg.norm(e3, axis=1, keepdims=True)
    return np.stack([e1, np.cross(e3, e1), e3], 2)


def p3p_ref(y, X):
    """Every pose R X_i + t = s_i y_i, s_i > 0, of T samples at once.  y [T, 3, 3]: unit bearings (rows), X [T, 3, 3]: 3D points.

    Route (not the kernel's): with u = s2 / s1, v = s3 / s1 the three distance equations give v = N(u) / D(u) and a quartic in u
    (Grunert's elimination, carried out on coefficient arrays); its roots come from companion-matrix eigenvalues; every root (and,
    for a nearly double root, both sides of it) seeds Newton on the three distance equations in the depths, run to a residual of
    1e-14 relative (times the conditioning (s_i + s_j) / |X_i - X_j| for triangles small against their depth); converged depth
    triples are de-duplicated, and the pose follows from orthonormal frames of the triangle in the two coordinate systems.

    Returns a dict: R [T, 4, 3, 3], t [T, 4, 3], s [T, 4, 3], valid [T, 4], collinear [T] = |d12 x d13|^2 / (a12 a13),
    coplanar [T] = |det[y0 y1 y2]|, sep [T] = the smallest relative distance between two depth solutions (inf with fewer than 2)."""
    y = np.asarray(y, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    T = len(y)
    d12, d13, d23 = X[:, 0] - X[:, 1], X[:, 0] - X[:, 2], X[:, 1] - X[:, 2]
    a = np.stack([(d12 * d12).sum(1), (d13 * d13).sum(1), (d23 * d23).sum(1)], 1)
    nx = np.cross(d12, d13)
    with np.errstate(all="ignore"):
        collinear = (nx * nx).sum(1) / (a[:, 0] * a[:, 1])
        coplanar = np.abs(np.linalg.det(y))
        usable = (collinear > COLLINEAR_MIN) & (coplanar > COPLANAR_MIN) & np.isfinite(collinear)
        c12, c13, c23 = (y[:, 0] * y[:, 1]).sum(1), (y[:, 0] * y[:, 2]).sum(1), (y[:, 1] * y[:, 2]).sum(1)
        a13, a23 = a[:, 1] / a[:, 0], a[:, 2] / a[:, 0]                  # distances in units of |X1 - X2|
        one, zero = np.ones(T), np.zeros(T)
        p = np.stack([one, -2 * c12, one], 1)                            # 1 + u^2 - 2 c12 u  (= 1 / s1^2 in those units)
        k = a23 - a13
        N = np.stack([1 + k, -2 * c12 * k, k - 1], 1)                    # (1 - u^2) + (a23 - a13) p
        D = np.stack([2 * c13, -2 * c23], 1)                             # 2 (c13 - c23 u)
        E = np.stack([one, zero, zero], 1) - a13[:, None] * p            # 1 - a13 p
        ND = np.concatenate([_polymul(N, D), zero[:, None]], 1)                # degree 3, padded
        quartic = _polymul(N, N) - 2 * c13[:, None] * ND + _polymul(E, _polymul(D, D))
        bad = ~np.isfinite(quartic).all(1) | ~usable
        quartic[bad] = np.array([1.0, 0, 0, 0, 1.0])
        r = _quartic_roots(quartic)                                       # [T, 4]
        re, im = r.real, np.abs(r.imag)
        ucand = np.stack([re, re + im, re - im], 2).reshape(T, 12)        # [T, 12]
        pu = 1 - 2 * c12[:, None] * ucand + ucand * ucand
        Nu = (1 - ucand * ucand) + k[:, None] * pu
        Du = 2 * (c13[:, None] - c23[:, None] * ucand)
        disc = np.sqrt(np.maximum(0.0, c13[:, None] ** 2 - 1 + a13[:, None] * pu))
        vcand = np.stack([Nu / Du, c13[:, None] + disc, c13[:, None] - disc], 2)      # [T, 12, 3]
        s1 = np.sqrt(a[:, 0:1] / pu)                                                  # back in the caller's units
        s = np.stack([np.broadcast_to(s1[:, :, None], vcand.shape), np.broadcast_to((ucand * s1)[:, :, None], vcand.shape),
                      vcand * s1[:, :, None]], 3).reshape(T, 36, 3)
        C = s.shape[1]
        s = s.reshape(T * C, 3)
        yy = np.repeat(y, C, axis=0)
        aa = np.repeat(a, C, axis=0)
        cc = np.repeat(np.stack([c12, c13, c23], 1), C, axis=0)
        alive = np.isfinite(s).all(1) & (s > 0).all(1) & np.repeat(usable, C)
        s[~alive] = 1.0
        for _ in range(12):                                               # Newton on the three distance equations
            res = _depth_residual(s, yy, aa)
            z = np.zeros(len(s))
            J0 = np.stack([2 * (s[:, 0] - cc[:, 0] * s[:, 1]), 2 * (s[:, 1] - cc[:, 0] * s[:, 0]), z], 1)
            J1 = np.stack([2 * (s[:, 0] - cc[:, 1] * s[:, 2]), z, 2 * (s[:, 2] - cc[:, 1] * s[:, 0])], 1)
            J2 = np.stack([z, 2 * (s[:, 1] - cc[:, 2] * s[:, 2]), 2 * (s[:, 2] - cc[:, 2] * s[:, 1])], 1)
            k0, k1, k2 = np.cross(J1, J2), np.cross(J2, J0), np.cross(J0, J1)            # columns of det * J^-1
            det = (J0 * k0).sum(1)
            step = (k0 * res[:, 0:1] + k1 * res[:, 1:2] + k2 * res[:, 2:3]) / det[:, None]
            s = s - np.where(np.isfinite(step), step, 0.0)
            alive &= np.isfinite(s).all(1) & (np.abs(s) < 1e300).all(1)
            s[~alive] = 1.0
        res = np.abs(_depth_residual(s, yy, aa)) / aa
        pair = np.stack([s[:, 0] + s[:, 1], s[:, 0] + s[:, 2], s[:, 1] + s[:, 2]], 1) / np.sqrt(aa)
        alive &= (s > 0).all(1) & (res <= 1e-14 * np.maximum(1.0, pair)).all(1)
    s = s.reshape(T, C, 3)
    alive = alive.reshape(T, C)
    sol = np.ones((T, 4, 3))
    nsol = np.zeros(T, dtype=np.int64)
    rows = np.arange(T)
    for cnd in range(C):                                                  # de-duplicate (1e-8 relative) into <= 4 slots
        sc = s[:, cnd]
        new = alive[:, cnd].copy()
        for slot in range(4):
            same = np.abs(sc - sol[:, slot]).max(1) <= 1e-8 * np.abs(sc).max(1)
            new &= ~(same & (slot < nsol))
        new &= nsol < 4
        sol[rows[new], nsol[new]] = sc[new]
        nsol[new] += 1
    valid = np.arange(4)[None, :] < nsol[:, None]
    sep = np.full(T, np.inf)
    for i in range(4):
        for j in range(i + 1, 4):
            both = valid[:, i] & valid[:, j]
            dd = np.abs(sol[:, i] - sol[:, j]).max(1) / np.maximum(np.abs(sol[:, i]).max(1), np.abs(sol[:, j]).max(1))
            sep = np.where(both, np.minimum(sep, dd), sep)
    R = np.tile(np.eye(3), (T, 4, 1, 1))
    t = np.zeros((T, 4, 3))
    t[..., 2] = -1.0
    with np.errstate(all="ignore"):
        Fw = _frame(X[:, 0], X[:, 1], X[:, 2])
        for slot in range(4):
            P = sol[:, slot, :, None] * y
            Fc = _frame(P[:, 0], P[:, 1], P[:, 2])
            Rs = Fc @ np.transpose(Fw, (0, 2, 1))
            ts = P.mean(1) - np.einsum("mij,mj->mi", Rs, X.mean(1))
            ok = valid[:, slot] & np.isfinite(Rs).all((1, 2)) & np.isfinite(ts).all(1)
            valid[:, slot] = ok
            R[ok, slot] = Rs[ok]
            t[ok, slot] = ts[ok]
    return {"R": R, "t": t, "s": sol, "valid": valid, "collinear": collinear, "coplanar": coplanar, "sep": sep}


def near_degenerate(collinear, coplanar, sep):
    """The samples too close to a threshold (or to a double root) for two correct fp64 solvers to agree on."""
    return ~(collinear > NEAR * COLLINEAR_MIN) | ~(coplanar > NEAR * COPLANAR_MIN) | (sep < ROOT_SEP)


# ------------------------------------------------------------------------------------------------------------ scoring (fp32)
def score_f32(pose, Xc, xn, th2, order="point"):
    """The inlier test in np.float32.  pose = (R [..., 3, 3], t [..., 3]) on centred 3D points Xc [n, 3] and normalised 2D points
    xn [n, 2]; a point is an inlier when its depth is > 0 and its squared normalised error is <= th2.  Returns (count [...], fp32
    sum of the inliers' errors [...], inlier flags [..., n], banded flags [..., n]: |e / th2 - 1| <= BAND in front of the camera).
    order 'point': the sum is accumulated in fp32 in point order (a lane's hypothesis); 'tree': summed in fp64 and rounded once
    (the workgroup's scoring of one pose)."""
    f = np.float32
    R, t = np.asarray(pose[0]).astype(f), np.asarray(pose[1]).astype(f)
    Xc, xn, th2 = np.asarray(Xc).astype(f), np.asarray(xn).astype(f), f(th2)
    X0, X1, X2 = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    row = lambda i: R[..., i, 0, None] * X0 + R[..., i, 1, None] * X1 + R[..., i, 2, None] * X2 + t[..., i, None]  # noqa: E731
    with np.errstate(all="ignore"):
        z = row(2)
        iz = f(1) / z
        ex, ey = row(0) * iz - xn[:, 0], row(1) * iz - xn[:, 1]
        e = ex * ex + ey * ey
        inl = (z > 0) & (e <= th2)
        banded = (z > 0) & (np.abs(e.astype(np.float64) / np.float64(th2) - 1.0) <= BAND)
    ein = np.where(inl, e, f(0))
    if order == "point":
        total = np.cumsum(ein, axis=-1, dtype=f)[..., -1] if ein.shape[-1] else np.zeros(ein.shape[:-1], f)
    else:
        total = ein.astype(np.float64).sum(-1).astype(f)
    return inl.sum(-1), total, inl, banded


# ------------------------------------------------------------------------------------------------------------ LO-RANSAC
num_trials_needed, trial_limits = rr.trial_rule(3)       # COLMAP's ComputeNumTrials and trial limits for sample size 3


def _exp_so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def _gauss_newton(R, t, Xc, xn, steps):
    """Gauss-Newton on sum |proj(R X + t) - xn|^2 with the left perturbation x_cam' = Exp(w) x_cam + d; None when the normal
    equations are not positive definite."""
    for _ in range(steps):
        P = Xc @ R.T + t
        f = P[:, 2] > 0
        P, x = P[f], xn[f]
        iz = 1.0 / P[:, 2]
        u, v = P[:, 0] * iz, P[:, 1] * iz
        z = np.zeros_like(iz)
        g0, g1 = np.stack([iz, z, -u * iz], 1), np.stack([z, iz, -v * iz], 1)          # d (u, v) / d P
        J = np.concatenate([np.concatenate([np.cross(P, g0), g0], 1), np.concatenate([np.cross(P, g1), g1], 1)])
        r = np.concatenate([u - x[:, 0], v - x[:, 1]])
        H, g = J.T @ J, J.T @ r
        try:
            np.linalg.cholesky(H)
            d = -np.linalg.solve(H, g)
        except np.linalg.LinAlgError:
            return None
        if not np.isfinite(d).all():
            return None
        E = _exp_so3(d[:3])
        R, t = E @ R, E @ t + d[3:]
    return R, t


def lo_ransac_ref(x, X, cam, max_error_px, min_inlier_ratio=0.01, min_num_trials=1000, max_num_trials=100000, confidence=0.9999,
                  seed=0, mutate=None):
    """The rounds of the solver, restated.  Returns a dict: success, num_trials, num_inliers, inliers (bool [n]), qvec / tvec (the
    RANSAC pose, world coordinates, unrefined), banded (the case has a decision fp32 cannot tell), why (the reasons),
    point_banded (bool [n]: points in the band at the final scoring), rounds (per round: the winner's count, the best count after it, the winner's key).

    mutate breaks one rule on purpose (the tests use it to show that they would notice): 'drop_root' forgets each sample's last
    P3P solution, 'mult2' uses multiplier 2 in the stopping rule, 'sum_gt' prefers the larger residual sum, 'no_lo' skips the
    local optimisation."""
    x, X = np.asarray(x, dtype=np.float64).reshape(-1, 2), np.asarray(X, dtype=np.float64).reshape(-1, 3)
    n = len(x)
    out = {"success": False, "num_trials": 0, "num_inliers": 0, "inliers": np.zeros(n, bool), "qvec": np.array([1.0, 0, 0, 0]),
           "tvec": np.zeros(3), "banded": False, "why": [], "point_banded": np.zeros(n, bool), "rounds": []}
    if n < 4:
        return out
    mult = 2.0 if mutate == "mult2" else 3.0
    min_trials, max_trials = trial_limits(min_inlier_ratio, min_num_trials, max_num_trials, confidence, mult)
    c = X.mean(0)
    Xc = X - c
    xn = undistort(cam, x)
    Xf, xf = Xc.astype(np.float32), xn.astype(np.float32)
    th2 = np.float32((max_error_px / mean_focal(cam)) ** 2)
    yb = np.concatenate([xn, np.ones((n, 1))], 1)
    yb /= np.linalg.norm(yb, axis=1, keepdims=True)
    sum_sign = -1.0 if mutate == "sum_gt" else 1.0
    why = out["why"]
    best = None                                   # dict cnt, sum, key, R, t
    trials, rnd = 0, 0
    while True:
        tr = rnd * ROUND + np.arange(ROUND)
        tr = tr[tr < max_trials]
        ids = sample3v(seed, tr, n)
        sol = p3p_ref(yb[ids], Xc[ids])
        T = len(tr)
        valid = sol["valid"].copy()
        if mutate == "drop_root":
            last = valid.sum(1) - 1
            valid[np.arange(T)[last >= 0], last[last >= 0]] = False
        R, t = sol["R"].reshape(T * 4, 3, 3), sol["t"].reshape(T * 4, 3)
        valid = valid.reshape(-1)
        cnt, sm, inl, bnd = score_f32((R, t), Xf, xf, th2)
        cnt = np.where(valid, cnt, -1)
        key = (tr[:, None] * 4 + np.arange(4)).reshape(-1)
        order = np.lexsort((key, sum_sign * sm.astype(np.float64), -cnt))
        w = order[0]
        won = False
        if cnt[w] >= 0:
            nb_out, nb_any = (bnd & ~inl).sum(1), bnd.sum(1)
            relevant = best is None or cnt[w] + nb_out[w] >= best["cnt"]
            same = (np.abs(R - R[w]).max((1, 2)) + np.abs(t - t[w]).max(1) / (1 + np.abs(t[w]).max())) <= 1e-7
            rivals = valid & ~same
            if relevant:
                if bnd[w].any():
                    why.append(f"round {rnd}: a point of the round's winner is banded")
                if (rivals & (nb_any > 0) & (cnt + nb_out >= cnt[w])).any():
                    why.append(f"round {rnd}: a banded point could lift a rival over the winner")
                tie = rivals & (cnt == cnt[w])
                if (np.abs(sm[tie].astype(np.float64) - float(sm[w])) <= BAND * float(sm[w])).any():
                    why.append(f"round {rnd}: winner and runner-up tie on the count with sums within BAND")
                deg = np.repeat(near_degenerate(sol["collinear"], sol["coplanar"], sol["sep"]), 4)
                if (deg & valid & (cnt >= cnt[w])).any():
                    why.append(f"round {rnd}: a contender comes from a nearly degenerate sample")
            if best is None:
                won = True
            elif cnt[w] != best["cnt"]:
                won = cnt[w] > best["cnt"]
            elif sm[w] != best["sum"]:
                won = sum_sign * float(sm[w]) < sum_sign * float(best["sum"])
                close = np.abs(R[w] - best["R0"]).max() + np.abs(t[w] - best["t0"]).max() / (1 + np.abs(t[w]).max()) <= 1e-7
                if abs(float(sm[w]) - float(best["sum"])) <= BAND * float(sm[w]) and not close:
                    why.append(f"round {rnd}: the winner ties with the best so far, sums within BAND")
            else:
                won = key[w] < best["key"]
        if won:
            best = {"cnt": int(cnt[w]), "sum": sm[w], "key": int(key[w]), "R": R[w].copy(), "t": t[w].copy(), "R0": R[w].copy(),
                    "t0": t[w].copy()}
            for _ in range(0 if mutate == "no_lo" else LO_STEPS):
                _, _, sel, b0 = score_f32((best["R"], best["t"]), Xf, xf, th2, "tree")
                if b0.any():
                    why.append(f"round {rnd}: local optimisation selects its points with one in the band")
                new = _gauss_newton(best["R"], best["t"], Xc[sel], xn[sel], LO_GN)
                if new is None:
                    break
                lc, ls, _, b1 = score_f32(new, Xf, xf, th2, "tree")
                if b1.any():
                    why.append(f"round {rnd}: a re-estimated pose is scored with a point in the band")
                moved = np.abs(new[0] - best["R"]).max() + np.abs(new[1] - best["t"]).max() / (1 + np.abs(best["t"]).max()) > 1e-7
                if moved and lc == best["cnt"] and abs(float(ls) - float(best["sum"])) <= BAND * float(best["sum"]):
                    why.append(f"round {rnd}: a re-estimation ties on the count with sums within BAND")
                if not (lc > best["cnt"] or (lc == best["cnt"] and sum_sign * float(ls) < sum_sign * float(best["sum"]))):
                    break
                best.update(cnt=int(lc), sum=ls, R=new[0], t=new[1])
        out["rounds"].append((int(cnt[w]), -1 if best is None else best["cnt"], int(key[w])))
        trials = min((rnd + 1) * ROUND, max_trials)
        if trials >= max_trials:
            break
        if trials >= min_trials and best is not None and best["cnt"] > 0:
            if trials >= num_trials_needed(best["cnt"] / n, confidence, mult):
                break
        rnd += 1
    out["num_trials"] = int(trials)
    if best is not None and best["cnt"] >= 3:
        _, _, inl, bnd = score_f32((best["R"], best["t"]), Xf, xf, th2, "tree")
        if bnd.any():
            why.append("final scoring: a point is banded")
        out.update(success=True, num_inliers=best["cnt"], inliers=inl, point_banded=bnd, qvec=rotmat2qvec(best["R"]),
                   tvec=best["t"] - best["R"] @ c)
    out["banded"] = bool(why)
    return out


def absolute_pose_ref(x, X, cam, max_error_px, **conf):
    """lo_ransac_ref, then refine_cauchy from its pose over its mask: adds qvec_refined / tvec_refined."""
    r = lo_ransac_ref(x, X, cam, max_error_px, **conf)
    if r["success"]:
        r["qvec_refined"], r["tvec_refined"] = refine_cauchy(cam, r["qvec"], r["tvec"], x, X, r["inliers"], iters=1000)
    return r


# ------------------------------------------------------------------------------------------------------------ committed cases
# (n, outlier ratio, camera model, scene seed, max_error_px) of the RANSAC comparison: with min_num_trials 0 and confidence 0.9999 an inlier
# ratio of >= 0.5 stops after one round, 0.3 after 4 (1 010 trials asked for) and 0.2 after 14 (3 440).  The seeds are those at
# which the restatement itself meets the accuracy bounds of the suite (few points and 1 px noise do not always allow 0.1 deg).
# Half of the cases use a 3 px threshold: at 3 sigma of the noise the count and the mask depend on which hypothesis wins and on
# the local optimisation, which a 12 px threshold hides (every pose near the truth has the same inliers there).
RANSAC_CASES = [(12, 0.0, "SIMPLE_PINHOLE", 1, 12.0), (12, 0.25, "PINHOLE", 101, 3.0), (12, 0.0, "SIMPLE_RADIAL", 201, 12.0),
                (12, 0.25, "OPENCV", 303, 3.0), (40, 0.5, "SIMPLE_PINHOLE", 401, 12.0), (40, 0.7, "PINHOLE", 502, 3.0),
                (40, 0.5, "SIMPLE_RADIAL", 601, 12.0), (40, 0.7, "OPENCV", 702, 3.0), (80, 0.5, "SIMPLE_PINHOLE", 801, 12.0),
                (80, 0.7, "PINHOLE", 901, 3.0), (80, 0.8, "SIMPLE_RADIAL", 1003, 3.0), (80, 0.5, "OPENCV", 1101, 3.0),
                (80, 0.7, "SIMPLE_PINHOLE", 1201, 12.0), (80, 0.8, "PINHOLE", 1302, 3.0), (80, 0.7, "SIMPLE_RADIAL", 1401, 12.0),
                (80, 0.8, "OPENCV", 1501, 3.0)]
RANSAC_CONF = dict(min_num_trials=0, confidence=0.9999)
THRESH = 12.0
FAR_OFFSET = (4e5, 5e6, 100.0)
_cached = rr.make_cached()


def ransac_cases():
    """[(x, X, cam, q, t, max_error_px)] of RANSAC_CASES (1 px noise)."""
    def make():
        out = []
        for n, o, model, seed, th in RANSAC_CASES:
            cam = camera(model)
            q, t, x, X, _ = scene(np.random.RandomState(seed), cam, n, o, noise_px=1.0)
            out.append((x, X, cam, q, t, th))
        return out
    return _cached("ransac_cases", make)


def ransac_refs():
    """absolute_pose_ref of every case of ransac_cases(), computed once per process."""
    return _cached("ransac_refs", lambda: [absolute_pose_ref(x, X, cam, th, **RANSAC_CONF) for x, X, cam, _, _, th in ransac_cases()])


OPTION_THRESH = 3.0       # as in half of RANSAC_CASES: the count and the mask depend on the winning hypothesis
OPTION_SCENES = {"half": (41, 0.5), "third": (42, 0.7), "tenth": (43, 0.9)}      # kind: (scene seed, outlier ratio); 40 points each
OPTION_RUNS = ([("half", dict(seed=s)) for s in (1, 2, 3)]
               + [("half", dict(max_num_trials=300)), ("half", dict(min_num_trials=2000)), ("half", dict(confidence=1.0, max_num_trials=600)),
                  ("tenth", dict(min_inlier_ratio=0.5, confidence=0.99))]
               + [(k, dict(min_num_trials=0, confidence=c)) for k in ("half", "third") for c in (0.5, 0.99, 0.999999)])


def option_problem(kind="half"):
    """The option tests' problems (x, X, cam, q, t): 40 points, 1 px noise, OPENCV; 'half' = 50 % outliers, 'third' = 30 %
    inliers, 'tenth' = 10 % inliers."""
    def make():
        cam = camera("OPENCV")
        seed, outliers = OPTION_SCENES[kind]
        q, t, x, X, _ = scene(np.random.RandomState(seed), cam, 40, outliers, noise_px=1.0)
        return x, X, cam, q, t
    return _cached(("option", kind), make)


def option_ref(kind="half", **conf):
    x, X, cam, _, _ = option_problem(kind)
    return _cached(("option_ref", kind, tuple(sorted(conf.items()))), lambda: absolute_pose_ref(x, X, cam, OPTION_THRESH, **conf))


def scene_px(rs, cam, px, offset=(0.0, 0.0, 0.0)):
    """A pose and exact correspondences whose projections are the given pixels [n, 2] (undistorted through the camera model, so
    that it holds for strong distortion too), depths 1-60.  Returns (qvec, tvec, points2D, points3D)."""
    q, t = random_pose(rs)
    R = qvec2rotmat(q)
    n = len(px)
    d = 1.0 / rs.uniform(1.0 / 60, 1.0, n)
    Pc = np.concatenate([undistort(cam, px), np.ones((n, 1))], 1) * d[:, None]
    X = (Pc - t) @ R + np.asarray(offset)
    t = t - R @ np.asarray(offset)
    x, _ = project(cam, q, t, X)
    return q, t, x, X


STRONG_CAMERAS = {   # strong barrel distortion (distortion_monotonic holds for both; tests/test_pose_ref_host.py checks it)
    "SIMPLE_RADIAL": [800.0, 320.0, 240.0, -0.25],
    "OPENCV": [805.0, 795.0, 318.0, 242.0, -0.3, 0.12, 0.01, -0.008],
}


def strong_scene(model):
    """200 exact points over the whole image of a strongly distorted camera, the four corners and the edge midpoints among them."""
    def make():
        cam = {"model": model, "width": 640, "height": 480, "params": list(STRONG_CAMERAS[model])}
        rs = np.random.RandomState(51)
        W, H = 640.0, 480.0
        px = np.array([[0, 0], [W, 0], [0, H], [W, H], [W / 2, 0], [W / 2, H], [0, H / 2], [W, H / 2]])
        px = np.concatenate([px, np.stack([rs.uniform(0, W, 192), rs.uniform(0, H, 192)], 1)])
        q, t, x, X = scene_px(rs, cam, px, offset=(300.0, -150.0, 40.0))
        return cam, q, t, x, X
    return _cached(("strong", model), make)


# P3P probes: one problem = n (4 or 5) exact correspondences whose sample of trial 0 (seed 0) is a triple of the family's shape;
# with max_num_trials = 1 the solver finds all n points if and only if its P3P returns the generating pose for that triple.
P3P_FAMILIES = [("generic", 0.0), ("collinear", 1e-1), ("collinear", 1e-2), ("collinear", 1e-3), ("coplanar", 1e-1), ("coplanar", 1e-2),
                ("coplanar", 1e-3), ("isosceles", 1e-2), ("isosceles", 1e-4), ("tiny", 1e-3), ("huge", 60.0), ("far", 0.0)]
P3P_PROBES = 512
P3P_ERROR_PX = 0.05


def _triple(rs, family, level):
    """Three points in the camera frame [3, 3] of the family's shape."""
    def generic(k):
        xn = np.stack([rs.uniform(-0.36, 0.36, k), rs.uniform(-0.27, 0.27, k)], 1)
        return np.concatenate([xn, np.ones((k, 1))], 1) / rs.uniform(1.0 / 60, 1.0, k)[:, None]
    if family in ("generic", "far"):
        return generic(3)
    if family == "collinear":                           # the sine of the angle at P0 is `level`
        P = generic(2)
        d = P[1] - P[0]
        perp = np.cross(d, rs.standard_normal(3))
        perp /= np.linalg.norm(perp)
        lam = rs.uniform(0.3, 0.7)
        return np.stack([P[0], P[1], P[0] + lam * d + level * lam * np.linalg.norm(d) * perp])
    if family == "coplanar":                            # three pixels on a line through the principal point's ray, the third
        phi = rs.uniform(0, 2 * np.pi)                  # lifted off the plane of the bearings by the sine `level`
        along, across = np.array([np.cos(phi), np.sin(phi)]), np.array([-np.sin(phi), np.cos(phi)])
        r = rs.permutation(np.array([rs.uniform(-0.27, -0.1), rs.uniform(-0.05, 0.05), rs.uniform(0.1, 0.27)]))
        xn = r[:, None] * along
        xn[2] += level * np.sqrt(1 + r[2] ** 2) * across
        return np.concatenate([xn, np.ones((3, 1))], 1) / rs.uniform(1.0 / 60, 1.0, 3)[:, None]
    if family == "isosceles":                           # equilateral, fronto-parallel, the camera on its axis; perturbed by `level`
        d = rs.uniform(2, 10)
        rho = d * rs.uniform(0.1, 0.25)
        a0 = rs.uniform(0, 2 * np.pi)
        ang = a0 + np.array([0, 2 * np.pi / 3, 4 * np.pi / 3])
        P = np.stack([rho * np.cos(ang), rho * np.sin(ang), np.full(3, d)], 1)
        return P + level * rho * rs.standard_normal((3, 3))
    if family == "tiny":                                # sides `level` of the depth
        P = generic(1)
        return np.concatenate([P, P + level * P[0, 2] * rs.standard_normal((2, 3))])
    if family == "huge":                                # depths 1 and `level`
        P = generic(3)
        P /= P[:, 2:3]
        return P * np.array([1.0, level, rs.choice([1.0, level])])[:, None]
    raise ValueError(family)


def p3p_probes(family, level):
    """The P3P_PROBES problems of one family: a dict with problems [(x, X, cam)], truth [(q, t)], triple [(i0, i1, i2)] and the
    restatement's verdict kept [bool]: p3p_ref finds the generating pose (1e-8) and the sample is clear of the degeneracy
    thresholds and of double roots (near_degenerate)."""
    def make():
        fi = [f for f, _ in P3P_FAMILIES].index(family) * 10 + [lv for f, lv in P3P_FAMILIES if f == family].index(level)
        rs = np.random.RandomState(7000 + fi)
        problems, truth, triples, ys, Xs = [], [], [], [], []
        for i in range(P3P_PROBES):
            cam = camera(MODELS[i % 4])
            n = 4 + (i // 4) % 2
            ids = sample3(0, 0, n)
            q, t = random_pose(rs)
            R = qvec2rotmat(q)
            Pc = np.zeros((n, 3))
            Pc[list(ids)] = _triple(rs, family, level)
            rest = [j for j in range(n) if j not in ids]
            xn = np.stack([rs.uniform(-0.36, 0.36, len(rest)), rs.uniform(-0.27, 0.27, len(rest))], 1)
            Pc[rest] = np.concatenate([xn, np.ones((len(rest), 1))], 1) / rs.uniform(1.0 / 60, 1.0, len(rest))[:, None]
            off = np.asarray(FAR_OFFSET if family == "far" else (0.0, 0.0, 0.0))
            X = (Pc - t) @ R + off
            t = t - R @ off
            x, _ = project(cam, q, t, X)
            problems.append((x, X, cam))
            truth.append((q, t))
            triples.append(ids)
            c = X.mean(0)
            yb = np.concatenate([undistort(cam, x[list(ids)]), np.ones((3, 1))], 1)
            ys.append(yb / np.linalg.norm(yb, axis=1, keepdims=True))
            Xs.append(X[list(ids)] - c)
        sol = p3p_ref(np.array(ys), np.array(Xs))
        kept = np.zeros(P3P_PROBES, bool)
        for i, (q, t) in enumerate(truth):
            R = qvec2rotmat(q)
            tc = t + R @ problems[i][1].mean(0)
            depth = np.median(problems[i][1] @ R.T[:, 2] + t[2])
            for k in range(4):
                if sol["valid"][i, k] and np.abs(sol["R"][i, k] - R).max() <= 1e-8 and np.abs(sol["t"][i, k] - tc).max() <= 1e-8 * depth:
                    kept[i] = True
        kept &= ~near_degenerate(sol["collinear"], sol["coplanar"], sol["sep"])
        return {"problems": problems, "truth": truth, "triple": triples, "kept": kept, "sol": sol}
    return _cached(("p3p", family, level), make)
