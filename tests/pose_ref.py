"""numpy fp64 helpers for the pose tests only (never imported by the product): COLMAP's camera models, a synthetic scene
generator and the Cauchy-IRLS refinement the device result is compared against."""
import numpy as np

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


def undistort(cam, px):
    """Pixels [n, 2] -> normalised image coordinates (Newton on the distortion, as COLMAP's ImageToWorld)."""
    fx, fy, cx, cy = _opencv(cam)[:4]
    xd, yd = (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy
    u, v = xd.copy(), yd.copy()
    for _ in range(50):
        h = 1e-7
        fu, fv = distort(cam, u, v)
        au, av = distort(cam, u + h, v)
        bu, bv = distort(cam, u, v + h)
        j00, j10, j01, j11 = (au - fu) / h, (av - fv) / h, (bu - fu) / h, (bv - fv) / h
        ru, rv = fu - xd, fv - yd
        det = j00 * j11 - j01 * j10
        u, v = u - (j11 * ru - j01 * rv) / det, v - (j00 * rv - j10 * ru) / det
    return np.stack([u, v], 1)


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
        if np.linalg.norm(d) < 1e-13:
            break
    q = rotmat2qvec(R)
    return q, t
