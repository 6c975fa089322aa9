"""numpy restatement of the absolute pose with an unknown focal length, for the tests only: the factor set, the
sweep as pose_ref.lo_ransac_ref per scaled camera, sum_px and the selection order, the main run, a Levenberg-Marquardt over pose and
intrinsics written from the specification (analytic Jacobian) with a second formulation by central differences, and the re-scoring
rounds.  The sweeps are cached: 31 restated runs per scene cost seconds."""
import numpy as np

import pose_ref as pr

DEFAULTS = dict(num_focal_length_samples=30, min_focal_length_ratio=0.2, max_focal_length_ratio=5.0, sweep_max_num_trials=1024)
N_FOCAL = {"SIMPLE_PINHOLE": 1, "PINHOLE": 2, "SIMPLE_RADIAL": 1, "OPENCV": 2}
MAX_ROUNDS = 3
LM_ITERS = 100

# (model, scene seed, n, outlier ratio, max_error_px, prior ratio): the prior is the true focal divided by the ratio, extras zeroed
SWEEP_SCENES = [("SIMPLE_RADIAL", 21, 80, 0.3, 12.0, 0.65), ("SIMPLE_PINHOLE", 22, 80, 0.5, 12.0, 1.6), ("OPENCV", 23, 80, 0.5, 4.0, 2.5),
                ("PINHOLE", 24, 40, 0.7, 12.0, 0.4)]
# the true factor lies between two samples and the threshold is tight: the winner holds part of the inliers before the re-scoring
MIDGAP_SCENES = [("PINHOLE", 13, 80, 0.5, 4.0, 1.035), ("SIMPLE_PINHOLE", 14, 80, 0.3, 4.0, 0.4267)]
CONF = dict(min_num_trials=0, confidence=0.9999)


def factors(S=30, lo=0.2, hi=5.0):
    """a_i = lo + (hi - lo) (i / S)^2 for i = 0..S, from the integer i (the square is one multiplication)."""
    t = np.arange(S + 1, dtype=np.float64) / np.float64(S)
    tt = t * t
    return lo + (hi - lo) * tt


def scaled_camera(cam, a):
    """The camera with its focal parameters multiplied by a; principal point and extras as given."""
    out = dict(cam)
    p = [float(v) for v in cam["params"]]
    for i in range(N_FOCAL[cam["model"]]):
        p[i] = float(np.float64(p[i]) * np.float64(a))
    out["params"] = p
    return out


def prior_camera(cam, ratio):
    """The test's prior: focal / ratio, extras zeroed."""
    out = dict(cam)
    p = [float(v) for v in cam["params"]]
    nf = N_FOCAL[cam["model"]]
    for i in range(nf):
        p[i] = p[i] / ratio
    for i in range(nf + 2, len(p)):
        p[i] = 0.0
    out["params"] = p
    return out


def make_scene(model, seed, n, outliers, thr, ratio):
    """(x, X, true camera, prior camera, q, t, max_error_px)."""
    cam = pr.camera(model)
    q, t, x, X, _ = pr.scene(np.random.RandomState(seed), cam, n, outliers, 1.0)
    return x, X, cam, prior_camera(cam, ratio), q, t, thr


def capped(conf, cap):
    c = dict(conf)
    c["min_num_trials"] = min(int(c.get("min_num_trials", 1000)), int(cap))
    c["max_num_trials"] = min(int(c.get("max_num_trials", 100000)), int(cap))
    return c


def _support_sum(r, x, X, cam, thr):
    """The winner's fp32 residual sum (normalised units), re-scored from the run's pose."""
    if not r["success"]:
        return np.float32(0)
    c = X.mean(0)
    R = pr.qvec2rotmat(r["qvec"])
    th2 = np.float32((thr / pr.mean_focal(cam)) ** 2)
    _, sm, _, _ = pr.score_f32((R, r["tvec"] + R @ c), X - c, pr.undistort(cam, x), th2, "tree")
    return np.float32(sm)


_sweeps = {}
_mains = {}          # the main runs of focal_pose_ref, by scene key and winning sample


def sweep_ref(x, X, cam, thr, S=30, lo=0.2, hi=5.0, cap=1024, ignore_cap=False, key=None, **conf):
    """Per sample: lo_ransac_ref at the scaled camera under the capped trial limits.  Returns a list of dicts (the run's, plus cnt,
    sum_px, camera).  key caches the result."""
    if key is not None and (key, ignore_cap) in _sweeps:
        return _sweeps[(key, ignore_cap)]
    out = []
    c = dict(conf) if ignore_cap else capped(conf, cap)
    for a in factors(S, lo, hi):
        sc = scaled_camera(cam, a)
        try:
            r = pr.lo_ransac_ref(x, X, sc, thr, **c)
        except ArithmeticError:                     # the extras as given may not undistort at a small factor
            r = {"success": False, "num_trials": 0, "num_inliers": 0, "banded": True, "why": ["undistortion failed"]}
        fm = np.float32(pr.mean_focal(sc))
        r["cnt"] = int(r["num_inliers"]) if r["success"] else 0
        r["sum"] = _support_sum(r, x, X, sc, thr) if r["success"] else np.float32(0)
        r["sum_px"] = np.float32(np.float32(r["sum"] * fm) * fm)
        r["camera"] = sc
        out.append(r)
    if key is not None:
        _sweeps[(key, ignore_cap)] = out
    return out


def select_ref(sweep, on="sum_px"):
    """(winner, runner-up) sample indices: more inliers, then the smaller sum (in squared pixels; on='sum': normalised units, the
    broken rule), then the smaller index; winner -1 when no sample has 3 inliers."""
    order = sorted(range(len(sweep)), key=lambda i: (-sweep[i]["cnt"], float(sweep[i][on]), i))
    if sweep[order[0]]["cnt"] < 3:
        return -1, -1
    return order[0], (order[1] if len(order) > 1 else -1)


def selection_banded(sweep):
    """True when fp32 cannot be trusted to make the same choice: the winner's or the runner-up's run is banded, or they tie on the
    count with sums within pose_ref.BAND."""
    w, r = select_ref(sweep)
    if w < 0:
        return any(s["banded"] for s in sweep)
    if sweep[w]["banded"] or (r >= 0 and sweep[r]["banded"]):
        return True
    if r >= 0 and sweep[r]["cnt"] == sweep[w]["cnt"]:
        return abs(float(sweep[r]["sum_px"]) - float(sweep[w]["sum_px"])) <= pr.BAND * float(sweep[w]["sum_px"])
    return False


# ------------------------------------------------------------------------------------------------------------ LM with intrinsics
def _groups(model, refine_focal, refine_extra):
    """Indices into the camera's COLMAP parameter list that are refined."""
    nf = N_FOCAL[model]
    idx = list(range(nf)) if refine_focal else []
    if refine_extra:
        idx += list(range(nf + 2, len(pr.PARAMS[model])))
    return idx


def _residuals(cam, R, t, x, X):
    P = X @ R.T + t
    u, v = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    ud, vd = pr.distort(cam, u, v)
    fx, fy, cx, cy = pr._opencv(cam)[:4]
    return np.stack([fx * ud + cx - x[:, 0], fy * vd + cy - x[:, 1]], 1), P, u, v, ud, vd


def _update(cam, R, t, idx, d):
    E = pr._exp_so3(d[:3])
    c2 = dict(cam)
    p = [float(v) for v in cam["params"]]
    for j, i in enumerate(idx):
        p[i] += float(d[6 + j])
    c2["params"] = p
    return c2, E @ R, E @ t + d[3:6]


def _jacobian_analytic(cam, R, t, x, X, idx):
    r, P, u, v, ud, vd = _residuals(cam, R, t, x, X)
    fx, fy = pr._opencv(cam)[:2]
    j00, j01, j10, j11 = pr.distort_jacobian(cam, u, v)
    iz = 1.0 / P[:, 2]
    g0 = np.stack([fx * j00 * iz, fx * j01 * iz, -fx * (j00 * u + j01 * v) * iz], 1)     # d r0 / d P
    g1 = np.stack([fy * j10 * iz, fy * j11 * iz, -fy * (j10 * u + j11 * v) * iz], 1)
    n = len(x)
    J = np.zeros((n, 2, 6 + len(idx)))
    J[:, 0, :3], J[:, 1, :3] = np.cross(P, g0), np.cross(P, g1)     # left perturbation: dP = w x P + d
    J[:, 0, 3:6], J[:, 1, 3:6] = g0, g1
    r2 = u * u + v * v
    model = cam["model"]
    nf = N_FOCAL[model]
    z = np.zeros(n)
    cols = {}
    if nf == 1:
        cols[0] = (ud, vd)
    else:
        cols[0], cols[1] = (ud, z), (z, vd)
    e = nf + 2
    cols[e] = (fx * u * r2, fy * v * r2)
    cols[e + 1] = (fx * u * r2 * r2, fy * v * r2 * r2)
    cols[e + 2] = (2 * fx * u * v, fy * (r2 + 2 * v * v))
    cols[e + 3] = (fx * (r2 + 2 * u * u), 2 * fy * u * v)
    for j, i in enumerate(idx):
        J[:, 0, 6 + j], J[:, 1, 6 + j] = cols[i]
    return r, P, J


def _jacobian_numeric(cam, R, t, x, X, idx):
    r, P, *_ = _residuals(cam, R, t, x, X)
    m = 6 + len(idx)
    J = np.zeros((len(x), 2, m))
    for k in range(m):
        h = 1e-6 if k < 6 else 1e-6 * max(1e-3, abs(float(cam["params"][idx[k - 6]])))
        d = np.zeros(m)
        d[k] = h
        ra = _residuals(*_update(cam, R, t, idx, d), x, X)[0]
        rb = _residuals(*_update(cam, R, t, idx, -d), x, X)[0]
        J[:, :, k] = (ra - rb) / (2 * h)
    return r, P, J


def lm_ref(cam, qvec, tvec, x, X, mask, refine_focal, refine_extra, given=None, lo=0.2, hi=5.0, jac="analytic"):
    """Levenberg-Marquardt on sum log(1 + |r|^2) over the masked points (depth > 0) from section 22: the pose by the left
    perturbation, the selected camera parameters additively; damping H + lambda diag(H) + 1e-15 max diag(H) I, lambda from 1e-4,
    / 10 on acceptance (floor 1e-12), x 10 on rejection (stop above 1e12); a trial state is rejected when its cost is not finite or
    larger, or a focal length is not positive or leaves [lo, hi] x the given camera's.  Returns (camera, qvec, tvec)."""
    mask = np.asarray(mask, bool)
    x, X = np.asarray(x, np.float64)[mask], np.asarray(X, np.float64)[mask]
    given = cam if given is None else given
    nf = N_FOCAL[cam["model"]]
    f_given = np.array(given["params"][:nf], np.float64)
    idx = _groups(cam["model"], refine_focal, refine_extra)
    jf = _jacobian_analytic if jac == "analytic" else _jacobian_numeric
    R, t = pr.qvec2rotmat(np.asarray(qvec, np.float64) / np.linalg.norm(qvec)), np.asarray(tvec, np.float64).copy()

    def sums(cam, R, t):
        r, P, J = jf(cam, R, t, x, X, idx)
        ok = P[:, 2] > 0
        r, J = r[ok], J[ok]
        sq = (r * r).sum(1)
        w = 1.0 / (1.0 + sq)
        H = np.einsum("n,nra,nrb->ab", w, J, J)
        g = np.einsum("n,nra,nr->a", w, J, r)
        return H, g, float(np.log1p(sq).sum())

    with np.errstate(all="ignore"):
        H, g, cost = sums(cam, R, t)
        lam = 1e-4
        for _ in range(LM_ITERS):
            dg = np.diag(H)
            mx = dg.max()
            if not (mx > 0 and np.isfinite(mx)):
                break
            try:
                L = np.linalg.cholesky(H + np.diag(lam * dg + 1e-15 * mx))
            except np.linalg.LinAlgError:
                break
            d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            if not np.isfinite(d).all():
                break
            cn, Rn, tn = _update(cam, R, t, idx, d)
            fn = np.array(cn["params"][:nf], np.float64)
            valid = np.isfinite(fn).all() and np.isfinite(cn["params"]).all() and (fn > 0).all() and (fn >= lo * f_given).all() and \
                (fn <= hi * f_given).all() and np.isfinite(Rn).all() and np.isfinite(tn).all()
            step = float(d[:3] @ d[:3] + d[3:6] @ d[3:6] / (1.0 + t @ t))
            for j, i in enumerate(idx):
                step += float((d[6 + j] / cam["params"][i]) ** 2) if i < nf else float(d[6 + j] ** 2)
            if valid:
                Hn, gn, costn = sums(cn, Rn, tn)
            if valid and np.isfinite(costn) and costn <= cost:
                cam, R, t, H, g, cost = cn, Rn, tn, Hn, gn, costn
                lam = max(lam * 0.1, 1e-12)
                if step < 1e-26:
                    break
            else:
                lam *= 10.0
                if lam > 1e12 or step < 1e-26:
                    break
    return cam, pr.rotmat2qvec(R), t


def lm_floor(cam, qvec, tvec, x, X, mask, refine_focal, refine_extra):
    """What fp64 can tell apart at a minimum of the refinement's cost, per compared quantity (focal relative, extras absolute, rotation
    as the Frobenius norm of the matrix difference, translation relative to 1 + |t|).  The cost c is a sum known to eps c, and near
    the minimum it is 1/2 d^T H d above it, so a state d away is indistinguishable while d^T H d <= 2 eps c: along parameter i that
    ellipsoid reaches sqrt(2 eps c (H^-1)_ii).  Two correct LM implementations can stop anywhere inside it; where focal length and
    depth explain the same image (a small eigenvalue of H) it is long.  Computed from the restatement's H at its own solution."""
    mask = np.asarray(mask, bool)
    x, X = np.asarray(x, np.float64)[mask], np.asarray(X, np.float64)[mask]
    idx = _groups(cam["model"], refine_focal, refine_extra)
    R, t = qvec2rot(qvec), np.asarray(tvec, np.float64)
    r, P, J = _jacobian_analytic(cam, R, t, x, X, idx)
    ok = P[:, 2] > 0
    r, J = r[ok], J[ok]
    sq = (r * r).sum(1)
    H = np.einsum("n,nra,nrb->ab", 1.0 / (1.0 + sq), J, J)
    cost = max(float(np.log1p(sq).sum()), 1.0)
    d = np.sqrt(2 * np.finfo(np.float64).eps * cost * np.diag(np.linalg.pinv(H)))
    nf = N_FOCAL[cam["model"]]
    fo = [d[6 + j] / abs(cam["params"][i]) for j, i in enumerate(idx) if i < nf]
    ex = [d[6 + j] for j, i in enumerate(idx) if i >= nf]
    dw, dt = float(np.linalg.norm(d[:3])), float(np.linalg.norm(d[3:6]))
    nt = float(np.linalg.norm(t))
    return (float(max(fo, default=0.0)), float(max(ex, default=0.0)), np.sqrt(2.0) * dw, (dt + dw * nt) / (1.0 + nt))


def qvec2rot(qvec):
    q = np.asarray(qvec, np.float64)
    return pr.qvec2rotmat(q / np.linalg.norm(q))


def rescore(cam, qvec, tvec, x, X, thr):
    """(mask, relative distance of every squared error to the threshold): depth > 0 and squared pixel error <= thr^2, fp64."""
    p, z = pr.project(cam, qvec, tvec, X)
    with np.errstate(all="ignore"):
        e = ((p - x) ** 2).sum(1)
    return (z > 0) & (e <= thr * thr), np.abs(e / (thr * thr) - 1.0)


def refine_rounds_ref(cam, qvec, tvec, x, X, mask, thr, refine_focal, refine_extra, given, lo=0.2, hi=5.0, jac="analytic", rounds=MAX_ROUNDS):
    """At most `rounds` refinements, each over the current mask, re-scored in between; a mask that does not grow stops.  Returns
    (camera, qvec, tvec, mask, sizes, near): the sizes of the masks refined over, and the points within 1e-9 of a threshold at a
    re-scoring."""
    mask = np.asarray(mask, bool).copy()
    sizes, near = [int(mask.sum())], np.zeros(len(mask), bool)
    for r in range(rounds):
        cam, qvec, tvec = lm_ref(cam, qvec, tvec, x, X, mask, refine_focal, refine_extra, given, lo, hi, jac)
        if r + 1 >= rounds:
            break
        new, dist = rescore(cam, qvec, tvec, x, X, thr)
        near |= dist <= 1e-9
        if not new.sum() > mask.sum():
            break
        mask = new
        sizes.append(int(mask.sum()))
    return cam, qvec, tvec, mask, sizes, near


def focal_pose_ref(x, X, cam, thr, estimate=True, refine_focal=False, refine_extra=False, S=30, lo=0.2, hi=5.0, cap=1024, key=None,
                   select_on="sum_px", ignore_cap=False, rounds=MAX_ROUNDS, jac="analytic", **conf):
    """The whole call restated.  Returns a dict: success, focal_sample, focal_factor, camera, qvec, tvec, inliers, num_inliers,
    ransac_num_inliers, num_trials, sizes, banded (the selection or the main run has a decision fp32 cannot tell), sweep."""
    out = {"success": False, "focal_sample": -1, "focal_factor": 1.0, "camera": cam, "banded": False, "sweep": None, "sizes": []}
    main_cam = cam
    if estimate:
        sw = sweep_ref(x, X, cam, thr, S, lo, hi, cap, ignore_cap=ignore_cap, key=key, **conf)
        w, _ = select_ref(sw, select_on)
        out.update(sweep=sw, banded=selection_banded(sw), focal_sample=w)
        if w < 0:
            return out
        out["focal_factor"] = float(factors(S, lo, hi)[w])
        main_cam = sw[w]["camera"]
    mkey = None if key is None else (key, out["focal_sample"], estimate, ignore_cap, select_on, tuple(sorted(conf.items())))
    if mkey is None or mkey not in _mains:
        _mains[mkey] = pr.absolute_pose_ref(x, X, main_cam, thr, **conf)
    r = _mains[mkey]
    out["banded"] = out["banded"] or r["banded"]
    out.update(success=r["success"], camera=main_cam, num_trials=r["num_trials"], ransac_num_inliers=r["num_inliers"],
               num_inliers=r["num_inliers"], inliers=r["inliers"], qvec=r.get("qvec_refined", r["qvec"]), tvec=r.get("tvec_refined", r["tvec"]))
    if r["success"] and (refine_focal or refine_extra):
        c2, q, t, mask, sizes, near = refine_rounds_ref(main_cam, out["qvec"], out["tvec"], x, X, r["inliers"], thr, refine_focal, refine_extra,
                                                        cam, lo, hi, jac, rounds)
        out.update(camera=c2, qvec=q, tvec=t, inliers=mask, num_inliers=int(mask.sum()), sizes=sizes, near=near)
    return out


def focal_error(cam, true_cam):
    nf = N_FOCAL[cam["model"]]
    a, b = np.array(cam["params"][:nf], np.float64), np.array(true_cam["params"][:nf], np.float64)
    return float(np.abs(a / b - 1.0).max())
