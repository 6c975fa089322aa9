"""numpy restatement of the bundle adjustment of DESIGN.md section 14, for the tests only (never imported by the product), and the
committed scenes the CPU checks of tests/test_bundle_host.py and the GPU tests of tests/test_gpu_bundle.py and
tests/test_gpu_bundle_edges.py share.

Written from the text of section 14, fp64.  It shares no step with the kernels' linear algebra: every damped step is solved densely
over all variable parameters, by two routes that share nothing but the residual function:

  route A  Jacobians by fourth-order central differences of the projection; Cholesky of the full damped normal equations.
  route B  its own analytic Jacobians (matrix form); a dense Schur complement, every solve by numpy.linalg.solve.

The largest disagreement of the two routes on a scene is that scene's floor (for a run to convergence: or the near-tie radius, see
floor()): the GPU tolerances are 10 x that floor (ceiling 1e-6).

Scenes with more than 1024 views or more than 2^19 observations have no dense H: lm_blocks() and arrow_step() solve the same damped
steps from the structure of H, each by both routes, and are checked against the dense routes on small scenes."""
import numpy as np

import pose_ref as pr

SCALE = 10.0                          # the scenes' size: the distance from the cameras to what they look at
ROUTE_A, ROUTE_B = ("fd", "chol"), ("analytic", "schur")


# ------------------------------------------------------------------------------------------------------------------ the model
def exp_so3(w):
    """Exp of rotation vectors [n, 3] -> [n, 3, 3]."""
    w = np.asarray(w, dtype=np.float64).reshape(-1, 3)
    th = np.linalg.norm(w, axis=1)
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th * th / 6, np.sin(ths) / ths)
    b = np.where(small, 0.5 - th * th / 24, (1 - np.cos(ths)) / (ths * ths))
    return np.eye(3)[None] + a[:, None, None] * K + b[:, None, None] * (K @ K)


def log_so3(R):
    """Rotation vector of one rotation matrix."""
    c = np.clip((np.trace(R) - 1) / 2, -1, 1)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v)
    if s < 1e-12:
        return v
    return v * (np.arctan2(s, c) / s)


class Problem:
    """cams: one camera dict per view; q [nv, 4], t [nv, 3]; X [np, 3]; vconst, pconst: bool; off [np + 1]; obs_view, obs_xy."""

    def __init__(self, cams, q, t, X, vconst, pconst, off, obs_view, obs_xy, loss="trivial", loss_scale=1.0, truth=None):
        self.cams = list(cams)
        self.K = np.array([pr._opencv(c) for c in cams], dtype=np.float64)
        self.q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
        self.R = np.stack([pr.qvec2rotmat(qi / np.linalg.norm(qi)) for qi in self.q])
        self.t = np.asarray(t, dtype=np.float64).reshape(-1, 3).copy()
        self.X = np.asarray(X, dtype=np.float64).reshape(-1, 3).copy()
        self.vconst, self.pconst = np.asarray(vconst, dtype=bool), np.asarray(pconst, dtype=bool)
        self.off = np.asarray(off, dtype=np.int64)
        self.obs_view = np.asarray(obs_view, dtype=np.int32)
        self.obs_xy = np.asarray(obs_xy, dtype=np.float64).reshape(-1, 2)
        self.obs_pt = np.repeat(np.arange(len(self.X)), np.diff(self.off)).astype(np.int64)
        self.loss, self.loss_scale = loss, float(loss_scale)
        self.truth = truth                                   # (R, t, X) of the scene, where there is one
        self.nv, self.np_ = len(self.t), len(self.X)
        # parameter numbering: the variable views' six each, then the variable points' three each; -1 = constant
        self.vidx = np.where(self.vconst, -1, 6 * (np.cumsum(~self.vconst) - 1))
        self.nc = 6 * int((~self.vconst).sum())
        self.pidx = np.where(self.pconst, -1, self.nc + 3 * (np.cumsum(~self.pconst) - 1))
        self.n = self.nc + 3 * int((~self.pconst).sum())

    def state(self):
        return self.R.copy(), self.t.copy(), self.X.copy()


def project_obs(K, R, t, X):
    """Per-row projection: K [n, 8] (fx fy cx cy k1 k2 p1 p2), R [n, 3, 3], t [n, 3], X [n, 3] -> pixels [n, 2], depth [n].  No depth test."""
    Pc = np.einsum("nij,nj->ni", R, X) + t
    u, v = Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2]
    r2 = u * u + v * v
    rad = K[:, 4] * r2 + K[:, 5] * r2 * r2
    ud = u + u * rad + 2 * K[:, 6] * u * v + K[:, 7] * (r2 + 2 * u * u)
    vd = v + v * rad + 2 * K[:, 7] * u * v + K[:, 6] * (r2 + 2 * v * v)
    return np.stack([K[:, 0] * ud + K[:, 2], K[:, 1] * vd + K[:, 3]], 1), Pc[:, 2]


def residuals(P, state):
    R, t, X = state
    px, z = project_obs(P.K[P.obs_view], R[P.obs_view], t[P.obs_view], X[P.obs_pt])
    return px - P.obs_xy, z


def rho(P, s):
    """(rho(s), rho'(s))."""
    if P.loss == "trivial":
        return s, np.ones_like(s)
    c2 = P.loss_scale ** 2
    return c2 * np.log1p(s / c2), 1.0 / (1.0 + s / c2)


def cost(P, state):
    r, _ = residuals(P, state)
    return 0.5 * float(np.sum(rho(P, (r * r).sum(1))[0]))


def jac_fd(P, state):
    """d residual / d (w, v, dX) per observation [no, 2, 9] by the five-point stencil on local copies of the observation's view and point."""
    R, t, X = state
    K, Ro, to, Xo = P.K[P.obs_view], R[P.obs_view], t[P.obs_view], X[P.obs_pt]
    J = np.zeros((len(Ro), 2, 9))
    steps = [1e-3] * 3 + [1e-3 * SCALE] * 6

    def f(k, h):
        d = np.zeros(9)
        d[k] = h
        Rk = exp_so3(d[None, :3]) @ Ro if k < 3 else Ro
        return project_obs(K, Rk, to + d[3:6], Xo + d[6:9])[0]

    for k in range(9):
        h = steps[k]
        J[:, :, k] = (-f(k, 2 * h) + 8 * f(k, h) - 8 * f(k, -h) + f(k, -2 * h)) / (12 * h)
    return J


def jac_analytic(P, state):
    """The same [no, 2, 9] by the chain rule in matrix form: d px / d Pc = diag(f) Jd Jproj; d Pc / d (w, v, X) = (-[R X]x, 1, R)."""
    R, t, X = state
    K, Ro, Xo = P.K[P.obs_view], R[P.obs_view], X[P.obs_pt]
    q = np.einsum("nij,nj->ni", Ro, Xo)
    Pc = q + t[P.obs_view]
    n = len(q)
    u, v, iz = Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2], 1.0 / Pc[:, 2]
    k1, k2, p1, p2 = K[:, 4], K[:, 5], K[:, 6], K[:, 7]
    r2 = u * u + v * v
    rad, dr = k1 * r2 + k2 * r2 * r2, k1 + 2 * k2 * r2
    Jd = np.zeros((n, 2, 2), dtype=q.dtype)
    Jd[:, 0, 0] = 1 + rad + 2 * u * u * dr + 2 * p1 * v + 6 * p2 * u
    Jd[:, 0, 1] = Jd[:, 1, 0] = 2 * u * v * dr + 2 * p1 * u + 2 * p2 * v
    Jd[:, 1, 1] = 1 + rad + 2 * v * v * dr + 2 * p2 * u + 6 * p1 * v
    Jp = np.zeros((n, 2, 3), dtype=q.dtype)
    Jp[:, 0, 0] = Jp[:, 1, 1] = iz
    Jp[:, 0, 2], Jp[:, 1, 2] = -u * iz, -v * iz
    A = K[:, :2, None] * (Jd @ Jp)
    qx = np.zeros((n, 3, 3), dtype=q.dtype)
    qx[:, 0, 1], qx[:, 0, 2], qx[:, 1, 0], qx[:, 1, 2], qx[:, 2, 0], qx[:, 2, 1] = -q[:, 2], q[:, 1], q[:, 2], -q[:, 0], -q[:, 1], q[:, 0]
    return np.concatenate([-A @ qx, A, A @ Ro], 2)


def normal_equations(P, state, jac):
    """(H, g, cost) over the variable parameters with the IRLS weights applied; H and g from the weighted J and r."""
    r, _ = residuals(P, state)
    s = (r * r).sum(1)
    rh, w = rho(P, s)
    J = (jac_fd if jac == "fd" else jac_analytic)(P, state) * np.sqrt(w)[:, None, None]
    rw = r * np.sqrt(w)[:, None]
    idx = np.concatenate([P.vidx[P.obs_view][:, None] + np.arange(6), P.pidx[P.obs_pt][:, None] + np.arange(3)], 1)
    live = np.concatenate([np.repeat(~P.vconst[P.obs_view][:, None], 6, 1), np.repeat(~P.pconst[P.obs_pt][:, None], 3, 1)], 1)
    H, g = np.zeros((P.n, P.n)), np.zeros(P.n)
    blocks = np.einsum("nki,nkj->nij", J, J)
    m = live[:, :, None] & live[:, None, :]
    I, Jx = np.broadcast_to(idx[:, :, None], m.shape), np.broadcast_to(idx[:, None, :], m.shape)
    np.add.at(H, (I[m], Jx[m]), blocks[m])
    np.add.at(g, idx[live], np.einsum("nki,nk->ni", J, rw)[live])
    return H, g, 0.5 * float(rh.sum())


def solve_step(P, H, g, lam, solver):
    D = np.clip(np.diag(H), 1e-6, 1e32)
    Hd = H + lam * np.diag(D)
    if solver == "chol":
        L = np.linalg.cholesky(Hd)
        return np.linalg.solve(L.T, np.linalg.solve(L, -g))
    nc = P.nc
    if nc == 0 or nc == P.n:
        return np.linalg.solve(Hd, -g)
    B, E, C = Hd[:nc, :nc], Hd[:nc, nc:], Hd[nc:, nc:]
    CiEt, Cig = np.linalg.solve(C, E.T), np.linalg.solve(C, g[nc:])
    dc = np.linalg.solve(B - E @ CiEt, -(g[:nc] - E @ Cig))
    return np.concatenate([dc, -(Cig + CiEt @ dc)])


def split_step(P, d):
    """The step as ([nv, 6], [np, 3]) with zeros for the constants."""
    dv, dp = np.zeros((P.nv, 6)), np.zeros((P.np_, 3))
    dv[~P.vconst] = d[:P.nc].reshape(-1, 6)
    dp[~P.pconst] = d[P.nc:].reshape(-1, 3)
    return dv, dp


def apply_step(P, state, d):
    R, t, X = state
    dv, dp = split_step(P, d)
    return exp_so3(dv[:, :3]) @ R, t + dv[:, 3:], X + dp


def lm(P, route, max_iterations=100, initial_lambda=1e-4, gradient_tolerance=1e-10, function_tolerance=0.0):
    """Section 14's loop.  Returns a dict: state, initial_cost, initial_gmax, cost, gmax, lambda, iterations, accepted, status and the
    first step tried."""
    jac, solver = route
    state, lam = P.state(), initial_lambda
    H, g, c = normal_equations(P, state, jac)
    out = {"initial_cost": c, "initial_gmax": float(np.abs(g).max()) if len(g) else 0.0, "first_step": None, "accepted": 0}
    it, status = 0, "max_iterations"
    if not np.isfinite(c):
        out.update(state=state, cost=c, gmax=out["initial_gmax"], iterations=0, status="non_finite_cost")
        out["lambda"] = lam
        return out
    while True:
        gmax = float(np.abs(g).max()) if len(g) else 0.0
        if gmax <= gradient_tolerance:
            status = "gradient_tolerance"
            break
        if lam > 1e12:
            status = "lambda_overflow"
            break
        if it >= max_iterations:
            break
        d = solve_step(P, H, g, lam, solver)
        if out["first_step"] is None:
            out["first_step"] = split_step(P, d)
        trial = apply_step(P, state, d)
        with np.errstate(all="ignore"):
            ct = cost(P, trial)
        it += 1
        if np.isfinite(ct) and ct < c:
            prev, state, lam = c, trial, lam * 0.1
            out["accepted"] += 1
            H, g, c = normal_equations(P, state, jac)
            if abs(prev - c) <= function_tolerance * prev:
                status = "function_tolerance"
                break
        else:
            lam *= 10.0
    out.update(state=state, cost=c, gmax=float(np.abs(g).max()) if len(g) else 0.0, iterations=it, status=status)
    out["lambda"] = lam
    return out


def state_diff(a, b):
    """The largest difference of two states: rotation angle between corresponding views (radians), translations and points relative
    to the scenes' size."""
    Ra, ta, Xa = a
    Rb, tb, Xb = b
    rot = max([np.linalg.norm(log_so3(Ra[i] @ Rb[i].T)) for i in range(len(Ra))] + [0.0])
    tr = float(np.abs(ta - tb).max()) / SCALE if len(ta) else 0.0
    pt = float(np.abs(Xa - Xb).max()) / SCALE if len(Xa) else 0.0
    return max(rot, tr, pt)


def step_diff(a, b):
    """|a - b| / |b| of two steps ([nv, 6], [np, 3]), 2-norms over everything."""
    num = np.sqrt(((a[0] - b[0]) ** 2).sum() + ((a[1] - b[1]) ** 2).sum())
    return float(num / np.sqrt((b[0] ** 2).sum() + (b[1] ** 2).sum()))


def step_between(P, new_state):
    """The step ([nv, 6], [np, 3]) that takes P's state to new_state."""
    R, t, X = new_state
    dv = np.zeros((P.nv, 6))
    for i in range(P.nv):
        dv[i, :3] = log_so3(R[i] @ P.R[i].T)
        dv[i, 3:] = t[i] - P.t[i]
    return dv, X - P.X


# ------------------------------------------------------------------------------------------------------------------ structured solvers
# For scenes whose dense H does not fit: lm_blocks() for a list of independent Problems (clusters), arrow_step() for a few views and
# very many points.  Both are checked against the dense routes on small scenes in tests/test_bundle_host.py.
def merge(problems):
    """The one Problem that a list of independent Problems makes: their views, points and observations one after the other."""
    vo = np.cumsum([0] + [p.nv for p in problems])
    oo = np.cumsum([0] + [len(p.obs_view) for p in problems])
    cat = lambda f: np.concatenate([f(p) for p in problems])
    off = np.concatenate([[0]] + [p.off[1:] + oo[i] for i, p in enumerate(problems)])
    return Problem([c for p in problems for c in p.cams], cat(lambda p: p.q), cat(lambda p: p.t), cat(lambda p: p.X), cat(lambda p: p.vconst),
                   cat(lambda p: p.pconst), off, np.concatenate([p.obs_view + vo[i] for i, p in enumerate(problems)]), cat(lambda p: p.obs_xy),
                   problems[0].loss, problems[0].loss_scale)


def _join(parts):
    return tuple(np.concatenate([s[k] for s in parts]) for k in range(len(parts[0])))


def lm_blocks(problems, route, max_iterations=100, initial_lambda=1e-4, gradient_tolerance=1e-10, function_tolerance=0.0):
    """lm() of merge(problems) without the merged H: one lambda, one accept / reject decision on the summed cost, the damped step solved
    cluster by cluster (H is block diagonal over the clusters).  Returns lm()'s dict (states joined in merge()'s order) and 'history':
    per iteration (cost before, trial cost, accepted, lambda used)."""
    jac, solver = route
    states, lam = [p.state() for p in problems], initial_lambda
    lin = lambda: [normal_equations(p, st, jac) for p, st in zip(problems, states)]
    gmax_of = lambda sy: max([float(np.abs(g).max()) for _, g, _ in sy if len(g)] + [0.0])
    sy = lin()
    c = sum(x[2] for x in sy)
    out = {"initial_cost": c, "initial_gmax": gmax_of(sy), "first_step": None, "accepted": 0, "history": []}
    it, status = 0, "max_iterations"
    while np.isfinite(c):
        if gmax_of(sy) <= gradient_tolerance:
            status = "gradient_tolerance"
            break
        if lam > 1e12:
            status = "lambda_overflow"
            break
        if it >= max_iterations:
            break
        ds = [solve_step(p, H, g, lam, solver) for p, (H, g, _) in zip(problems, sy)]
        if out["first_step"] is None:
            out["first_step"] = _join([split_step(p, d) for p, d in zip(problems, ds)])
        trials = [apply_step(p, st, d) for p, st, d in zip(problems, states, ds)]
        with np.errstate(all="ignore"):
            ct = sum(cost(p, tr) for p, tr in zip(problems, trials))
        it += 1
        ok = bool(np.isfinite(ct) and ct < c)
        out["history"].append((c, ct, ok, lam))
        if ok:
            prev, states, lam = c, trials, lam * 0.1
            out["accepted"] += 1
            sy = lin()
            c = sum(x[2] for x in sy)
            if abs(prev - c) <= function_tolerance * prev:
                status = "function_tolerance"
                break
        else:
            lam *= 10.0
    if not np.isfinite(c):
        status = "non_finite_cost"
    out.update(state=_join(states), cost=c, gmax=gmax_of(sy), iterations=it, status=status)
    out["lambda"] = lam
    return out


def _linearised(P, state, jac):
    """(J [no, 2, 9], r [no, 2], cost) with the IRLS weights applied and the columns of constant views and points zeroed."""
    r, _ = residuals(P, state)
    rh, w = rho(P, (r * r).sum(1))
    sw = np.sqrt(w)
    J = (jac_fd if jac == "fd" else jac_analytic)(P, state) * sw[:, None, None]
    J[:, :, :6] *= (~P.vconst[P.obs_view])[:, None, None]
    J[:, :, 6:] *= (~P.pconst[P.obs_pt])[:, None, None]
    return J, r * sw[:, None], rh


def gradients(P, state, jac="analytic"):
    """(gc [nv, 6], gp [np, 3], cost): J^T r summed per view and per point (zero for the constants)."""
    J, rw, rh = _linearised(P, state, jac)
    g = np.einsum("nki,nk->ni", J, rw)
    gc, gp = np.zeros((P.nv, 6), dtype=g.dtype), np.zeros((P.np_, 3), dtype=g.dtype)
    np.add.at(gc, P.obs_view, g[:, :6])
    np.add.at(gp, P.obs_pt, g[:, 6:])
    return gc, gp, 0.5 * float(rh.sum())


def arrow_step(P, state, lam, route):
    """The damped step ([nv, 6], [np, 3]) of solve_step() from the arrow structure of H: the points' 3x3 blocks eliminated in batched form
    (route A: batched Cholesky, Jacobians by central differences; route B: numpy.linalg.solve on the stacked blocks, analytic Jacobians),
    the reduced camera system over all 6 nv view parameters solved densely.  A constant (or unobserved) view or point has a zero block,
    which the clamped damping lambda 1e-6 makes regular, and a zero gradient: its step is zero."""
    jac, solver = route
    J, rw, _ = _linearised(P, state, jac)
    Jc, Jp = J[:, :, :6], J[:, :, 6:]
    g = np.einsum("nki,nk->ni", J, rw)
    gc, gp = np.zeros((P.nv, 6)), np.zeros((P.np_, 3))
    B, V, E = np.zeros((P.nv, 6, 6)), np.zeros((P.np_, 3, 3)), np.zeros((P.np_, 6 * P.nv, 3))
    np.add.at(gc, P.obs_view, g[:, :6])
    np.add.at(gp, P.obs_pt, g[:, 6:])
    np.add.at(B, P.obs_view, np.einsum("nki,nkj->nij", Jc, Jc))
    np.add.at(V, P.obs_pt, np.einsum("nki,nkj->nij", Jp, Jp))
    np.add.at(E, (P.obs_pt[:, None], 6 * P.obs_view[:, None].astype(np.int64) + np.arange(6)), np.einsum("nki,nkj->nij", Jc, Jp))
    damp = lambda M: M + lam * np.clip(np.einsum("nii->ni", M), 1e-6, 1e32)[:, :, None] * np.eye(M.shape[1])
    Bd, Vd = damp(B), damp(V)
    if solver == "chol":
        L = np.linalg.cholesky(Vd)
        vsolve = lambda M: np.linalg.solve(np.swapaxes(L, 1, 2), np.linalg.solve(L, M))
    else:
        vsolve = lambda M: np.linalg.solve(Vd, M)
    ViEt, Vig = vsolve(np.swapaxes(E, 1, 2)), vsolve(gp[:, :, None])[:, :, 0]
    S = -np.einsum("pik,pkj->ij", E, ViEt)
    for v in range(P.nv):
        S[6 * v:6 * v + 6, 6 * v:6 * v + 6] += Bd[v]
    rhs = -(gc.reshape(-1) - np.einsum("pik,pk->i", E, Vig))
    if solver == "chol":
        L = np.linalg.cholesky(S)
        dc = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    else:
        dc = np.linalg.solve(S, rhs)
    return dc.reshape(-1, 6), -(Vig + ViEt @ dc)


def apply_split(state, step):
    R, t, X = state
    return exp_so3(step[0][:, :3]) @ R, t + step[0][:, 3:], X + step[1]


def extended_figures(P):
    """(cost, max |gradient entry|) of P's state by the same formulas in numpy.longdouble, the cost's terms summed by math.fsum (each
    as its double part and the rest, so nothing is rounded on the way in): what the fp64 sums of the restatement are measured against."""
    import copy
    import math
    ld = np.longdouble
    Q = copy.copy(P)
    Q.K, Q.R, Q.t, Q.X, Q.obs_xy = (np.asarray(a, dtype=ld) for a in (P.K, P.R, P.t, P.X, P.obs_xy))
    J, rw, rh = _linearised(Q, (Q.R, Q.t, Q.X), "analytic")
    hi = rh.astype(np.float64)
    c = 0.5 * math.fsum(np.concatenate([hi, (rh - hi).astype(np.float64)]))
    g = np.einsum("nki,nk->ni", J, rw)
    gc, gp = np.zeros((P.nv, 6), dtype=ld), np.zeros((P.np_, 3), dtype=ld)
    np.add.at(gc, P.obs_view, g[:, :6])
    np.add.at(gp, P.obs_pt, g[:, 6:])
    return c, float(max(np.abs(gc).max(), np.abs(gp).max()))


# ------------------------------------------------------------------------------------------------------------------ the scenes
TARGET = np.array([0.0, 0.0, SCALE])


def _look_at(centre, target, roll):
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    c, s = np.cos(roll), np.sin(roll)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ R
    return R, -R @ centre


MODELS = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "OPENCV"]


def arc_views(n, arc_deg=90.0):
    """n cameras of the four models in turn on an arc around TARGET, SCALE away, all looking at it: (cams, R, t)."""
    cams, Rs, ts = [], [], []
    for i in range(n):
        th = np.radians(arc_deg) * (i / max(n - 1, 1) - 0.5)
        c = TARGET + SCALE * np.array([np.sin(th), 0.03 * np.sin(1.3 * i), -np.cos(th)])
        R, t = _look_at(c, TARGET, 0.04 * np.sin(0.8 * i))
        cams.append(pr.camera(MODELS[i % 4]))
        Rs.append(R)
        ts.append(t)
    return cams, np.stack(Rs), np.stack(ts)


def _perturb(rs, R, t, rot_deg, trans):
    w = rs.standard_normal((len(R), 3))
    w *= np.radians(rot_deg) / np.linalg.norm(w, axis=1, keepdims=True)
    v = rs.standard_normal((len(R), 3))
    v *= trans / np.linalg.norm(v, axis=1, keepdims=True)
    return exp_so3(w) @ R, t + v


def build(seed, cams, R, t, X, tracks, vconst, pconst, noise_px, rot_deg, trans, point_sigma, outlier_share=0.0, loss="trivial", loss_scale=1.0,
          pconst_true=True, csr=None):
    """A Problem from the true scene: tracks[p] = the views that see point p in track order (or csr = (offsets, views) of all tracks, for
    scenes too large for a list); observations = projections + noise (a share of them moved by 30 to 60 px); the variable views' poses
    and points perturbed."""
    rs = np.random.RandomState(seed)
    if csr is not None:
        off, ov = np.asarray(csr[0], dtype=np.int64), np.asarray(csr[1], dtype=np.int32)
    else:
        off = np.concatenate([[0], np.cumsum([len(tk) for tk in tracks])]).astype(np.int64)
        ov = np.concatenate([np.asarray(tk, dtype=np.int32) for tk in tracks]) if len(tracks) else np.zeros(0, np.int32)
    op = np.repeat(np.arange(len(X)), np.diff(off))
    K = np.array([pr._opencv(c) for c in cams])
    xy, z = project_obs(K[ov], R[ov], t[ov], X[op])
    assert (z > 0).all()
    xy = xy + noise_px * rs.standard_normal(xy.shape)
    n_out = int(round(outlier_share * len(xy)))
    if n_out:
        sel = rs.choice(len(xy), n_out, replace=False)
        ang = rs.uniform(0, 2 * np.pi, n_out)
        xy[sel] += rs.uniform(30, 60, n_out)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    vconst, pconst = np.asarray(vconst, dtype=bool), np.asarray(pconst, dtype=bool)
    R0, t0 = _perturb(rs, R, t, rot_deg, trans)
    R0[vconst], t0[vconst] = R[vconst], t[vconst]
    X0 = X + point_sigma * rs.standard_normal(X.shape)
    if pconst_true:
        X0[pconst] = X[pconst]
    q0 = np.stack([pr.rotmat2qvec(Ri) for Ri in R0])
    return Problem(cams, q0, t0, X0, vconst, pconst, off, ov, xy, loss, loss_scale, truth=(R, t, X))


def _ball(rs, n, radius):
    return TARGET + rs.uniform(-radius, radius, (n, 3))


def arc_scene(noise_px=0.5, outlier_share=0.0, loss="trivial", loss_scale=1.0, vconst=(0, 1), pconst=(), seed=7, point_sigma=0.05, rot_deg=1.0,
              trans=0.02 * SCALE, arc_deg=90.0):
    """6 views of the four models on a 90 degree arc, 60 points seen by all, 0.5 px noise, poses off by 1 degree and 2 % of the depth."""
    rs = np.random.RandomState(seed)
    cams, R, t = arc_views(6, arc_deg)
    X = _ball(rs, 60, 2.5)
    vc, pc = np.zeros(6, bool), np.zeros(60, bool)
    vc[list(vconst)] = True
    pc[list(pconst)] = True
    return build(seed + 1, cams, R, t, X, [np.arange(6)] * 60, vc, pc, noise_px, rot_deg, trans, point_sigma, outlier_share, loss, loss_scale)


TRACK_LENGTHS = (2, 3, 63, 64, 65, 255, 256, 257, 300)
VIEW_COUNTS = (0, 1, 2, 255, 256, 257, 1000)


def long_track_scene(seed=11):
    """300 views; nine points observed TRACK_LENGTHS times (evenly spread views) and 60 points observed 20 times each."""
    rs = np.random.RandomState(seed)
    cams, R, t = arc_views(300)
    tracks = [np.unique(np.round(np.linspace(0, 299, k)).astype(np.int32)) for k in TRACK_LENGTHS]
    assert [len(tk) for tk in tracks] == list(TRACK_LENGTHS)
    tracks += [np.sort(rs.choice(300, 20, replace=False)).astype(np.int32) for _ in range(60)]
    X = _ball(rs, len(tracks), 2.0)
    vc = np.zeros(300, bool)
    vc[[0, 299]] = True
    return build(seed + 1, cams, R, t, X, tracks, vc, np.zeros(len(X), bool), 0.5, 0.3, 0.005 * SCALE, 0.03)


def busy_view_scene(seed=13):
    """Nine views: seven variable ones with VIEW_COUNTS observations and two constant ones that see all 1 000 points; 900 points constant."""
    rs = np.random.RandomState(seed)
    cams, R, t = arc_views(9)
    X = _ball(rs, 1000, 2.5)
    sees = [set(rs.choice(1000, k, replace=False).tolist()) for k in VIEW_COUNTS]
    tracks = [np.array([7, 8] + [v for v in range(7) if p in sees[v]], dtype=np.int32) for p in range(1000)]
    vc = np.zeros(9, bool)
    vc[[7, 8]] = True
    pc = np.ones(1000, bool)
    pc[rs.choice(1000, 100, replace=False)] = False
    return build(seed + 1, cams, R, t, X, tracks, vc, pc, 0.5, 0.3, 0.005 * SCALE, 0.03)


def trajectory_scene(seed=17):
    """The geometry of tri_ref.make_scene (the end-to-end test's map) as a Problem: 8 views along x looking at a slab 5 to 20 units away,
    250 points each seen where it projects into the image, 1 px noise, the first and the last view constant
    (the long baseline fixes the scale).  The stand-in on which the margin of
    the end-to-end test is measured without a GPU."""
    rs = np.random.RandomState(seed)
    cams, Rs, ts = [], [], []
    for i in range(8):
        c = np.array([float(i), 0.3 * np.sin(0.9 * i), 0.2 * np.cos(0.7 * i)])
        R, t = _look_at(c, np.array([i + rs.uniform(-0.5, 0.5), rs.uniform(-0.3, 0.3), 14.0]), rs.uniform(-0.05, 0.05))
        cams.append(pr.camera(MODELS[i % 4]))
        Rs.append(R)
        ts.append(t)
    R, t = np.stack(Rs), np.stack(ts)
    X = np.stack([rs.uniform(-3, 10, 250), rs.uniform(-3.5, 3.5, 250), rs.uniform(5, 20, 250)], 1)
    K = np.array([pr._opencv(c) for c in cams])
    tracks = []
    for p in range(250):
        px, z = project_obs(K, R, t, np.repeat(X[p][None], 8, 0))
        tracks.append(np.nonzero((z > 0) & (px[:, 0] > 5) & (px[:, 0] < 635) & (px[:, 1] > 5) & (px[:, 1] < 475))[0].astype(np.int32))
    keep = [p for p in range(250) if len(tracks[p]) >= 2]
    vc = np.zeros(8, bool)
    vc[[0, 7]] = True
    return build(seed + 1, cams, R, t, X[keep], [tracks[p] for p in keep], vc, np.zeros(len(keep), bool), 1.0, 0.3, 0.005 * SCALE, 0.05)


def constant_scenes():
    """name -> Problem: all views constant, all points constant, a constant point inside variable tracks, a mix."""
    out = {"views_constant": arc_scene(vconst=range(6), seed=21), "points_constant": arc_scene(pconst=range(60), seed=22, point_sigma=0.0),
           "one_point_constant": arc_scene(pconst=(17,), seed=23), "mix": arc_scene(vconst=(0, 3, 5), pconst=tuple(range(0, 60, 7)), seed=24)}
    return out


N_CLUSTERS = 206                      # x 5 views = 1030: cluster 204 straddles view 1024, cluster 205 lies beyond it
WIDE_POINTS = 262145                  # 2 observations each and 1 000 third ones: 525 290 observations, 257 and 385 reduction partials
SHORT_AT = (3, 11, 20, 29, 37, 46, 55, 64)       # 'short_tracks': one observation (views 2, 3, 4, 5) and none, in turn
CLUSTER_SCENES = ("clusters", "clusters_point_max")
POINT_MAX_CLUSTER = 100
CLUSTER_RUNS = {"clusters": dict(max_iterations=2), "clusters_point_max": dict(max_iterations=1)}      # the runs their references are computed for


def cluster_problems(point_max=False, seed=41):
    """N_CLUSTERS independent scenes of 5 views (the four models in turn, starting one further per cluster) on an arc of 60 to 80 degrees and
    12 points seen by all 5; the first and the last view of each constant.  The last cluster's variable views are turned 3 degrees, not 1: the
    largest gradient entry belongs to one of them (flat index >= 2048 of the view gradient).  point_max: a point's gradient is the largest
    entry instead.  A pixel of residual weighs ten times more in a view's rotation entries (f = 800) than in a point's (f / depth = 80), so
    this takes small pose perturbations everywhere (0.02 degrees, 0.04 % of the depth, points 0.02), all views of cluster POINT_MAX_CLUSTER
    constant and its last point moved by a whole unit (behind the first chunk of the point gradient; the clusters beyond view 1024 stay
    variable)."""
    rs = np.random.RandomState(seed)
    out = []
    for c in range(N_CLUSTERS):
        _, R, t = arc_views(5, rs.uniform(60.0, 80.0))
        cams = [pr.camera(MODELS[(i + c) % 4]) for i in range(5)]
        X = _ball(rs, 12, 2.5)
        last, planted = c == N_CLUSTERS - 1, c == POINT_MAX_CLUSTER
        vc = [True, False, False, False, True]
        if point_max:
            P = build(seed + 1 + c, cams, R, t, X, [np.arange(5)] * 12, [True] * 5 if planted else vc, np.zeros(12, bool), 0.5, 0.02, 0.0004 * SCALE, 0.02)
            if planted:
                P.X[11, 0] += 1.0
        else:
            P = build(seed + 1 + c, cams, R, t, X, [np.arange(5)] * 12, vc, np.zeros(12, bool), 0.5, 3.0 if last else 1.0, 0.02 * SCALE, 0.05)
        out.append(P)
    return out


def wide_scene(first=False, seed=51):
    """3 views on a 40 degree arc, the outer two constant; WIDE_POINTS points seen by the outer two, 1 000 of them also by the middle view (in
    the middle of the track); 0.5 px noise.  The middle view's pose is perturbed and then refined against its own observations with the
    points held, so that its gradient is small; the last point (first: point 0) is moved by 0.5 units, so that its gradient is the largest
    entry of all.  Built from arrays, not from a list of tracks."""
    rs = np.random.RandomState(seed)
    n = WIDE_POINTS
    cams, R, t = arc_views(3, 40.0)
    X = _ball(rs, n, 2.5)
    mid = np.zeros(n, bool)
    mid[1 + rs.choice(n - 2, 1000, replace=False)] = True      # neither point 0 nor the last
    off = np.concatenate([[0], np.cumsum(2 + mid)])
    ov = np.ones(off[-1], np.int32)
    ov[off[:-1]], ov[off[1:] - 1] = 0, 2
    P = build(seed + 1, cams, R, t, X, None, [True, False, True], np.zeros(n, bool), 0.5, 0.2, 0.002 * SCALE, 0.02, csr=(off, ov))
    own = Problem([cams[1]], P.q[1:2], P.t[1:2], P.X[mid], [False], np.ones(1000, bool), np.arange(1001), np.zeros(1000, np.int32), P.obs_xy[P.obs_view == 1])
    Rm, tm, _ = lm(own, ROUTE_B, max_iterations=20)["state"]
    q, tt = P.q.copy(), P.t.copy()
    q[1], tt[1] = pr.rotmat2qvec(Rm[0]), tm[0]
    X0 = P.X.copy()
    X0[0 if first else n - 1, 0] += 0.5
    return Problem(cams, q, tt, X0, P.vconst, P.pconst, off, ov, P.obs_xy, truth=P.truth)


def short_track_scene(seed=61):
    """'arc' with 8 more points among the 60 (at SHORT_AT): four seen once (by views 2, 3, 4, 5) and four never."""
    rs = np.random.RandomState(seed)
    cams, R, t = arc_views(6)
    X = _ball(rs, 68, 2.5)
    tracks = [np.arange(6)] * 68
    for k, j in enumerate(SHORT_AT):
        tracks[j] = np.array([2 + k // 2], np.int32) if k % 2 == 0 else np.zeros(0, np.int32)
    vc = np.zeros(6, bool)
    vc[[0, 1]] = True
    return build(seed + 1, cams, R, t, X, tracks, vc, np.zeros(68, bool), 0.5, 1.0, 0.02 * SCALE, 0.05)


REJECT_FIRST = dict(initial_lambda=1e-5, max_iterations=5)


def reject_first_scene():
    """'arc' on an arc of 3 degrees (little parallax: the depths are weakly determined), poses off by 3 degrees and 10 % of the depth, points by
    0.5, a Cauchy loss of scale 200 px.  From REJECT_FIRST's lambda the restatement accepts, rejects three times and accepts, by both routes
    and with every trial cost at least 5 % away from the cost it is compared with (found by a search over seeds, perturbations and scales
    on the CPU: with a short loss scale or a wide arc every step of this scene is accepted)."""
    return arc_scene(outlier_share=0.1, loss="cauchy", loss_scale=200.0, seed=72, rot_deg=3.0, trans=0.1 * SCALE, point_sigma=0.5, arc_deg=3.0)


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def scene(name):
    makers = {"arc": arc_scene, "arc_cauchy": lambda: arc_scene(outlier_share=0.1, loss="cauchy", loss_scale=2.0, seed=9),
              "long_tracks": long_track_scene, "busy_views": busy_view_scene, "trajectory": trajectory_scene}
    makers.update({k: (lambda k=k: constant_scenes()[k]) for k in ("views_constant", "points_constant", "one_point_constant", "mix")})
    makers.update({k: (lambda k=k: merge(clusters(k))) for k in CLUSTER_SCENES})
    makers.update({"wide": wide_scene, "wide_first": lambda: wide_scene(first=True), "short_tracks": short_track_scene, "reject_first": reject_first_scene})
    return cached(("scene", name), makers[name])


def clusters(name):
    """The list of Problems that scene(name) is the merge() of."""
    return cached(("clusters", name), lambda: cluster_problems(point_max=name == "clusters_point_max"))


def solution(name, route=ROUTE_A, **kw):
    """lm() of a scene (lm_blocks() of a scene of clusters), computed once per (scene, route, options) and left unchanged."""
    make = (lambda: lm_blocks(clusters(name), route, **kw)) if name in CLUSTER_SCENES else (lambda: lm(scene(name), route, **kw))
    return cached(("lm", name, route, tuple(sorted(kw.items()))), make)


def near_tie_radius(P, state):
    """How far from the minimum an accept / reject decision is still a near-tie, in state_diff's measure.  Section 14 accepts a step
    when the new cost is lower.  A residual component is the difference of two pixel coordinates and carries a rounding error of about
    one ulp of them, so a cost is known to N = sum rho' |r| ulp(xy) (first order).  A state at distance d from the minimum costs
    1/2 d^T H d more than the minimum; while that is below N, whether a step towards the minimum is accepted is decided by rounding,
    on the device and in the restatement alike.  The largest |d_k| with 1/2 d^T H d <= N is sqrt(2 N (H^-1)_kk)."""
    H, _, _ = normal_equations(P, state, "analytic")
    r, _ = residuals(P, state)
    w = rho(P, (r * r).sum(1))[1]
    N = float((w[:, None] * np.abs(r) * np.spacing(np.abs(P.obs_xy))).sum())
    dv, dp = split_step(P, np.sqrt(2 * N * np.diag(np.linalg.inv(H))))
    return max(dv[:, :3].max(initial=0.0), dv[:, 3:].max(initial=0.0) / SCALE, dp.max(initial=0.0) / SCALE)


def disagreement(name, **kw):
    """The largest difference between the two routes' results on a scene (state_diff)."""
    return cached(("disagreement", name, tuple(sorted(kw.items()))),
                  lambda: state_diff(solution(name, ROUTE_A, **kw)["state"], solution(name, ROUTE_B, **kw)["state"]))


def floor(name, **kw):
    """A scene's floor.  For a fixed number of steps (max_iterations given): the two routes' disagreement.  For a run to convergence:
    the larger of that disagreement and the near-tie radius at the restatement's minimum -- where both routes happen to take the same
    accept / reject decisions their disagreement (2.7e-14 on 'arc_cauchy') says nothing about a run that takes one decision differently."""
    def make():
        f = disagreement(name, **kw)
        if "max_iterations" not in kw:
            f = max(f, near_tie_radius(scene(name), solution(name, ROUTE_B, **kw)["state"]))
        if name in CLUSTER_SCENES:
            f = max(f, pcg_allowance(name)[1])
        return f
    return cached(("floor", name, tuple(sorted(kw.items()))), make)


def tolerance(name, **kw):
    """10 x the scene's floor, ceiling 1e-6."""
    return min(10 * floor(name, **kw), 1e-6)


def step_tolerance(name):
    """10 x step_floor(), ceiling 1e-6, relative to the step's norm."""
    return min(10 * step_floor(name), 1e-6)


# ------------------------------------------------------------------------------------------------------------------ floors of the large scenes
PCG_TOLERANCE = 1e-14                 # the relative residual the GPU tests' tight options let the device's conjugate gradients stop at
SUM_DEPTH = 32                        # additions a term of the device's largest reduction passes through: 8 serial + 8 tree + 2 serial + 8 tree, rounded up


def pcg_allowance(name, initial_lambda=1e-4):
    """What a relative residual of PCG_TOLERANCE may do to the first step of a scene of clusters, where a dense solve goes down to rounding:
    the change of the restatement's step when its right-hand side g becomes g + PCG_TOLERANCE |g| e, the largest over 8 seeded unit
    vectors e.  (relative to the step's norm, in state_diff's measure)."""
    def make():
        ps = clusters(name)
        sy = [normal_equations(p, p.state(), "analytic") for p in ps]
        gn = np.sqrt(sum(float(g @ g) for _, g, _ in sy))
        d0 = _join([split_step(p, solve_step(p, H, g, initial_lambda, "schur")) for p, (H, g, _) in zip(ps, sy)])
        rel = ab = 0.0
        for seed in range(8):
            rs = np.random.RandomState(1000 + seed)
            es = [rs.standard_normal(len(g)) for _, g, _ in sy]
            en = np.sqrt(sum(float(e @ e) for e in es))
            # the step is linear in g: the change is the step of the perturbation alone
            dv, dp = _join([split_step(p, solve_step(p, H, PCG_TOLERANCE * gn * e / en, initial_lambda, "schur")) for p, (H, _, _), e in zip(ps, sy, es)])
            rel = max(rel, step_diff((dv + d0[0], dp + d0[1]), d0))
            ab = max(ab, np.abs(dv[:, :3]).max(), np.abs(dv[:, 3:]).max() / SCALE, np.abs(dp).max() / SCALE)
        return rel, ab
    return cached(("pcg_allowance", name, initial_lambda), make)


def first_steps(name):
    """The first damped step of a scene (lambda 1e-4, lm()'s default) by both routes: arrow_step() for the 'wide' scenes, else the first step
    of the scene's solution() (lm_blocks() for clusters, shared with their other checks)."""
    def make():
        if name.startswith("wide"):
            return tuple(arrow_step(scene(name), scene(name).state(), 1e-4, r) for r in (ROUTE_A, ROUTE_B))
        kw = CLUSTER_RUNS.get(name, dict(max_iterations=1))
        return tuple(solution(name, r, **kw)["first_step"] for r in (ROUTE_A, ROUTE_B))
    return cached(("first_steps", name), make)


def step_floor(name):
    """The floor of a scene's first step, relative to the step's norm: the two routes' disagreement; for clusters the larger of that and
    pcg_allowance()."""
    a, b = first_steps(name)
    f = step_diff(a, b)
    return max(f, pcg_allowance(name)[0]) if name in CLUSTER_SCENES else f


def start(name):
    """(cost, max |gradient entry|) of a scene's initial state by gradients(), computed once."""
    def make():
        gc, gp, c = gradients(scene(name), scene(name).state())
        return c, float(max(np.abs(gc).max(), np.abs(gp).max()))
    return cached(("start", name), make)


def sum_floors(name):
    """(cost, max |g|) floors of a scene too large for its sums' rounding to be ignored: the relative difference between the fp64 restatement
    and extended_figures(), or SUM_DEPTH 2^-53 where that is larger -- a sum of non-negative terms over a tree of depth d is off by at most
    d 2^-53 of itself, and no fixed order of summation can promise less.  Returns (cost floor, gmax floor, measured cost, measured gmax)."""
    def make():
        c, gmax = start(name)
        ce, ge = extended_figures(scene(name))
        mc, mg = abs(c - ce) / ce, abs(gmax - ge) / ge
        return max(mc, SUM_DEPTH * 2.0 ** -53), max(mg, SUM_DEPTH * 2.0 ** -53), mc, mg
    return cached(("sum_floors", name), make)
