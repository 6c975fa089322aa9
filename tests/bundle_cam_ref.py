"""numpy restatement of the bundle adjustment with camera intrinsics among the unknowns, for the tests only,
and the scenes tests/test_bundle_cam_host.py and tests/test_gpu_bundle_cam.py share.  Built on tests/bundle_ref.py: the same residual
function (bundle_ref.project_obs), the same loop, the same two routes that share nothing else:

  route A  Jacobians by fourth-order central differences over all parameters, the cameras' included; Cholesky of the full damped
           normal equations.
  route B  its own analytic Jk (matrix form) beside bundle_ref.jac_analytic; a dense Schur complement over [views ; cameras].

A state is (R, t, X, Kc): Kc [n_cameras, 8] holds every camera in OPENCV form (fx fy cx cy k1 k2 p1 p2).  An active parameter is a
direction in those eight words (the one focal length of a SIMPLE_* model is e_fx + e_fy), so a step is additive in Kc."""
import copy

import numpy as np

import bundle_ref as br
import pose_ref as pr

SCALE = br.SCALE
ROUTE_A, ROUTE_B = br.ROUTE_A, br.ROUTE_B
FOCAL, PRINCIPAL, EXTRA = 1, 2, 4
KMAX = 8
MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "OPENCV": 4}


def directions(model, refine):
    """The active parameters of a camera as rows of an [K, 8] matrix over the OPENCV words, in COLMAP order."""
    e = np.eye(8)
    simple = model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL")
    rows = []
    if refine & FOCAL:
        rows += [e[0] + e[1]] if simple else [e[0], e[1]]
    if refine & PRINCIPAL:
        rows += [e[2], e[3]]
    if refine & EXTRA:
        rows += {"SIMPLE_RADIAL": [e[4]], "OPENCV": [e[4], e[5], e[6], e[7]]}.get(model, [])
    return np.array(rows, dtype=np.float64).reshape(-1, 8)


def colmap_params(model, k8):
    """The model's parameters in COLMAP order from the OPENCV words."""
    k8 = np.asarray(k8, dtype=np.float64)
    return {"SIMPLE_PINHOLE": k8[[0, 2, 3]], "PINHOLE": k8[:4], "SIMPLE_RADIAL": k8[[0, 2, 3, 4]], "OPENCV": k8}[model]


class CamProblem(br.Problem):
    """bundle_ref.Problem plus cameras: cam_list (camera dicts, the start values), view_camera [nv], refine [n_cameras] (bit masks).
    Parameter numbering: the variable views' six each, the cameras' active parameters, the variable points' three each."""

    def __init__(self, cam_list, view_camera, refine, q, t, X, vconst, pconst, off, obs_view, obs_xy, loss="trivial", loss_scale=1.0, truth=None,
                 cam_truth=None):
        view_camera = np.asarray(view_camera, dtype=np.int32)
        super().__init__([cam_list[c] for c in view_camera], q, t, X, vconst, pconst, off, obs_view, obs_xy, loss, loss_scale, truth)
        self.cam_list, self.view_camera, self.refine = list(cam_list), view_camera, np.asarray(refine, dtype=np.int32)
        self.Kc = np.array([pr._opencv(c) for c in cam_list], dtype=np.float64).reshape(-1, 8)
        self.cam_truth = cam_truth
        self.ncam = len(cam_list)
        self.dirs = np.zeros((self.ncam, KMAX, 8))
        self.kcount = np.zeros(self.ncam, dtype=np.int64)
        for c, cam in enumerate(cam_list):
            d = directions(cam["model"], int(self.refine[c]))
            self.dirs[c, :len(d)] = d
            self.kcount[c] = len(d)
        self.kidx = self.nc + np.concatenate([[0], np.cumsum(self.kcount)[:-1]])
        self.na = self.nc + int(self.kcount.sum())              # the reduced system: views, then cameras
        self.pidx = np.where(self.pconst, -1, self.na + 3 * (np.cumsum(~self.pconst) - 1))
        self.n = self.na + 3 * int((~self.pconst).sum())
        self.obs_cam = self.view_camera[self.obs_view]

    def state(self):
        return self.R.copy(), self.t.copy(), self.X.copy(), self.Kc.copy()


def _at(P, Kc):
    """P as a bundle_ref.Problem whose views carry the cameras Kc."""
    Q = copy.copy(P)
    Q.K = Kc[P.view_camera]
    return Q


def residuals(P, state):
    return br.residuals(_at(P, state[3]), state[:3])


def cost(P, state):
    return br.cost(_at(P, state[3]), state[:3])


def jac_cam_fd(P, state):
    """d residual / d (the camera's active parameters) [no, 2, KMAX] by the five-point stencil on local copies of the observation's camera."""
    R, t, X, Kc = state
    Ko, Ro, to, Xo = Kc[P.obs_cam], R[P.obs_view], t[P.obs_view], X[P.obs_pt]
    J = np.zeros((len(Ro), 2, KMAX))
    for k in range(KMAX):
        d = P.dirs[P.obs_cam, k]                                # zero rows where the camera has fewer parameters
        h = np.where(np.abs(d[:, :4]).sum(1) > 0, 1.0, 1e-2)[:, None]      # pixels for f and c, 1e-2 for the distortion coefficients
        f = lambda s: br.project_obs(Ko + s * h * d, Ro, to, Xo)[0]
        J[:, :, k] = (-f(2) + 8 * f(1) - 8 * f(-1) + f(-2)) / (12 * h)
    return J


def jac_cam_analytic(P, state):
    """The same [no, 2, KMAX]: G = d px / d (fx fy cx cy k1 k2 p1 p2) in closed form, times the cameras' directions."""
    R, t, X, Kc = state
    K = Kc[P.obs_cam]
    Pc = np.einsum("nij,nj->ni", R[P.obs_view], X[P.obs_pt]) + t[P.obs_view]
    u, v = Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2]
    r2 = u * u + v * v
    rad = K[:, 4] * r2 + K[:, 5] * r2 * r2
    ud = u + u * rad + 2 * K[:, 6] * u * v + K[:, 7] * (r2 + 2 * u * u)
    vd = v + v * rad + 2 * K[:, 7] * u * v + K[:, 6] * (r2 + 2 * v * v)
    G = np.zeros((len(u), 2, 8))
    G[:, 0, 0], G[:, 1, 1], G[:, 0, 2], G[:, 1, 3] = ud, vd, 1.0, 1.0
    G[:, 0, 4], G[:, 1, 4] = K[:, 0] * u * r2, K[:, 1] * v * r2
    G[:, 0, 5], G[:, 1, 5] = K[:, 0] * u * r2 * r2, K[:, 1] * v * r2 * r2
    G[:, 0, 6], G[:, 1, 6] = K[:, 0] * 2 * u * v, K[:, 1] * (r2 + 2 * v * v)
    G[:, 0, 7], G[:, 1, 7] = K[:, 0] * (r2 + 2 * u * u), K[:, 1] * 2 * u * v
    return G @ np.swapaxes(P.dirs[P.obs_cam], 1, 2)


def jacobians(P, state, jac):
    """[no, 2, 6 + KMAX + 3]: view, camera, point columns."""
    Q = _at(P, state[3])
    J9 = (br.jac_fd if jac == "fd" else br.jac_analytic)(Q, state[:3])
    Jk = (jac_cam_fd if jac == "fd" else jac_cam_analytic)(P, state)
    return np.concatenate([J9[:, :, :6], Jk, J9[:, :, 6:]], 2)


def normal_equations(P, state, jac):
    """(H, g, cost) over the variable parameters with the IRLS weights applied."""
    r, _ = residuals(P, state)
    rh, w = br.rho(P, (r * r).sum(1))
    J = jacobians(P, state, jac) * np.sqrt(w)[:, None, None]
    rw = r * np.sqrt(w)[:, None]
    ar = np.arange(KMAX)
    idx = np.concatenate([P.vidx[P.obs_view][:, None] + np.arange(6), P.kidx[P.obs_cam][:, None] + ar, P.pidx[P.obs_pt][:, None] + np.arange(3)], 1)
    live = np.concatenate([np.repeat(~P.vconst[P.obs_view][:, None], 6, 1), ar[None] < P.kcount[P.obs_cam][:, None],
                           np.repeat(~P.pconst[P.obs_pt][:, None], 3, 1)], 1)
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
    na = P.na
    if na == 0 or na == P.n:
        return np.linalg.solve(Hd, -g)
    A, E, V = Hd[:na, :na], Hd[:na, na:], Hd[na:, na:]
    ViEt, Vig = np.linalg.solve(V, E.T), np.linalg.solve(V, g[na:])
    da = np.linalg.solve(A - E @ ViEt, -(g[:na] - E @ Vig))
    return np.concatenate([da, -(Vig + ViEt @ da)])


def split_step(P, d):
    """The step as ([nv, 6], [np, 3], [n_cameras, KMAX]) with zeros for what does not move."""
    dv, dp, dk = np.zeros((P.nv, 6)), np.zeros((P.np_, 3)), np.zeros((P.ncam, KMAX))
    dv[~P.vconst] = d[:P.nc].reshape(-1, 6)
    dk[np.arange(KMAX)[None] < P.kcount[:, None]] = d[P.nc:P.na]
    dp[~P.pconst] = d[P.na:].reshape(-1, 3)
    return dv, dp, dk


def apply_step(P, state, d):
    R, t, X, Kc = state
    dv, dp, dk = split_step(P, d)
    return br.exp_so3(dv[:, :3]) @ R, t + dv[:, 3:], X + dp, Kc + np.einsum("ck,cki->ci", dk, P.dirs)


def lm(P, route, max_iterations=100, initial_lambda=1e-4, gradient_tolerance=1e-10, function_tolerance=0.0):
    """bundle_ref.lm with the cameras among the unknowns; a trial state with a non-finite camera word or a focal length <= 0 is rejected."""
    jac, solver = route
    state, lam = P.state(), initial_lambda
    H, g, c = normal_equations(P, state, jac)
    out = {"initial_cost": c, "initial_gmax": float(np.abs(g).max()) if len(g) else 0.0, "first_step": None, "accepted": 0, "history": []}
    it, status = 0, "max_iterations"
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
        ok = bool(np.isfinite(ct) and ct < c and np.isfinite(trial[3]).all() and (trial[3][:, :2] > 0).all())
        out["history"].append((c, ct, ok, lam))
        if ok:
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


# ------------------------------------------------------------------------------------------------------------------ measures
def active_words(P):
    """[n_cameras, 8] bool: the OPENCV words some active parameter moves."""
    return (np.abs(P.dirs).sum(1) > 0)


def cam_diff(P, Ka, Kb):
    """The largest difference of the cameras' active words, relative to the word's own size in Kb (absolute where that is zero)."""
    m = active_words(P)
    if not m.any():
        return 0.0
    size = np.where(Kb[m] != 0, np.abs(Kb[m]), 1.0)
    return float((np.abs(Ka[m] - Kb[m]) / size).max())


def state_diff(P, a, b):
    """bundle_ref.state_diff for poses and points, cam_diff for the cameras: the larger."""
    return max(br.state_diff(a[:3], b[:3]), cam_diff(P, a[3], b[3]))


def step_diff(a, b):
    """|a - b| / |b| of two steps ([nv, 6], [np, 3], [n_cameras, KMAX]), 2-norms over everything."""
    num = sum(((x - y) ** 2).sum() for x, y in zip(a, b))
    return float(np.sqrt(num / sum((y ** 2).sum() for y in b)))


def near_tie_radius(P, state):
    """bundle_ref.near_tie_radius with the cameras among the parameters (a camera parameter's radius relative to its size)."""
    H, _, _ = normal_equations(P, state, "analytic")
    r, _ = residuals(P, state)
    w = br.rho(P, (r * r).sum(1))[1]
    N = float((w[:, None] * np.abs(r) * np.spacing(np.abs(P.obs_xy))).sum())
    dv, dp, dk = split_step(P, np.sqrt(2 * N * np.diag(np.linalg.inv(H))))
    words = np.einsum("ck,cki->ci", dk, np.abs(P.dirs))
    size = np.where(state[3] != 0, np.abs(state[3]), 1.0)
    return max(dv[:, :3].max(initial=0.0), dv[:, 3:].max(initial=0.0) / SCALE, dp.max(initial=0.0) / SCALE, (words / size).max(initial=0.0))


# ------------------------------------------------------------------------------------------------------------------ the scenes
def with_cameras(P, start_cams, view_camera, refine, cam_truth=None):
    """A bundle_ref.Problem (its observations made with the true cameras) as a CamProblem that starts from start_cams."""
    return CamProblem(start_cams, view_camera, refine, P.q, P.t, P.X, P.vconst, P.pconst, P.off, P.obs_view, P.obs_xy, P.loss, P.loss_scale,
                      truth=P.truth, cam_truth=cam_truth)


def _cam(model, params):
    return {"model": model, "width": 640, "height": 480, "params": list(params)}


def _arc(n_views, n_points, true_cams, view_camera, seed, noise_px=0.5, vconst=(0, 1), loss="trivial", loss_scale=1.0, outlier_share=0.0, radius=2.5,
         tracks=None, rot_deg=1.0, trans=0.02 * SCALE, point_sigma=0.05):
    rs = np.random.RandomState(seed)
    _, R, t = br.arc_views(n_views)
    X = br._ball(rs, n_points, radius)
    vc = np.zeros(n_views, bool)
    vc[list(vconst)] = True
    tracks = [np.arange(n_views)] * n_points if tracks is None else tracks
    return br.build(seed + 1, [true_cams[c] for c in view_camera], R, t, X, tracks, vc, np.zeros(n_points, bool), noise_px, rot_deg, trans, point_sigma,
                    outlier_share, loss, loss_scale)


def shared_step_scene(refine):
    """8 arc views, 60 points, one shared SIMPLE_RADIAL camera (truth f 800, k -0.05; start f 830, c 4 px off, k 0)."""
    true = [_cam("SIMPLE_RADIAL", [800.0, 320.0, 240.0, -0.05])]
    vcam = np.zeros(8, np.int32)
    return with_cameras(_arc(8, 60, true, vcam, 101), [_cam("SIMPLE_RADIAL", [830.0, 324.0, 237.0, 0.0])], vcam, [refine], cam_truth=true)


def shared_focal_scene(loss="trivial", noise_px=0.5):
    """8 arc views, 60 points, two constant views, one shared SIMPLE_RADIAL camera: truth f 800, k -0.08, start f 960, k 0; focal and extra
    refined.  cauchy: 10 % gross outliers, scale 2 px."""
    true = [_cam("SIMPLE_RADIAL", [800.0, 320.0, 240.0, -0.08])]
    vcam = np.zeros(8, np.int32)
    kw = dict(loss="cauchy", loss_scale=2.0, outlier_share=0.1) if loss == "cauchy" else {}
    return with_cameras(_arc(8, 60, true, vcam, 103, noise_px=noise_px, **kw), [_cam("SIMPLE_RADIAL", [960.0, 320.0, 240.0, 0.0])], vcam, [FOCAL | EXTRA],
                        cam_truth=true)


def _off(cam, rs):
    """A camera's start values: focal lengths 3 % off, the principal point 3 px, the distortion coefficients by 0.01."""
    p = np.array(cam["params"], dtype=np.float64)
    k8 = np.array(pr._opencv(cam), dtype=np.float64)
    k8[:2] *= 1.03
    k8[2:4] += rs.uniform(-3, 3, 2)
    k8[4:] += np.where(k8[4:] != 0, 0.01, 0.0) * rs.choice([-1.0, 1.0], 4)
    if cam["model"].startswith("SIMPLE"):
        k8[1] = k8[0]
    return _cam(cam["model"], colmap_params(cam["model"], k8)[:len(p)])


def per_view_scene():
    """8 arc views of the four models in turn, a camera each, focal and extra refined; 80 points."""
    rs = np.random.RandomState(105)
    true = [pr.camera(br.MODELS[i % 4]) for i in range(8)]
    vcam = np.arange(8, dtype=np.int32)
    return with_cameras(_arc(8, 80, true, vcam, 105), [_off(c, rs) for c in true], vcam, [FOCAL | EXTRA] * 8, cam_truth=true)


def two_cameras_scene():
    """8 arc views, two OPENCV cameras on alternating views, all 8 parameters; camera 1 constant (at its true values)."""
    rs = np.random.RandomState(107)
    true = [_cam("OPENCV", [800.0, 790.0, 320.0, 240.0, -0.05, 0.01, 0.001, -0.001]), _cam("OPENCV", [700.0, 710.0, 310.0, 250.0, -0.03, 0.005, -0.001, 0.002])]
    vcam = (np.arange(8) % 2).astype(np.int32)
    return with_cameras(_arc(8, 100, true, vcam, 107), [_off(true[0], rs), true[1]], vcam, [7, 0], cam_truth=true)


SEAM_VIEWS = (255, 256, 257, 300)


def seam_views_scene(n_views):
    """n_views arc views that share one SIMPLE_RADIAL camera (focal and extra refined): 120 points observed 30 times each."""
    rs = np.random.RandomState(109 + n_views)
    true = [_cam("SIMPLE_RADIAL", [800.0, 320.0, 240.0, -0.05])]
    vcam = np.zeros(n_views, np.int32)
    tracks = [np.sort(rs.choice(n_views, 30, replace=False)).astype(np.int32) for _ in range(120)]
    P = _arc(n_views, 120, true, vcam, 111 + n_views, vconst=(0, n_views - 1), radius=2.0, tracks=tracks, rot_deg=0.3, trans=0.005 * SCALE, point_sigma=0.03)
    return with_cameras(P, [_cam("SIMPLE_RADIAL", [815.0, 320.0, 240.0, -0.04])], vcam, [FOCAL | EXTRA], cam_truth=true)


def busy_camera_scene():
    """bundle_ref.busy_view_scene's construction with cameras: the seven variable views (0, 1, 2, 255, 256, 257 and 1 000 observations) share
    SIMPLE_RADIAL camera 0 (focal and extra refined), the two constant views OPENCV camera 1 (focal refined), and no view uses camera 2."""
    rs = np.random.RandomState(13)
    true = [_cam("SIMPLE_RADIAL", [800.0, 320.0, 240.0, -0.05]), pr.camera("OPENCV"), pr.camera("PINHOLE")]
    vcam = np.array([0] * 7 + [1, 1], np.int32)
    _, R, t = br.arc_views(9)
    X = br._ball(rs, 1000, 2.5)
    sees = [set(rs.choice(1000, k, replace=False).tolist()) for k in br.VIEW_COUNTS]
    tracks = [np.array([7, 8] + [v for v in range(7) if p in sees[v]], dtype=np.int32) for p in range(1000)]
    vc = np.zeros(9, bool)
    vc[[7, 8]] = True
    pc = np.ones(1000, bool)
    pc[rs.choice(1000, 100, replace=False)] = False
    P = br.build(14, [true[c] for c in vcam], R, t, X, tracks, vc, pc, 0.5, 0.3, 0.005 * SCALE, 0.03)
    rs2 = np.random.RandomState(15)
    return with_cameras(P, [_cam("SIMPLE_RADIAL", [815.0, 320.0, 240.0, -0.04]), _off(true[1], rs2), true[2]], vcam, [FOCAL | EXTRA, FOCAL, 7], cam_truth=true)


def constant_cameras(name):
    """A scene of bundle_ref with one constant camera per view: what sfd2_bundle_adjust computes, through the new call."""
    P = br.scene(name)
    return with_cameras(P, P.cams, np.arange(P.nv, dtype=np.int32), [0] * P.nv)


def scene(name):
    makers = {"shared_step_focal": lambda: shared_step_scene(FOCAL), "shared_step_all": lambda: shared_step_scene(7),
              "shared_focal": shared_focal_scene, "shared_focal_cauchy": lambda: shared_focal_scene("cauchy"),
              "shared_focal_exact": lambda: shared_focal_scene(noise_px=0.0), "per_view": per_view_scene, "two_cameras_opencv": two_cameras_scene,
              "busy_camera": busy_camera_scene}
    makers.update({"seam_%d" % n: (lambda n=n: seam_views_scene(n)) for n in SEAM_VIEWS})
    return br.cached(("cam_scene", name), makers[name])


# the runs the scenes' references are computed for ({}: to convergence)
RUNS = {"shared_step_focal": dict(max_iterations=1), "shared_step_all": dict(max_iterations=1), "shared_focal": {}, "shared_focal_cauchy": {},
        "per_view": dict(max_iterations=2), "two_cameras_opencv": dict(max_iterations=2), "busy_camera": dict(max_iterations=2)}
RUNS.update({"seam_%d" % n: dict(max_iterations=2) for n in SEAM_VIEWS})


def solution(name, route=ROUTE_A):
    """lm() of a scene under RUNS, computed once per (scene, route) and left unchanged."""
    return br.cached(("cam_lm", name, route), lambda: lm(scene(name), route, **RUNS[name]))


DECISIVE = 1e-6                       # a decision is decisive when the trial cost is at least this far (relative) from the cost it is compared with


def decisive_prefix(name):
    """The leading accept / reject decisions of a scene's run that both routes take alike and far from a tie.  Near the minimum a decision
    compares two costs that agree to rounding, and the two routes themselves part ways there (on 'shared_focal' route A accepts 7 steps in
    30, route B 10 in 36): only this prefix is a property of the scene."""
    def make():
        out = []
        for (ca, ta, oka, _), (cb, tb, okb, _) in zip(solution(name, ROUTE_A)["history"], solution(name, ROUTE_B)["history"]):
            if oka != okb or not all(abs(t - c) > DECISIVE * c or not np.isfinite(t) for c, t in ((ca, ta), (cb, tb))):
                break
            out.append(bool(oka))
        return out
    return br.cached(("cam_prefix", name), make)


def disagreement(name):
    """The largest difference between the two routes' results on a scene (state_diff; for the one-step scenes also their steps')."""
    return br.cached(("cam_disagreement", name), lambda: state_diff(scene(name), solution(name, ROUTE_A)["state"], solution(name, ROUTE_B)["state"]))


def floor(name):
    """A scene's floor as bundle_ref.floor: the two routes' disagreement, and for a run to convergence the near-tie radius if larger."""
    def make():
        f = disagreement(name)
        if "max_iterations" not in RUNS[name]:
            f = max(f, near_tie_radius(scene(name), solution(name, ROUTE_B)["state"]))
        return f
    return br.cached(("cam_floor", name), make)


def tolerance(name):
    """10 x the scene's floor, ceiling 1e-6."""
    return min(10 * floor(name), 1e-6)
