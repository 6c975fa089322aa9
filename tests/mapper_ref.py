"""numpy fp64 helpers for the mapper tests only (never imported by the product): a plain restatement of the four device calls of
sfd2_amd.reconstruction (include/sfd2_hip.h: sfd2_mapper_restrict, sfd2_mapper_filter, sfd2_mapper_visible, sfd2_mapper_assemble)
exactly as they are specified, the filter a second time in another formulation (long double, angles by arctan2 of cross and dot
instead of arccos) so that it has a floor of its own, the scenes the GPU tests run them on, numpy stand-ins for every stage call of
reconstruct() so that its round logic runs without a GPU, and the alignment of a model to the truth.

The stand-ins are not restatements of the device stages: they are the simplest thing that lets a reconstruction succeed on
tri_ref.make_scene() (two-view results from the true poses, midpoint triangulation, an adjustment that only measures, a small DLT RANSAC
with a Gauss-Newton polish).  The four new calls are restated exactly and used as they are."""
import numpy as np

import bundle_ref as br
import pose_ref as pr
import tri_ref as tr

BAND = 1e-9                            # relative half-width of the band round either threshold of the filter
LONG = 64                              # beyond this many observations a point's mean is 64 strided partial sums joined by a tree
MAX_POINTS = 4


# ------------------------------------------------------------------------------------------------------------------ restrict
def restrict_ref(track_offsets, obs_view, obs_xy, registered):
    off, ov = np.asarray(track_offsets, np.int64), np.asarray(obs_view, np.int32)
    xy, reg = np.asarray(obs_xy, np.float32).reshape(-1, 2), np.asarray(registered).astype(bool)
    st, so, sb = [], [0], []
    for t in range(len(off) - 1):
        o = np.arange(off[t], off[t + 1])
        o = o[reg[ov[o]]]
        if len(set(ov[o].tolist())) < 2:
            continue
        st.append(t)
        sb.extend(o.tolist())
        so.append(len(sb))
    sb = np.array(sb, dtype=np.int32)
    return {"sub_track": np.array(st, dtype=np.int32), "sub_offsets": np.array(so, dtype=np.int64), "sub_obs": sb, "sub_view": ov[sb],
            "sub_xy": xy[sb].reshape(-1, 2)}


# ------------------------------------------------------------------------------------------------------------------ filter
def _views_arrays(views, n_views):
    """(K [n, 8], R [n, 3, 3], t [n, 3]) of a ctypes sfd2_tri_view array or of a list of (camera dict, qvec, tvec)."""
    K, R, t = [], [], []
    for i in range(n_views):
        v = views[i]
        if isinstance(v, tuple):
            cam, q, tv = v
            K.append(pr._opencv(cam))
        else:
            names = {0: "SIMPLE_PINHOLE", 1: "PINHOLE", 2: "SIMPLE_RADIAL", 4: "OPENCV"}
            n = {0: 3, 1: 4, 2: 4, 4: 8}[v.model]
            K.append(pr._opencv({"model": names[v.model], "params": list(v.params[:n])}))
            q, tv = np.array(v.qvec[:]), np.array(v.tvec[:])
        q = np.asarray(q, dtype=np.float64)
        R.append(pr.qvec2rotmat(q / np.linalg.norm(q)))
        t.append(np.asarray(tv, dtype=np.float64))
    return np.array(K, dtype=np.float64), np.array(R), np.array(t)


def _tree_sum(x, dtype):
    """64 strided partial sums in index order, joined by the tree p[l] += p[l + s], s = 32 .. 1."""
    p = np.zeros(64, dtype=dtype)
    for i, v in enumerate(x):
        p[i % 64] = p[i % 64] + v
    s = 32
    while s:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0]


def filter_ref(views, n_views, xyz, point_offsets, obs_view, obs_xy, max_reproj_error=4.0, min_tri_angle=1.5, mapping=None, second=False):
    """mapping: None (by length), 'lane' or 'wave' -- the order of the mean's sum.  second: the other formulation (long double, arctan2).
    Returns obs_keep, point_live, point_error, point_angle and, for the tests, 'obs_error', 'depth' and 'banded' (a point any of whose
    comparisons lies inside the band)."""
    ft = np.longdouble if second else np.float64
    K, R, t = _views_arrays(views, n_views)
    X, off = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(point_offsets, np.int64)
    ov, xy = np.asarray(obs_view, np.int32), np.asarray(obs_xy, np.float64).reshape(-1, 2)
    op = np.repeat(np.arange(len(X)), np.diff(off))
    Kf, Rf, tf, Xf = K.astype(ft)[ov], R.astype(ft)[ov], t.astype(ft)[ov], X.astype(ft)[op]
    Pc = (Rf * Xf[:, None, :]).sum(2) + tf
    with np.errstate(all="ignore"):
        u, v = Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2]
        r2 = u * u + v * v
        rad = Kf[:, 4] * r2 + Kf[:, 5] * r2 * r2
        ud = u + u * rad + 2 * Kf[:, 6] * u * v + Kf[:, 7] * (r2 + 2 * u * u)
        vd = v + v * rad + 2 * Kf[:, 7] * u * v + Kf[:, 6] * (r2 + 2 * v * v)
        dx, dy = Kf[:, 0] * ud + Kf[:, 2] - xy[:, 0].astype(ft), Kf[:, 1] * vd + Kf[:, 3] - xy[:, 1].astype(ft)
        e = np.hypot(dx, dy) if second else np.sqrt(dx * dx + dy * dy)
        keep = (Pc[:, 2] > 0) & (e <= max_reproj_error)
    C = -(np.transpose(Rf, (0, 2, 1)) * tf[:, None, :]).sum(2)
    ray = C - Xf
    near_e = np.abs(e - max_reproj_error) <= BAND * max_reproj_error
    P = len(X)
    live, perr, pang, banded = np.zeros(P, bool), np.zeros(P), np.full(P, np.nan), np.zeros(P, bool)
    for p in range(P):
        a, b = off[p], off[p + 1]
        k = np.flatnonzero(keep[a:b]) + a
        banded[p] = near_e[a:b].any()
        if len(k):
            wave = mapping == "wave" or (mapping is None and b - a > LONG)
            if wave:                                          # the strided partial sums run over all observations, the dropped ones adding nothing
                perr[p] = float(_tree_sum(np.where(keep[a:b], e[a:b], ft(0)), ft) / len(k))
            else:
                s = ft(0)
                for o in k:
                    s = s + e[o]
                perr[p] = float(s / len(k))
        if len(k) >= 2:
            r = ray[k]
            if second:
                cr = np.cross(r[:, None, :], r[None, :, :])
                ang = np.arctan2(np.sqrt((cr * cr).sum(2)), (r[:, None, :] * r[None, :, :]).sum(2))
                amax = ang[np.triu_indices(len(k), 1)].max()
            else:
                n = np.sqrt((r * r).sum(1))
                cos = (r @ r.T) / np.outer(n, n)
                amax = np.arccos(np.clip(cos[np.triu_indices(len(k), 1)].min(), -1.0, 1.0))
            deg = float(amax * (ft(180) / ft(np.pi) if second else 180.0 / np.pi))
            pang[p] = deg
            two = len(set(ov[k].tolist())) >= 2
            live[p] = two and deg >= min_tri_angle
            banded[p] |= abs(deg - min_tri_angle) <= BAND * min_tri_angle
    return {"obs_keep": keep, "point_live": live, "point_error": perr, "point_angle": pang, "obs_error": e.astype(np.float64),
            "depth": Pc[:, 2].astype(np.float64), "banded": banded}


def filter_floor(a, b):
    """The largest relative difference between two filter results' point_error and point_angle."""
    out = 0.0
    for k in ("point_error", "point_angle"):
        x, y = a[k], b[k]
        ok = np.isfinite(x) & np.isfinite(y) & (y != 0)
        assert (np.isfinite(x) == np.isfinite(y)).all(), k
        if ok.any():
            out = max(out, float((np.abs(x[ok] - y[ok]) / np.abs(y[ok])).max()))
    return out


# ------------------------------------------------------------------------------------------------------------------ visible / assemble
def track_live(n_tracks, point_track, point_live):
    return np.bincount(np.asarray(point_track, np.int64)[np.asarray(point_live).astype(bool)], minlength=n_tracks).astype(np.int64)


def visible_ref(track_offsets, obs_view, registered, point_track, point_live):
    off, ov, reg = np.asarray(track_offsets, np.int64), np.asarray(obs_view, np.int32), np.asarray(registered).astype(bool)
    per_obs = np.repeat(track_live(len(off) - 1, point_track, point_live), np.diff(off))
    counts = np.zeros(len(reg), np.int64)
    np.add.at(counts, ov, per_obs)
    counts[reg] = 0
    return counts


def assemble_ref(track_offsets, obs_view, obs_xy, n_views, point_track, point_live, xyz, cand, capacity=None):
    off, ov = np.asarray(track_offsets, np.int64), np.asarray(obs_view, np.int32)
    xy, X = np.asarray(obs_xy, np.float32).reshape(-1, 2), np.asarray(xyz, np.float64).reshape(-1, 3)
    pt, pl = np.asarray(point_track, np.int64), np.asarray(point_live).astype(bool)
    obs_track = np.repeat(np.arange(len(off) - 1), np.diff(off))
    offsets, p2, p3, so, sp = [0], [], [], [], []
    for v in cand:
        for o in np.flatnonzero(ov == v):
            for p in np.flatnonzero((pt == obs_track[o]) & pl):
                p2.append(xy[o].astype(np.float64) + 0.5)
                p3.append(X[p])
                so.append(o)
                sp.append(p)
        offsets.append(len(so))
    return {"offsets": np.array(offsets, np.int64), "points2D": np.array(p2, np.float64).reshape(-1, 2), "points3D": np.array(p3, np.float64).reshape(-1, 3),
            "src_obs": np.array(so, np.int32), "src_point": np.array(sp, np.int32)}


# ------------------------------------------------------------------------------------------------------------------ kernel-test scenes
def table_scene(name, seed=5):
    """A track table, registered sets, points and a filter problem from bundle_ref's 'long_tracks' (tracks of 2, 3, 63, 64, 65, 255, 256,
    257 and 300 observations) or 'busy_views' (views with 0, 1, 2, 255, 256, 257 and 1 000 observations) scene at the adjusted state
    (two LM steps of the restatement): the track table is the scene's point table, key points as float32 without the +0.5.  Points: track t
    carries t % 5 points (0 to 4), the first at the scene's adjusted position, the others displaced; every third point is dead.  One
    observation of track 5 is moved 60 px and point 12 is put behind its first camera (filter cases)."""
    def make():
        P = br.scene(name)
        s = br.solution(name, max_iterations=2)
        R, t, X = s["state"]
        rs = np.random.RandomState(seed)
        T = P.np_
        obs_xy32 = (P.obs_xy - 0.5).astype(np.float32)
        views = [(P.cams[i], pr.rotmat2qvec(R[i]), t[i]) for i in range(P.nv)]
        # filter problem: the scene's points and observations as the adjustment was given them (float32 key points + 0.5)
        fxy = obs_xy32.astype(np.float64) + 0.5
        fX = X.copy()
        fxy[P.off[5]] += [36.0, 48.0]                                               # 60 px off
        c0 = -R[P.obs_view[P.off[12]]].T @ t[P.obs_view[P.off[12]]]
        fX[12] = c0 - (fX[12] - c0)                                                   # mirrored through its first camera's centre: behind it
        # points per track for visible / assemble
        pt, px = [], []
        for tr_ in range(T):
            for k in range(tr_ % 5):
                pt.append(tr_)
                px.append(X[tr_] + (0.0 if k == 0 else rs.uniform(-0.5, 0.5, 3)))
        pt, px = np.array(pt, np.int32), np.array(px).reshape(-1, 3)
        live = (np.arange(len(pt)) % 3) != 2
        regs = {"none": np.zeros(P.nv, bool), "one": np.arange(P.nv) == min(3, P.nv - 1), "all": np.ones(P.nv, bool), "every_other": np.arange(P.nv) % 2 == 0}
        return dict(name=name, n_views=P.nv, off=P.off.copy(), obs_view=P.obs_view.copy(), obs_xy=obs_xy32, views=views, fxyz=fX, fxy=fxy,
                    point_track=pt, point_xyz=px, point_live=live, registered=regs)
    return br.cached(("mapper_table", name, seed), make)


def filter_refs(name):
    """The restatement of the filter on table_scene(name) for the three mappings: {None, 'lane', 'wave'} -> result."""
    def make():
        sc = table_scene(name)
        return {m: filter_ref(sc["views"], sc["n_views"], sc["fxyz"], sc["off"], sc["obs_view"], sc["fxy"], 4.0, 1.5, mapping=m) for m in (None, "lane", "wave")}
    return br.cached(("mapper_filter_ref", name), make)


def filter_second(name):
    def make():
        sc = table_scene(name)
        return filter_ref(sc["views"], sc["n_views"], sc["fxyz"], sc["off"], sc["obs_view"], sc["fxy"], 4.0, 1.5, second=True)
    return br.cached(("mapper_filter_second", name), make)


# ------------------------------------------------------------------------------------------------------------------ alignment
def umeyama(src, dst):
    """(s, R, t) of the similarity dst ~ s R src + t (least squares, Umeyama 1991)."""
    src, dst = np.asarray(src, float), np.asarray(dst, float)
    ms, md = src.mean(0), dst.mean(0)
    a, b = src - ms, dst - md
    U, D, Vt = np.linalg.svd(b.T @ a / len(src))
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    s = np.trace(np.diag(D) @ S) / (a * a).sum() * len(src)
    return s, R, md - s * R @ ms


def model_errors(images, points3D, truth_images):
    """A model against the true poses (matched by image name) after the similarity that best maps its camera centres onto the true ones:
    {'rotation' (largest, radians), 'centre' (largest, scene units), 'mean_reproj' (mean of the points' error), 'points', 'images'}."""
    by_name = {im.name: im for im in truth_images.values()}
    ims = [im for im in images.values()]
    C = np.array([pr.centre(np.asarray(im.qvec), np.asarray(im.tvec)) for im in ims])
    Ct = np.array([pr.centre(by_name[im.name].qvec, by_name[im.name].tvec) for im in ims])
    s, R, t = umeyama(C, Ct)
    rot = max(float(np.arccos(np.clip((np.trace(pr.qvec2rotmat(np.asarray(im.qvec)) @ R.T @ pr.qvec2rotmat(by_name[im.name].qvec).T) - 1) / 2, -1, 1)))
              for im in ims)
    cen = float(np.linalg.norm(s * C @ R.T + t - Ct, axis=1).max())
    err = float(np.mean([p.error for p in points3D.values()])) if points3D else float("nan")
    return {"rotation": rot, "centre": cen, "mean_reproj": err, "points": len(points3D), "images": len(images)}


# ------------------------------------------------------------------------------------------------------------------ stand-in stages
def _exp(w):
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx


class RefStages:
    """numpy stand-ins for DeviceStages on a tri_ref.make_scene() scene.  fail_views: view indices whose pose call always fails."""

    def __init__(self, scene, fail_views=()):
        self.scene = scene
        self.fail_views = set(fail_views)
        self.calls = {"absolute_pose": [], "two_view": 0}

    # two-view results from the true poses: the survivors of the known-pose verification, the true relative pose, the median angle at the
    # true points of the surviving true matches
    def two_view(self, cameras, images, keypoints, pair_matches, max_error, min_num_inliers, seed):
        sc = self.scene
        self.calls["two_view"] += 1
        truth = {iid: im for iid, im in sc["images"].items()}
        by_name = {im.name: iid for iid, im in truth.items()}
        tid = {i: by_name[images[i].name] for i in images if images[i].name in by_name}
        L = tr.Layout(sc["cameras"], truth, sc["keypoints"])
        pm = [(tid[a], tid[b], m) for a, b, m in pair_matches]
        m, off, counts, _, _ = tr.verify_ref(L, pm, max_error, min_num_inliers)
        results = []
        for p, (a, b, _) in enumerate(pm):
            Ra, Rb = pr.qvec2rotmat(truth[a].qvec), pr.qvec2rotmat(truth[b].qvec)
            R = Rb @ Ra.T
            t = truth[b].tvec - R @ truth[a].tvec
            rows = m[off[p]:off[p + 1]]
            rows = rows[rows[:, 0] >= 0]
            ga, gb = sc["kp_truth"][a][rows[:, 0]], sc["kp_truth"][b][rows[:, 1]]
            g = ga[(ga >= 0) & (ga == gb)]
            ang = float("nan")
            if len(g):
                ra, rb = pr.centre(truth[a].qvec, truth[a].tvec) - sc["X"][g], pr.centre(truth[b].qvec, truth[b].tvec) - sc["X"][g]
                ang = float(np.degrees(np.median(np.arctan2(np.linalg.norm(np.cross(ra, rb), axis=1), (ra * rb).sum(1)))))
            ok = counts[p] >= min_num_inliers and np.linalg.norm(t) > 0
            results.append({"success": bool(ok), "qvec": pr.rotmat2qvec(R), "tvec": t / max(np.linalg.norm(t), 1e-300), "num_inliers": int(counts[p]),
                            "tri_angle_deg": ang})
        return m, off, counts, results

    def build_tracks(self, n_nodes, edges, max_rounds):
        return tr.tracks_ref(n_nodes, edges)

    def restrict(self, track_offsets, obs_view, obs_xy, registered):
        return restrict_ref(track_offsets, obs_view, obs_xy, registered)

    # one point per track: the midpoint of all its rays, its observations those within the reprojection bound in front of the camera
    def triangulate(self, views, n_views, track_offsets, track_labels, obs_view, obs_xy, min_tri_angle, create_max_angle_error, filter_max_reproj_error,
                    seed, max_refine_iterations):
        K, R, t = _views_arrays(views, n_views)
        off, ov = np.asarray(track_offsets, np.int64), np.asarray(obs_view, np.int32)
        px = np.asarray(obs_xy, np.float32).astype(np.float64) + 0.5
        T = len(off) - 1
        xn = np.zeros((len(ov), 2))
        for v in np.unique(ov):
            cam = {"model": "OPENCV", "params": list(K[v])}
            xn[ov == v] = pr.undistort(cam, px[ov == v])
        d = np.einsum("nji,nj->ni", R[ov], np.concatenate([xn, np.ones((len(ov), 1))], 1))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        C = -np.einsum("nji,nj->ni", R[ov], t[ov])
        A = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
        xyz, err, n_obs = np.zeros((T, MAX_POINTS, 3)), np.zeros((T, MAX_POINTS)), np.zeros((T, MAX_POINTS), np.int32)
        obs_point = np.full(len(ov), -1, np.int8)
        for k in range(T):
            a, b = off[k], off[k + 1]
            M = A[a:b].sum(0)
            if b - a < 2 or np.linalg.cond(M) > 1e8:
                continue
            X = np.linalg.solve(M, np.einsum("nij,nj->i", A[a:b], C[a:b]))
            pxy, z = br.project_obs(K[ov[a:b]], R[ov[a:b]], t[ov[a:b]], np.repeat(X[None], b - a, 0))
            e = np.linalg.norm(pxy - px[a:b], axis=1)
            ok = (z > 0) & (e <= filter_max_reproj_error)
            if len(set(ov[a:b][ok].tolist())) < 2:
                continue
            xyz[k, 0], err[k, 0], n_obs[k, 0] = X, e[ok].mean(), ok.sum()
            obs_point[a:b][ok] = 0
        return {"xyz": xyz, "error": err, "n_obs": n_obs, "obs_point": obs_point, "status": np.zeros(T, np.int32)}

    # measures only: the points and the poses stay
    def adjust(self, views, n_views, view_constant, xyz, point_constant, point_offsets, obs_view, obs_xy, **kw):
        self.calls.setdefault("adjust", []).append(np.array(view_constant, dtype=bool))
        K, R, t = _views_arrays(views, n_views)
        X, ov = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(obs_view, np.int32)
        op = np.repeat(np.arange(len(X)), np.diff(point_offsets))
        pxy, _ = br.project_obs(K[ov], R[ov], t[ov], X[op]) if len(ov) else (np.zeros((0, 2)), None)
        err = np.linalg.norm(pxy - np.asarray(obs_xy).reshape(-1, 2), axis=1)
        return X.copy(), err, {"status": "stand_in", "iterations": 0, "options": dict(kw)}

    def filter(self, views, n_views, xyz, point_offsets, obs_view, obs_xy, max_reproj_error, min_tri_angle):
        return filter_ref(views, n_views, xyz, point_offsets, obs_view, obs_xy, max_reproj_error, min_tri_angle)

    def visible(self, track_offsets, obs_view, registered, point_track, point_live):
        return visible_ref(track_offsets, obs_view, registered, point_track, point_live)

    def assemble(self, track_offsets, obs_view, obs_xy, n_views, point_track, point_live, xyz, cand, capacity):
        out = assemble_ref(track_offsets, obs_view, obs_xy, n_views, point_track, point_live, xyz, cand)
        assert out["offsets"][-1] == capacity, (out["offsets"][-1], capacity)     # the caller sized the arrays from the visible counts
        return out

    # DLT on six correspondences inside a small RANSAC, then Gauss-Newton on the inliers
    def absolute_pose(self, problems, cand, max_error_px, min_inlier_ratio, seed):
        self.calls["absolute_pose"].append(list(cand))
        out = []
        for (p2, p3, cam), v in zip(problems, cand):
            n = len(p2)
            fail = {"success": False, "qvec": np.array([1.0, 0, 0, 0]), "tvec": np.zeros(3), "num_inliers": 0, "inliers": np.zeros(n, bool), "num_trials": 0}
            if v in self.fail_views or n < 6:
                out.append(fail)
                continue
            rs = np.random.RandomState((int(seed) + 7919 * int(v)) % (2 ** 31))
            xn = np.concatenate([pr.undistort(cam, p2), np.ones((n, 1))], 1)
            best, best_pose = -1, None
            for _ in range(60):
                pose_ = _dlt_pose(xn, p3, rs.choice(n, 6, replace=False))
                if pose_ is None:
                    continue
                e = pr.reproj_error(cam, pr.rotmat2qvec(pose_[0]), pose_[1], p2, p3)
                k = int((e <= max_error_px).sum())
                if k > best:
                    best, best_pose = k, pose_
            if best_pose is None:
                out.append(fail)
                continue
            R, t = best_pose
            for _ in range(6):
                inl = pr.reproj_error(cam, pr.rotmat2qvec(R), t, p2, p3) <= max_error_px
                if inl.sum() < 6:
                    break
                R, t = _gauss_newton(cam, R, t, p2[inl], p3[inl])
            inl = pr.reproj_error(cam, pr.rotmat2qvec(R), t, p2, p3) <= max_error_px
            out.append({"success": bool(inl.sum() >= 6), "qvec": pr.rotmat2qvec(R), "tvec": t, "num_inliers": int(inl.sum()), "inliers": inl, "num_trials": 60})
        return out


def _dlt_pose(xn, X, idx):
    """(R, t) from the correspondences idx by the direct linear transform on normalised image coordinates, or None."""
    rows = []
    for i in idx:
        Xh = np.append(X[i], 1.0)
        u, v = xn[i, 0], xn[i, 1]
        rows.append(np.concatenate([Xh, np.zeros(4), -u * Xh]))
        rows.append(np.concatenate([np.zeros(4), Xh, -v * Xh]))
    _, s, Vt = np.linalg.svd(np.array(rows))
    Pm = Vt[-1].reshape(3, 4)
    if np.linalg.det(Pm[:, :3]) < 0:
        Pm = -Pm
    U, D, Wt = np.linalg.svd(Pm[:, :3])
    if D.min() < 1e-12:
        return None
    R = U @ Wt
    if np.linalg.det(R) < 0:
        return None
    return R, Pm[:, 3] / D.mean()


def _gauss_newton(cam, R, t, p2, p3):
    def res(Rm, tv):
        px, _ = pr.project(cam, pr.rotmat2qvec(Rm), tv, p3)
        return (px - p2).reshape(-1)
    r0 = res(R, t)
    J = np.zeros((len(r0), 6))
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        J[:, k] = (res(_exp(d[:3]) @ R, t + d[3:]) - r0) / h
    step = np.linalg.lstsq(J, -r0, rcond=None)[0]
    return _exp(step[:3]) @ R, t + step[3:]
