"""numpy fp64 helpers for the SfM map tests only (never imported by the product): a synthetic scene generator and a plain restatement
of the three device stages of sfd2_amd.triangulation (include/sfd2_hip.h: sfd2_verify_matches_batch, sfd2_build_tracks,
sfd2_triangulate_tracks) exactly as they are specified, with the camera helpers of tests/pose_ref.py.

The restatement also says which of its decisions were close: a comparison whose value lies within +-1 % of its threshold (BAND)
is `banded`.  For the verification that is per match; for the triangulation a track is banded when a banded comparison could have
changed its result (an observation's error against a threshold for the winning pose, a hypothesis whose support could reach the
winner's once its banded comparisons flip, a triangulation angle at its bound)."""
import numpy as np

import pose_ref as pr

BAND = 0.01
MODELS = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "OPENCV"]
DEFAULTS = dict(max_error=4.0, min_num_inliers=15, min_tri_angle=1.5, create_max_angle_error=2.0, filter_max_reproj_error=4.0, seed=0)
MAX_POINTS, HYPS = 4, 64
M64 = (1 << 64) - 1


class Cam(dict):
    """A camera both ways: the mapping sfd2_amd.pose takes and the attributes of a COLMAP record."""

    def __getattr__(self, k):
        return self[k]


class Img:
    def __init__(self, id, qvec, tvec, camera_id, name, xys=None, point3D_ids=None):
        self.id, self.qvec, self.tvec, self.camera_id, self.name = id, np.asarray(qvec, float), np.asarray(tvec, float), camera_id, name
        self.xys = np.zeros((0, 2)) if xys is None else xys
        self.point3D_ids = np.zeros(0, np.int64) if point3D_ids is None else point3D_ids


def _near(x, thr):
    return abs(x - thr) <= BAND * thr


def _look_at(centre, target, roll):
    z = target - centre
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])                                   # world -> camera
    c, s = np.cos(roll), np.sin(roll)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ R
    return pr.rotmat2qvec(R), -R @ centre


# ------------------------------------------------------------------------------------------------------------------ the scene
def make_scene(seed=0, n_images=12, n_points=900, n_clutter=100, window=4, p_visible=0.8, p_match=0.9, false_share=0.1, n_joiners=12,
               n_weak_pairs=3, noise_px=1.0, n_queries=0, spacing=1.0, depth=(5.0, 20.0)):
    """Cameras of the four models on a trajectory along x looking at a slab of points `depth` units away; per image a key-point table
    (noisy projections of the visible points plus clutter, shuffled; stored as float32 WITHOUT the +0.5, as a feature store holds them);
    pairs inside a window with matches: true ones, a share of random false ones, `n_joiners` false ones that join two true points
    (the second point sits on the first image's ray of the first, so the match satisfies the epipolar geometry), and `n_weak_pairs`
    pairs thinned below 15 true matches.  n_queries held-out cameras between the others with their own observations.
    Returns a dict (see the keys at the end)."""
    rs = np.random.RandomState(seed)
    cameras = {m + 1: Cam(id=m + 1, **pr.camera(MODELS[m])) for m in range(4)}
    span = spacing * (n_images - 1)
    images, centres = {}, {}
    for i in range(n_images):
        c = np.array([spacing * i, 0.3 * np.sin(0.9 * i), 0.2 * np.cos(0.7 * i)])
        q, t = _look_at(c, np.array([spacing * i + rs.uniform(-0.5, 0.5), rs.uniform(-0.3, 0.3), 14.0]), rs.uniform(-0.05, 0.05))
        images[i + 1] = Img(i + 1, q, t, i % 4 + 1, f"db/img{i:03d}.jpg")
        centres[i + 1] = c
    X = np.stack([rs.uniform(-3, span + 3, n_points), rs.uniform(-3.5, 3.5, n_points), rs.uniform(depth[0], depth[1], n_points)], 1)
    # joiners: point B on the ray from image i's centre through point A
    joiners = []
    for k in range(n_joiners):
        a = int(rs.randint(n_points))
        i = int(np.clip(round(X[a, 0] / spacing) + rs.randint(-1, 2), 0, n_images - 2)) + 1
        b = len(X)
        X = np.concatenate([X, (centres[i] + 1.25 * (X[a] - centres[i]))[None]])
        joiners.append((i, a, b))
    hidden = {(i, b) for i, a, b in joiners}                  # B is behind A in image i
    keypoints, kp_truth = {}, {}
    for iid, im in images.items():
        cam = cameras[im.camera_id]
        px, z = pr.project(cam, im.qvec, im.tvec, X)
        vis = (z > 0) & (px[:, 0] > 5) & (px[:, 0] < cam["width"] - 5) & (px[:, 1] > 5) & (px[:, 1] < cam["height"] - 5)
        vis &= rs.uniform(size=len(X)) < p_visible
        for (i, b) in hidden:
            if i == iid:
                vis[b] = False
        for (i, a, b) in joiners:
            if i == iid:
                vis[a] = (z[a] > 0) and 5 < px[a, 0] < cam["width"] - 5 and 5 < px[a, 1] < cam["height"] - 5
        idx = np.nonzero(vis)[0]
        pts = px[idx] + noise_px * rs.standard_normal((len(idx), 2))
        clutter = np.stack([rs.uniform(0, cam["width"], n_clutter), rs.uniform(0, cam["height"], n_clutter)], 1)
        allp = np.concatenate([pts, clutter])
        truth = np.concatenate([idx, np.full(n_clutter, -1)])
        perm = rs.permutation(len(allp))
        keypoints[iid] = (allp[perm] - 0.5).astype(np.float32)
        kp_truth[iid] = truth[perm]
    ids = sorted(images)
    pairs = [(ids[a], ids[b]) for a in range(len(ids)) for b in range(a + 1, min(a + 1 + window, len(ids)))]
    weak = set(rs.choice(len(pairs), min(n_weak_pairs, len(pairs)), replace=False).tolist())
    pair_matches, match_truth = [], []
    for p, (i0, i1) in enumerate(pairs):
        t0, t1 = kp_truth[i0], kp_truth[i1]
        where1 = {int(g): k for k, g in enumerate(t1) if g >= 0}
        rows, truth = [], []
        for k0, g in enumerate(t0):
            if g >= 0 and int(g) in where1 and rs.uniform() < p_match:
                rows.append((k0, where1[int(g)]))
                truth.append(True)
        if p in weak:
            keep = rs.choice(len(rows), min(8, len(rows)), replace=False)
            rows, truth = [rows[k] for k in keep], [True] * len(keep)
        used0, used1 = {r[0] for r in rows}, {r[1] for r in rows}
        for (i, a, b) in joiners:                             # A in image i against B in the other image
            if i == i0 and p not in weak:
                k0, k1 = np.nonzero(t0 == a)[0], np.nonzero(t1 == b)[0]
                if len(k0) and len(k1) and int(k0[0]) not in used0 and int(k1[0]) not in used1:
                    rows.append((int(k0[0]), int(k1[0])))
                    truth.append(False)
                    used0.add(int(k0[0]))
                    used1.add(int(k1[0]))
        n_false = int(round(false_share * len(rows)))
        for _ in range(n_false):
            k0, k1 = int(rs.randint(len(t0))), int(rs.randint(len(t1)))
            if k0 in used0 or k1 in used1 or (t0[k0] >= 0 and t0[k0] == t1[k1]):
                continue
            rows.append((k0, k1))
            truth.append(False)
            used0.add(k0)
            used1.add(k1)
        order = np.argsort([r[0] for r in rows], kind="stable")
        pair_matches.append((i0, i1, np.array(rows, dtype=np.int32).reshape(-1, 2)[order]))
        match_truth.append(np.array(truth, dtype=bool)[order])
    queries = []
    for k in range(n_queries):
        c = np.array([spacing * (k + 0.5) * (n_images - 1) / max(n_queries, 1), rs.uniform(-0.4, 0.4), rs.uniform(-0.4, 0.4)])
        q, t = _look_at(c, np.array([c[0] + rs.uniform(-0.5, 0.5), rs.uniform(-0.3, 0.3), 14.0]), rs.uniform(-0.05, 0.05))
        cam = cameras[k % 4 + 1]
        px, z = pr.project(cam, q, t, X[:n_points])
        vis = np.nonzero((z > 0) & (px[:, 0] > 5) & (px[:, 0] < cam["width"] - 5) & (px[:, 1] > 5) & (px[:, 1] < cam["height"] - 5))[0]
        queries.append({"qvec": q, "tvec": t, "camera": cam, "point_idx": vis, "xy": px[vis] + noise_px * rs.standard_normal((len(vis), 2))})
    return {"cameras": cameras, "images": images, "keypoints": keypoints, "kp_truth": kp_truth, "pairs": pairs, "pair_matches": pair_matches,
            "match_truth": match_truth, "X": X, "n_points": n_points, "joiners": joiners, "weak_pairs": sorted(weak), "queries": queries}


# ------------------------------------------------------------------------------------------------------------------ shared layout
class Layout:
    """Views in ascending image id, the key-point table concatenated in that order, every key point normalised through its camera."""

    def __init__(self, cameras, images, keypoints):
        self.ids = sorted(images)
        self.index = {iid: k for k, iid in enumerate(self.ids)}
        self.cams = [cameras[images[i].camera_id] for i in self.ids]
        self.R = [pr.qvec2rotmat(np.asarray(images[i].qvec, float) / np.linalg.norm(images[i].qvec)) for i in self.ids]
        self.t = [np.asarray(images[i].tvec, float) for i in self.ids]
        self.C = [-R.T @ t for R, t in zip(self.R, self.t)]
        self.kp = [np.asarray(keypoints[i], dtype=np.float32).reshape(-1, 2) for i in self.ids]
        self.off = np.concatenate([[0], np.cumsum([len(k) for k in self.kp])]).astype(np.int64)
        self.px = np.concatenate([k.astype(np.float64) + 0.5 for k in self.kp])
        self.xn = np.concatenate([pr.undistort(c, k.astype(np.float64) + 0.5) if len(k) else np.zeros((0, 2)) for c, k in zip(self.cams, self.kp)])
        self.node_view = np.repeat(np.arange(len(self.ids)), np.diff(self.off))


# ------------------------------------------------------------------------------------------------------------------ (a) verification
def verify_ref(L, pair_matches, max_error=DEFAULTS["max_error"], min_num_inliers=DEFAULTS["min_num_inliers"]):
    """Returns (matches [M, 2] with the rejected rows (-1, -1), offsets, counts, banded bool [M], keep_sure bool [n_pairs] or None where a
    banded match decides the pair)."""
    out, counts, banded, sure, off = [], [], [], [], [0]
    for i0, i1, m in pair_matches:
        a, b = L.index[i0], L.index[i1]
        R = L.R[b] @ L.R[a].T
        t = L.t[b] - R @ L.t[a]
        E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
        m = np.asarray(m).reshape(-1, 2)
        xi = np.concatenate([L.xn[L.off[a] + m[:, 0]], np.ones((len(m), 1))], 1)
        xj = np.concatenate([L.xn[L.off[b] + m[:, 1]], np.ones((len(m), 1))], 1)
        lj, li = xi @ E.T, xj @ E
        with np.errstate(invalid="ignore", divide="ignore"):
            dj = np.abs((xj * lj).sum(1)) / np.hypot(lj[:, 0], lj[:, 1])
            di = np.abs((xi * li).sum(1)) / np.hypot(li[:, 0], li[:, 1])
        ti, tj = max_error / pr.mean_focal(L.cams[a]), max_error / pr.mean_focal(L.cams[b])
        ok = (di <= ti) & (dj <= tj)
        near = (np.abs(di - ti) <= BAND * ti) | (np.abs(dj - tj) <= BAND * tj)
        n_sure, n_max = int((ok & ~near).sum()), int((ok | near).sum())
        sure.append(True if n_sure >= min_num_inliers else (False if n_max < min_num_inliers else None))
        o = np.where(ok[:, None], m, -1).astype(np.int32)
        counts.append(int(ok.sum()))
        if counts[-1] < min_num_inliers:
            o[:] = -1
        out.append(o)
        banded.append(near)
        off.append(off[-1] + len(m))
    cat = (lambda xs, d: np.concatenate(xs) if xs else np.zeros((0,) + d))
    return cat(out, (2,)).astype(np.int32), np.array(off, np.int64), np.array(counts, np.int32), cat(banded, ()).astype(bool), sure


def edges_of(L, pair_matches, matches, offsets):
    rows = []
    for p, (i0, i1, _) in enumerate(pair_matches):
        m = matches[offsets[p]:offsets[p + 1]]
        m = m[(m[:, 0] >= 0) & (m[:, 1] >= 0)]
        rows.append(np.stack([L.off[L.index[i0]] + m[:, 0], L.off[L.index[i1]] + m[:, 1]], 1))
    return np.concatenate(rows).astype(np.int64) if rows else np.zeros((0, 2), np.int64)


# ------------------------------------------------------------------------------------------------------------------ (b) tracks
def tracks_ref(n_nodes, edges):
    """labels[v] = smallest node of v's component; the components of >= 2 nodes as a CSR by label, nodes ascending."""
    parent = np.arange(n_nodes, dtype=np.int64)

    def find(v):
        r = v
        while parent[r] != r:
            r = parent[r]
        while parent[v] != r:
            parent[v], v = r, parent[v]
        return r

    for u, v in np.asarray(edges).reshape(-1, 2):
        if u < 0 or v < 0:
            continue
        ru, rv = find(int(u)), find(int(v))
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    labels = np.array([find(v) for v in range(n_nodes)], dtype=np.int32)
    order = np.argsort(labels, kind="stable")
    sl = labels[order]
    size = np.bincount(labels, minlength=n_nodes)[sl] if n_nodes else np.zeros(0, int)
    keep = size >= 2
    nodes = order[keep].astype(np.int32)
    kl = sl[keep]
    heads = np.nonzero(np.concatenate([[True], kl[1:] != kl[:-1]]))[0] if len(kl) else np.zeros(0, int)
    return labels, np.concatenate([heads, [len(nodes)]]).astype(np.int32), nodes


# ------------------------------------------------------------------------------------------------------------------ (c) triangulation
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class _Track:
    def __init__(self, L, nodes):
        self.L = L
        self.view = L.node_view[nodes]
        self.px, self.xn = L.px[nodes], L.xn[nodes]
        self.n = len(nodes)
        self.point = np.full(self.n, -1, dtype=np.int8)

    def cam_pts(self, o, X):
        v = self.view[o]
        return X @ self.L.R[v].T + self.L.t[v]                # X: [..., 3]

    def err_angle(self, o, X):
        """(tan of the angular error, in front) for X [k, 3] or [3]."""
        Pc = self.cam_pts(o, X)
        b = np.array([self.xn[o, 0], self.xn[o, 1], 1.0])
        cr = np.cross(Pc, b)
        dot = Pc @ b
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.sqrt((cr * cr).sum(-1)) / dot
        return e, (Pc[..., 2] > 0) & (dot > 0)

    def err_pixel(self, o, X):
        Pc = self.cam_pts(o, X)
        cam = self.L.cams[self.view[o]]
        with np.errstate(invalid="ignore", divide="ignore"):
            ud, vd = pr.distort(cam, Pc[..., 0] / Pc[..., 2], Pc[..., 1] / Pc[..., 2])
        fx, fy, cx, cy = pr._opencv(cam)[:4]
        return np.hypot(fx * ud + cx - self.px[o, 0], fy * vd + cy - self.px[o, 1]), Pc[..., 2] > 0

    def residuals(self, members, X):
        r = []
        for o in members:
            Pc = self.cam_pts(o, X)
            cam = self.L.cams[self.view[o]]
            ud, vd = pr.distort(cam, Pc[0] / Pc[2], Pc[1] / Pc[2])
            fx, fy, cx, cy = pr._opencv(cam)[:4]
            r += [fx * ud + cx - self.px[o, 0], fy * vd + cy - self.px[o, 1]]
        return np.array(r)

    def select(self, p, X, pixel, thr):
        """Free observations within thr join point p: one per image, none for an image p holds; smallest error, then smallest index.
        Returns (joined, any comparison banded)."""
        cand, near = {}, False
        held = {self.view[o] for o in range(self.n) if self.point[o] == p}
        for o in range(self.n):
            if self.point[o] != -1:
                continue
            e, front = (self.err_pixel if pixel else self.err_angle)(o, X)
            if front and _near(float(e), thr) and self.view[o] not in held:
                near = True
            if front and e <= thr and self.view[o] not in held:
                v = self.view[o]
                if v not in cand or e < cand[v][0]:
                    cand[v] = (float(e), o)
        for e, o in cand.values():
            self.point[o] = p
        return len(cand), near

    def refine(self, p, X, iters=200):
        """Gauss-Newton / Levenberg-Marquardt to convergence on the squared reprojection error of point p's observations."""
        members = [o for o in range(self.n) if self.point[o] == p]
        X = X.copy()
        lam = 1e-3
        r = self.residuals(members, X)
        for _ in range(iters):
            J = np.zeros((len(r), 3))
            for k in range(3):
                h = 1e-6 * max(1.0, abs(X[k]))
                d = np.zeros(3)
                d[k] = h
                J[:, k] = (self.residuals(members, X + d) - self.residuals(members, X - d)) / (2 * h)
            H, g = J.T @ J, J.T @ r
            step = None
            for _ in range(30):
                try:
                    d = -np.linalg.solve(H + lam * np.diag(np.diag(H)), g)
                except np.linalg.LinAlgError:
                    lam *= 10
                    continue
                rn = self.residuals(members, X + d)
                if np.isfinite(rn).all() and rn @ rn <= r @ r:
                    step = d
                    X, r, lam = X + d, rn, max(lam * 0.1, 1e-15)
                    break
                lam *= 10
            if step is None or step @ step <= 1e-28 * (X @ X):
                break
        return X


def _hypothesis(T, L, oa, ob, cos_min):
    """(X, valid, banded) of the midpoint of the two observations' rays."""
    va, vb = T.view[oa], T.view[ob]
    if va == vb:
        return np.zeros(3), False, False
    da = L.R[va].T @ np.array([T.xn[oa, 0], T.xn[oa, 1], 1.0])
    db = L.R[vb].T @ np.array([T.xn[ob, 0], T.xn[ob, 1], 1.0])
    w = L.C[va] - L.C[vb]
    aa, ab, bb, aw, bw = da @ da, da @ db, db @ db, da @ w, db @ w
    den = aa * bb - ab * ab
    if not den > 0:
        return np.zeros(3), False, False
    sa, sb = (ab * bw - bb * aw) / den, (aa * bw - ab * aw) / den
    X = 0.5 * ((L.C[va] + sa * da) + (L.C[vb] + sb * db))
    if not np.isfinite(X).all():
        return X, False, False
    front = (L.R[va] @ X + L.t[va])[2] > 0 and (L.R[vb] @ X + L.t[vb])[2] > 0
    ra, rb = L.C[va] - X, L.C[vb] - X
    cs = abs(ra @ rb) / np.sqrt((ra @ ra) * (rb @ rb))
    ang, thr = np.degrees(np.arccos(min(1.0, cs))), np.degrees(np.arccos(cos_min))
    return X, bool(front and cs <= cos_min), bool(front and _near(ang, thr))


def triangulate_ref(L, track_offsets, track_nodes, min_tri_angle=DEFAULTS["min_tri_angle"], create_max_angle_error=DEFAULTS["create_max_angle_error"],
                    filter_max_reproj_error=DEFAULTS["filter_max_reproj_error"], seed=DEFAULTS["seed"]):
    """Returns {'xyz' [T, 4, 3], 'error' [T, 4], 'n_obs' [T, 4], 'obs_point' int8 [O], 'banded' bool [T]}."""
    Tn = len(track_offsets) - 1
    out = {"xyz": np.zeros((Tn, MAX_POINTS, 3)), "error": np.zeros((Tn, MAX_POINTS)), "n_obs": np.zeros((Tn, MAX_POINTS), np.int32),
           "obs_point": np.full(len(track_nodes), -1, np.int8), "banded": np.zeros(Tn, bool)}
    tan_create, cos_min = np.tan(np.radians(create_max_angle_error)), np.cos(np.radians(min_tri_angle))
    for t in range(Tn):
        lo, hi = int(track_offsets[t]), int(track_offsets[t + 1])
        T = _Track(L, np.asarray(track_nodes[lo:hi], dtype=np.int64))
        key = mix64((seed & M64) ^ mix64(int(track_nodes[lo])))
        banded = False
        for p in range(MAX_POINTS):
            free = [o for o in range(T.n) if T.point[o] == -1]
            m = len(free)
            if m < 2:
                break
            if m * (m - 1) // 2 <= HYPS:
                lanes = [(a, b) for a in range(m) for b in range(a + 1, m)]
            else:
                lanes = []
                for h in range(HYPS):
                    h0 = mix64(key ^ mix64(HYPS * p + h))
                    h1 = mix64(h0)
                    i0, i1 = h0 % m, h1 % (m - 1)
                    if i1 >= i0:
                        i1 += 1
                    lanes.append((min(i0, i1), max(i0, i1)))
            best, cands = None, []                            # best = (-count, sum, lane) smallest; cands for the banding rule
            for lane, (a, b) in enumerate(lanes):
                X, valid, vnear = _hypothesis(T, L, free[a], free[b], cos_min)
                if not (valid or vnear):
                    continue
                cnt, s, k, cur, have, bst = 0, 0.0, 0, -1, False, 0.0
                for o in free:
                    if T.view[o] != cur:
                        if have:
                            cnt, s = cnt + 1, s + bst
                        have, cur = False, T.view[o]
                    e, front = T.err_angle(o, X)
                    if front and _near(float(e), tan_create):
                        k += 1
                    if front and e <= tan_create and (not have or e < bst):
                        bst, have = float(e), True
                if have:
                    cnt, s = cnt + 1, s + bst
                cands.append((-1 if vnear else cnt - k, cnt + k, k > 0 or vnear))
                if valid and (best is None or (-cnt, s, lane) < best[0]):
                    best = ((-cnt, s, lane), X)
            floor = max([c[0] for c in cands] + [2])
            if any(c[2] and c[1] >= floor for c in cands):
                banded = True
            if best is None or -best[0][0] < 2:
                break
            X = best[1]
            _, near = T.select(p, X, False, tan_create)
            X = T.refine(p, X)
            joined, near2 = T.select(p, X, True, filter_max_reproj_error)
            if joined:
                X = T.refine(p, X)
            members, esum = [], 0.0
            for o in range(T.n):
                if T.point[o] != p:
                    continue
                e, front = T.err_pixel(o, X)
                if front and _near(float(e), filter_max_reproj_error):
                    banded = True
                if front and e <= filter_max_reproj_error:
                    members.append(o)
                    esum += float(e)
                else:
                    T.point[o] = -1
            banded = banded or near or near2
            mc = 2.0
            for x, o in enumerate(members):
                for q in members[x + 1:]:
                    ra, rb = L.C[T.view[o]] - X, L.C[T.view[q]] - X
                    mc = min(mc, abs(ra @ rb) / np.sqrt((ra @ ra) * (rb @ rb)))
            if len(members) >= 2 and _near(np.degrees(np.arccos(min(1.0, mc))), min_tri_angle):
                banded = True
            if not np.isfinite(X).all() or len(members) < 2 or not mc <= cos_min:
                T.point[T.point == p] = -1
                break
            out["xyz"][t, p], out["error"][t, p], out["n_obs"][t, p] = X, esum / len(members), len(members)
        out["obs_point"][lo:hi] = T.point
        out["banded"][t] = banded
    return out


# ------------------------------------------------------------------------------------------------------------------ against ground truth
def truth_figures(scene, L, track_offsets, track_nodes, tri):
    """(share of the true points seen in >= 3 images that some output point recovers with >= 3 of their observations, share of the
    output points whose observations mix two true points, median |xyz - truth| / depth over the unmixed points)."""
    truth = np.concatenate([scene["kp_truth"][i] for i in L.ids])
    seen = np.zeros(len(scene["X"]), int)
    for i in L.ids:
        g = scene["kp_truth"][i]
        np.add.at(seen, g[g >= 0], 1)
    want = set(np.nonzero(seen >= 3)[0].tolist())
    got, mixed, n_out, errs = set(), 0, 0, []
    for t in range(len(track_offsets) - 1):
        lo, hi = int(track_offsets[t]), int(track_offsets[t + 1])
        for p in range(MAX_POINTS):
            if tri["n_obs"][t, p] == 0:
                continue
            n_out += 1
            nodes = track_nodes[lo:hi][tri["obs_point"][lo:hi] == p]
            g = truth[nodes]
            kinds = set(g[g >= 0].tolist())
            if len(kinds) > 1 or (g < 0).any():
                mixed += 1
                continue
            if not kinds:
                continue
            k = kinds.pop()
            if len(nodes) >= 3:
                got.add(k)
            v = L.node_view[nodes[0]]
            depth = (L.R[v] @ scene["X"][k] + L.t[v])[2]
            errs.append(np.linalg.norm(tri["xyz"][t, p] - scene["X"][k]) / depth)
    return len(got & want) / max(len(want), 1), mixed / max(n_out, 1), float(np.median(errs)) if errs else np.inf
