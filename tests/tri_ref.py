"""numpy fp64 helpers for the SfM map tests only (never imported by the product): a synthetic scene generator and a plain restatement
of the three device stages of sfd2_amd.triangulation (include/sfd2_hip.h: sfd2_verify_matches_batch, sfd2_build_tracks,
sfd2_triangulate_tracks) exactly as they are specified, with the camera helpers of tests/pose_ref.py.

The restatement also says which of its decisions were close: a comparison whose value lies within +-1 % of its threshold (BAND)
is `banded`.  For the verification that is per match; for the triangulation a track is banded when a banded comparison could have
changed its result (an observation's error against a threshold for the winning pose, a hypothesis whose support could reach the
winner's once its banded comparisons flip, a triangulation angle at its bound)."""
import functools

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


# ------------------------------------------------------------------------------------------------------------------ designed tracks
ARC_TARGET = np.array([0.0, 0.0, 10.0])
# (true points merged into the track, every stride-th image): 36 images give 12 to 181 observations per track
TRACKS_36 = ((1, 1), (1, 1), (1, 2), (1, 3), (2, 2), (3, 2), (2, 3), (2, 1), (3, 1), (4, 1), (5, 1), (4, 1), (5, 1))
TRACKS_80 = ((1, 1), (1, 1), (1, 1), (2, 1), (2, 1), (2, 1))


def arc_cameras(n_images, radius=10.0, arc_deg=90.0):
    """Cameras of the four models in turn on an arc in the x-z plane around ARC_TARGET (`radius` units away), all looking at it."""
    cameras = {m + 1: Cam(id=m + 1, **pr.camera(MODELS[m])) for m in range(4)}
    images = {}
    for i in range(n_images):
        th = np.radians(arc_deg) * (i / max(n_images - 1, 1) - 0.5)
        c = ARC_TARGET + radius * np.array([np.sin(th), 0.03 * np.sin(1.3 * i), -np.cos(th)])
        q, t = _look_at(c, ARC_TARGET.copy(), 0.04 * np.sin(0.8 * i))
        images[i + 1] = Img(i + 1, q, t, i % 4 + 1, f"arc/img{i:03d}.jpg")
    return cameras, images


def make_track_scene(seed=0, n_images=36, tracks=TRACKS_36, noise_px=0.15, n_outliers=3, outlier_px=60.0, gap=0.9):
    """Tracks for sfd2_triangulate_tracks directly, without verification.  Track t merges k true points and is seen in every
    stride-th image of arc_cameras(n_images), so it holds k observations per image: the points sit `gap` units apart in y, across the
    camera motion (more than 2 degrees apart from every view, so no observation of one supports another); every observation is the
    projection plus noise_px of Gaussian noise, and n_outliers more per track lie further than outlier_px from every true projection
    of their track in their image.  The key-point tables hold the observations image by image, so a track's nodes ascend and its
    label is its first node, as sfd2_build_tracks gives them.
    Returns {'cameras', 'images', 'keypoints', 'L', 't_off', 't_nodes', 'k' [T], 'X' (per track [k, 3]), 'truth' [O]: the true point
    of an observation or -1}."""
    rs = np.random.RandomState(seed)
    cameras, images = arc_cameras(n_images)
    ids = sorted(images)
    per_image = {i: [] for i in ids}                          # (track, true point or -1, pixel)
    Xs = []
    for t, (k, stride) in enumerate(tracks):
        base = ARC_TARGET + np.array([rs.uniform(-1.2, 1.2), rs.uniform(-0.5, 0.5), rs.uniform(-1.2, 1.2)])
        X = np.stack([base + np.array([rs.uniform(-0.3, 0.3), gap * (j - 0.5 * (k - 1)), rs.uniform(-0.3, 0.3)]) for j in range(k)])
        Xs.append(X)
        seen = ids[(t % stride)::stride]
        proj = {}
        for i in seen:
            px, z = pr.project(cameras[images[i].camera_id], images[i].qvec, images[i].tvec, X)
            assert (z > 0).all() and (px > 8).all() and (px[:, 0] < 632).all() and (px[:, 1] < 472).all(), (t, i)
            proj[i] = px
            for j in range(k):
                per_image[i].append((t, j, px[j] + noise_px * rs.standard_normal(2)))
        for _ in range(n_outliers):
            i = seen[int(rs.randint(len(seen)))]
            while True:
                p = np.array([rs.uniform(8, 632), rs.uniform(8, 472)])
                if np.linalg.norm(proj[i] - p, axis=1).min() > outlier_px:
                    break
            rows = [r for r, e in enumerate(per_image[i]) if e[0] == t]
            per_image[i].insert(rows[int(rs.randint(len(rows)))], (t, -1, p))   # somewhere inside the track's run of that image
    keypoints = {i: (np.array([e[2] for e in per_image[i]]).reshape(-1, 2) - 0.5).astype(np.float32) for i in ids}
    L = Layout(cameras, images, keypoints)
    nodes = [[] for _ in tracks]
    truth = [[] for _ in tracks]
    for v, i in enumerate(ids):
        for r, (t, j, _) in enumerate(per_image[i]):
            nodes[t].append(int(L.off[v]) + r)
            truth[t].append(j)
    t_off = np.concatenate([[0], np.cumsum([len(n) for n in nodes])]).astype(np.int64)
    return {"cameras": cameras, "images": images, "keypoints": keypoints, "L": L, "t_off": t_off, "t_nodes": np.concatenate(nodes).astype(np.int32),
            "k": np.array([k for k, _ in tracks]), "X": Xs, "truth": np.concatenate(truth)}


def sub_tracks(t_off, t_nodes, which):
    """(offsets, nodes) of the tracks `which` alone, in that order."""
    seg = [np.asarray(t_nodes[t_off[t]:t_off[t + 1]]) for t in which]
    return np.concatenate([[0], np.cumsum([len(s) for s in seg])]).astype(np.int64), np.concatenate(seg) if seg else np.zeros(0, np.int32)


def track_classes(sc, tri):
    """The classes the long-track tests need, counted over the unbanded tracks of a make_track_scene: longer than 64 and than 128
    observations, a point in pass 3, k = 5 with four points and every observation of the fifth true point left free, 12 to 64
    observations."""
    t_off, k = sc["t_off"], sc["k"]
    n = np.diff(t_off)
    clear = ~tri["banded"]
    fifth = np.zeros(len(n), bool)
    for t in np.nonzero(k == 5)[0]:
        truth, point = sc["truth"][t_off[t]:t_off[t + 1]], tri["obs_point"][t_off[t]:t_off[t + 1]]
        fifth[t] = (tri["n_obs"][t] > 0).all() and any((point[truth == j] == -1).all() for j in range(5))
    return {"tracks": len(n), "banded": int((~clear).sum()), "gt64": int((clear & (n > 64)).sum()), "gt128": int((clear & (n > 128)).sum()),
            "pass3": int((clear & (tri["n_obs"][:, MAX_POINTS - 1] > 0)).sum()), "k5_fifth_free": int((clear & fifth).sum()),
            "n12to64": int((clear & (n >= 12) & (n <= 64)).sum())}


def layout_from_tracks(cameras, images, tracks):
    """tracks: per track the observations [(image id, pixel [2] in the COLMAP frame)] in the order they are to be passed.  The
    key-point table of an image holds its observations track by track.  Returns (keypoints, Layout, t_off, t_nodes)."""
    ids = sorted(images)
    per_image = {i: [] for i in ids}
    where = []
    for obs in tracks:
        where.append([])
        for i, p in obs:
            where[-1].append((i, len(per_image[i])))
            per_image[i].append(np.asarray(p, float))
    keypoints = {i: (np.array(per_image[i]).reshape(-1, 2) - 0.5).astype(np.float32) for i in ids}
    L = Layout(cameras, images, keypoints)
    nodes = [[int(L.off[L.index[i]]) + r for i, r in w] for w in where]
    t_off = np.concatenate([[0], np.cumsum([len(n) for n in nodes])]).astype(np.int64)
    return keypoints, L, t_off, np.concatenate(nodes).astype(np.int32)


RULE_VIEWS = (3, 7, 11, 15, 19, 23, 27, 31, 35)
RULE_LONG_LABELS = {"narrow_far_long": 1, "plain_long": 1}   # labels under which one of the track's 64 draws is a pair that makes its point
RULE_LATE = dict(create_max_angle_error=0.1, filter_max_reproj_error=4.0)   # 0.1 deg is 1.4 px at these focal lengths


def make_rule_tracks(n_images=36):
    """Hand-built tracks on the views of make_track_scene(n_images=36) for the one-per-image rule; 0.05 px of noise except where designed.
      'dup_mid', 'dup_first'  one true point in RULE_VIEWS, the observation of view 19 / view 3 listed twice, bit for bit;
      'plain'                 one true point, nothing special (the unaffected neighbour);
      'narrow'                a point 100 units away seen by views 17-20: every pair of views subtends less than 1 degree;
      'narrow_far'            the same plus view 33 with an observation 14 px off: the pair with it is a valid hypothesis that all
                              five support, the refinement then puts it 11 px out, the filter frees it, and the four left subtend
                              less than min_tri_angle, so the point is dropped after it was made;
      'narrow_far_long'       'narrow_far' behind 70 stray key points of view 1, so the point's observations lie beyond index 64 and its
                              hypothesis is drawn (RULE_LONG_LABELS picks a draw that finds it);
      'plain_long'            a true point in RULE_VIEWS behind the same 70 stray key points: every pair of views that gives the point its
                              triangulation angle lies beyond index 64;
      'late'                  (for RULE_LATE) view 11 holds two observations 0.9 and 0.3 px off (both support; the closer one, the
                              second, must be taken), view 23 two at -3.2 and -2.4 px (outside the creation bound, inside the filter's:
                              the view joins in the completion only, with the second), view 31 an exact one and one 2.5 px off (the
                              point holds the view already: nothing of it joins in the completion).
    Returns {'cameras', 'images', 'keypoints', 'L', 't_off', 't_nodes', 'names', 'at': name -> {role: observation index in the track}}."""
    rs = np.random.RandomState(5)
    cameras, images = arc_cameras(n_images)

    def seen(X, views, dy=None):
        out = []
        for i in views:
            px, z = pr.project(cameras[images[i].camera_id], images[i].qvec, images[i].tvec, X[None])
            assert z[0] > 0
            out.append((i, px[0] + 0.05 * rs.standard_normal(2) + np.array([0.0, 0.0 if dy is None else dy.get(i, 0.0)])))
        return out

    names, tracks, at = [], [], {}
    for name, view, X in (("dup_mid", 19, ARC_TARGET + [0.3, 0.2, -0.4]), ("dup_first", 3, ARC_TARGET + [-0.5, -0.3, 0.6])):
        obs = seen(np.asarray(X), RULE_VIEWS)
        k = RULE_VIEWS.index(view)
        obs.insert(k + 1, (view, obs[k][1].copy()))
        names.append(name), tracks.append(obs)
        at[name] = {"lower": k, "higher": k + 1}
    names.append("plain"), tracks.append(seen(ARC_TARGET + [0.1, -0.4, 0.2], RULE_VIEWS))
    far = ARC_TARGET + [0.0, 0.0, 90.0]
    names.append("narrow"), tracks.append(seen(far, (17, 18, 19, 20)))
    names.append("narrow_far"), tracks.append(seen(far, (17, 18, 19, 20, 33), {33: 14.0}))
    # 70 stray key points of view 1 in front (none within 60 px of the two points they precede): what follows sits past a wave
    near = ARC_TARGET + [0.4, 0.1, -0.3]
    keep_off = pr.project(cameras[images[1].camera_id], images[1].qvec, images[1].tvec, np.stack([far, near]))[0]
    stray = []
    while len(stray) < 70:
        p = np.array([rs.uniform(8, 632), rs.uniform(8, 472)])
        if np.linalg.norm(keep_off - p, axis=1).min() > 60:
            stray.append((1, p))
    names.append("narrow_far_long"), tracks.append(stray + seen(far, (17, 18, 19, 20, 33), {33: 14.0}))
    names.append("plain_long"), tracks.append(stray + seen(near, RULE_VIEWS))
    X = ARC_TARGET + [-0.2, 0.3, 0.3]
    obs, roles = [], {}
    for i, p in seen(X, RULE_VIEWS):
        extra = {11: (("a_far", 0.9), ("a_near", 0.3)), 23: (("b_far", -3.2), ("b_near", -2.4)), 31: (("c_held", 0.0), ("c_other", 2.5))}.get(i)
        if extra is None:
            obs.append((i, p))
            continue
        for role, dy in extra:
            roles[role] = len(obs)
            obs.append((i, p + [0.0, dy]))
    names.append("late"), tracks.append(obs)
    at["late"] = roles
    keypoints, L, t_off, t_nodes = layout_from_tracks(cameras, images, tracks)
    labels = [RULE_LONG_LABELS.get(n, int(t_nodes[t_off[t]])) for t, n in enumerate(names)]
    return {"cameras": cameras, "images": images, "keypoints": keypoints, "L": L, "t_off": t_off, "t_nodes": t_nodes, "names": names, "at": at,
            "labels": labels}


# ------------------------------------------------------------------------------------------------------------------ designed pairs
SEAM_EMPTY = (1, 6, 10)
SEAM_MIN_INLIERS = 15


def make_seam_pairs(seed=0, max_error=DEFAULTS["max_error"]):
    """Hand-built pairs for the verification at its block seams (a block is 256 matches) on ten arc cameras of which images 1, 6 and
    10 (front, middle, end of the table) have no key points.  A true match is the exact projection of a point into both images; a
    false one has its second key point moved across the epipolar line by 3.5 to 8 thresholds.  Every pair brings its own key points,
    appended to its images' tables in pair order.
    Returns {'cameras', 'images', 'keypoints', 'L', 'pair_matches', 'truth' (per pair, bool; False also for the rows that are no
    match), 'names'}."""
    rs = np.random.RandomState(seed)
    cameras, images = arc_cameras(10)
    kps = {i: [] for i in images}
    cam = (lambda i: cameras[images[i].camera_id])
    R = {i: pr.qvec2rotmat(images[i].qvec) for i in images}

    def moved(i, j, pi, pj):                                 # pj across the epipolar line of pi
        Rr = R[j] @ R[i].T
        t = images[j].tvec - Rr @ images[i].tvec
        E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ Rr
        line = E @ np.append(pr.undistort(cam(i), pi[None])[0], 1.0)
        n = line[:2] / np.linalg.norm(line[:2])
        xj = pr.undistort(cam(j), pj[None])[0] + rs.choice([-1.0, 1.0]) * rs.uniform(3.5, 8.0) * max_error / pr.mean_focal(cam(j)) * n
        fx, fy, cx, cy = pr._opencv(cam(j))[:4]
        ud, vd = pr.distort(cam(j), xj[0], xj[1])
        return np.array([fx * ud + cx, fy * vd + cy])

    def add(i, j, n, false_at, points=None):
        rows = np.zeros((n, 2), np.int32)
        truth = np.ones(n, bool)
        for r in range(n):
            if points is None:
                X = ARC_TARGET + np.array([rs.uniform(-2, 2), rs.uniform(-1.5, 1.5), rs.uniform(-2, 2)])
            else:
                X = points[r]
            pi, zi = pr.project(cam(i), images[i].qvec, images[i].tvec, X[None])
            pj, zj = pr.project(cam(j), images[j].qvec, images[j].tvec, X[None])
            assert zi[0] > 0 and zj[0] > 0
            pi, pj = pi[0], pj[0]
            if r in false_at:
                pj, truth[r] = moved(i, j, pi, pj), False
            rows[r, 0] = len(kps[i])
            kps[i].append(pi)
            rows[r, 1] = len(kps[j])
            kps[j].append(pj)
        return rows, truth

    def seams(n):
        return {r for r in (0, 255, 256, 511, 512, n - 1) if 0 <= r < n and n > 1} | set(rs.choice(n, n // 20, replace=False).tolist() if n > 40 else [])

    def back(i, corners, depth):                              # the points that image i sees at these stored key points
        xn = pr.undistort(cam(i), np.asarray(corners, float) + 0.5)
        return (np.concatenate([xn, np.ones((len(xn), 1))], 1) * depth - images[i].tvec) @ R[i]

    names, pairs, truths = [], [], []

    def pair(name, i, j, rows, truth):
        names.append(name), pairs.append((i, j, rows)), truths.append(truth)

    for name, i, j, n in (("n700", 2, 3, 700), ("n0", 3, 4, 0), ("n1", 4, 5, 1), ("n255", 5, 7, 255), ("n256", 7, 8, 256), ("n257", 8, 9, 257),
                          ("n512", 2, 5, 512), ("n513", 3, 7, 513)):
        pair(name, i, j, *add(i, j, n, seams(n)))
    pair("reversed_last_block", 9, 2, *add(9, 2, 600, set(range(520, 600, 2))))            # listed as (j, i), j > i
    rows, truth = add(4, 4, 20, set())                        # an image with itself: no epipolar geometry, every match is rejected
    rows[10:, 1] = rows[10:, 0]                               # (half of them a key point against itself)
    pair("self", 4, 4, rows, np.zeros(20, bool))
    rows, truth = add(5, 9, 40, {3, 17})
    rows[8], truth[8] = rows[7], truth[7]                     # a match listed twice
    rows[20], rows[21] = (-1, 5), (5, -1)
    truth[20] = truth[21] = False
    pair("twice_and_negative", 5, 9, rows, truth)
    corners = [(0, 0), (639, 0), (0, 479), (639, 479)]
    a, ta = add(7, 8, 5, {4}, back(7, corners + [(639, 479)], 10.0))                       # SIMPLE_RADIAL corners into OPENCV
    b, tb = add(8, 7, 5, {4}, back(8, corners + [(0, 0)], 10.0))                           # OPENCV corners into SIMPLE_RADIAL
    for i, rows, last in ((7, a, (639, 479)), (8, b, (0, 0))):                             # the corner itself, not its round trip
        for r, c in zip(rows[:, 0], corners + [last]):
            kps[i][r] = np.asarray(c, float) + 0.5
    pair("corners", 7, 8, np.concatenate([a, b[:, ::-1]]), np.concatenate([ta, tb]))
    spread = [10, 100, 200, 250, 255, 256, 300, 400, 500, 511, 512, 550, 580, 590, 599]
    assert len(spread) == SEAM_MIN_INLIERS
    pair("exactly_min", 2, 9, *add(2, 9, 600, set(range(600)) - set(spread)))
    pair("one_short", 2, 9, *add(2, 9, 600, set(range(600)) - set(spread[:-1])))
    keypoints = {i: (np.array(kps[i]).reshape(-1, 2) - 0.5).astype(np.float32) for i in images}
    for i in SEAM_EMPTY:
        assert len(keypoints[i]) == 0
    return {"cameras": cameras, "images": images, "keypoints": keypoints, "L": Layout(cameras, images, keypoints), "pair_matches": pairs,
            "truth": truths, "names": names}


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
        if a == b:
            E = np.zeros((3, 3))                              # an image with itself has no epipolar geometry: every distance is NaN
        m = np.asarray(m).reshape(-1, 2)
        xi = np.concatenate([L.xn[L.off[a] + m[:, 0]], np.ones((len(m), 1))], 1)
        xj = np.concatenate([L.xn[L.off[b] + m[:, 1]], np.ones((len(m), 1))], 1)
        lj, li = xi @ E.T, xj @ E
        with np.errstate(invalid="ignore", divide="ignore"):
            dj = np.abs((xj * lj).sum(1)) / np.hypot(lj[:, 0], lj[:, 1])
            di = np.abs((xi * li).sum(1)) / np.hypot(li[:, 0], li[:, 1])
        ti, tj = max_error / pr.mean_focal(L.cams[a]), max_error / pr.mean_focal(L.cams[b])
        live = (m >= 0).all(1)                                # a row with a negative end is no match: it leaves as (-1, -1), uncounted
        ok = (di <= ti) & (dj <= tj) & live
        near = ((np.abs(di - ti) <= BAND * ti) | (np.abs(dj - tj) <= BAND * tj)) & live
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
                    filter_max_reproj_error=DEFAULTS["filter_max_reproj_error"], seed=DEFAULTS["seed"], labels=None):
    """labels: the tracks' labels (64-bit, they key the draws); None = each track's first node, as sfd2_build_tracks labels them.
    Returns {'xyz' [T, 4, 3], 'error' [T, 4], 'n_obs' [T, 4], 'obs_point' int8 [O], 'banded' bool [T]}."""
    Tn = len(track_offsets) - 1
    out = {"xyz": np.zeros((Tn, MAX_POINTS, 3)), "error": np.zeros((Tn, MAX_POINTS)), "n_obs": np.zeros((Tn, MAX_POINTS), np.int32),
           "obs_point": np.full(len(track_nodes), -1, np.int8), "banded": np.zeros(Tn, bool)}
    tan_create, cos_min = np.tan(np.radians(create_max_angle_error)), np.cos(np.radians(min_tri_angle))
    for t in range(Tn):
        lo, hi = int(track_offsets[t]), int(track_offsets[t + 1])
        T = _Track(L, np.asarray(track_nodes[lo:hi], dtype=np.int64))
        key = mix64((seed & M64) ^ mix64(int(track_nodes[lo] if labels is None else labels[t]) & M64))
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


# ------------------------------------------------------------------------------------------------------------------ committed cases
# The scenes, option values, seeds and labels of tests/test_gpu_triangulation_edges.py, with their restatement results cached here so
# that the GPU tests and the CPU guards of tests/test_triangulation_host.py compute each once per run.  The seeds of the scenes were
# chosen so that the restatement meets LONG_CLASSES inside the band cap; the guards hold them to it.
LONG_SCENES = {"arc36": dict(seed=0), "arc80": dict(seed=10, n_images=80, tracks=TRACKS_80)}
LONG_BAND_CAP, GRID_BAND_CAP = 0.10, 0.15
LONG_CLASSES = {"arc36": dict(gt64=4, gt128=2, pass3=2, k5_fifth_free=1, n12to64=6), "arc80": dict(gt64=4, gt128=2)}
# (min_tri_angle, create_max_angle_error, filter_max_reproj_error): the defaults, one option at a time, two corners
GRID = ((1.5, 2.0, 4.0), (0.0, 2.0, 4.0), (5.0, 2.0, 4.0), (19.0, 2.0, 4.0), (1.5, 0.5, 4.0), (1.5, 1.0, 4.0), (1.5, 2.0, 1.0), (1.5, 2.0, 12.0),
        (0.0, 1.0, 12.0), (19.0, 0.5, 1.0))
SEEDS = (0, 1, 2 ** 63 + 5, -1)
LABELS = (7, 2 ** 31 - 2, 2 ** 40 + 3)
LABEL_STRIDE = 3                      # track t of a case carries label + LABEL_STRIDE * t


@functools.lru_cache(maxsize=None)
def track_scene(name):
    return make_track_scene(**LONG_SCENES[name])


@functools.lru_cache(maxsize=None)
def long_ref(name):
    sc = track_scene(name)
    return triangulate_ref(sc["L"], sc["t_off"], sc["t_nodes"])


@functools.lru_cache(maxsize=None)
def short_tracks():
    """The tracks of arc36 of at most 80 observations (k = 1, 2 and 3; all but one draw their hypotheses): the option grid and the
    seed / label cases run on these, a second per restatement."""
    sc = track_scene("arc36")
    which = [t for t in range(len(sc["k"])) if sc["t_off"][t + 1] - sc["t_off"][t] <= 80]
    return (sc,) + sub_tracks(sc["t_off"], sc["t_nodes"], which)


@functools.lru_cache(maxsize=None)
def grid_ref(g):
    sc, off, nodes = short_tracks()
    return triangulate_ref(sc["L"], off, nodes, min_tri_angle=g[0], create_max_angle_error=g[1], filter_max_reproj_error=g[2])


def case_labels(label, n):
    return [label + LABEL_STRIDE * t for t in range(n)]


@functools.lru_cache(maxsize=None)
def seed_ref(seed, label, seed_mask=M64, label_mask=M64):
    """The restatement of short_tracks() under a seed and labels; the masks restate it as a 32-bit truncation would have it."""
    sc, off, nodes = short_tracks()
    return triangulate_ref(sc["L"], off, nodes, seed=seed & seed_mask, labels=[v & label_mask for v in case_labels(label, len(off) - 1)])


@functools.lru_cache(maxsize=None)
def rule_ref():
    """(make_rule_tracks(), names of the tracks run at the defaults (labels: rt['labels']), their offsets and nodes and restatement, the
    same of 'late' under RULE_LATE)."""
    rt = make_rule_tracks()
    plain = [n for n in rt["names"] if n != "late"]
    off, nodes = sub_tracks(rt["t_off"], rt["t_nodes"], [rt["names"].index(n) for n in plain])
    loff, lnodes = sub_tracks(rt["t_off"], rt["t_nodes"], [rt["names"].index("late")])
    labels = [rt["labels"][rt["names"].index(n)] for n in plain]
    return (rt, plain, off, nodes, triangulate_ref(rt["L"], off, nodes, labels=labels), loff, lnodes,
            triangulate_ref(rt["L"], loff, lnodes, **RULE_LATE))


@functools.lru_cache(maxsize=None)
def seam_scene():
    return make_seam_pairs()
