"""Helpers shared by tests/golden/gen_covis_goldens.py and the covisibility tests (never imported by the product): seeded
synthetic maps, a scripted matcher, and scripted stand-ins for the two pose calls."""
import numpy as np

import pose_ref as pr


class Img:
    def __init__(self, name, qvec, tvec, point3D_ids):
        self.name, self.qvec, self.tvec, self.point3D_ids = name, np.asarray(qvec, float), np.asarray(tvec, float), np.asarray(point3D_ids, dtype=np.int64)


class Pt:
    def __init__(self, xyz, image_ids):
        self.xyz, self.image_ids = np.asarray(xyz, float), np.asarray(image_ids, dtype=np.int64)


def small_rot(rs, deg):
    ax = rs.standard_normal(3)
    ax /= np.linalg.norm(ax)
    a = np.radians(deg) / 2
    return np.concatenate([[np.cos(a)], np.sin(a) * ax])


def compose(dq, q):
    return pr.rotmat2qvec(pr.qvec2rotmat(dq) @ pr.qvec2rotmat(q))


def selection_map(seed=0, n_img=40, n_pts=3000):
    """A map for the frame selections: cameras along a line with slowly turning orientations, each observing a random subset of the
    points; images 7 and 8 observe the same points (equal counts), image 5 lists one id twice, some names hold left / right."""
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-20, 20, (n_pts, 3)) + [0, 0, 60]
    obs = {}
    for i in range(1, n_img + 1):
        centre = i * 3.0
        lo = int(n_pts * (i - 1) / (n_img + 12))
        window = np.arange(lo, min(n_pts, lo + n_pts * 13 // (n_img + 12)))
        obs[i] = rs.choice(window, 260, replace=False)
    obs[8] = obs[7].copy()
    images, seen = {}, {p: [] for p in range(n_pts)}
    for i in range(1, n_img + 1):
        ids = np.full(400, -1, dtype=np.int64)
        slots = rs.choice(400, len(obs[i]), replace=False)
        ids[slots] = obs[i] + 10
        if i == 5:
            free = np.flatnonzero(ids == -1)[0]
            ids[free] = ids[slots[0]]                       # a duplicated id inside one image
        q = compose(small_rot(rs, 0.6 * i), np.array([1.0, 0, 0, 0]))
        C = np.array([i * 3.0, rs.uniform(-0.5, 0.5), 0.0])
        t = -pr.qvec2rotmat(q) @ C
        name = ("left/" if i % 7 == 3 else "right/" if i % 7 == 5 else "db/") + f"{i:04d}.jpg"
        images[i] = Img(name, q, t, ids)
        for p in ids[ids != -1]:
            seen[int(p) - 10].append(i)
    points3D = {p + 10: Pt(xyz[p], seen[p]) for p in range(n_pts) if seen[p]}
    for im in images.values():                              # ids nobody kept (none here) would be a KeyError in the reference
        assert all(int(p) in points3D for p in im.point3D_ids if p != -1)
    return images, points3D


SELECTION_CASES = [  # (type, frame, covisibility_frame, obs_th, pose: None / 'near' / 'far')
    ("obs", 10, 0, 0, None), ("obs", 10, 5, 0, None), ("obs", 10, 50, 3, None), ("obs", 7, 50, 0, None), ("obs", 5, 0, 3, None),
    ("obs", 10, 50, 0, "near"), ("obs", 10, 5, 3, "near"), ("obs", 10, 0, 0, "near"), ("obs", 10, 50, 0, "far"), ("obs", 20, 5, 0, "far"),
    ("pos", 10, 0, 3, "near"), ("pos", 10, 5, 3, "near"), ("pos", 10, 50, 0, "near"), ("pos", 24, 50, 3, "near"), ("pos", 24, 5, 0, "near"),
]


def selection_pose(images, frame, kind, seed):
    if kind is None:
        return None, None
    rs = np.random.RandomState(seed)
    im = images[frame]
    q = compose(small_rot(rs, 2.0), im.qvec)
    C = pr.centre(im.qvec, im.tvec) + (rs.uniform(-1, 1, 3) if kind == "near" else np.array([500.0, 0, 0]))
    return q, -pr.qvec2rotmat(q) @ C


# ---------------------------------------------------------------------------------------------------------------- refinement scenes
CAMERA = pr.camera("SIMPLE_RADIAL")
QNAME = "query/q0.jpg"


def refinement_scene(seed=0, n=300, n_img=8, n_kp=260):
    """One query (pose, key points = projections - 0.5 as fp32, scores) over a map of n points and n_img database images.
    Image 3 has no point3D_ids at all (but the points list it, so the selection returns it), image 4 only two key points with a
    point.  plan[image id] = the matches0 (unmasked indexing) the scripted matcher answers with: mostly correct matches, some
    wrong ones (a key point paired with a point that projects elsewhere), among them key point 0 matched to the same wrong
    point in images 1 and 2 -- the first is gated out and still blocks the second."""
    rs = np.random.RandomState(seed)
    q, t, x, X, _ = pr.scene(rs, CAMERA, n, offset=(40.0, -10.0, 5.0))
    kpq = (x - 0.5).astype(np.float32)
    scores = rs.rand(n).astype(np.float32)
    images, plan, seen = {}, {}, {p: [] for p in range(n)}
    for i in range(1, n_img + 1):
        ids = np.full(n_kp, -1, dtype=np.int64)
        if i == 3:
            ids = np.zeros(0, dtype=np.int64)
        else:
            pts = rs.choice(n, 200, replace=False) if i != 4 else first_pts[5:7]     # image 4: two of image 1's points
            if i in (1, 2):
                pts[0] = 17                                  # both observe point 17 ...
            if i == 1:
                first_pts = pts.copy()
            slots = rs.choice(n_kp, len(pts), replace=False)
            ids[slots] = pts + 100
            m = np.full(n, -1, dtype=np.int64)
            right = rs.rand(len(pts)) < 0.75
            m[pts[right]] = slots[right]                     # correct: key point p sees point p
            wrong = np.flatnonzero(~right)
            for w in wrong[:25]:                             # wrong: another key point paired with this point
                kp = int(rs.randint(1, n))
                if m[kp] == -1:
                    m[kp] = slots[w]
            if i in (1, 2):
                m[0] = slots[0]                              # ... and key point 0 is (wrongly) matched to it in both
                m[17] = -1
            plan[i] = m
        images[i] = Img(f"db/{i:03d}.jpg", compose(small_rot(rs, 3.0), q), t + rs.uniform(-0.2, 0.2, 3), ids)
        for p in ids[ids != -1]:
            seen[int(p) - 100].append(i)
    seen[int(first_pts[3])].append(3)                                        # image 3 is connected without observing anything itself
    points3D = {p + 100: Pt(X[p], seen[p]) for p in range(n) if seen[p]}
    return dict(q=q, t=t, kpq=kpq, scores=scores, images=images, points3D=points3D, plan=plan, X=X)


def start_pose(sc, seed, deg=0.4, shift=0.05):
    rs = np.random.RandomState(seed)
    q0 = compose(small_rot(rs, deg), sc["q"])
    return q0, -pr.qvec2rotmat(q0) @ (pr.centre(sc["q"], sc["t"]) + shift * rs.standard_normal(3))


def feature_file(sc):
    """What the reference reads: keypoints [n,2], scores [n], descriptors [128, n]; column 0 of a database set carries the image id so
    that the scripted matcher knows which image it is asked about."""
    ff = {QNAME: {"keypoints": sc["kpq"], "scores": sc["scores"], "descriptors": np.zeros((128, len(sc["kpq"])))}}
    for i, im in sc["images"].items():
        d = np.zeros((128, max(len(im.point3D_ids), 4)))
        d[0, :] = i
        ff[im.name] = {"keypoints": np.zeros((d.shape[1], 2), np.float32), "scores": np.zeros(d.shape[1], np.float32), "descriptors": d}
    return ff


def scripted_matcher(sc):
    """matcher(qname, db_names, point3D_ids_list) -> the planned matches0 per image (the caller's form)."""
    by_name = {im.name: i for i, im in sc["images"].items()}

    def matcher(qname, db_names, ids_list):
        return [sc["plan"].get(by_name[n], np.full(len(sc["kpq"]), -1, dtype=np.int64)).copy() for n in db_names]
    return matcher


REFINE_CASES = {  # name: (opt_type, iters, estimator success, inlier limit)
    "iters1": ("clurefobs", 1, True, None),
    "iters2": ("clurefobs", 2, True, None),
    "ransac_failure": ("clurefobs", 1, False, None),
    "few_inliers": ("clurefobs", 2, True, 9),
    "no_ref": ("cluobs", 2, True, None),
    "by_pose": ("clurefpos", 1, True, None),
}
RADIUS, OPT_TH, OBS_TH, FRAMES = 20.0, 12.0, 3, 50


def make_estimator(sc, seed, success=True, limit=None):
    """absolute_pose_estimation's stand-in: inliers = points within the threshold under the true pose (at most `limit` of them), a
    scripted pose near the truth; takes the problem list of the product's estimator protocol."""
    qr, tr = start_pose(sc, seed + 1000, 0.1, 0.01)

    def one(x, X, cam, thr):
        x, X = np.asarray(x, float).reshape(-1, 2), np.asarray(X, float).reshape(-1, 3)
        inl = pr.reproj_error(cam, sc["q"], sc["t"], x, X) <= thr if len(x) else np.zeros(0, bool)
        if limit is not None:
            inl[np.flatnonzero(inl)[limit:]] = False
        return {"success": bool(success), "qvec": qr.copy(), "tvec": tr.copy(), "num_inliers": int(inl.sum()), "inliers": inl}

    def estimator(problems):
        return [one(*p) for p in problems]
    estimator.one = one
    return estimator


def make_refiner(sc, seed):
    """pose_refinement's stand-in: call number c returns scripted pose c (ever closer to the truth); records its masks."""
    poses = [start_pose(sc, seed + 2000 + c, 0.2 / (c + 1), 0.02 / (c + 1)) for c in range(4)]
    calls = []

    def one(tvec, qvec, x, X, mask, cam):
        calls.append(np.asarray(mask, bool).copy())
        qv, tv = poses[len(calls) - 1]
        return {"success": True, "qvec": qv.copy(), "tvec": tv.copy()}

    def refiner(problems):
        return [one(*p) for p in problems]
    refiner.one, refiner.calls, refiner.poses = one, calls, poses
    return refiner
