"""Helpers of the frame-selection tests (never imported by the product): a plain-numpy restatement of sfd2_covis_frames as
include/sfd2_hip.h words it -- the two rules over the CSRs of MapIndex.frames_csr() and the status rule -- and the seeded maps and
task lists the host and the GPU tests share."""
import numpy as np

import covis_ref as cr
import pose_ref as pr

MAX_CANDIDATES = 4096


def _poses(q, t):
    """Normalised quaternions [n, 4] and camera centres -R^T t [n, 3] of qvec [n, 4], tvec [n, 3]."""
    q = np.asarray(q, np.float64).reshape(-1, 4)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = q / np.sqrt((q * q).sum(1))[:, None]
        w, x, y, z = q.T
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])          # [3, 3, n]
        C = -np.einsum("jin,nj->ni", R, t)
    return q, C


def select(fc, frame, kind, cf, obs_th, q_th=5.0, qvec=None, tvec=None, ref_rows=None, cap=None):
    """(image indices in result order, status) of one task, from the header's wording.  fc: MapIndex.frames_csr()."""
    oo, op, to, ti, so, si = (fc[k] for k in ("obs_offsets", "obs_point", "track_offsets", "track_image", "seen_offsets", "seen_image"))
    n = len(fc["ids"])
    V = op[oo[frame]:oo[frame + 1]] if ref_rows is None else np.asarray(ref_rows, dtype=np.int64)
    connected, count = np.zeros(n, bool), np.zeros(n, np.int64)
    for v in V:
        connected[ti[to[v]:to[v + 1]]] = True
        if to[v + 1] - to[v] >= obs_th:
            count[si[so[v]:so[v + 1]]] += 1
    posed = kind == "pos" or (qvec is not None and tvec is not None)
    if kind == "pos":
        connected &= fc["excluded"] == 0
    cand = np.flatnonzero(connected)
    band = False
    if posed:
        qp, Cp = _poses(qvec, tvec)
        qd, Cd = _poses(fc["qvec"][cand], fc["tvec"][cand])
        with np.errstate(all="ignore"):
            pcn = np.sqrt((Cp[0] ** 2).sum())
            band |= not (np.isfinite(qp).all() and np.isfinite(pcn))
            dot = np.minimum(np.abs(qd @ qp[0]), 1.0)
            q_err = 2 * np.arccos(dot) * 180 / np.pi
            t_err = np.sqrt(((Cp - Cd) ** 2).sum(1))
            cn = np.sqrt((Cd ** 2).sum(1))
            q_band = 1e-9 + np.minimum(1e-13 / np.sqrt(np.maximum(1 - dot * dot, 0.0)), 1e-5)
            t_band = 1e-9 * (1 + pcn + cn)
            th = q_th if kind == "pos" else 30.0
            band |= bool((~np.isfinite(q_err) | ~np.isfinite(t_err) | ~np.isfinite(cn) | (np.abs(q_err - th) <= q_band)).any())
            if kind == "obs":
                band |= bool((np.abs(t_err - 30.0) <= t_band).any())
    by_count = np.lexsort((cand, -count[cand]))                      # larger count first, then smaller index
    if kind == "obs":
        out, aside = [], []
        for o in by_count:
            d = int(cand[o])
            if posed and (q_err[o] >= 30 or t_err[o] >= 30 or count[d] <= 30):
                aside.append(d)
                continue
            out.append(d)
            if cf > 0 and len(out) >= cf:
                break
        if len(out) <= 3:
            for d in aside:
                out.append(d)
                if len(out) >= cf:
                    break
    else:
        with np.errstate(invalid="ignore"):
            ok = q_err <= q_th
        first = np.flatnonzero(ok)
        first = first[np.argsort(t_err[first], kind="stable")]
        lim = len(first) if cf == 0 else min(len(first), cf + 1)
        ts = t_err[first[:lim]]
        with np.errstate(invalid="ignore"):
            band |= bool((np.diff(ts) < 1e-9 * (1 + 2 * pcn + ts[1:])).any())
        out = [int(cand[o]) for o in (first if cf == 0 else first[:cf])]
        if cf > 0 and len(out) < cf:
            out += [int(cand[o]) for o in by_count if not ok[o]][:cf - len(out)]
    if cap is None:
        cap = max(cf, 4) if cf > 0 else min(n, MAX_CANDIDATES)
    status = 2 if (len(cand) > MAX_CANDIDATES or len(out) > cap) else 1 if band else 0
    return (out if status == 0 else []), status


def task_select(mi, t, kind="obs", covisibility_frame=50, obs_th=0, q_th=5):
    """select() for a task dict of MapIndex.covisible_frames_batch: (image ids, status)."""
    fc = mi.frames_csr()
    ref = t.get("ref_3Dpoints")
    rows = None
    if ref is not None:
        ref = np.asarray(ref, np.int64).reshape(-1)
        rows = mi.point_rows(ref[ref != -1])
    idx, st = select(fc, fc["index"][t["frame_id"]], t.get("kind", kind), int(t.get("covisibility_frame", covisibility_frame)),
                     int(np.ceil(t.get("obs_th", obs_th))), t.get("q_th", q_th), t.get("qvec"), t.get("tvec"), rows)
    return [int(fc["ids"][i]) for i in idx], st


def host_select(mi, t, kind="obs", covisibility_frame=50, obs_th=0, q_th=5):
    """The host function's list for a task dict."""
    k, cf = t.get("kind", kind), int(t.get("covisibility_frame", covisibility_frame))
    if k == "obs":
        return mi.covisible_frames(t["frame_id"], covisibility_frame=cf, ref_3Dpoints=t.get("ref_3Dpoints"), obs_th=t.get("obs_th", obs_th),
                                   pred_qvec=t.get("qvec"), pred_tvec=t.get("tvec"))
    return mi.covisible_frames_by_pose(t["frame_id"], t["qvec"], t["tvec"], covisibility_frame=cf, q_th=t.get("q_th", q_th),
                                       obs_th=t.get("obs_th", obs_th), ref_3Dpoints=t.get("ref_3Dpoints"))


def selection_tasks(images):
    """The 15 SELECTION_CASES of covis_ref as task dicts, with the poses and q_th 10 of tests/golden/gen_covis_goldens.py."""
    tasks = []
    for c, (kind, frame, cf, obs_th, pose) in enumerate(cr.SELECTION_CASES):
        q, t = cr.selection_pose(images, frame, pose, c)
        tasks.append(dict(frame_id=frame, kind=kind, covisibility_frame=cf, obs_th=obs_th, qvec=q, tvec=t, q_th=10))
    return tasks


def random_map(seed=0, n_img=300, n_kp=120, n_pts=2000):
    """About n_img images x n_kp key points over n_pts points: cameras on a line, each observing points of a window around it.
    Tracks list non-observing images and repeat an image, images repeat an id, many tracks are shorter than 3, image groups share
    their whole observation list (large groups of equal counts), some names hold left/ or right/.  Ids are not 0-based and the dict
    is not in id order."""
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-20, 20, (n_pts, 3))
    obs = {}
    for i in range(n_img):
        lo = int((n_pts - 500) * i / n_img)
        obs[i] = rs.choice(np.arange(lo, lo + 500), rs.randint(60, n_kp - 10), replace=False)
    for g in range(0, n_img, 25):                                   # groups of 6 images with identical observations
        for k in range(1, 6):
            obs[g + k] = obs[g].copy()
    rare = rs.choice(n_pts, 300, replace=False)                     # points only one or two images keep: short tracks
    seen = {p: [] for p in range(n_pts)}
    images = {}
    order = rs.permutation(n_img)
    for i in order:
        pts = obs[i]
        pts = pts[~np.isin(pts, rare) | (rs.rand(len(pts)) < 0.05)]
        ids = np.full(n_kp, -1, dtype=np.int64)
        slots = rs.choice(n_kp, len(pts), replace=False)
        ids[slots] = pts + 1000
        free = np.flatnonzero(ids == -1)
        if i % 4 == 0 and len(free) >= 2 and len(pts) >= 2:         # ids repeated inside an image
            ids[free[0]], ids[free[1]] = ids[slots[0]], ids[slots[1]]
        q = cr.compose(cr.small_rot(rs, 0.08 * i), np.array([1.0, 0, 0, 0]))
        C = np.array([i * 0.4, rs.uniform(-0.5, 0.5), rs.uniform(-0.5, 0.5)])
        name = ("left/" if i % 11 == 3 else "right/" if i % 11 == 7 else "db/") + f"{i:04d}.jpg"
        images[int(i) * 3 + 7] = cr.Img(name, q, -pr.qvec2rotmat(q) @ C, ids)
        for p in ids[ids != -1]:
            seen[int(p) - 1000].append(int(i) * 3 + 7)
    all_ids = sorted(images)
    points3D = {}
    for p in range(n_pts):
        if not seen[p]:
            continue
        track = list(seen[p])
        if p % 5 == 0:
            track.append(all_ids[rs.randint(n_img)])                # an image that does not observe the point
        if p % 7 == 0:
            track.append(track[0])                                  # an image repeated inside the track
        points3D[p + 1000] = cr.Pt(xyz[p], [track[k] for k in rs.permutation(len(track))])
    return images, points3D


def random_tasks(images, points3D, seed=1, n=64):
    """n tasks mixing obs with and without pose, pos, cf in {0, 4, 10, 50}, obs_th in {0, 3} and explicit ref_3Dpoints with repeats."""
    rs = np.random.RandomState(seed)
    ids = sorted(images)
    pids = np.array(sorted(points3D))
    tasks = []
    for k in range(n):
        f = ids[rs.randint(len(ids))]
        im = images[f]
        t = dict(frame_id=f, kind=("obs", "obs", "pos")[k % 3], covisibility_frame=(0, 4, 10, 50)[(k // 3) % 4], obs_th=(0, 3)[(k // 12) % 2])
        if t["kind"] == "pos" or k % 6 == 1:
            q = cr.compose(cr.small_rot(rs, rs.uniform(0.5, 3.0)), im.qvec)
            C = pr.centre(im.qvec, im.tvec) + rs.uniform(-2, 2, 3)
            t.update(qvec=q, tvec=-pr.qvec2rotmat(q) @ C, q_th=(3.0, 8.0)[k % 2])
        if k % 5 == 0:
            own = im.point3D_ids[im.point3D_ids != -1]
            extra = pids[rs.randint(0, len(pids), 40)]
            t["ref_3Dpoints"] = np.concatenate([own[:30], own[:10], extra, [-1, -1]])          # repeats and -1s
        tasks.append(t)
    return tasks


def star_map(n_img=1500):
    """n_img images that all observe one shared point; image i also observes i % 5 private points with image i + 1 (counts 1..5 in
    large groups)."""
    images, tracks = {}, {1: []}
    nxt = 2
    priv = {}
    for i in range(1, n_img + 1):
        k = i % 5
        priv[i] = list(range(nxt, nxt + k))
        nxt += k
    for i in range(1, n_img + 1):
        ids = [1] + priv[i] + (priv[i - 1] if i > 1 else [])
        images[i] = cr.Img(f"db/{i:05d}.jpg", [1.0, 0, 0, 0], [-float(i), 0, 0], ids)
        for p in ids:
            tracks.setdefault(p, []).append(i)
    points3D = {p: cr.Pt([0.0, 0, 5], t) for p, t in tracks.items()}
    return images, points3D
