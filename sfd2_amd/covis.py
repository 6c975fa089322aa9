"""The map side of the localiser's covisibility stage (it_loc/localize_cv2.py:120-233 and the helpers of it_loc/common.py it uses):
a dense index over COLMAP's images / points3D dicts, the two covisible-frame selections, vectorised on the host and batched on the
device (sfd2_covis_frames), and the device buffers sfd2_assemble_2d3d reads (point table, per-image key point -> point row tables)."""
import math

import numpy as np

from .pose import CAMERA_MODELS


def qvec2rotmat(qvec):
    """R of COLMAP's (w, x, y, z); the quaternion is normalised first, as scipy's Rotation.from_quat does (common.py:235)."""
    q = np.asarray(qvec, dtype=np.float64).reshape(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _opencv(camera):
    model = camera["model"]
    if not isinstance(model, str):
        model = getattr(model, "name", str(model))
    if model not in CAMERA_MODELS:
        raise ValueError(f"camera model {model!r} is not supported (one of {', '.join(CAMERA_MODELS)})")
    p = np.asarray(camera["params"], dtype=np.float64).reshape(-1)
    if model == "SIMPLE_PINHOLE":
        return p[0], p[0], p[1], p[2], 0.0, 0.0, 0.0, 0.0
    if model == "PINHOLE":
        return p[0], p[1], p[2], p[3], 0.0, 0.0, 0.0, 0.0
    if model == "SIMPLE_RADIAL":
        return p[0], p[0], p[1], p[2], p[3], 0.0, 0.0, 0.0
    return tuple(p[:8])


def reproject(points3D, rvec, tvec, camera):
    """it_loc/common.py:225-277 reproject for the four models of pose.CAMERA_MODELS: pixels [N, 2] of world points [N, 3] under
    (rvec = qvec (w, x, y, z), tvec), no depth test."""
    X = np.asarray(points3D, dtype=np.float64).reshape(-1, 3)
    P = qvec2rotmat(rvec) @ X.T + np.asarray(tvec, dtype=np.float64).reshape(3, 1)
    fx, fy, cx, cy, k1, k2, p1, p2 = _opencv(camera)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = P[0] / P[2], P[1] / P[2]
        r2 = u * u + v * v
        rad = k1 * r2 + k2 * r2 * r2
        ud = u + u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u)
        vd = v + v * rad + 2 * p2 * u * v + p1 * (r2 + 2 * v * v)
    return np.stack([ud * fx + cx, vd * fy + cy], 1)


def compute_pose_error(pred_qcw, pred_tcw, gt_qcw, gt_tcw):
    """it_loc/common.py:298-317: (rotation error in degrees, distance of the camera centres, its three components)."""
    Rp, Rg = qvec2rotmat(pred_qcw), qvec2rotmat(gt_qcw)
    d = (-Rp.T @ np.asarray(pred_tcw, float).reshape(3, 1)) - (-Rg.T @ np.asarray(gt_tcw, float).reshape(3, 1))
    t_error = np.sqrt(np.sum(d ** 2))
    qp = np.asarray(pred_qcw, float).reshape(4)
    qg = np.asarray(gt_qcw, float).reshape(4)
    c = abs(np.dot(qp / np.linalg.norm(qp), qg / np.linalg.norm(qg)))
    q_error = 2 * np.arccos(min(1.0, max(-1.0, c))) * 180 / np.pi
    return q_error, t_error, (d[0, 0], d[1, 0], d[2, 0])


class MapIndex:
    """images, points3D: the dicts COLMAP's read_write_model returns (image id -> .name .qvec .tvec .point3D_ids, point id ->
    .xyz .image_ids).  Holds the dense point table (ids ascending: point_ids, xyz fp64 [P, 3], track_len int32 [P] =
    len(image_ids), duplicates counted) and, per image, the table key point -> row of the point table (-1 = none).
    to_device() puts the point table on the GPU; the per-image tables follow on first use and stay (device_rows)."""

    def __init__(self, images, points3D):
        self.images, self.points3D = images, points3D
        self.point_ids = np.array(sorted(points3D), dtype=np.int64)
        P = len(self.point_ids)
        self.xyz = np.ascontiguousarray(np.array([points3D[int(i)].xyz for i in self.point_ids], dtype=np.float64).reshape(P, 3))
        self.track_len = np.array([len(points3D[int(i)].image_ids) for i in self.point_ids], dtype=np.int32)
        self.name_to_id = {im.name: i for i, im in images.items()}
        self._rows, self._dev_rows = {}, {}
        self.device = None
        self._dev_xyz = self._dev_track = None
        self._csr = None
        self._frames = self._dev_frames = None
        self.frames_tasks = self.frames_host = 0      # tasks covisible_frames_batch has seen / decided with the host functions

    # ------------------------------------------------------------------------------------------------ tables
    def point_rows(self, ids):
        """Rows of the point table for an array of point3D ids (-1 for -1 and for ids the map does not hold)."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if len(self.point_ids) == 0:
            return np.full(ids.shape, -1, dtype=np.int32)
        pos = np.minimum(np.searchsorted(self.point_ids, ids), len(self.point_ids) - 1)
        return np.where(self.point_ids[pos] == ids, pos, -1).astype(np.int32)

    def rows(self, image_id):
        r = self._rows.get(image_id)
        if r is None:
            r = self._rows[image_id] = self.point_rows(self.images[image_id].point3D_ids)
        return r

    def to_device(self, device=0):
        import torch
        self.device = torch.device("cuda", int(device))
        self._dev_xyz = torch.from_numpy(self.xyz if self.xyz.size else np.zeros((1, 3))).to(self.device)
        self._dev_track = torch.from_numpy(self.track_len if self.track_len.size else np.zeros(1, np.int32)).to(self.device)
        self._dev_rows = {}
        self._dev_frames = None                       # the CSRs of frames_csr() follow on first use (covisible_frames_batch)
        return self

    def device_rows(self, image_id):
        """(device pointer or None, n1) of an image's table; uploaded on first use and kept."""
        ent = self._dev_rows.get(image_id)
        if ent is None:
            import torch
            r = self.rows(image_id)
            t = torch.from_numpy(r).to(self.device) if r.size else None
            ent = self._dev_rows[image_id] = (t, None if t is None else t.data_ptr(), int(r.size))
        return ent[1], ent[2]

    def point_table(self):
        from . import _lib
        if self._dev_xyz is None:
            raise RuntimeError("MapIndex.to_device() has not been called")
        return _lib.PointTable(self._dev_xyz.data_ptr(), self._dev_track.data_ptr(), len(self.point_ids), 0)

    # ------------------------------------------------------------------------------------------------ clustering
    def csr(self):
        """(image id -> image index, obs_offsets, obs_point, track_offsets, track_image): the two CSRs of sfd2_pairs_covisibility /
        sfd2_covis_clusters (sfd2_amd.pairs.covisibility_csr), built on first use and kept."""
        if self._csr is None:
            from .pairs import covisibility_csr
            ids, oo, op, to, ti = covisibility_csr(self.images, self.points3D)
            self._csr = ({iid: i for i, iid in enumerate(ids)}, oo, op, to, ti)
        return self._csr

    def cluster_lists(self, frame_ids_per_query):
        """The host part of clusters(): per query the ids with repeats dropped (the first occurrence stays, which is what the
        reference's visited set does), and the concatenated form sfd2_covis_clusters takes: frame_offsets int64 [nq + 1], frames
        int32 (image indices of csr()).  An id the map does not hold is a KeyError, as in the reference."""
        index = self.csr()[0]
        lists = [list(dict.fromkeys(int(f) for f in frame_ids)) for frame_ids in frame_ids_per_query]
        off = np.zeros(len(lists) + 1, dtype=np.int64)
        np.cumsum([len(li) for li in lists], out=off[1:])
        frames = np.array([index[f] for li in lists for f in li], dtype=np.int32)
        return lists, off, frames

    @staticmethod
    def clusters_from_ranks(lists, frame_offsets, cluster, n_clusters):
        """Per query the list of clusters (lists of image ids): cluster[p] is position p's cluster, members by ascending position."""
        out = []
        for q, li in enumerate(lists):
            cl = [[] for _ in range(int(n_clusters[q]))]
            for f, c in zip(li, cluster[frame_offsets[q]:frame_offsets[q + 1]]):
                cl[int(c)].append(f)
            out.append(cl)
        return out

    def clusters(self, frame_ids_per_query, device=0, global_slots=False):
        """do_covisibility_clustering (it_loc/localize_cv2.py:87-117) for many queries in ONE sfd2_covis_clusters call:
        frame_ids_per_query[q] is query q's retrieved image ids in retrieval order.  Returns per query the reference's list of lists
        of image ids: largest cluster first, equal sizes in order of creation; members by ascending list position (the reference's
        member order is set.pop()'s).  At most _lib.CLUSTER_MAX_FRAMES distinct ids per query.  global_slots forces the path of maps
        too large for the LDS table."""
        from . import _lib
        lists, off, frames = self.cluster_lists(frame_ids_per_query)
        if not lists:
            return []
        _, oo, op, to, ti = self.csr()
        cluster = np.empty(len(frames), dtype=np.int32)
        n_clusters = np.empty(len(lists), dtype=np.int32)
        ctx = _lib.default_context(device)
        _lib.check(ctx.lib.sfd2_covis_clusters(ctx.h, oo.ctypes.data, op.ctypes.data if len(op) else None, len(oo) - 1, to.ctypes.data,
                                               ti.ctypes.data if len(ti) else None, len(to) - 1, off.ctypes.data,
                                               frames.ctypes.data if len(frames) else None, len(lists), cluster.ctypes.data if len(frames) else None,
                                               n_clusters.ctypes.data, _lib.CLUSTER_FLAG_GLOBAL_SLOTS if global_slots else 0))
        return self.clusters_from_ranks(lists, off, cluster, n_clusters)

    # ------------------------------------------------------------------------------------------------ selections on the device
    def frames_csr(self):
        """What sfd2_covis_frames reads of the map, built on first use and kept: a dict with ids (image ids ascending: index order is
        id order, so that ties by index are the reference's ties by id), index (id -> image index), the CSRs of csr() over that
        order (obs_offsets, obs_point, track_offsets, track_image), the seen CSR (seen_offsets, seen_image: per point the distinct
        images whose point3D_ids hold it, ascending), excluded (uint8: the name holds 'left' or 'right'), qvec [n, 4], tvec [n, 3]."""
        if self._frames is None:
            ids = sorted(self.images)
            if ids == list(self.images):
                _, oo, op, to, ti = self.csr()
            else:
                from .pairs import covisibility_csr
                _, oo, op, to, ti = covisibility_csr({i: self.images[i] for i in ids}, self.points3D)
            n, P = len(ids), len(self.point_ids)
            pairs = np.unique(op.astype(np.int64) * n + np.repeat(np.arange(n, dtype=np.int64), np.diff(oo)))
            so = np.zeros(P + 1, dtype=np.int64)
            np.cumsum(np.bincount(pairs // n, minlength=P), out=so[1:])
            names = [self.images[i].name for i in ids]
            self._frames = dict(
                ids=np.array(ids, dtype=np.int64), index={iid: i for i, iid in enumerate(ids)}, obs_offsets=oo, obs_point=op, track_offsets=to,
                track_image=ti, seen_offsets=so, seen_image=np.ascontiguousarray((pairs % n).astype(np.int32)),
                excluded=np.array([nm.find("left") >= 0 or nm.find("right") >= 0 for nm in names], dtype=np.uint8),
                qvec=np.ascontiguousarray(np.array([self.images[i].qvec for i in ids], dtype=np.float64).reshape(n, 4)),
                tvec=np.ascontiguousarray(np.array([self.images[i].tvec for i in ids], dtype=np.float64).reshape(n, 3)))
        return self._frames

    _FRAMES_ARRAYS = ("obs_offsets", "obs_point", "track_offsets", "track_image", "seen_offsets", "seen_image", "excluded", "qvec", "tvec")

    def _frames_map(self):
        """(sfd2_frames_map, what must outlive the call): device pointers once to_device() was called -- the arrays are uploaded on
        first use and stay -- else host pointers."""
        from . import _lib
        fc = self.frames_csr()
        if self.device is not None:
            if self._dev_frames is None:
                import torch
                self._dev_frames = {k: torch.from_numpy(fc[k] if fc[k].size else np.zeros(1, fc[k].dtype)).to(self.device) for k in self._FRAMES_ARRAYS}
            src, at = self._dev_frames, (lambda a: a.data_ptr())
        else:
            src, at = fc, (lambda a: a.ctypes.data if a.size else None)
        m = _lib.FramesMap(*[at(src[k]) for k in self._FRAMES_ARRAYS], len(fc["obs_point"]), len(fc["track_image"]), len(fc["seen_image"]),
                           len(fc["ids"]), len(self.point_ids), 1 if self.device is not None else 0, 0)
        return m, src

    def covisible_frames_batch(self, tasks, kind="obs", covisibility_frame=50, obs_th=0, q_th=5, ref_3Dpoints=None, device=0,
                               global_counters=False, cap=None, lib=None):
        """covisible_frames (kind 'obs') / covisible_frames_by_pose ('pos') for many tasks in ONE sfd2_covis_frames call.  tasks: dicts
        with frame_id and qvec / tvec (None or absent: no pose; 'pos' needs one), which may also hold kind, covisibility_frame,
        obs_th, q_th and ref_3Dpoints to override the arguments.  Returns per task the list of image ids the host function returns.

        The library reports per task whether its row is the host's result (status 0), whether a decision lay inside a rounding band
        (1) or whether a capacity was exceeded (2: more than cap results -- the default cap cannot overflow -- or more than
        _lib.FRAMES_MAX_CANDIDATES connected frames); every task whose status is not 0 is decided by the host function here, and so
        is every task with covisibility_frame 1, 2 or 3, where the reference's `<= 3 frames` fall-back appends to a list that is
        already full: those never reach the library.  A ref_3Dpoints id the map does not hold goes to the host function as well,
        which raises the reference's KeyError.  With the map on the device (to_device()) the CSRs are uploaded on first use and
        stay; otherwise the call takes host arrays and uploads them itself.  lib: a stand-in for the library (tests)."""
        from . import _lib
        tasks = list(tasks)
        if not tasks:
            return []
        fc = self.frames_csr()
        n_images = len(fc["ids"])
        spec, out = [], [None] * len(tasks)

        def host(s):
            if s["kind"] == "obs":
                return self.covisible_frames(s["frame_id"], covisibility_frame=s["cf"], ref_3Dpoints=s["ref"], obs_th=s["obs_th"], pred_qvec=s["qvec"],
                                             pred_tvec=s["tvec"])
            return self.covisible_frames_by_pose(s["frame_id"], s["qvec"], s["tvec"], covisibility_frame=s["cf"], q_th=s["q_th"], obs_th=s["obs_th"],
                                                 ref_3Dpoints=s["ref"])
        live, rows_list = [], []
        for i, t in enumerate(tasks):
            s = dict(frame_id=t["frame_id"], kind=t.get("kind", kind), cf=int(t.get("covisibility_frame", covisibility_frame)),
                     obs_th=t.get("obs_th", obs_th), q_th=t.get("q_th", q_th), qvec=t.get("qvec"), tvec=t.get("tvec"),
                     ref=t.get("ref_3Dpoints", ref_3Dpoints))
            if s["kind"] not in ("obs", "pos"):
                raise ValueError(f"kind {s['kind']!r}: 'obs' or 'pos'")
            spec.append(s)
            rows = None
            if s["ref"] is not None:
                ids = np.asarray(s["ref"], dtype=np.int64).reshape(-1)
                rows = self.point_rows(ids[ids != -1])
            posed = s["qvec"] is not None and s["tvec"] is not None
            if 1 <= s["cf"] <= 3 or s["cf"] < 0 or s["frame_id"] not in fc["index"] or (rows is not None and (rows < 0).any()) or \
                    (s["kind"] == "pos" and not posed):
                out[i] = host(s)
                continue
            live.append(i)
            rows_list.append(rows)
        self.frames_tasks += len(tasks)
        self.frames_host += len(tasks) - len(live)
        if not live:
            return out
        arr = (_lib.FramesTask * len(live))()
        ref_off = np.zeros(len(live) + 1, dtype=np.int64)
        for j, (i, rows) in enumerate(zip(live, rows_list)):
            s, a = spec[i], arr[j]
            a.frame, a.kind, a.covisibility_frame = fc["index"][s["frame_id"]], _lib.FRAMES_POS if s["kind"] == "pos" else _lib.FRAMES_OBS, s["cf"]
            a.obs_th = int(min(max(math.ceil(s["obs_th"]), -2 ** 31), 2 ** 31 - 1))      # track_len >= obs_th over integers
            a.q_th = float(s["q_th"])
            a.has_pose = 1 if (s["qvec"] is not None and s["tvec"] is not None) else 0
            if a.has_pose:
                qv, tv = np.asarray(s["qvec"], dtype=np.float64).reshape(4), np.asarray(s["tvec"], dtype=np.float64).reshape(3)
                for k in range(4):
                    a.qvec[k] = qv[k]
                for k in range(3):
                    a.tvec[k] = tv[k]
            a.use_ref = 0 if rows is None else 1
            ref_off[j + 1] = ref_off[j] + (0 if rows is None else len(rows))
        any_ref = any(r is not None for r in rows_list)
        ref_pts = np.ascontiguousarray(np.concatenate([r for r in rows_list if r is not None]).astype(np.int32)) if any_ref else np.zeros(0, np.int32)
        if cap is None:
            cap = max(max(spec[i]["cf"], 4) if spec[i]["cf"] > 0 else min(n_images, _lib.FRAMES_MAX_CANDIDATES) for i in live)
        cap = int(cap)
        fmap, keep = self._frames_map()
        idx = np.empty((len(live), max(cap, 1)), dtype=np.int32)
        n_out = np.empty(len(live), dtype=np.int32)
        status = np.empty(len(live), dtype=np.int32)
        h = None
        if lib is None:
            ctx = _lib.default_context(self.device.index if self.device is not None else device)
            lib, h = ctx.lib, ctx.h
        import ctypes
        rc = lib.sfd2_covis_frames(h, ctypes.byref(fmap), arr, len(live), ref_off.ctypes.data if any_ref else None,
                                   ref_pts.ctypes.data if len(ref_pts) else None, cap, idx.ctypes.data, n_out.ctypes.data, status.ctypes.data,
                                   _lib.FRAMES_FLAG_GLOBAL_COUNTERS if global_counters else 0)
        del keep
        if rc != 0:
            raise RuntimeError("libsfd2hip: " + _lib.load().sfd2_last_error().decode("utf-8", "replace"))
        ids = fc["ids"]
        for j, i in enumerate(live):
            if status[j] != 0:
                self.frames_host += 1
                out[i] = host(spec[i])
            else:
                out[i] = [int(v) for v in ids[idx[j, :n_out[j]]]]
        return out

    # ------------------------------------------------------------------------------------------------ selections
    def _observed(self, frame_id, ref_3Dpoints):
        observed = np.asarray(self.images[frame_id].point3D_ids if ref_3Dpoints is None else ref_3Dpoints, dtype=np.int64).reshape(-1)
        valid = observed[observed != -1]
        lists = [np.asarray(self.points3D[int(i)].image_ids).reshape(-1) for i in valid]
        connected = np.unique(np.concatenate(lists)) if lists else np.zeros(0, dtype=np.int64)
        return valid, connected

    def _counts(self, valid, connected, obs_th):
        """Per connected frame: how many entries of `valid` (duplicates counted) have a track of >= obs_th and occur in the
        frame's point3D_ids (localize_cv2.py:135, :195)."""
        rows = self.point_rows(valid)
        tl = np.where(rows >= 0, self.track_len[np.maximum(rows, 0)], 0)
        if (rows < 0).any():
            raise KeyError(int(valid[rows < 0][0]))
        v = valid[tl >= obs_th]
        return np.array([int(np.isin(v, np.asarray(self.images[int(d)].point3D_ids)).sum()) for d in connected], dtype=np.int64)

    def covisible_frames(self, frame_id, covisibility_frame=50, ref_3Dpoints=None, obs_th=0, pred_qvec=None, pred_tvec=None):
        """get_covisibility_frames (localize_cv2.py:120-169, the `obs` type): the frames sharing 3D points with frame_id, most
        shared first (equal counts in ascending id order: the reference's stable sort over np.unique's order); with a predicted
        pose a frame is set aside when it is >= 30 degrees or >= 30 units away or shares <= 30 points; covisibility_frame = 0
        means no limit; with <= 3 frames left the set-aside ones are appended (:162-166).  Returns a list of image ids."""
        valid, connected = self._observed(frame_id, ref_3Dpoints)
        counts = self._counts(valid, connected, obs_th)
        order = np.argsort(-counts, kind="stable")
        with_pose = pred_qvec is not None and pred_tvec is not None
        out, not_used = [], []
        for o in order:
            db_id, n = int(connected[o]), int(counts[o])
            if with_pose:
                im = self.images[db_id]
                q_error, t_error, _ = compute_pose_error(pred_qvec, pred_tvec, im.qvec, im.tvec)
                if q_error >= 30 or t_error >= 30 or n <= 30:
                    not_used.append(db_id)
                    continue
            out.append(db_id)
            if covisibility_frame > 0 and len(out) >= covisibility_frame:
                break
        if len(out) <= 3:
            for v in not_used:
                out.append(v)
                if len(out) >= covisibility_frame:
                    break
        return out

    def covisible_frames_by_pose(self, frame_id, pred_qvec, pred_tvec, covisibility_frame=50, q_th=5, obs_th=5, t_th=10, ref_3Dpoints=None):
        """get_covisibility_frames_by_pose (localize_cv2.py:172-233, the `pos` type): connected frames whose name holds neither
        'left' nor 'right' and whose rotation differs by <= q_th degrees from the predicted pose, nearest camera centre first; when
        fewer than covisibility_frame, filled up from the frames by shared points (left / right names still excluded).  t_th is
        accepted and unused, as in the reference."""
        valid, connected = self._observed(frame_id, ref_3Dpoints)
        named = np.array([not (self.images[int(d)].name.find("left") >= 0 or self.images[int(d)].name.find("right") >= 0)
                          for d in connected], dtype=bool)
        connected = connected[named]
        counts = self._counts(valid, connected, obs_th)
        db_ids, t_dists = [], []
        for d in connected:
            im = self.images[int(d)]
            q_error, t_error, _ = compute_pose_error(pred_qvec, pred_tvec, im.qvec, im.tvec)
            if q_error > q_th:
                continue
            db_ids.append(int(d))
            t_dists.append(t_error)
        out = []
        for did in np.argsort(t_dists):
            out.append(db_ids[did])
            if covisibility_frame > 0 and len(out) >= covisibility_frame:
                break
        if len(out) >= covisibility_frame:
            return out
        for o in np.argsort(-counts, kind="stable"):
            db_id = int(connected[o])
            if db_id in out:
                continue
            out.append(db_id)
            if covisibility_frame > 0 and len(out) >= covisibility_frame:
                break
        return out
