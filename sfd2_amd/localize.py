"""Caller-side mirror of it_loc/localize_cv2.py:511-560 feature_matching: mask the database
descriptors to those with a triangulated 3D point, early-out when 3 or fewer remain, call the
matcher, map the match indices back to the unmasked database indexing."""
import numpy as np


def feature_matching(desc_q, desc_db, matcher, label_q=None, label_db=None, db_3D_ids=None):
    with_label = (label_q is not None and label_db is not None)
    if with_label:
        raise NotImplementedError("label-aware matching is not on the shipped pipelines' path "
                                  "(it_loc/localize_cv2.py:714 with_label=False)")
    if db_3D_ids is None:
        return matcher({"descriptors0": desc_q, "descriptors1": desc_db})["matches0"]
    masks = (np.asarray(db_3D_ids) != -1)
    if np.sum(masks) <= 3:
        return np.ones((desc_q.shape[0],), dtype=int) * -1
    valid_ids = np.flatnonzero(masks)
    matches = np.array(matcher({"descriptors0": desc_q, "descriptors1": desc_db[masks]})["matches0"])
    hit = matches >= 0
    matches[hit] = valid_ids[matches[hit]]
    return matches


def feature_matching_batch(desc_q, desc_db_list, matcher, db_3D_ids_list):
    """The loop of match_cluster_2D (it_loc/localize_cv2.py:563-590) over one query's retrieved
    database images as ONE device call: per image the 3D-point mask, the <= 3 early-out
    (:536-537), mutual-NN matching and the index remap all happen inside sfd2_match_batch
    (row-selected database sets), so nothing is gathered or remapped on the host.
    matcher: sfd2_amd.matcher.Matcher.  Returns a list of [N] int arrays (matches per image)."""
    k = len(desc_db_list)
    out = [None] * k
    live, rows = [], []
    for i, (d, ids) in enumerate(zip(desc_db_list, db_3D_ids_list)):
        if ids is None:
            live.append(i); rows.append(None)
            continue
        valid = np.flatnonzero(np.asarray(ids) != -1).astype(np.int32)
        if len(valid) <= 3:
            out[i] = np.ones((desc_q.shape[0],), dtype=int) * -1
        else:
            live.append(i); rows.append(valid)
    if live:
        m, _ = matcher.match_batch(desc_q, [desc_db_list[i] for i in live], rows)
        for j, i in enumerate(live):
            out[i] = m[j].astype(int)
    return out


class StoreMatcher:
    """The localiser's matching loop against a FEATURE STORE with the database descriptor sets resident in HBM (round 5).

    it_loc/localize_cv2.py:563-590 reads, for every query and every retrieved database image, that image's descriptors from the
    feature file (:571-574), masks them to the key points with a 3D point, uploads both sets and runs one matcher call.
    Here a database image's set is read and converted ONCE (sfd2_desc_pack, through sfd2_amd.pipeline.ResidentSets: LRU in HBM,
    fp16 [n][128]) and a query costs one sfd2_match_batch whose row selections (the 3D-point masks) are the only per-query
    uploads.  Results equal feature_matching_batch on the same arrays (same conversion kernel, same matcher kernels).

    matcher: sfd2_amd.matcher.Matcher (mode nnm / nnr); feats: an open feature store (sfd2_amd.feature_io.open_store)."""

    def __init__(self, matcher, feats, cache_bytes=None, readers=4):
        from . import _lib
        from .pipeline import ResidentSets
        self.matcher = matcher
        self.ctx = _lib.default_context(matcher._device)
        self.sets = ResidentSets(self.ctx, feats, budget=cache_bytes, readers=readers)
        self._seq = 0

    def prefetch(self, db_names):
        """Start reading sets a coming query will need (host side; the conversion happens at first use)."""
        self.sets.prefetch(db_names)

    def match(self, desc_q, db_names, db_3D_ids_list=None):
        """desc_q: [N,128] array (float64 / float32) or the NAME of a set in the store; db_names: the retrieved database images;
        db_3D_ids_list[i]: that image's point3D ids (-1 = none) or None.  Returns a list of [N] int arrays (matches0 per image,
        indices into the UNMASKED database key points, -1 = no match) -- feature_matching's contract."""
        import ctypes
        from . import _lib
        k = len(db_names)
        ids_list = [None] * k if db_3D_ids_list is None else list(db_3D_ids_list)
        seq = self._seq
        self._seq += 1
        self.sets.completed_seq = seq - 1          # match() is synchronous: every earlier query has finished
        if isinstance(desc_q, str):
            qp, n0 = self.sets.get(desc_q, seq)
            q = _lib.DescSet(qp, n0, _lib.DT_F16, _lib.LAYOUT_ND, 1, None, 0, 0)
            keep_q = None
        else:
            keep_q = np.ascontiguousarray(desc_q)
            if keep_q.dtype not in (np.float64, np.float32):
                keep_q = keep_q.astype(np.float64)
            n0 = keep_q.shape[0]
            q = _lib.DescSet(keep_q.ctypes.data, n0, _lib.DT_F64 if keep_q.dtype == np.float64 else _lib.DT_F32, _lib.LAYOUT_ND, 0, None, 0, 0)
        out = [None] * k
        live, rows, sets = [], [], []
        for i, (name, ids) in enumerate(zip(db_names, ids_list)):
            r = None
            if ids is not None:
                r = np.flatnonzero(np.asarray(ids) != -1).astype(np.int32)
                if len(r) <= 3:                       # localize_cv2.py:536-537
                    out[i] = np.ones((n0,), dtype=int) * -1
                    continue
            p, n1 = self.sets.get(name, seq)
            if ids is not None and len(np.asarray(ids)) != n1:
                raise ValueError(f"{name}: {len(np.asarray(ids))} point ids for {n1} key points")
            live.append(i); rows.append(r); sets.append((p, n1))
        if live and n0 > 0:
            db = (_lib.DescSet * len(live))(*[_lib.DescSet(p, n1, _lib.DT_F16, _lib.LAYOUT_ND, 1, None if r is None else r.ctypes.data,
                                                           0 if r is None else len(r), 0) for (p, n1), r in zip(sets, rows)])
            m = np.empty((len(live), n0), dtype=np.int64)
            s = np.empty((len(live), n0), dtype=np.float32)
            conf = self.matcher._conf()
            _lib.check(self.ctx.lib.sfd2_match_batch(self.ctx.h, ctypes.byref(q), db, len(live), 128, ctypes.byref(conf), m.ctypes.data,
                                                     s.ctypes.data, 0, 0))
            for j, i in enumerate(live):
                out[i] = m[j].astype(int)
        else:
            for i in live:
                out[i] = np.ones((n0,), dtype=int) * -1
        return out

    def _match_on_device(self, map_index, desc_q, image_ids, seq, conf, keep):
        """One sfd2_match_batch of a query against image_ids, queued on the context's stream with the result left in HBM.  Returns
        (matches0 device tensor [rows][n0] or None, [(image id, row of matches0 or -1)], n0); keep collects what must outlive the
        launch."""
        import ctypes
        import torch
        from . import _lib
        if isinstance(desc_q, str):
            qp, n0 = self.sets.get(desc_q, seq)
            qs = _lib.DescSet(qp, n0, _lib.DT_F16, _lib.LAYOUT_ND, 1, None, 0, 0)
        else:
            a = np.ascontiguousarray(desc_q)
            if a.dtype not in (np.float64, np.float32):
                a = a.astype(np.float64)
            keep.append(a)
            n0 = a.shape[0]
            qs = _lib.DescSet(a.ctypes.data, n0, _lib.DT_F64 if a.dtype == np.float64 else _lib.DT_F32, _lib.LAYOUT_ND, 0, None, 0, 0)
        images, sets, rows = [], [], []
        for image_id in image_ids:
            im = map_index.images[image_id]
            ids = np.asarray(im.point3D_ids)
            r = np.flatnonzero(ids != -1).astype(np.int32)
            if ids.size == 0 or len(r) <= 3:
                images.append((image_id, -1))
                continue
            p, n1 = self.sets.get(im.name, seq)
            if ids.size != n1:
                raise ValueError(f"{im.name}: {ids.size} point ids for {n1} key points")
            images.append((image_id, len(sets)))
            sets.append((p, n1))
            rows.append(r)
        m = None
        if sets and n0 > 0:
            db = (_lib.DescSet * len(sets))(*[_lib.DescSet(p, n1, _lib.DT_F16, _lib.LAYOUT_ND, 1, r.ctypes.data, len(r), 0)
                                              for (p, n1), r in zip(sets, rows)])
            m = torch.empty((len(sets), n0), dtype=torch.int64, device=map_index.device)
            sc = torch.empty((len(sets), n0), dtype=torch.float32, device=map_index.device)
            keep += [rows, db, sc, qs]
            _lib.check(self.ctx.lib.sfd2_match_batch(self.ctx.h, ctypes.byref(qs), db, len(sets), 128, ctypes.byref(conf), m.data_ptr(),
                                                     sc.data_ptr(), 1, _lib.FLAG_ASYNC))
        else:
            images = [(i, -1) for i, _ in images]
        return m, images, n0

    def match_assemble(self, map_index, queries):
        """Matching and 2D-3D assembly on the device for a batch of queries: per query one sfd2_match_batch whose result stays in
        HBM, then ONE sfd2_assemble_2d3d for all of them behind it on the same stream.  map_index: sfd2_amd.covis.MapIndex;
        queries: dicts with desc_q (array or the name of a set in the store), kpq [N,2], scores [N] or None, image_ids (the database
        images, ids of map_index.images), obs_th, gate (None or (qvec, tvec, camera, radius)), optionally capacity.  An image with
        3 or fewer key points that have a 3D point never reaches the matcher (localize_cv2.py:537-538) and takes part as an image
        without matches, so image_idx indexes image_ids.  Returns per query what assemble_2d3d returns; equal to match() followed
        by match_cluster_2D."""
        if map_index.device is None:
            map_index.to_device(self.ctx.device)
        seq = self._seq
        self._seq += 1
        self.sets.completed_seq = seq - 1          # every earlier call has synchronised
        conf = self.matcher._conf()
        keep, jobs = [], []
        for q in queries:
            m, images, _ = self._match_on_device(map_index, q["desc_q"], q["image_ids"], seq, conf, keep)
            jobs.append(dict(matches0=m, images=images, kpq=q["kpq"], scores=q.get("scores"), obs_th=q.get("obs_th", 0), gate=q.get("gate"),
                             capacity=q.get("capacity")))
        return assemble_2d3d(self.ctx, map_index, jobs)

    def match_assemble_clusters(self, map_index, queries):
        """match_assemble for the cluster stage: queries are dicts with desc_q, kpq, clusters (a list of lists of image ids) and obs_th.
        Per query ONE sfd2_match_batch over the union of its clusters' images, each image once, and then ONE sfd2_assemble_2d3d for
        all clusters of all queries: a job per cluster whose images point into that query's shared matches0.  No gate, no scores.
        Returns per query a list over its clusters of what assemble_2d3d returns, plus 'image_ids'.  The library takes at most
        65535 jobs per call: callers bound their rounds (sfd2_amd.localizer.ROUND)."""
        if map_index.device is None:
            map_index.to_device(self.ctx.device)
        seq = self._seq
        self._seq += 1
        self.sets.completed_seq = seq - 1          # every earlier call has synchronised
        conf = self.matcher._conf()
        keep, jobs, spans = [], [], []
        for q in queries:
            union = list(dict.fromkeys(i for cl in q["clusters"] for i in cl))
            m, images, _ = self._match_on_device(map_index, q["desc_q"], union, seq, conf, keep)
            row = dict(images)
            spans.append((len(jobs), len(q["clusters"])))
            for cl in q["clusters"]:
                jobs.append(dict(matches0=m, images=[(i, row[i]) for i in cl], kpq=q["kpq"], scores=None, obs_th=q.get("obs_th", 0), gate=None,
                                 image_ids=list(cl)))
        res = assemble_2d3d(self.ctx, map_index, jobs)
        for r, j in zip(res, jobs):
            r["image_ids"] = j["image_ids"]
        return [res[o:o + n] for o, n in spans]

    def close(self):
        self.sets.close()


class AssembleError(RuntimeError):
    """sfd2_assemble_2d3d reported a job with a non-zero status; m and status hold every job's values."""

    def __init__(self, text, m, status):
        super().__init__(text)
        self.m, self.status = m, status


def assemble_2d3d(ctx, map_index, jobs, out_on_device=False):
    """sfd2_assemble_2d3d (include/sfd2_hip.h): jobs are dicts with matches0 (a device int64 torch tensor [rows][n], or None), images
    (a list of (image id of map_index, row of matches0 or -1)), kpq [n,2], scores [n] or None, obs_th, gate (None or (qvec, tvec,
    camera, radius)) and capacity (default k * n, which cannot overflow).  Returns per job a dict: points2D [m,2], points3D [m,3],
    point_row, query_idx, image_idx (int32 [m]), score (fp32 [m]), image_counts (int32 [k]), m -- numpy arrays, or torch tensors of
    `capacity` rows on the device with out_on_device.  Raises AssembleError when a job's status is not 0."""
    import ctypes
    from . import _lib
    from .pose import camera_model
    if map_index.device is None:
        map_index.to_device(ctx.device)
    table = map_index.point_table()
    arr = (_lib.AssembleJob * max(len(jobs), 1))()
    keep, outs = [], []
    if out_on_device:
        import torch

        def buf(shape, dt):
            t = torch.empty(shape, dtype={np.float64: torch.float64, np.int32: torch.int32, np.float32: torch.float32}[dt], device=map_index.device)
            return t, t.data_ptr()
    else:
        def buf(shape, dt):
            a = np.empty(shape, dtype=dt)
            return a, a.ctypes.data
    for j, job in zip(arr, jobs):
        kpq = np.ascontiguousarray(job["kpq"], dtype=np.float32).reshape(-1, 2)
        n, k = kpq.shape[0], len(job["images"])
        imgs = (_lib.AssembleImage * max(k, 1))()
        for a, (image_id, mrow) in zip(imgs, job["images"]):
            a.point_rows, a.n1 = map_index.device_rows(image_id)
            a.match_row = int(mrow)
        m0 = job.get("matches0")
        j.matches0 = None if m0 is None else m0.data_ptr()
        j.match_rows = 0 if m0 is None else int(m0.shape[0])
        if m0 is not None and (m0.dim() != 2 or m0.shape[1] != n or not m0.is_contiguous() or str(m0.dtype) != "torch.int64"):
            raise ValueError("matches0 must be a contiguous int64 [rows][n] device tensor")
        j.images, j.k, j.n, j.inputs_on_device = imgs, k, n, 0
        j.keypoints = kpq.ctypes.data
        sc = job.get("scores")
        if sc is not None:
            sc = np.ascontiguousarray(sc, dtype=np.float32).reshape(-1)
            if sc.size != n:
                raise ValueError(f"{sc.size} scores for {n} key points")
            j.scores = sc.ctypes.data
        j.obs_th = float(job.get("obs_th", 0))
        gate = job.get("gate")
        if gate is not None:
            qvec, tvec, cam, radius = gate
            j.gate = 1
            j.model, params = camera_model(cam)
            for i in range(8):
                j.params[i] = params[i]
            for i in range(4):
                j.qvec[i] = float(qvec[i])
            for i in range(3):
                j.tvec[i] = float(tvec[i])
            j.radius = float(radius)
        cap = job.get("capacity")
        cap = k * n if cap is None else int(cap)
        j.capacity = cap
        o = {"points2D": buf((cap, 2), np.float64), "points3D": buf((cap, 3), np.float64), "point_row": buf((cap,), np.int32),
             "query_idx": buf((cap,), np.int32), "image_idx": buf((cap,), np.int32), "score": buf((cap,), np.float32)}
        j.points2D, j.points3D, j.point_row = o["points2D"][1], o["points3D"][1], o["point_row"][1]
        j.query_idx, j.image_idx, j.score = o["query_idx"][1], o["image_idx"][1], o["score"][1]
        counts = np.zeros(max(k, 1), dtype=np.int32)
        j.image_counts = counts.ctypes.data
        keep += [kpq, sc, imgs, counts, m0]
        outs.append((o, counts, k))
    rc = ctx.lib.sfd2_assemble_2d3d(ctx.h, ctypes.byref(table), arr, len(jobs), 1 if out_on_device else 0, 0)
    if rc != 0:
        text = "libsfd2hip: " + ctx.lib.sfd2_last_error().decode("utf-8", "replace")
        if any(arr[i].status for i in range(len(jobs))):
            raise AssembleError(text, [arr[i].m for i in range(len(jobs))], [arr[i].status for i in range(len(jobs))])
        raise RuntimeError(text)
    res = []
    for i, (o, counts, k) in enumerate(outs):
        m = arr[i].m
        r = {name: (t if out_on_device else t[:m]) for name, (t, _) in o.items()}
        r["image_counts"] = counts[:k]
        r["m"] = m
        res.append(r)
    return res


def _gate_error(kp, xyz, gate):
    """The covisibility stage's reprojection gate (it_loc/localize_cv2.py:341-349): distance of the key point (no +0.5) from the 3D
    point projected with gate = (qvec, tvec, camera, radius)."""
    from .covis import reproject
    proj = reproject(np.asarray(xyz, dtype=np.float64).reshape(-1, 3), gate[0], gate[1], gate[2])
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.sum((np.asarray(kp) - proj) ** 2))


def match_cluster_2D(kpq, matches_list, db_point3D_ids_list, points3D, obs_th=0, db_names=None, gate=None):
    """it_loc/localize_cv2.py:563-650 match_cluster_2D on matches already computed (StoreMatcher.match / feature_matching_batch):
    matches_list[i] is database image i's matches0 (indices into its key points, -1 = none), db_point3D_ids_list[i] its point3D_ids.
    Applies the -1 skips, the obs_th rule on len(points3D[id].image_ids), the per-query-keypoint de-duplication of 3D ids and the
    +0.5 pixel offset (:647).  points3D: any mapping id -> object with .xyz and .image_ids (read_write_model's).  db_names: the keys
    of cluster_info (default: the image's position in the lists).  gate = (qvec, tvec, camera, radius): the same loop as the
    covisibility stage runs it (:286-360) -- after the de-duplication entry is made, a point whose projection lies more than
    radius pixels from the key point is dropped (`error > radius`, a NaN error is kept).  This is the host restatement of
    sfd2_assemble_2d3d.  Returns (cluster_info, mp3d [m,3], mkpq [m,2], mp3d_ids, q_ids);
    cluster_info[name] holds 'mkpq', 'qids', 'matches', 'mp_3d_ids', 'mp3d' (:637-643, without the database key points)."""
    kpq = np.asarray(kpq)
    all_mp3d, all_mkpq, all_mp3d_ids, all_q_ids = [], [], [], []
    outputs = {}
    valid = {}
    for i, (matches, ids) in enumerate(zip(matches_list, db_point3D_ids_list)):
        name = i if db_names is None else db_names[i]
        ids = np.asarray(ids)
        if ids.size == 0:                                    # :578-580
            continue
        matches = np.asarray(matches)
        mp3d, mp3d_ids, q_ids, mkpq, vm = [], [], [], [], []
        for idx in range(matches.shape[0]):
            m = matches[idx]
            if m == -1 or ids[m] == -1:
                continue
            id_3D = ids[m]
            if len(points3D[id_3D].image_ids) < obs_th:
                continue
            seen = valid.setdefault(idx, [])
            if id_3D in seen:
                continue
            seen.append(id_3D)
            if gate is not None and _gate_error(kpq[idx], points3D[id_3D].xyz, gate) > gate[3]:
                continue
            mp3d.append(points3D[id_3D].xyz)
            mp3d_ids.append(id_3D)
            all_mp3d_ids.append(id_3D)
            mkpq.append(kpq[idx])
            q_ids.append(idx)
            all_q_ids.append(idx)
            all_mkpq.append(kpq[idx])
            all_mp3d.append(points3D[id_3D].xyz)
            vm.append(m)
        outputs[name] = {"mkpq": mkpq, "qids": q_ids, "matches": np.array(vm, dtype=int), "mp_3d_ids": mp3d_ids,
                         "mp3d": np.array(mp3d, dtype=float).reshape(-1, 3)}
    all_mp3d = np.array(all_mp3d, float).reshape(-1, 3)
    all_mkpq = np.array(all_mkpq, float).reshape(-1, 2) + 0.5
    return outputs, all_mp3d, all_mkpq, all_mp3d_ids, all_q_ids


def _default_estimator(ransac):
    from . import pose as _pose

    def estimator(problems):
        return _pose.absolute_pose_estimation_batch(problems, **ransac)
    return estimator


def _default_refiner(problems):
    from . import pose as _pose
    return _pose.pose_refinement_batch(problems)


class Covis:
    """The settings of the covisibility stage (the `--do_covisible_opt` arguments of the reference's localiser) and what it runs
    on: map_index (sfd2_amd.covis.MapIndex), matcher and feature_file as pose_refinement_covisibility takes them.  opt_type must
    hold 'clu' (both call sites of localize_cv2.py test it), 'obs' or 'pos' for the frame selection and 'ref' for the refinement,
    e.g. 'clurefobs' (Aachen: 50 frames, radius 30), 'clurefpos' (RobotCar: 20, 20).  frames: 'host' or 'device', where a round's
    frame selections run (pose_refinement_covisibility_batch)."""

    def __init__(self, map_index, matcher, feature_file, opt_type="clurefobs", covisibility_frame=50, iters=1, radius=20, obs_th=3,
                 opt_th=12, estimator=None, refiner=None, frames="host"):
        if opt_type.find("clu") < 0:
            raise ValueError(f"opt_type {opt_type!r}: the covisibility stage runs for the 'clu' types only")
        self.map_index, self.matcher, self.feature_file = map_index, matcher, feature_file
        self.opt_type, self.covisibility_frame, self.iters, self.radius = opt_type, covisibility_frame, iters, radius
        self.obs_th, self.opt_th, self.estimator, self.refiner, self.frames = obs_th, opt_th, estimator, refiner, frames

    def refine(self, requests):
        """requests: a list of (qname, camera, db_frame_id, thresh, qvec, tvec); one batched run of the stage."""
        return pose_refinement_covisibility_batch(
            [dict(qname=q, cfg=cam, db_frame_id=f, thresh=th, qvec=qv, tvec=tv) for q, cam, f, th, qv, tv in requests],
            self.feature_file, self.map_index, self.matcher, covisibility_frame=self.covisibility_frame, iters=self.iters,
            obs_th=self.obs_th, opt_th=self.opt_th, radius=self.radius, opt_type=self.opt_type, estimator=self.estimator,
            refiner=self.refiner, frames=self.frames)


class Stage1:
    """What the cluster stage needs to run from image ids instead of matches computed beforehand -- the Covis idea applied to stage 1:
    map_index (sfd2_amd.covis.MapIndex), matcher and feature_file as Covis takes them.  With a StoreMatcher (anything with its
    match_assemble_clusters) a round's clusters are matched and assembled on the device; a callable matcher (qname, db_names,
    point3D_ids_list) -> matches0 per image keeps the host loop of match_cluster_2D."""

    def __init__(self, map_index, matcher, feature_file):
        self.map_index, self.matcher, self.feature_file = map_index, matcher, feature_file
        self.on_device = hasattr(matcher, "match_assemble_clusters")

    def assemble(self, requests):
        """requests: a list of (qname, kpq, cluster_ids, obs_th).  Returns per request the list over its clusters of
        (cluster_info, mp3d, mkpq, mp3d_ids, q_ids) as match_cluster_2D returns them; cluster_info holds 'qids' and 'mp_3d_ids' per
        database image, rebuilt from the job's per-image segments.  An image without key points has no entry (match_cluster_2D:
        ids.size == 0 -> continue); one with <= 3 key points that have a 3D point has an empty one."""
        mi = self.map_index
        res = self.matcher.match_assemble_clusters(mi, [dict(desc_q=qname, kpq=kpq, clusters=cluster_ids, obs_th=obs_th)
                                                        for qname, kpq, cluster_ids, obs_th in requests])
        out = []
        for per_query in res:
            prepared = []
            for r in per_query:
                ids3d = mi.point_ids[r["point_row"]]
                q_ids = r["query_idx"].copy()
                info, o = {}, 0
                for image_id, n in zip(r["image_ids"], r["image_counts"]):
                    im = mi.images[image_id]
                    if np.asarray(im.point3D_ids).size == 0:
                        continue
                    info[im.name] = {"qids": q_ids[o:o + n], "mp_3d_ids": ids3d[o:o + n]}
                    o += int(n)
                prepared.append((info, r["points3D"].copy(), r["points2D"].copy(), ids3d, q_ids))
            out.append(prepared)
        return out


def do_covisibility_clustering(frame_ids, all_images, points3D, device=0):
    """it_loc/localize_cv2.py:87-117 for one list of retrieved image ids, on the device (sfd2_covis_clusters): the clusters, largest
    first, equal sizes in order of creation.  Members are listed by ascending list position; the reference's member order is
    whatever set.pop() yields.  For many queries build one sfd2_amd.covis.MapIndex and call its clusters()."""
    from .covis import MapIndex
    return MapIndex(all_images, points3D).clusters([frame_ids], device=device)[0]


def _assemble(matcher, map_index, feature_file, jobs):
    """jobs: dicts with qname, kpq, score_q, db_ids, obs_th, gate.  matcher: a StoreMatcher or anything else with its match_assemble (device: one match launch per query, one
    sfd2_assemble_2d3d for all of them) or a callable (qname, db_names, point3D_ids_list) -> matches0 per image (then the host loop
    of match_cluster_2D).  Returns per job (mkpq [m,2], mp3d [m,3], 3D ids, query scores)."""
    if hasattr(matcher, "match_assemble"):
        res = matcher.match_assemble(map_index, [dict(desc_q=j["qname"], kpq=j["kpq"], scores=j["score_q"], image_ids=j["db_ids"],
                                                      obs_th=j["obs_th"], gate=j["gate"]) for j in jobs])
        return [(r["points2D"], r["points3D"], [int(v) for v in map_index.point_ids[r["point_row"]]], [s for s in r["score"]]) for r in res]
    out = []
    for j in jobs:
        ims = [map_index.images[d] for d in j["db_ids"]]
        ids_list = [np.asarray(im.point3D_ids) for im in ims]
        ml = matcher(j["qname"], [im.name for im in ims], ids_list)
        _, mp3d, mkpq, ids3d, q_ids = match_cluster_2D(j["kpq"], ml, ids_list, map_index.points3D, obs_th=j["obs_th"], gate=j["gate"])
        out.append((mkpq, mp3d, [int(v) for v in ids3d], [j["score_q"][q] for q in q_ids]))
    return out


def pose_refinement_covisibility_batch(tasks, feature_file, map_index, matcher, covisibility_frame=50, iters=1, obs_th=3, opt_th=12,
                                       radius=20, opt_type="ref", estimator=None, refiner=None, ref_3Dpoints=None, frames="host"):
    """pose_refinement_covisibility for many queries at once: tasks are dicts with qname, cfg, db_frame_id, thresh, qvec, tvec.  One
    match / assemble call, one estimator call and one refiner call per iteration for all of them; each result equals the single
    call's (the device calls are batch-independent).  frames: 'host' selects every task's covisible frames with
    MapIndex.covisible_frames / _by_pose, 'device' with ONE MapIndex.covisible_frames_batch call (sfd2_covis_frames) for all tasks;
    the lists are the same."""
    estimator = estimator or _default_estimator({})
    refiner = refiner or _default_refiner
    if frames not in ("host", "device"):
        raise ValueError(f"frames {frames!r}: 'host' or 'device'")
    for t in tasks:
        if t["qvec"] is None or t["tvec"] is None:
            raise ValueError("pose_refinement_covisibility needs the pose to refine (qvec, tvec)")
    if tasks and opt_type.find("obs") < 0 and opt_type.find("pos") < 0:
        raise ValueError(f"opt_type {opt_type!r} names no method for getting reference images ('obs' or 'pos')")
    selected = None
    if frames == "device" and tasks:
        selected = map_index.covisible_frames_batch(
            [dict(frame_id=t["db_frame_id"], qvec=t["qvec"], tvec=t["tvec"]) for t in tasks], kind="obs" if opt_type.find("obs") >= 0 else "pos",
            covisibility_frame=covisibility_frame, obs_th=obs_th, q_th=10, ref_3Dpoints=ref_3Dpoints)
    jobs = []
    for i, t in enumerate(tasks):
        if selected is not None:
            db_ids = selected[i]
        elif opt_type.find("obs") >= 0:
            db_ids = map_index.covisible_frames(t["db_frame_id"], covisibility_frame=covisibility_frame, ref_3Dpoints=ref_3Dpoints,
                                                obs_th=obs_th, pred_qvec=t["qvec"], pred_tvec=t["tvec"])
        else:
            db_ids = map_index.covisible_frames_by_pose(t["db_frame_id"], t["qvec"], t["tvec"], covisibility_frame=covisibility_frame,
                                                        ref_3Dpoints=ref_3Dpoints, q_th=10, t_th=10, obs_th=obs_th)
        f = feature_file[t["qname"]]
        jobs.append(dict(qname=t["qname"], kpq=f["keypoints"].__array__(), score_q=f["scores"].__array__(), db_ids=db_ids, obs_th=obs_th,
                         gate=(t["qvec"], t["tvec"], t["cfg"], radius)))
    asm = _assemble(matcher, map_index, feature_file, jobs) if jobs else []
    rets = estimator([(a[0], a[1], t["cfg"], opt_th) for a, t in zip(asm, tasks)]) if tasks else []      # opt_th, not thresh (:390)
    out = [None] * len(tasks)
    from .covis import reproject
    state = {}
    for i, (t, j, (mkpq, mp3d, ids3d, score_q), ret) in enumerate(zip(tasks, jobs, asm, rets)):
        ret = dict(ret)
        extra = {"mkpq": mkpq, "3D_ids": ids3d, "db_ids": j["db_ids"], "score_q": score_q}
        if not ret["success"]:                                                                            # :392-402
            ret.update(extra)
            ret.update({"qvec": t["qvec"], "tvec": t["tvec"], "inliers": [False for _ in range(mkpq.shape[0])], "num_inliers": 0})
            out[i] = ret
            continue
        inliers_rsac = np.asarray(ret["inliers"]).astype(bool)
        ret["num_inliers"] = np.sum(ret["inliers"])
        if opt_type.find("ref") >= 0 and np.sum(inliers_rsac) >= 10 and iters > 0:
            state[i] = dict(qvec=t["qvec"], tvec=t["tvec"], inl=inliers_rsac, extra=extra, ret=ret)
        else:
            ret.update(extra)
            out[i] = ret
    for _ in range(iters):
        if not state:
            break
        order = sorted(state)
        probs = []
        for i in order:
            st, (mkpq, mp3d, _, _) = state[i], asm[i]
            proj = reproject(mp3d, st["qvec"], st["tvec"], tasks[i]["cfg"])
            err = (mkpq - proj) ** 2
            with np.errstate(invalid="ignore"):
                err = np.sqrt(err[:, 0] + err[:, 1])
                st["mask"] = [bool(err[p] <= opt_th and st["inl"][p]) for p in range(err.shape[0])]
            probs.append((st["tvec"], st["qvec"], mkpq, mp3d, st["mask"], tasks[i]["cfg"]))
        for i, r in zip(order, refiner(probs)):
            st = state[i]
            r = dict(r)
            st["qvec"], st["tvec"] = r["qvec"], r["tvec"]
            r["inliers"] = st["mask"]
            r["num_inliers"] = np.sum(st["mask"])
            st["ret"] = r
    for i, st in state.items():
        st["ret"].update(st["extra"])
        out[i] = st["ret"]
    return out


def pose_refinement_covisibility(qname, cfg, feature_file, db_frame_id, map_index, thresh, matcher, covisibility_frame=50,
                                 ref_3Dpoints=None, iters=1, obs_th=3, opt_th=12, qvec=None, tvec=None, radius=20, opt_type="ref",
                                 estimator=None, refiner=None):
    """it_loc/localize_cv2.py:236-508 pose_refinement_covisibility: the frames covisible with db_frame_id (opt_type 'obs':
    MapIndex.covisible_frames, 'pos': covisible_frames_by_pose with q_th 10), the query matched against all of them, the 2D-3D
    correspondences assembled with the reprojection gate (radius, around the pose passed in), RANSAC, and the refinement.
    map_index stands for the reference's db_images / points3D pair; matcher: a StoreMatcher (device matching and assembly) or a
    callable (qname, db_names, point3D_ids_list) -> matches0 per image; estimator / refiner: replacements for
    pose.absolute_pose_estimation_batch / pose.pose_refinement_batch, taking their problem lists.  Returns the reference's dict:
    success qvec tvec inliers num_inliers mkpq 3D_ids db_ids score_q (no log_info, no plots).

    Reproduced from the reference as it is written:
      * RANSAC runs with opt_th, not thresh (:390); thresh is accepted and unused.
      * RANSAC's pose is NOT used: the refinement starts from the qvec / tvec passed in, and iteration 0's reprojection errors are
        computed with them (:406, :451).
      * refinement only when opt_type holds 'ref' and RANSAC has >= 10 inliers; the mask of iteration i is
        `error <= opt_th and RANSAC inlier`, the error under the pose of iteration i - 1.
      * RANSAC failure returns its dict with the pose passed in, an all-False inlier list and num_inliers 0 (:392-402).
      * when no refinement runs the dict returned is RANSAC's own, so the pose is then RANSAC's (:437-441, :503-508).
      * when it runs, success / qvec / tvec are the last pose_refinement's, inliers / num_inliers the last mask's (:496-497).
    Deviation: the min / median / max error statistics of :410 and :469, which raise on an empty inlier set, are not computed."""
    return pose_refinement_covisibility_batch([dict(qname=qname, cfg=cfg, db_frame_id=db_frame_id, thresh=thresh, qvec=qvec, tvec=tvec)],
                                              feature_file, map_index, matcher, covisibility_frame=covisibility_frame, iters=iters,
                                              obs_th=obs_th, opt_th=opt_th, radius=radius, opt_type=opt_type, estimator=estimator,
                                              refiner=refiner, ref_3Dpoints=ref_3Dpoints)[0]


def _cluster_steps(kpq, clusters, camera, thresh, inlier_th, points3D, obs_th, qname, covis, cluster_ids=None, stage1=None):
    """pose_from_clusters as a coroutine: yields ('estimate', problems) once and ('covis', request) at most once per visit of a call
    site, receives the results; returns what pose_from_clusters returns.  localize_queries drives many of these in rounds.  With
    cluster_ids (lists of image ids of stage1.map_index) instead of clusters the correspondences come from stage1: a device stage
    first yields ('assemble', request); a callable matcher is asked per cluster and match_cluster_2D runs here."""
    n_q = len(kpq)
    if cluster_ids is not None:
        if stage1 is None:
            raise ValueError("cluster_ids need a stage1 (sfd2_amd.localize.Stage1)")
        images = stage1.map_index.images
        first = images[cluster_ids[0][0]]
    else:
        first = clusters[0][0][0]
    best_results = {"tvec": None, "qvec": None, "num_inliers": 0, "single_num_inliers": 0, "db_id": -1, "order": -1, "qname": qname,
                    "optimize": False, "dbname": first.name, "ret_source": "", "inliers": []}
    if cluster_ids is not None and stage1.on_device:
        prepared = yield ("assemble", (qname, kpq, cluster_ids, obs_th))
    else:
        if cluster_ids is not None:
            clusters = []
            for cl in cluster_ids:
                ims = [images[i] for i in cl]
                clusters.append(list(zip(ims, stage1.matcher(qname, [im.name for im in ims], [np.asarray(im.point3D_ids) for im in ims]))))
        prepared = []
        for cl in clusters:
            info, mp3d, mkpq, mp3d_ids, q_ids = match_cluster_2D(kpq, [m for _, m in cl], [im.point3D_ids for im, _ in cl], points3D,
                                                                 obs_th=obs_th, db_names=[im.name for im, _ in cl])
            prepared.append((info, mp3d, mkpq, mp3d_ids, q_ids))
    live = [i for i, p in enumerate(prepared) if p[1].shape[0] >= 8]
    rets = dict(zip(live, (yield ("estimate", [(prepared[i][2], prepared[i][1], camera, thresh) for i in live])) if live else []))
    last = None
    for cluster_idx, (info, mp3d, mkpq, mp3d_ids, q_ids) in enumerate(prepared):
        if cluster_idx not in rets:
            continue
        ret = last = rets[cluster_idx]
        if not ret["success"]:
            continue
        inliers = ret["inliers"]
        q_p3d_ids = np.full(n_q, -1, dtype=np.int64)
        for idx, qid in enumerate(q_ids):
            if inliers[idx]:
                q_p3d_ids[qid] = mp3d_ids[idx]
        best_dbname, best_inliers = None, -1
        for db_name, ci in info.items():
            n = sum(1 for idx, qid in enumerate(ci["qids"]) if ci["mp_3d_ids"][idx] == q_p3d_ids[qid])
            if n > best_inliers:
                best_inliers, best_dbname = n, db_name
        keep = not (best_inliers < 8 or ret["num_inliers"] <= best_results["num_inliers"])
        upd = {"qvec": ret["qvec"], "tvec": ret["tvec"], "inlier": ret["inliers"], "num_inliers": ret["num_inliers"],
               "single_num_inliers": best_inliers, "dbname": best_dbname, "order": cluster_idx + 1}
        if "camera" in ret:                                     # the estimator estimated or refined the intrinsics
            upd["camera"] = ret["camera"]
        if keep:
            best_results.update(upd)
        if ret["num_inliers"] < inlier_th or best_inliers < 10:
            continue
        if not keep:
            best_results.update(upd)
        if covis is not None:                                   # :981-1014
            ret = last = yield ("covis", (qname, ret.get("camera", camera), covis.map_index.name_to_id[best_dbname], thresh, ret["qvec"],
                                          ret["tvec"]))                # (an estimated camera is the stage's cfg, held fixed there)
            if not ret["success"]:
                continue
        return ret["qvec"], ret["tvec"], ret["num_inliers"], best_results
    if best_results["num_inliers"] >= 10:
        if covis is not None:                                   # :1139-1265: refined from the kept pose, returned with 0 either way
            ret = yield ("covis", (qname, best_results.get("camera", camera), covis.map_index.name_to_id[best_results["dbname"]], thresh,
                                   best_results["qvec"], best_results["tvec"]))
            return ret["qvec"], ret["tvec"], 0, best_results
        src = last if (last is not None and last["success"]) else best_results
        return src["qvec"], src["tvec"], 0, best_results
    return first.qvec, first.tvec, -1, best_results


def _drive(gens, estimator, covis, stage1=None):
    """Runs the coroutines of _cluster_steps in rounds: the pending requests of one kind go out in one call."""
    results = [None] * len(gens)
    pending = {}
    for i, g in enumerate(gens):
        try:
            pending[i] = next(g)
        except StopIteration as e:
            results[i] = e.value
    while pending:
        answers = {}
        asm = [i for i in sorted(pending) if pending[i][0] == "assemble"]
        if asm:
            for i, r in zip(asm, stage1.assemble([pending[i][1] for i in asm])):
                answers[i] = r
        est = [i for i in sorted(pending) if pending[i][0] == "estimate"]
        if est:
            flat = [p for i in est for p in pending[i][1]]
            got = estimator(flat) if flat else []
            o = 0
            for i in est:
                n = len(pending[i][1])
                answers[i] = got[o:o + n]
                o += n
        cov = [i for i in sorted(pending) if pending[i][0] == "covis"]
        if cov:
            for i, r in zip(cov, covis.refine([pending[i][1] for i in cov])):
                answers[i] = r
        nxt = {}
        for i, a in answers.items():
            try:
                nxt[i] = gens[i].send(a)
            except StopIteration as e:
                results[i] = e.value
        pending = nxt
    return results


def pose_from_clusters(kpq, clusters, camera, thresh, inlier_th=50, *, points3D, obs_th=3, qname=None, estimator=None, covis=None,
                       cluster_ids=None, stage1=None, **ransac):
    """The initialisation loop of it_loc/localize_cv2.py:653-1273 pose_from_cluster_with_matcher, on matches already computed.
    clusters: a list over the retrieved clusters, each a list of (db_image, matches0) pairs (db_image with
    .name, .qvec, .tvec, .point3D_ids as read_write_model returns them; matches0 from StoreMatcher.match / feature_matching_batch).

    Every cluster with >= 8 correspondences (:719) goes into ONE absolute_pose_estimation_batch call (estimator: a replacement
    taking a list of (points2D, points3D, camera, thresh) and returning pose dicts; **ransac goes to the default one, the options
    for a query without intrinsics included: estimate_focal_length, refine_focal_length, refine_extra_params, ...; the kept
    result then carries 'camera', and a covis stage takes that camera, held fixed, as its cfg).  The
    sequential decisions are then replayed in cluster order: best_inliers per db image (:742-760), keep / continue (:930-966), the
    first success returns its num_inliers (:1124-1130); otherwise, when the kept result has >= 10 inliers, the pose of the LAST
    estimate made is returned with 0, as the reference does (:1132-1265 reads `ret`; if that estimate failed, the kept pose is
    used); otherwise the first db image's pose with -1 (:1267-1273).  Returns (qvec, tvec, n, best_results).

    covis: None is do_covisility_opt=False.  A Covis replays the two call sites of pose_refinement_covisibility: after a successful
    cluster (:981-1014) the pose is refined from the cluster's best database image -- a failed refinement goes on to the next
    cluster, a successful one returns its pose and num_inliers -- and on the fallback path (:1139-1265) the kept pose is refined
    and returned with 0 whether or not the refinement succeeded.  qname then names the query's set in covis.feature_file.

    cluster_ids + stage1 (a Stage1) replace clusters (pass None): lists of image ids, matched and assembled by the stage."""
    if estimator is None:
        estimator = _default_estimator(ransac)
    return _drive([_cluster_steps(kpq, clusters, camera, thresh, inlier_th, points3D, obs_th, qname, covis, cluster_ids, stage1)], estimator,
                  covis, stage1)[0]


def localize_queries(queries, thresh, inlier_th=50, *, points3D, obs_th=3, estimator=None, covis=None, stage1=None, **ransac):
    """pose_from_clusters for many queries in rounds: queries is a list of dicts with kpq, clusters, camera and qname.  Stage 1 of
    all queries is one estimator call; then every covisibility refinement pending in a round is one match / assemble / estimate /
    refine call each, until no query is pending.  Every result equals the per-query call's exactly.

    A query may give cluster_ids (a list of lists of image ids) instead of clusters; stage1 (a Stage1) then matches the query named
    qname against them.  On the device that is, for all such queries together, one sfd2_match_batch per query over the union of its
    clusters' images and ONE sfd2_assemble_2d3d with a job per cluster, before the one estimator call."""
    if estimator is None:
        estimator = _default_estimator(ransac)
    gens = [_cluster_steps(q["kpq"], q.get("clusters"), q["camera"], thresh, inlier_th, points3D, obs_th, q.get("qname"), covis,
                           q.get("cluster_ids"), stage1) for q in queries]
    return _drive(gens, estimator, covis, stage1)
