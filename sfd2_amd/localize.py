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

    def close(self):
        self.sets.close()


def match_cluster_2D(kpq, matches_list, db_point3D_ids_list, points3D, obs_th=0, db_names=None):
    """it_loc/localize_cv2.py:563-650 match_cluster_2D on matches already computed (StoreMatcher.match / feature_matching_batch):
    matches_list[i] is database image i's matches0 (indices into its key points, -1 = none), db_point3D_ids_list[i] its point3D_ids.
    Applies the -1 skips, the obs_th rule on len(points3D[id].image_ids), the per-query-keypoint de-duplication of 3D ids and the
    +0.5 pixel offset (:647).  points3D: any mapping id -> object with .xyz and .image_ids (read_write_model's).  db_names: the keys
    of cluster_info (default: the image's position in the lists).  Returns (cluster_info, mp3d [m,3], mkpq [m,2], mp3d_ids, q_ids);
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


def pose_from_clusters(kpq, clusters, camera, thresh, inlier_th=50, *, points3D, obs_th=3, qname=None, estimator=None, **ransac):
    """The initialisation loop of it_loc/localize_cv2.py:653-1273 pose_from_cluster_with_matcher with do_covisility_opt=False, on
    matches already computed.  clusters: a list over the retrieved clusters, each a list of (db_image, matches0) pairs (db_image with
    .name, .qvec, .tvec, .point3D_ids as read_write_model returns them; matches0 from StoreMatcher.match / feature_matching_batch).

    Every cluster with >= 8 correspondences (:719) goes into ONE absolute_pose_estimation_batch call (estimator: a replacement
    taking a list of (points2D, points3D, camera, thresh) and returning pose dicts; **ransac goes to the default one).  The
    sequential decisions are then replayed in cluster order: best_inliers per db image (:742-760), keep / continue (:930-966), the
    first success returns its num_inliers (:1124-1130); otherwise, when the kept result has >= 10 inliers, the pose of the LAST
    estimate made is returned with 0, as the reference does (:1132-1265 reads `ret`; if that estimate failed, the kept pose is
    used); otherwise the first db image's pose with -1 (:1267-1273).  Returns (qvec, tvec, n, best_results)."""
    if estimator is None:
        from . import pose as _pose

        def estimator(problems):
            return _pose.absolute_pose_estimation_batch(problems, **ransac)
    n_q = len(kpq)
    first = clusters[0][0][0]
    best_results = {"tvec": None, "qvec": None, "num_inliers": 0, "single_num_inliers": 0, "db_id": -1, "order": -1, "qname": qname,
                    "optimize": False, "dbname": first.name, "ret_source": "", "inliers": []}
    prepared = []
    for cl in clusters:
        info, mp3d, mkpq, mp3d_ids, q_ids = match_cluster_2D(kpq, [m for _, m in cl], [im.point3D_ids for im, _ in cl], points3D,
                                                             obs_th=obs_th, db_names=[im.name for im, _ in cl])
        prepared.append((info, mp3d, mkpq, mp3d_ids, q_ids))
    live = [i for i, p in enumerate(prepared) if p[1].shape[0] >= 8]
    rets = dict(zip(live, estimator([(prepared[i][2], prepared[i][1], camera, thresh) for i in live]) if live else []))
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
        if keep:
            best_results.update(upd)
        if ret["num_inliers"] < inlier_th or best_inliers < 10:
            continue
        if not keep:
            best_results.update(upd)
        return ret["qvec"], ret["tvec"], ret["num_inliers"], best_results
    if best_results["num_inliers"] >= 10:
        src = last if (last is not None and last["success"]) else best_results
        return src["qvec"], src["tvec"], 0, best_results
    return first.qvec, first.tvec, -1, best_results
