"""The SfM map on the device: hloc/triangulation.py without COLMAP.  From a reference model (cameras and posed images), the feature
store and the match store to sfm_dir/{cameras,images,points3D}.bin and statics.txt, the map sfd2_amd.covis.MapIndex and
sfd2_amd.localize read.  The reference shells out to `colmap matches_importer` and `colmap point_triangulator` with the poses and the
intrinsics fixed (triangulation.py:114-147); here the three stages run through include/sfd2_hip.h:

  verify_pairs      sfd2_verify_matches_batch: with the poses given the relative pose of a pair is known, so a match is kept when its
                    point-to-epipolar-line distance is <= max_error / mean focal in both images, a pair when >= min_num_inliers stay.
  build_tracks      sfd2_build_tracks: connected components over (image, key point) nodes, label = smallest node, CSR of the tracks.
  triangulate       sfd2_triangulate_tracks: hypotheses from pairs of observations, angular-error support, Levenberg-Marquardt on
                    the point, completion and filter by reprojection error, up to four points per component.

Defaults (this project's choice, modelled on COLMAP's options; there is no COLMAP here to compare against): max_error 4 px,
min_num_inliers 15, min_tri_angle 1.5 deg, create_max_angle_error 2 deg, filter_max_reproj_error 4 px, seed 0.  Deviations from
COLMAP: known-pose verification instead of two-view RANSAC (a pair whose reference poses are wrong is rejected, not re-estimated),
no merging or re-triangulation rounds, no adjustment of poses or intrinsics, no database.db.  Key points are taken as float32 (as
COLMAP's database stores them) plus the +0.5 of triangulation.py:64.  Nothing here computes on the CPU: without a GPU the stages
raise."""
import argparse
import ctypes
import logging
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

try:        # torch's HIP runtime first (see sfd2_amd/jpeg.py)
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    pass

from . import _lib, colmap_io, feature_io
from .match_features import names_to_pair
from .pose import camera_model

DEFAULTS = dict(max_error=4.0, min_num_inliers=15, min_tri_angle=1.5, create_max_angle_error=2.0, filter_max_reproj_error=4.0,
                seed=0, max_refine_iterations=50, max_rounds=64)
READ_THREADS = 16
STAT_KEYS = ("mean_reproj_error", "mean_track_length", "num_observations", "num_observations_per_image", "num_reg_images", "num_sparse_points")


def make_views(cameras, images, image_ids=None):
    """(sorted image ids, ctypes array of sfd2_tri_view in that order)."""
    ids = sorted(images) if image_ids is None else list(image_ids)
    arr = (_lib.TriView * max(len(ids), 1))()
    for k, iid in enumerate(ids):
        im = images[iid]
        mid, params = camera_model(cameras[im.camera_id])
        arr[k].model = mid
        for i in range(8):
            arr[k].params[i] = params[i]
        q, t = np.asarray(im.qvec, dtype=np.float64).reshape(4), np.asarray(im.tvec, dtype=np.float64).reshape(3)
        if not (np.isfinite(q).all() and np.isfinite(t).all()):
            raise ValueError(f"image {iid}: non-finite pose")
        for i in range(4):
            arr[k].qvec[i] = q[i]
        for i in range(3):
            arr[k].tvec[i] = t[i]
    return ids, arr


def keypoint_table(image_ids, keypoints):
    """(offsets int64 [n + 1], key points float32 [N, 2]) of the per-image arrays concatenated in image_ids order."""
    kps = [np.ascontiguousarray(np.asarray(keypoints[i], dtype=np.float32).reshape(-1, 2)) for i in image_ids]
    off = np.zeros(len(kps) + 1, dtype=np.int64)
    np.cumsum([len(k) for k in kps], out=off[1:])
    allk = np.concatenate(kps) if kps else np.zeros((0, 2), np.float32)
    if not np.isfinite(allk).all():
        raise ValueError("non-finite key points")
    return off, np.ascontiguousarray(allk)


def _pack_matches(pair_matches, index):
    pv = np.zeros((len(pair_matches), 2), dtype=np.int32)
    ms, off = [], np.zeros(len(pair_matches) + 1, dtype=np.int64)
    for p, (i0, i1, m) in enumerate(pair_matches):
        pv[p] = index[i0], index[i1]
        m = np.asarray(m).reshape(-1, 2).astype(np.int32)
        ms.append(m)
        off[p + 1] = off[p] + len(m)
    return pv, off, np.ascontiguousarray(np.concatenate(ms) if ms else np.zeros((0, 2), np.int32))


def verify_pairs(cameras, images, keypoints, pair_matches, max_error=DEFAULTS["max_error"], min_num_inliers=DEFAULTS["min_num_inliers"],
                 device=0):
    """pair_matches: [(image id 0, image id 1, matches [m, 2] = key point in 0, key point in 1)].  Returns (matches int32 [M, 2] of all
    pairs concatenated with the rejected rows (-1, -1), offsets int64 [n_pairs + 1], counts int32 [n_pairs] = survivors of a pair before
    the min_num_inliers rule)."""
    ids, views = make_views(cameras, images)
    index = {iid: k for k, iid in enumerate(ids)}
    kp_off, kp = keypoint_table(ids, keypoints)
    pv, off, m = _pack_matches(pair_matches, index)
    counts = np.zeros(max(len(pair_matches), 1), dtype=np.int32)
    status = np.zeros(max(len(pair_matches), 1), dtype=np.int32)
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_verify_matches_batch(ctx.h, views, len(ids), kp_off.ctypes.data, kp.ctypes.data, pv.ctypes.data, off.ctypes.data,
                                                 len(pair_matches), m.ctypes.data, float(max_error), int(min_num_inliers), counts.ctypes.data,
                                                 status.ctypes.data, 0))
    return m, off, counts[:len(pair_matches)]


def build_tracks(n_nodes, edges, max_rounds=DEFAULTS["max_rounds"], device=0):
    """edges int [E, 2] over nodes 0..n_nodes-1 (rows with a negative end are skipped).  Returns (labels int32 [n_nodes] = smallest
    node of the component, track_offsets int32 [T + 1], track_nodes int32): the components of >= 2 nodes by label, nodes ascending.
    RuntimeError when the hooking rounds do not converge within max_rounds."""
    n_nodes = int(n_nodes)
    e = np.ascontiguousarray(np.asarray(edges).reshape(-1, 2).astype(np.int32))
    labels = np.zeros(max(n_nodes, 1), dtype=np.int32)
    t_off = np.zeros(n_nodes // 2 + 2, dtype=np.int32)
    t_nodes = np.zeros(max(n_nodes, 1), dtype=np.int32)
    nt, nn = ctypes.c_int64(0), ctypes.c_int64(0)
    status = np.zeros(2, dtype=np.int32)
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_build_tracks(ctx.h, n_nodes, e.ctypes.data, len(e), int(max_rounds), labels.ctypes.data, t_off.ctypes.data,
                                         t_nodes.ctypes.data, ctypes.byref(nt), ctypes.byref(nn), status.ctypes.data, 0))
    return labels[:n_nodes], t_off[:nt.value + 1].copy(), t_nodes[:nn.value].copy()


def triangulate(views, n_views, track_offsets, track_labels, obs_view, obs_xy, min_tri_angle=DEFAULTS["min_tri_angle"],
                create_max_angle_error=DEFAULTS["create_max_angle_error"], filter_max_reproj_error=DEFAULTS["filter_max_reproj_error"],
                seed=DEFAULTS["seed"], max_refine_iterations=DEFAULTS["max_refine_iterations"], device=0):
    """views: make_views()'s array; track t = observations track_offsets[t]..track_offsets[t + 1] of (obs_view, obs_xy float32 as
    stored).  Returns {'xyz' [T, 4, 3], 'error' [T, 4], 'n_obs' [T, 4] (0 = no point), 'obs_point' int8 [O] (pass or -1), 'status' [T]}."""
    off = np.ascontiguousarray(track_offsets, dtype=np.int64)
    lab = np.ascontiguousarray(track_labels, dtype=np.int64)
    ov = np.ascontiguousarray(obs_view, dtype=np.int32)
    xy = np.ascontiguousarray(np.asarray(obs_xy, dtype=np.float32).reshape(-1, 2))
    T = len(off) - 1
    if len(lab) != T or len(ov) != len(xy) or (T > 0 and off[-1] != len(ov)):
        raise ValueError("track_offsets, track_labels and the observation arrays do not fit together")
    if not np.isfinite(xy).all():
        raise ValueError("non-finite observations")
    P = _lib.TRI_MAX_POINTS
    out = {"xyz": np.zeros((T, P, 3)), "error": np.zeros((T, P)), "n_obs": np.zeros((T, P), dtype=np.int32),
           "obs_point": np.full(len(ov), -1, dtype=np.int8), "status": np.zeros(T, dtype=np.int32)}
    conf = _lib.TriConf(float(min_tri_angle), float(create_max_angle_error), float(filter_max_reproj_error), int(seed) & (2 ** 64 - 1),
                        int(max_refine_iterations), 0)
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_triangulate_tracks(ctx.h, views, int(n_views), off.ctypes.data, lab.ctypes.data, T, ov.ctypes.data, xy.ctypes.data,
                                               ctypes.byref(conf), out["xyz"].ctypes.data, out["error"].ctypes.data, out["n_obs"].ctypes.data,
                                               out["obs_point"].ctypes.data, out["status"].ctypes.data, 0))
    return out


def assemble_model(images, image_ids, kp_off, kp, track_offsets, track_nodes, tri):
    """The COLMAP dicts from the stage outputs: point ids 1-based in (label, pass) order; every image carries its key points (+0.5) and
    point3D ids (-1 = none)."""
    P = _lib.TRI_MAX_POINTS
    slot_live = tri["n_obs"].reshape(-1) > 0
    slot_id = np.where(slot_live, np.cumsum(slot_live), -1).astype(np.int64)            # tracks are ordered by label already
    T = len(track_offsets) - 1
    obs_track = np.repeat(np.arange(T, dtype=np.int64), np.diff(track_offsets))
    taken = tri["obs_point"] >= 0
    obs_pid = np.full(len(track_nodes), -1, dtype=np.int64)
    obs_pid[taken] = slot_id[obs_track[taken] * P + tri["obs_point"][taken].astype(np.int64)]
    node_pid = np.full(int(kp_off[-1]), -1, dtype=np.int64)
    node_pid[track_nodes[taken]] = obs_pid[taken]
    out_images = {}
    for k, iid in enumerate(image_ids):
        im = images[iid]
        lo, hi = int(kp_off[k]), int(kp_off[k + 1])
        out_images[iid] = colmap_io.Image(iid, np.asarray(im.qvec, dtype=np.float64), np.asarray(im.tvec, dtype=np.float64), im.camera_id,
                                          im.name, kp[lo:hi].astype(np.float64) + 0.5, node_pid[lo:hi].copy())
    sel = np.nonzero(taken)[0]
    sel = sel[np.argsort(obs_pid[sel], kind="stable")]                                   # by point, nodes ascending inside
    nodes = track_nodes[sel].astype(np.int64)
    view = np.searchsorted(kp_off, nodes, side="right") - 1
    img_ids = np.asarray(image_ids, dtype=np.int64)[view] if len(view) else np.zeros(0, np.int64)
    idx = nodes - kp_off[view]
    bounds = np.concatenate([[0], np.cumsum(tri["n_obs"].reshape(-1)[slot_live])]).astype(np.int64)
    xyz, err = tri["xyz"].reshape(-1, 3)[slot_live], tri["error"].reshape(-1)[slot_live]
    points3D = {}
    for r in range(len(xyz)):
        a, b = bounds[r], bounds[r + 1]
        points3D[r + 1] = colmap_io.Point3D(r + 1, xyz[r].copy(), np.zeros(3, np.uint8), float(err[r]), img_ids[a:b].astype(np.int32),
                                            idx[a:b].astype(np.int32))
    return out_images, points3D


def triangulate_model(cameras, images, keypoints, pair_matches, skip_geometric_verification=False, device=0, timings=None, **options):
    """cameras, images: the reference model's dicts; keypoints: image id -> [n, 2] as the feature store holds them; pair_matches:
    [(image id 0, image id 1, matches [m, 2])].  options: DEFAULTS.  Returns (images, points3D) as colmap_io writes them."""
    import time
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown options {sorted(unknown)}")
    o = dict(DEFAULTS, **options)
    ids, views = make_views(cameras, images)
    index = {iid: k for k, iid in enumerate(ids)}
    kp_off, kp = keypoint_table(ids, keypoints)
    t0 = time.perf_counter()
    if skip_geometric_verification:
        pv, off, m = _pack_matches(pair_matches, index)
        if len(m) and ((m[:, 0] >= np.repeat(np.diff(kp_off)[pv[:, 0]], np.diff(off))) | (m[:, 1] >= np.repeat(np.diff(kp_off)[pv[:, 1]], np.diff(off)))).any():
            raise ValueError("a match index beyond its image's key points")
    else:
        m, off, _ = verify_pairs(cameras, images, keypoints, pair_matches, o["max_error"], o["min_num_inliers"], device)
        pv = np.array([[index[a], index[b]] for a, b, _ in pair_matches], dtype=np.int32).reshape(-1, 2)
    t1 = time.perf_counter()
    live = (m[:, 0] >= 0) & (m[:, 1] >= 0) if len(m) else np.zeros(0, bool)
    n_per = np.diff(off)
    edges = np.stack([np.repeat(kp_off[pv[:, 0]], n_per) + m[:, 0], np.repeat(kp_off[pv[:, 1]], n_per) + m[:, 1]], 1)[live] if len(m) else np.zeros((0, 2), np.int64)
    labels, t_off, t_nodes = build_tracks(int(kp_off[-1]), edges, o["max_rounds"], device)
    t2 = time.perf_counter()
    nodes = t_nodes.astype(np.int64)
    obs_view = (np.searchsorted(kp_off, nodes, side="right") - 1).astype(np.int32)
    tri = triangulate(views, len(ids), t_off, t_nodes[t_off[:-1]] if len(t_off) > 1 else np.zeros(0, np.int64), obs_view, kp[nodes],
                      o["min_tri_angle"], o["create_max_angle_error"], o["filter_max_reproj_error"], o["seed"], o["max_refine_iterations"], device)
    t3 = time.perf_counter()
    if timings is not None:
        timings.update(verify_s=t1 - t0, tracks_s=t2 - t1, triangulate_s=t3 - t2, n_pairs=len(pair_matches), n_matches=int(len(m)),
                       n_verified=int(live.sum()), n_tracks=len(t_off) - 1)
    return assemble_model(images, ids, kp_off, kp, t_off, t_nodes, tri)


def model_statistics(images, points3D):
    """The six figures the reference takes from `colmap model_analyzer` (triangulation.py:149-165)."""
    n_obs = int(sum(len(p.image_ids) for p in points3D.values()))
    n_pts = len(points3D)
    return {"num_reg_images": len(images), "num_sparse_points": n_pts, "num_observations": n_obs,
            "mean_track_length": n_obs / n_pts if n_pts else 0.0, "num_observations_per_image": n_obs / len(images) if images else 0.0,
            "mean_reproj_error": float(np.mean([p.error for p in points3D.values()])) if n_pts else 0.0}


def read_inputs(images, pairs_path, features_path, matches_path, min_match_score=None):
    """Key points of every image of the model and the matches of the pair list, with the reference's rules (triangulation.py:57-107):
    pairs with an image outside the model are skipped, as is a pair seen before in either order; a pair the match store lacks is an
    error; matches0 > -1, and above min_match_score when one is given.  At most READ_THREADS reader threads."""
    name_to_id = {im.name: i for i, im in images.items()}
    with open(str(pairs_path), "r") as f:
        pairs = [p.split() for p in f.readlines()]
    feats = feature_io.open_store(features_path, "r")
    store = feature_io.open_store(matches_path, "r")
    try:
        def read_kp(item):
            iid, name = item
            return iid, np.asarray(feats[name]["keypoints"].__array__(), dtype=np.float32).reshape(-1, 2)[:, :2]

        todo, matched = [], set()
        for name0, name1 in pairs:
            if name0 not in name_to_id or name1 not in name_to_id:
                continue
            id0, id1 = name_to_id[name0], name_to_id[name1]
            if len({(id0, id1), (id1, id0)} & matched) > 0:
                continue
            pair = names_to_pair(name0, name1)
            if pair not in store:
                raise ValueError(f"Could not find pair {(name0, name1)}... Maybe you matched with a different list of pairs? "
                                 f"Reverse in file: {names_to_pair(name1, name0) in store}.")
            todo.append((id0, id1, pair))
            matched |= {(id0, id1), (id1, id0)}

        def read_pair(item):
            id0, id1, pair = item
            g = store[pair]
            matches = np.asarray(g["matches0"].__array__()).reshape(-1)
            valid = matches > -1
            if min_match_score:
                valid = valid & (np.asarray(g["matching_scores0"].__array__()).reshape(-1) > min_match_score)
            return id0, id1, np.stack([np.where(valid)[0], matches[valid]], -1).astype(np.int32)

        with ThreadPoolExecutor(max_workers=READ_THREADS) as pool:
            keypoints = dict(pool.map(read_kp, [(i, im.name) for i, im in images.items()]))
            pair_matches = list(pool.map(read_pair, todo))
    finally:
        feats.close()
        store.close()
    return keypoints, pair_matches


def main(sfm_dir, reference_sfm_model, image_dir, pairs, features, matches, colmap_path=None, skip_geometric_verification=False,
         min_match_score=None, **options):
    """hloc/triangulation.py main(): image_dir and colmap_path are accepted and unused.  Writes sfm_dir/{cameras,images,points3D}.bin and
    statics.txt; returns the statistics."""
    sfm_dir, reference_sfm_model = Path(sfm_dir), Path(reference_sfm_model)
    assert reference_sfm_model.exists(), reference_sfm_model
    assert Path(pairs).exists(), pairs
    sfm_dir.mkdir(parents=True, exist_ok=True)
    cameras = colmap_io.read_cameras_binary(reference_sfm_model / "cameras.bin")
    images = colmap_io.read_images_binary(reference_sfm_model / "images.bin")
    keypoints, pair_matches = read_inputs(images, pairs, features, matches, min_match_score)
    logging.info("Triangulating %d pairs over %d images...", len(pair_matches), len(images))
    out_images, points3D = triangulate_model(cameras, images, keypoints, pair_matches, skip_geometric_verification, **options)
    colmap_io.write_model(cameras, out_images, points3D, sfm_dir)
    stats = model_statistics(out_images, points3D)
    with open(sfm_dir / "statics.txt", "w") as f:
        for k in sorted(stats.keys()):
            f.write("{:s} {:4f}".format(k, stats[k]) + "\n")
    logging.info("Statistics: %s", stats)
    return stats


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--sfm_dir", type=Path, required=True)
    parser.add_argument("--reference_sfm_model", type=Path, required=True)
    parser.add_argument("--image_dir", type=Path, required=True)
    parser.add_argument("--pairs", type=Path, required=True)
    parser.add_argument("--features", type=Path, required=True)
    parser.add_argument("--matches", type=Path, required=True)
    parser.add_argument("--colmap_path", type=Path, default="colmap")
    parser.add_argument("--skip_geometric_verification", action="store_true")
    parser.add_argument("--min_match_score", type=float)
    args = parser.parse_args()
    main(**args.__dict__)
