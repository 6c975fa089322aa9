"""The SfM map stages (sfd2_amd.triangulation) on a synthetic scene of configurable size: cameras of the four models on a trajectory,
points in a slab in front of them, 1 px noise, clutter key points, pairs inside a window, a share of false matches.  Writes the
stores and the reference model to a scratch directory, then times: reading the stores, verification, tracks, triangulation, writing
the model; reports pairs/s, matches/s and tracks/s.  No speed ratio: there is no COLMAP here and no earlier path to compare with.

    python tools/triangulate_bench.py [--images 200] [--points 60000] [--window 10] [--reps 3] [--out profiles/triangulate_bench.json]

Kernel times come from a kernel trace of the same tool (no counters in that run):
    rocprofv3 --kernel-trace --stats -d DIR -o tri -- python tools/triangulate_bench.py --reps 1"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_scene(n_images, n_points, window, false_share, clutter_share, seed):
    import pose_ref as pr
    import tri_ref as tr
    rs = np.random.RandomState(seed)
    cameras = {m + 1: tr.Cam(id=m + 1, **pr.camera(tr.MODELS[m])) for m in range(4)}
    span = float(n_images - 1)
    X = np.stack([rs.uniform(-3, span + 3, n_points), rs.uniform(-3.5, 3.5, n_points), rs.uniform(5, 20, n_points)], 1)
    images, keypoints, truth = {}, {}, {}
    for i in range(n_images):
        c = np.array([float(i), 0.3 * np.sin(0.9 * i), 0.2 * np.cos(0.7 * i)])
        q, t = tr._look_at(c, np.array([i + rs.uniform(-0.5, 0.5), rs.uniform(-0.3, 0.3), 14.0]), rs.uniform(-0.05, 0.05))
        images[i + 1] = tr.Img(i + 1, q, t, i % 4 + 1, f"db/img{i:05d}.jpg")
        cam = cameras[i % 4 + 1]
        near = np.nonzero(np.abs(X[:, 0] - i) < 12)[0]
        px, z = pr.project(cam, q, t, X[near])
        vis = (z > 0) & (px[:, 0] > 5) & (px[:, 0] < cam["width"] - 5) & (px[:, 1] > 5) & (px[:, 1] < cam["height"] - 5) & (rs.uniform(size=len(near)) < 0.8)
        n_cl = int(clutter_share * vis.sum())
        pts = np.concatenate([px[vis] + rs.standard_normal((int(vis.sum()), 2)),
                              np.stack([rs.uniform(0, cam["width"], n_cl), rs.uniform(0, cam["height"], n_cl)], 1)])
        g = np.concatenate([near[vis], np.full(n_cl, -1)])
        perm = rs.permutation(len(pts))
        keypoints[i + 1], truth[i + 1] = (pts[perm] - 0.5).astype(np.float32), g[perm]
    pair_matches = []
    for a in range(1, n_images + 1):
        for b in range(a + 1, min(a + window, n_images) + 1):
            ga, gb = truth[a], truth[b]
            _, ka, kb = np.intersect1d(np.where(ga >= 0, ga, -1 - np.arange(len(ga))), np.where(gb >= 0, gb, -10 ** 9 - np.arange(len(gb))),
                                       return_indices=True)
            m0 = np.full(len(ga), -1, dtype=np.int64)
            m0[ka] = kb
            free = np.nonzero(m0 < 0)[0]
            n_false = min(int(false_share * len(ka)), len(free))
            m0[rs.choice(free, n_false, replace=False)] = rs.randint(0, len(gb), n_false)
            pair_matches.append((a, b, m0))
    return cameras, images, keypoints, pair_matches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--false_share", type=float, default=0.05)
    ap.add_argument("--clutter_share", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--store", default="pack", help="pack, npz or h5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sfd2_amd import colmap_io, feature_io, triangulation as T
    from sfd2_amd.match_features import names_to_pair
    cameras, images, keypoints, pair_m0 = make_scene(a.images, a.points, a.window, a.false_share, a.clutter_share, 0)
    root = tempfile.mkdtemp(prefix="tri_bench_")
    try:
        empty = {i: colmap_io.Image(i, im.qvec, im.tvec, im.camera_id, im.name, np.zeros((0, 2)), np.zeros(0, np.int64)) for i, im in images.items()}
        colmap_io.write_model(cameras, empty, {}, os.path.join(root, "ref"))
        feats = feature_io.open_store(os.path.join(root, "feats.h5"), "a", standin=a.store)
        for i, kp in keypoints.items():
            feature_io.write_features(feats, images[i].name, {"keypoints": kp.astype(np.float64)})
        feats.close()
        store = feature_io.open_store(os.path.join(root, "matches.h5"), "a", standin=a.store)
        with open(os.path.join(root, "pairs.txt"), "w") as f:
            for i0, i1, m0 in pair_m0:
                feature_io.write_matches(store, names_to_pair(images[i0].name, images[i1].name), m0, np.where(m0 >= 0, 0.9, 0.0).astype(np.float32))
                f.write(f"{images[i0].name} {images[i1].name}\n")
        store.close()
        rows = []
        for rep in range(a.reps + 1):                          # the first pass warms up (context, buffers) and is not reported
            t0 = time.perf_counter()
            kps, pair_matches = T.read_inputs(images, os.path.join(root, "pairs.txt"), os.path.join(root, "feats.h5"), os.path.join(root, "matches.h5"))
            t1 = time.perf_counter()
            tm = {}
            out_images, points3D = T.triangulate_model(cameras, images, kps, pair_matches, timings=tm)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            colmap_io.write_model(cameras, out_images, points3D, os.path.join(root, "sfm"))
            t3 = time.perf_counter()
            row = {"read_s": t1 - t0, "verify_s": tm["verify_s"], "tracks_s": tm["tracks_s"], "triangulate_s": tm["triangulate_s"],
                   "assemble_model_s": (t2 - t1) - tm["verify_s"] - tm["tracks_s"] - tm["triangulate_s"], "write_s": t3 - t2,
                   "pairs_per_s": tm["n_pairs"] / tm["verify_s"], "matches_per_s": tm["n_matches"] / tm["verify_s"],
                   "tracks_per_s": tm["n_tracks"] / tm["triangulate_s"]}
            if rep:
                rows.append(row)
                print(json.dumps(row), flush=True)
        stats = T.model_statistics(out_images, points3D)
        med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
        out = {"device": torch.cuda.get_device_name(0), "images": a.images, "key_points": int(sum(len(k) for k in keypoints.values())),
               "pairs": tm["n_pairs"], "matches": tm["n_matches"], "verified_matches": tm["n_verified"], "tracks": tm["n_tracks"],
               "model": stats, "store": a.store, "median": med, "reps": rows,
               "note": "wall clock per stage, each stage call includes its host packing and copies; no baseline exists (no COLMAP, no earlier path)"}
        print(json.dumps({k: v for k, v in out.items() if k != "reps"}), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
