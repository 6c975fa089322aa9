"""Fundamental matrix throughput (sfd2_fundamental_batch): ms per batch and pairs/s for 1000 pairs of 2048 matches at inlier ratios
{0.3, 0.6} with 1 px of noise, timed by HIP events around the whole call and by the wall clock, beside profiles/two_view_bench.json's
figures for the same sizes; and the case the call is there for: the true matches that survive verification by F, by E at the true
cameras and by E at COLMAP's prior cameras (f = 1.2 max(w, h), the principal point at the centre) on one synthetic pair set whose
true focal lengths are 800 (1024 x 768) and 600 / 610 (640 x 480).  There is no CPU baseline: COLMAP and cv2 are not available here.

    python tools/fundamental_bench.py [--reps 3] [--out profiles/fundamental_bench.json]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def survivors(a):
    """verify_pairs_fundamental against verify_pairs_two_view at the true and at the prior cameras: true and false matches kept."""
    import fundamental_ref as fr
    import two_view_ref as tv
    from sfd2_amd import reconstruction, two_view
    rs = np.random.RandomState(7)
    true_cams = {0: fr.CAM0, 1: fr.CAM1}
    prior = {i: reconstruction.prior_camera(i, c["width"], c["height"]) for i, c in true_cams.items()}
    keypoints, images, pair_matches, false = {}, {}, [], []
    for p in range(a.verify_pairs):
        _, _, p0, p1, out = tv.two_view_scene(rs, fr.CAM0, fr.CAM1, a.verify_matches, a.verify_false, noise_px=1.0)
        keypoints[2 * p], keypoints[2 * p + 1] = (p0 - 0.5).astype(np.float32), (p1 - 0.5).astype(np.float32)
        images[2 * p], images[2 * p + 1] = SimpleNamespace(camera_id=0, name=f"a{p}"), SimpleNamespace(camera_id=1, name=f"b{p}")
        idx = np.arange(a.verify_matches)
        pair_matches.append((2 * p, 2 * p + 1, np.stack([idx, idx], 1)))
        false.append(out)
    false = np.concatenate(false)
    row = {"pairs": a.verify_pairs, "matches_per_pair": a.verify_matches, "false_share": a.verify_false, "noise_px": 1.0, "max_error_px": 4.0,
           "true_matches": int((~false).sum()), "false_matches": int(false.sum())}
    runs = {"F": lambda: two_view.verify_pairs_fundamental(keypoints, pair_matches, 4.0, 15),
            "E_true_cameras": lambda: two_view.verify_pairs_two_view(true_cams, images, keypoints, pair_matches, 4.0, 15),
            "E_prior_cameras": lambda: two_view.verify_pairs_two_view(prior, images, keypoints, pair_matches, 4.0, 15)}
    for name, run in runs.items():
        m = run()[0]
        kept = m[:, 0] >= 0
        row[name] = {"true_kept": int((kept & ~false).sum()), "false_kept": int((kept & false).sum()),
                     "pairs_verified": int(sum(kept[p * a.verify_matches:(p + 1) * a.verify_matches].any() for p in range(a.verify_pairs)))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=2048)
    ap.add_argument("--ratios", default="0.3,0.6")
    ap.add_argument("--verify_pairs", type=int, default=200)
    ap.add_argument("--verify_matches", type=int, default=300)
    ap.add_argument("--verify_false", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fundamental_bench.json"))
    a = ap.parse_args()
    import torch
    import fundamental_ref as fr
    import two_view_ref as tv
    from sfd2_amd import two_view
    rows = []
    for ratio in [float(v) for v in a.ratios.split(",")]:
        rs = np.random.RandomState(int(1000 * ratio))
        probs, truth = [], []
        for i in range(a.pairs):
            R, t, p0, p1, _ = tv.two_view_scene(rs, fr.CAM0, fr.CAM1, a.matches, 1.0 - ratio, noise_px=1.0)
            probs.append((p0, p1))
            truth.append(fr.true_F(R, t))
        res = two_view.fundamental_matrix_batch(probs)             # warm-up (and the accuracy of this set)
        # the distance of the returned unit-norm matrix to the scene's own, over the first 50 pairs
        err = []
        for (p0, p1), r, Ft in zip(probs[:50], res[:50], truth[:50]):
            err.append(float(np.min([np.linalg.norm(r["F"] - s * Ft / np.linalg.norm(Ft)) for s in (1, -1)])))
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms_ev, ms_wall = [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev0.record()
            two_view.fundamental_matrix_batch(probs)
            ev1.record()
            torch.cuda.synchronize()
            ms_wall.append(1e3 * (time.perf_counter() - t0))
            ms_ev.append(ev0.elapsed_time(ev1))
        row = {"pairs": a.pairs, "matches": a.matches, "inlier_ratio": ratio, "ms_per_batch_events": float(np.median(ms_ev)),
               "ms_per_batch_wall": float(np.median(ms_wall)), "pairs_per_s": a.pairs / (np.median(ms_wall) / 1e3),
               "trials_mean": float(np.mean([r["num_trials"] for r in res])), "all_success": all(r["success"] for r in res),
               "inlier_share_mean": float(np.mean([r["num_inliers"] for r in res])) / a.matches,
               "median_distance_to_true_F": float(np.median(err))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    ref = {}
    path = os.path.join(ROOT, "profiles", "two_view_bench.json")
    if os.path.exists(path):
        with open(path) as f:
            ref = {str(r["inlier_ratio"]): {"pairs_per_s": r["pairs_per_s"], "trials_mean": r["trials_mean"]} for r in json.load(f)["rows"]}
    surv = survivors(a)
    print(json.dumps(surv), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows, "relative_pose_same_sizes": ref, "survivors": surv,
           "note": "events bracket the whole call on the default stream (host packing, upload, kernel, download, the Python loop over "
                   "the results); no CPU baseline (COLMAP and cv2 absent).  relative_pose_same_sizes: profiles/two_view_bench.json, the "
                   "five-point call on scenes of the same sizes (other cameras), for orientation: at 30 % inliers the seven-point trial "
                   "count runs into max_num_trials where the five-point one does not."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
