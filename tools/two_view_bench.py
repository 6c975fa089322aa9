"""Relative pose throughput (sfd2_relative_pose_batch): ms per batch and pairs/s for 1000 pairs of 2048 matches at inlier ratios
{0.3, 0.6} with 1 px of noise, timed by HIP events around the whole call and by the wall clock.  There is no CPU baseline: COLMAP and
cv2 are not available here, and the numpy test helper is no stand-in for them.

    python tools/two_view_bench.py [--reps 3] [--out profiles/two_view_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=2048)
    ap.add_argument("--ratios", default="0.3,0.6")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_bench.json"))
    a = ap.parse_args()
    import torch
    import pose_ref as pr
    import two_view_ref as tv
    from sfd2_amd import two_view
    rows = []
    for ratio in [float(v) for v in a.ratios.split(",")]:
        rs = np.random.RandomState(int(1000 * ratio))
        probs, truth = [], []
        for i in range(a.pairs):
            cam0 = pr.camera(["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "OPENCV"][i % 4])
            cam1 = pr.camera(["OPENCV", "SIMPLE_RADIAL", "PINHOLE", "SIMPLE_PINHOLE"][(i // 4) % 4])
            R, t, p0, p1, _ = tv.two_view_scene(rs, cam0, cam1, a.matches, 1.0 - ratio, noise_px=1.0)
            probs.append((p0, p1, cam0, cam1))
            truth.append((R, t))
        res = two_view.relative_pose_batch(probs)                  # warm-up (and the accuracy of this set)
        err = [max(tv.pose_error(pr.qvec2rotmat(r["qvec"]), r["tvec"], R, t)) for r, (R, t) in zip(res, truth)]
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms_ev, ms_wall = [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev0.record()
            two_view.relative_pose_batch(probs)
            ev1.record()
            torch.cuda.synchronize()
            ms_wall.append(1e3 * (time.perf_counter() - t0))
            ms_ev.append(ev0.elapsed_time(ev1))
        row = {"pairs": a.pairs, "matches": a.matches, "inlier_ratio": ratio, "ms_per_batch_events": float(np.median(ms_ev)),
               "ms_per_batch_wall": float(np.median(ms_wall)), "pairs_per_s": a.pairs / (np.median(ms_wall) / 1e3),
               "trials_mean": float(np.mean([r["num_trials"] for r in res])), "all_success": all(r["success"] for r in res),
               "median_pose_err_deg": float(np.degrees(np.median(err))), "max_pose_err_deg": float(np.degrees(np.max(err)))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows,
           "note": "events bracket the whole call on the default stream (host packing, upload, kernel, download, the Python loop over "
                   "the results); no CPU baseline (COLMAP and cv2 absent).  For orientation only: profiles/pose_bench.json has the "
                   "absolute pose solver's problems/s at n = 1000 and 3000."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
