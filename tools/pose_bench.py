"""Absolute pose throughput (sfd2_absolute_pose_batch): ms per query of 50 problems and problems/s for n in {300, 1000, 3000}
correspondences at inlier ratios {0.2, 0.5}, timed by HIP events around the call and by the wall clock.  There is no CPU baseline:
pycolmap is not available here, and the numpy test helper is no stand-in for it.

    python tools/pose_bench.py [--reps 5] [--out profiles/pose_bench.json]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--problems", type=int, default=50)
    ap.add_argument("--sizes", default="300,1000,3000")
    ap.add_argument("--ratios", default="0.2,0.5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pose_ref as pr
    from sfd2_amd import pose
    rows = []
    for n in [int(v) for v in a.sizes.split(",")]:
        for ratio in [float(v) for v in a.ratios.split(",")]:
            rs = np.random.RandomState(n)
            probs, truth = [], []
            for i in range(a.problems):
                cam = pr.camera(["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "OPENCV"][i % 4])
                q, t, x, X, _ = pr.scene(rs, cam, n, 1.0 - ratio, noise_px=1.0, offset=(rs.uniform(-500, 500), 0.0, 30.0))
                probs.append((x, X, cam))
                truth.append((q, t))
            res = pose.absolute_pose_estimation_batch(probs, 12.0)     # warm-up (and the accuracy of this set)
            err = max(np.degrees(pr.rot_angle(r["qvec"], q)) for r, (q, t) in zip(res, truth))
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms_ev, ms_wall = [], []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev0.record()
                pose.absolute_pose_estimation_batch(probs, 12.0)
                ev1.record()
                torch.cuda.synchronize()
                ms_wall.append(1e3 * (time.perf_counter() - t0))
                ms_ev.append(ev0.elapsed_time(ev1))
            row = {"n": n, "inlier_ratio": ratio, "problems": a.problems, "ms_per_query_events": float(np.median(ms_ev)),
                   "ms_per_query_wall": float(np.median(ms_wall)), "problems_per_s": a.problems / (np.median(ms_wall) / 1e3),
                   "trials_mean": float(np.mean([r["num_trials"] for r in res])), "all_success": all(r["success"] for r in res),
                   "max_rot_err_deg": float(err)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows,
           "note": "events bracket the whole call on the default stream (host packing, upload, kernel, download); no CPU baseline (pycolmap absent)"}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
