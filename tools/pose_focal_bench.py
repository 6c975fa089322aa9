"""Absolute pose with an unknown focal length (sfd2_absolute_pose_focal_batch): ms per query of 50 problems of the
focal call (sweep of 31 samples, main run, refinement of the focal length) beside the fixed-focal call at the true camera in the same
run, for n in {300, 1000} correspondences, inlier ratios {0.5, 0.2} and priors off by 0.65 and 1.6, with the focal and rotation error
after it.  Wall clock around the calls (host packing, upload, kernels, download).

    python tools/pose_focal_bench.py [--reps 5] [--out profiles/pose_focal_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _time(fn, reps):
    import torch
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--problems", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_focal_bench.json"))
    a = ap.parse_args()
    import torch
    import pose_focal_ref as fr
    import pose_ref as pr
    from sfd2_amd import pose
    rows = []
    for n in (300, 1000):
        for ratio in (0.5, 0.2):
            for off in (0.65, 1.6):
                rs = np.random.RandomState(n)
                true, prior, truth = [], [], []
                for i in range(a.problems):
                    cam = pr.camera(pr.MODELS[i % 4])
                    q, t, x, X, _ = pr.scene(rs, cam, n, 1.0 - ratio, noise_px=1.0)
                    true.append((x, X, cam))
                    prior.append((x, X, fr.prior_camera(cam, off)))
                    truth.append((q, t, cam))
                kw = dict(estimate_focal_length=True, refine_focal_length=True)
                res = pose.absolute_pose_estimation_batch(prior, 12.0, **kw)          # warm-up, and the accuracy of this set
                pose.absolute_pose_estimation_batch(true, 12.0)
                ferr = [fr.focal_error(r["camera"], c) for r, (q, t, c) in zip(res, truth) if r["success"]]
                rerr = [np.degrees(pr.rot_angle(r["qvec"], q)) for r, (q, t, c) in zip(res, truth) if r["success"]]
                row = {"n": n, "inlier_ratio": ratio, "prior_off_by": off, "problems": a.problems,
                       "ms_per_query_focal": _time(lambda: pose.absolute_pose_estimation_batch(prior, 12.0, **kw), a.reps),
                       "ms_per_query_fixed_true_camera": _time(lambda: pose.absolute_pose_estimation_batch(true, 12.0), a.reps),
                       "successes": int(sum(r["success"] for r in res)), "median_focal_err": float(np.median(ferr)) if ferr else None,
                       "max_focal_err": float(max(ferr)) if ferr else None, "median_rot_err_deg": float(np.median(rerr)) if rerr else None,
                       "max_rot_err_deg": float(max(rerr)) if rerr else None}
                row["focal_over_fixed"] = row["ms_per_query_focal"] / row["ms_per_query_fixed_true_camera"]
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows,
           "note": "wall clock around the whole call; 31 focal samples, sweep_max_num_trials 1024, defaults otherwise"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
