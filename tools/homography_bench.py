"""Homography throughput (sfd2_homography_batch) and what the E / F / H decision buys: ms per batch and pairs/s for 1000 planar pairs of
2048 matches at inlier ratios {0.3, 0.6} with 1 px of noise, timed by HIP events around the whole call and by the wall clock, with
sfd2_fundamental_batch timed in the same process on general scenes of the same sizes; and the motivating cases -- 200 synthetic pairs
of 300 matches with 30 % false ones of a plane, of a pure rotation and of a general scene, exact and with 1 px of noise -- with the true and false matches
that verify_pairs_fundamental, verify_pairs_homography and verify_pairs_geometry (without and with cameras) keep, and a histogram of
the configs.  There is no CPU baseline: COLMAP and cv2 are not available here.

    python tools/homography_bench.py [--reps 3] [--out profiles/homography_bench.json]"""
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


def timed(call, reps):
    import torch
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms_ev, ms_wall = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0.record()
        call()
        ev1.record()
        torch.cuda.synchronize()
        ms_wall.append(1e3 * (time.perf_counter() - t0))
        ms_ev.append(ev0.elapsed_time(ev1))
    return float(np.median(ms_ev)), float(np.median(ms_wall))


def throughput(a):
    import fundamental_ref as fr
    import homography_ref as hr
    import two_view_ref as tv
    from sfd2_amd import two_view
    rows = []
    for ratio in [float(v) for v in a.ratios.split(",")]:
        rs = np.random.RandomState(int(1000 * ratio))
        planar, general, truth = [], [], []
        for i in range(a.pairs):
            H, p0, p1, _ = hr.scene(int(rs.randint(1 << 30)), a.matches, 1.0 - ratio, noise_px=1.0)
            planar.append((p0, p1))
            truth.append(H)
            general.append(tuple(tv.two_view_scene(rs, fr.CAM0, fr.CAM1, a.matches, 1.0 - ratio, noise_px=1.0)[2:4]))
        res = two_view.homography_batch(planar)                    # warm-up (and the accuracy of this set)
        resF = two_view.fundamental_matrix_batch(general)
        err = [float(np.min([np.linalg.norm(r["H"] - s * Ht / np.linalg.norm(Ht)) for s in (1, -1)])) for r, Ht in zip(res[:50], truth[:50])]
        h_ev, h_wall = timed(lambda: two_view.homography_batch(planar), a.reps)
        f_ev, f_wall = timed(lambda: two_view.fundamental_matrix_batch(general), a.reps)
        tH, tF = float(np.mean([r["num_trials"] for r in res])), float(np.mean([r["num_trials"] for r in resF]))
        row = {"pairs": a.pairs, "matches": a.matches, "inlier_ratio": ratio,
               "homography": {"ms_per_batch_events": h_ev, "ms_per_batch_wall": h_wall, "pairs_per_s": a.pairs / (h_wall / 1e3), "trials_mean": tH,
                              "ms_per_round_of_256": h_ev / (tH / 256.0), "all_success": all(r["success"] for r in res),
                              "inlier_share_mean": float(np.mean([r["num_inliers"] for r in res])) / a.matches,
                              "median_distance_to_true_H": float(np.median(err))},
               "fundamental_same_sizes": {"ms_per_batch_events": f_ev, "ms_per_batch_wall": f_wall, "pairs_per_s": a.pairs / (f_wall / 1e3),
                                          "trials_mean": tF, "ms_per_round_of_256": f_ev / (tF / 256.0),
                                          "all_success": all(r["success"] for r in resF)}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def motivating(a, noise):
    """An exact plane, a pure rotation and a general scene: what each verification keeps, and the configs."""
    import fundamental_ref as fr
    import two_view_ref as tv
    from sfd2_amd import two_view
    cams = {0: fr.CAM0, 1: fr.CAM1}
    out = {}
    for k, (name, kw) in enumerate((("plane", dict(planar=True)), ("rotation", dict(baseline=0.0)), ("general", {}))):
        rs = np.random.RandomState(70 + k)
        keypoints, images, pair_matches, false = {}, {}, [], []
        idx = np.arange(a.verify_matches)
        for p in range(a.verify_pairs):
            _, _, p0, p1, o = tv.two_view_scene(rs, fr.CAM0, fr.CAM1, a.verify_matches, a.verify_false, noise_px=noise, **kw)
            keypoints[2 * p], keypoints[2 * p + 1] = (p0 - 0.5).astype(np.float32), (p1 - 0.5).astype(np.float32)
            images[2 * p], images[2 * p + 1] = SimpleNamespace(camera_id=0, name=f"a{p}"), SimpleNamespace(camera_id=1, name=f"b{p}")
            pair_matches.append((2 * p, 2 * p + 1, np.stack([idx, idx], 1)))
            false.append(o)
        false = np.concatenate(false)
        row = {"pairs": a.verify_pairs, "matches_per_pair": a.verify_matches, "false_share": a.verify_false, "noise_px": noise,
               "max_error_px": 4.0, "true_matches": int((~false).sum()), "false_matches": int(false.sum())}
        runs = {"fundamental": lambda: two_view.verify_pairs_fundamental(keypoints, pair_matches, 4.0, 15),
                "homography": lambda: two_view.verify_pairs_homography(keypoints, pair_matches, 4.0, 15),
                "geometry_without_cameras": lambda: two_view.verify_pairs_geometry(keypoints, pair_matches, None, None, 4.0, 15),
                "geometry_with_cameras": lambda: two_view.verify_pairs_geometry(keypoints, pair_matches, cams, images, 4.0, 15)}
        for run, call in runs.items():
            m, _, _, res = call()
            kept = m[:, 0] >= 0
            row[run] = {"true_kept": int((kept & ~false).sum()), "false_kept": int((kept & false).sum()),
                        "pairs_verified": int(sum(kept[p * a.verify_matches:(p + 1) * a.verify_matches].any() for p in range(a.verify_pairs)))}
            if run.startswith("geometry"):
                configs = [r["config"] for r in res]
                row[run]["configs"] = {c: configs.count(c) for c in sorted(set(configs))}
        out[name] = row
        print(name, json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=2048)
    ap.add_argument("--ratios", default="0.3,0.6")
    ap.add_argument("--verify_pairs", type=int, default=200)
    ap.add_argument("--verify_matches", type=int, default=300)
    ap.add_argument("--verify_false", type=float, default=0.3)
    ap.add_argument("--verify_noise", default="0,1", help="0: the exact plane and rotation of the motivating cases")
    ap.add_argument("--skip_cases", action="store_true", help="the throughput rows only (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_bench.json"))
    a = ap.parse_args()
    import torch
    rows = throughput(a)
    cases = {} if a.skip_cases else {f"noise_{v}px": motivating(a, float(v)) for v in a.verify_noise.split(",")}
    out = {"device": torch.cuda.get_device_name(0), "rows": rows, "motivating_cases": cases,
           "note": "events bracket the whole call on the default stream (host packing, upload, kernel, download, the Python loop over the "
                   "results); no CPU baseline (COLMAP and cv2 absent).  homography: planar scenes; fundamental_same_sizes: "
                   "sfd2_fundamental_batch in the same process on general scenes of the same sizes and inlier ratios.  ms_per_round_of_256 "
                   "divides the whole call by the mean number of rounds, so it carries the call's fixed costs.  motivating_cases: the "
                   "true matches are exact or carry 1 px of noise (noise_px), 30 % of the matches are random pixels."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
