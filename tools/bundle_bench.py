"""Bundle adjustment (sfd2_amd.bundle_adjustment) on the synthetic scene of tools/triangulate_bench.py: the true poses are perturbed
(all but the first two images), the map is triangulated with the perturbed poses, then adjusted with the first two images constant.
Reports ms per LM iteration, PCG iterations per step, ms per reduced-system product (from two one-step runs with a fixed number of
PCG iterations each: the difference in time over the difference in iterations, vector updates included), observations/s (observations
x LM iterations / time) and the pose error against the scene's truth before and after.  No speed ratio: there is no COLMAP or Ceres here
and no earlier path to compare with.

    python tools/bundle_bench.py [--images 200] [--points 60000] [--window 10] [--reps 3] [--out profiles/bundle_bench.json]

With one of --refine_focal_length / --refine_principal_point / --refine_extra_params 1 every camera's focal
lengths start --focal_off (0.1) too long, the map is triangulated with those cameras, and the same figures are taken three times in
the same run: intrinsics fixed (adjust, today's call), the scene's four cameras each shared by its images, and a camera per image
(adjust_cameras); with the mean relative focal-length error before and after.
    python tools/bundle_bench.py --refine_focal_length 1 --refine_extra_params 1 --out profiles/bundle_cam_bench.json

With --solver dense the adjustment runs with both solvers of the reduced camera system in the same run, PCG first:
per solver ms per LM iteration, LM steps tried and accepted, status, final cost, final max |g| and the pose errors; for the dense solver
also the length of the pair list and the one-off cost of building it (a call with max_iterations=0 against the same call with PCG).
    python tools/bundle_bench.py --solver dense --out profiles/bundle_dense_bench.json

Kernel times come from a kernel trace of the same tool (no counters in that run):
    rocprofv3 --kernel-trace --stats -d DIR -o ba -- python tools/bundle_bench.py --reps 1"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def pose_errors(images, truth, ids):
    import pose_ref as pr
    rot = [np.degrees(pr.rot_angle(images[i].qvec, truth[i].qvec)) for i in ids]
    pos = [float(np.linalg.norm(pr.centre(images[i].qvec, images[i].tvec) - pr.centre(truth[i].qvec, truth[i].tvec))) for i in ids]
    return {"rotation_deg_mean": float(np.mean(rot)), "rotation_deg_max": float(np.max(rot)), "position_mean": float(np.mean(pos)),
            "position_max": float(np.max(pos))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--rot_deg", type=float, default=0.2)
    ap.add_argument("--shift", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--refine_focal_length", type=int, choices=(0, 1), default=0)
    ap.add_argument("--refine_principal_point", type=int, choices=(0, 1), default=0)
    ap.add_argument("--refine_extra_params", type=int, choices=(0, 1), default=0)
    ap.add_argument("--focal_off", type=float, default=0.1)
    ap.add_argument("--solver", choices=("pcg", "dense"), default="pcg")
    a = ap.parse_args()
    import torch
    import pose_ref as pr
    import tri_ref as tr
    from triangulate_bench import make_scene
    from sfd2_amd import bundle_adjustment as B, triangulation as T
    cameras, truth, keypoints, pair_m0 = make_scene(a.images, a.points, a.window, 0.0, 0.3, 0)
    mask = B.refine_mask(a.refine_focal_length, a.refine_principal_point, a.refine_extra_params)
    true_cameras = cameras
    if mask:
        focal = lambda c: [0] if c["model"].startswith("SIMPLE") else [0, 1]
        cameras = {i: tr.Cam(c, params=[p * (1 + a.focal_off) if k in focal(c) else p for k, p in enumerate(c["params"])]) for i, c in cameras.items()}
    pair_matches = [(i0, i1, np.stack([np.nonzero(m0 >= 0)[0], m0[m0 >= 0]], 1).astype(np.int32)) for i0, i1, m0 in pair_m0]
    rs = np.random.RandomState(1)
    start = {}
    for i, im in truth.items():
        if i <= 2:
            start[i] = im
            continue
        w, v = rs.standard_normal(3), rs.standard_normal(3)
        th = np.radians(a.rot_deg)
        k = w / np.linalg.norm(w)
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K) @ pr.qvec2rotmat(im.qvec)
        start[i] = tr.Img(i, pr.rotmat2qvec(R), im.tvec + a.shift * v / np.linalg.norm(v), im.camera_id, im.name)
    images, points3D = T.triangulate_model(cameras, start, keypoints, pair_matches, max_error=12.0, filter_max_reproj_error=12.0)
    ids, views, pids, xyz, off, ov, xy = B.pack_model(cameras, images, points3D)
    moving = [i for i in ids if i > 2]
    vc = np.array([i <= 2 for i in ids], dtype=np.uint8)
    pc = np.zeros(len(pids), dtype=np.uint8)
    n_obs = int(len(ov))

    cam_ids = sorted(cameras)
    shared = [cam_ids.index(images[i].camera_id) for i in ids]

    def focal_error(params, view_camera):
        """Mean relative error of the focal lengths of the cameras view_camera names, against the scene's."""
        errs = []
        for k in sorted(set(view_camera)):
            t = true_cameras[images[ids[view_camera.index(k)]].camera_id]
            n = 1 if t["model"].startswith("SIMPLE") else 2
            errs += [abs(params[k][j] - t["params"][j]) / t["params"][j] for j in range(n)]
        return float(np.mean(errs))

    def once(mode="fixed", **opts):
        """mode: fixed (adjust), shared (one camera per camera id) or per_image (adjust_cameras)."""
        v = B.make_views(cameras, images, ids)[1]
        view_camera = shared if mode == "shared" else list(range(len(ids)))
        packed = [B.camera_model(cameras[c]) for c in (cam_ids if mode == "shared" else [images[i].camera_id for i in ids])]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "fixed":
            out = B.adjust(v, len(ids), vc, xyz, pc, off, ov, xy, **opts)
            params = [p for _, p in packed]
        else:
            params, *out = B.adjust_cameras([m for m, _ in packed], [p for _, p in packed], [mask] * len(packed), view_camera, v, len(ids), vc, xyz, pc, off,
                                            ov, xy, **opts)
        t = time.perf_counter() - t0
        once.focal = (focal_error([p for _, p in packed], view_camera), focal_error(params, view_camera))
        return t, v, tuple(out)

    if mask:
        return camera_comparison(a, once, out_head=dict(device=torch.cuda.get_device_name(0), images=len(ids), points=len(pids), observations=n_obs,
                                                        refine=mask, focal_off=a.focal_off))
    if a.solver == "dense":
        def errors_of(v):
            return pose_errors({i: tr.Img(i, np.array(v[k].qvec[:]), np.array(v[k].tvec[:]), images[i].camera_id, images[i].name) for k, i in enumerate(ids)},
                               truth, moving)
        n_pairs = 0
        for j in range(len(pids)):                             # (a, b) of one point with view(a) >= view(b)
            vs = np.sort(ov[off[j]:off[j + 1]])
            n_pairs += int(np.searchsorted(vs, vs, side="right").sum())
        return solver_comparison(a, once, errors_of, dict(device=torch.cuda.get_device_name(0), images=len(ids), points=len(pids), observations=n_obs,
                                                          mean_track_length=n_obs / max(len(pids), 1), pair_list_length=n_pairs,
                                                          reduced_system_size=6 * len(ids), pose_error_before=pose_errors(images, truth, moving),
                                                          mean_reprojection_error_before=float(np.mean([p.error for p in points3D.values()]))))
    rows = []
    for rep in range(a.reps + 1):                              # the first pass warms up (context, buffers) and is not reported
        t_full, v, (new_xyz, err, report) = once()
        t_lo, _, (_, _, r_lo) = once(max_iterations=1, pcg_tolerance=0.0, pcg_max_iterations=10)
        t_hi, _, (_, _, r_hi) = once(max_iterations=1, pcg_tolerance=0.0, pcg_max_iterations=60)
        row = {"adjust_s": t_full, "lm_iterations": report["iterations"], "accepted_steps": report["accepted_steps"],
               "pcg_iterations": report["pcg_iterations"], "ms_per_lm_iteration": 1e3 * t_full / max(report["iterations"], 1),
               "pcg_iterations_per_step": report["pcg_iterations"] / max(report["iterations"], 1),
               "ms_per_product": 1e3 * (t_hi - t_lo) / max(r_hi["pcg_iterations"] - r_lo["pcg_iterations"], 1),
               "observations_per_s": n_obs * report["iterations"] / t_full}
        if rep:
            rows.append(row)
            print(json.dumps(row), flush=True)
    after = {i: tr.Img(i, np.array(v[k].qvec[:]), np.array(v[k].tvec[:]), images[i].camera_id, images[i].name) for k, i in enumerate(ids)}
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    out = {"device": torch.cuda.get_device_name(0), "images": len(ids), "points": len(pids), "observations": n_obs,
           "mean_track_length": n_obs / max(len(pids), 1), "options": dict(B.DEFAULTS), "status": report["status"],
           "initial_cost": report["initial_cost"], "final_cost": report["final_cost"], "gradient_max": report["gradient_max"],
           "mean_reprojection_error_before": float(np.mean([p.error for p in points3D.values()])), "mean_reprojection_error_after": float(err.mean()),
           "pose_error_before": pose_errors(images, truth, moving), "pose_error_after": pose_errors(after, truth, moving), "median": med, "reps": rows,
           "note": "wall clock of the whole call, host packing and copies included; no baseline exists (no COLMAP or Ceres, no earlier path); the "
                   "flagship path (bench.py) calls none of this code"}
    print(json.dumps({k: v for k, v in out.items() if k != "reps"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def solver_comparison(a, once, errors_of, out_head):
    """Both solvers in one run, PCG first: per solver the medians over --reps of the whole call and of ms per LM iteration, the report
    and the pose errors after; for the dense solver the one-off cost of the pair list."""
    out = dict(out_head, solvers={}, note="wall clock of the whole call, host packing and copies included; both solvers in the same run of the tool; "
                                          "the flagship path (bench.py) calls none of this code")
    setup = {}
    for solver in ("pcg", "dense"):
        rows = []
        for rep in range(a.reps + 1):                          # the first pass warms up and is not reported
            t_full, v, (_, err, report) = once(solver=solver)
            t_zero = once(solver=solver, max_iterations=0)[0]
            if rep:
                rows.append({"adjust_s": t_full, "ms_per_lm_iteration": 1e3 * (t_full - t_zero) / max(report["iterations"], 1),
                             "ms_per_lm_iteration_whole_call": 1e3 * t_full / max(report["iterations"], 1), "call_without_steps_s": t_zero,
                             "pcg_iterations_per_step": report["pcg_iterations"] / max(report["iterations"], 1)})
        med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
        setup[solver] = med["call_without_steps_s"]
        out["solvers"][solver] = dict(med, lm_iterations=report["iterations"], accepted_steps=report["accepted_steps"], status=report["status"],
                                      initial_cost=report["initial_cost"], final_cost=report["final_cost"], gradient_max=report["gradient_max"],
                                      mean_reprojection_error_after=float(err.mean()), pose_error_after=errors_of(v), reps=rows)
        print(solver, json.dumps({k: v for k, v in out["solvers"][solver].items() if k != "reps"}), flush=True)
    out["pair_list_build_ms"] = 1e3 * (setup["dense"] - setup["pcg"])
    print(json.dumps({k: v for k, v in out.items() if k != "solvers"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def camera_comparison(a, once, out_head):
    """The three modes in one run: per mode the medians over --reps of ms per LM iteration, PCG iterations per step and ms per product, and
    the focal-length error before and after."""
    out = dict(out_head, modes={}, note="wall clock of the whole call, host packing and copies included; the three modes in the same run of the tool")
    for mode in ("fixed", "shared", "per_image"):
        rows = []
        for rep in range(a.reps + 1):                          # the first pass warms up and is not reported
            t_full, _, (_, err, report) = once(mode)
            focal = once.focal
            t_lo, _, (_, _, r_lo) = once(mode, max_iterations=1, pcg_tolerance=0.0, pcg_max_iterations=10)
            t_hi, _, (_, _, r_hi) = once(mode, max_iterations=1, pcg_tolerance=0.0, pcg_max_iterations=60)
            if rep:
                rows.append({"adjust_s": t_full, "ms_per_lm_iteration": 1e3 * t_full / max(report["iterations"], 1),
                             "pcg_iterations_per_step": report["pcg_iterations"] / max(report["iterations"], 1),
                             "ms_per_product": 1e3 * (t_hi - t_lo) / max(r_hi["pcg_iterations"] - r_lo["pcg_iterations"], 1)})
        med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
        out["modes"][mode] = dict(med, lm_iterations=report["iterations"], accepted_steps=report["accepted_steps"], status=report["status"],
                                  initial_cost=report["initial_cost"], final_cost=report["final_cost"], mean_reprojection_error_after=float(err.mean()),
                                  focal_error_before=focal[0], focal_error_after=focal[1], reps=rows)
        print(mode, json.dumps({k: v for k, v in out["modes"][mode].items() if k != "reps"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
