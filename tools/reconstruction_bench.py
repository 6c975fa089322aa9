"""The round-based mapper (sfd2_amd.reconstruction) on the synthetic scene of tools/triangulate_bench.py, from the matches alone: no pose
goes in.  Reports the rounds, the registered images, the seconds per stage summed over the rounds, the four new device calls against
tests/mapper_ref.py's numpy on the arrays of the last round -- a host restatement written for the tests, not a baseline anybody would
run -- and the final model's errors after a similarity alignment of its camera centres to the truth.  No speed ratio for the mapper as a
whole: there is no COLMAP here and no earlier path to compare with.

    python tools/reconstruction_bench.py [--images 200] [--points 60000] [--window 10] [--out profiles/reconstruction_bench.json]

With --ba_solver dense the mapper runs twice in the same run, first with the PCG adjustment and then with the dense
one: per solver the rounds, the seconds per stage, the adjustment's share, the final adjustment's report and the errors after alignment.
    python tools/reconstruction_bench.py --ba_solver dense --out profiles/reconstruction_dense_bench.json"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--ref_candidates", type=int, default=2, help="candidates of the assemble comparison (the numpy restatement is quadratic)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ba_solver", choices=("pcg", "dense"), default="pcg")
    a = ap.parse_args()
    import torch
    import mapper_ref as mr
    from triangulate_bench import make_scene
    from sfd2_amd import reconstruction as RC
    cameras, truth, keypoints, pair_m0 = make_scene(a.images, a.points, a.window, 0.0, 0.3, 0)
    pair_matches = [(i0, i1, np.stack([np.nonzero(m0 >= 0)[0], m0[m0 >= 0]], 1).astype(np.int32)) for i0, i1, m0 in pair_m0]

    class Recording(RC.DeviceStages):
        """The device stages, keeping the arguments of the last call of each new stage."""
        last = {}

        def restrict(self, *args):
            self.last["restrict"] = args
            return super().restrict(*args)

        def filter(self, *args):
            self.last["filter"] = args
            return super().filter(*args)

        def visible(self, *args):
            self.last["visible"] = args
            return super().visible(*args)

        def assemble(self, *args):
            self.last["assemble"] = args
            return super().assemble(*args)

    RC.restrict_tracks(np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), [1])      # the context, outside the clock
    if a.ba_solver == "dense":
        out = {"device": torch.cuda.get_device_name(0), "input_images": len(truth), "pairs": len(pair_matches), "solvers": {},
               "note": "wall clock, host packing and copies included; both solvers in the same run of the tool, PCG first; the flagship path (bench.py) "
                       "calls none of this code"}
        for solver in ("pcg", "dense"):
            rep = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            images, points3D = RC.reconstruct(cameras, truth, keypoints, pair_matches, report=rep, ba_solver=solver)
            total = time.perf_counter() - t0
            stages = {}
            for r in rep["rounds"] + [rep["final"]]:
                for k, v in r["seconds"].items():
                    stages[k] = stages.get(k, 0.0) + v
            stages.update(verify_s=rep["verify_s"], tracks_s=rep["tracks_s"])
            errs = mr.model_errors(images, points3D, truth)
            errs["rotation_deg"] = float(np.degrees(errs.pop("rotation")))
            out["solvers"][solver] = {"rounds": len(rep["rounds"]), "registered": len(images), "points": len(points3D), "observations": rep["final"]["observations"],
                                      "total_s": total, "stage_s": stages, "adjust_share_of_total": stages.get("adjust_s", 0.0) / total,
                                      "adjust_calls": len(rep["rounds"]) + 1, "round_adjustments": [r["ba"] for r in rep["rounds"]],
                                      "final_adjustment": rep["final"]["ba"], "errors_after_alignment": errs}
            print(solver, json.dumps({k: v for k, v in out["solvers"][solver].items() if k != "round_adjustments"}), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    S, rep = Recording(0), {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    images, points3D = RC.reconstruct(cameras, truth, keypoints, pair_matches, stages=S, report=rep)
    total = time.perf_counter() - t0
    stages = {}
    for r in rep["rounds"] + [rep["final"]]:
        for k, v in r["seconds"].items():
            stages[k] = stages.get(k, 0.0) + v
    stages.update(verify_s=rep["verify_s"], tracks_s=rep["tracks_s"])
    new_calls = sum(stages.get(k, 0.0) for k in ("restrict_s", "filter_s", "visible_s", "assemble_s"))

    def clock(f, *args, reps=3):
        best = float("inf")
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = f(*args)
            best = min(best, time.perf_counter() - t)
        return best, out

    calls = {}
    args = S.last["restrict"]
    d, got = clock(RC.restrict_tracks, *args)
    h, want = clock(mr.restrict_ref, *args, reps=1)
    calls["restrict"] = {"device_s": d, "numpy_s": h, "tracks": len(args[0]) - 1, "observations": len(args[1]),
                         "equal": all(got[k].tobytes() == want[k].tobytes() for k in want)}
    args = S.last["filter"]
    d, got = clock(RC.filter_points, *args)
    h, want = clock(mr.filter_ref, *args, reps=1)
    ok = np.isfinite(want["point_angle"]) & (want["point_angle"] != 0)
    calls["filter"] = {"device_s": d, "numpy_s": h, "points": len(args[2]), "observations": len(args[4]),
                       "keep_equal": bool((got["obs_keep"] == want["obs_keep"]).all()), "live_differ": int((got["point_live"] != want["point_live"]).sum()),
                       "banded": int(want["banded"].sum()),
                       "angle_rel_max": float((np.abs(got["point_angle"][ok] - want["point_angle"][ok]) / want["point_angle"][ok]).max())}
    if "visible" in S.last:
        args = S.last["visible"]
        d, got = clock(RC.visible_counts, *args)
        h, want = clock(mr.visible_ref, *args, reps=1)
        calls["visible"] = {"device_s": d, "numpy_s": h, "points": len(args[3]), "equal": got.tolist() == want.tolist()}
    if "assemble" in S.last:
        args = list(S.last["assemble"])
        d_all, got_all = clock(RC.assemble_problems, *args)
        cand = list(args[7])[:a.ref_candidates]
        args[7], args[8] = cand, int(got_all["offsets"][len(cand)])
        d, got = clock(RC.assemble_problems, *args)
        h, want = clock(mr.assemble_ref, *args[:8], reps=1)
        calls["assemble"] = {"device_s_all_candidates": d_all, "candidates": len(S.last["assemble"][7]), "correspondences": int(got_all["offsets"][-1]),
                             "device_s": d, "numpy_s": h, "compared_candidates": len(cand), "equal": all(got[k].tobytes() == want[k].tobytes() for k in want)}
    errs = mr.model_errors(images, points3D, truth)
    errs["rotation_deg"] = float(np.degrees(errs.pop("rotation")))
    out = {"device": torch.cuda.get_device_name(0), "input_images": len(truth), "pairs": len(pair_matches), "tracks": rep["n_tracks"],
           "initial_pair": list(rep["initial_pair"]), "initial_tri_angle_bound": rep["initial_tri_angle_bound"], "rounds": len(rep["rounds"]),
           "registered": len(images), "registered_per_round": [len(r["registered"]) for r in rep["rounds"]], "points": len(points3D),
           "observations": rep["final"]["observations"], "total_s": total, "stage_s": stages, "new_calls_share_of_total": new_calls / total,
           "new_calls_vs_numpy": calls, "errors_after_alignment": errs, "final_adjustment": rep["final"]["ba"], "options": dict(RC.DEFAULTS),
           "note": "wall clock, host packing and copies included: every call uploads its tables; mapper_ref's numpy is a host restatement written for the "
                   "tests, not a baseline; the flagship path (bench.py) calls none of this code"}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
