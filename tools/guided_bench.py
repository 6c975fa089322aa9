"""Guided matching throughput (sfd2_match_guided_batch) against the matcher's (sfd2_match_batch) in the same process on the same
descriptor sets, and what the gate buys on the twin scene.

Throughput: 50 pairs of 4096 x 4096 under an F and an H guide (tests/guided_ref.py's scenes, gate 4 px), NNM and ratio 0.8, from host
float32 sets and from device-resident packed fp16 sets (sfd2_desc_pack); every pair has image 0's descriptor set of pair 0, so that
sfd2_match_batch -- one query set against 50 database sets -- runs on exactly these 50 x 4096^2 similarities.  Wall-clock time of the
synchronous calls, median of --reps.  The twin scene (guided_ref.twin_scene scaled to 4096 key points in image 0): true matches the
plain rule and the guided rule keep, on the device.

    python tools/guided_bench.py [--reps 5] [--skip_cases] [--out profiles/guided_bench.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFS = {"NNM": (1, 0.0, 0.0), "ratio0.8": (1, 0.8, 0.0)}      # do_mutual_check, ratio_threshold, distance_threshold


def timed(call, reps):
    import torch
    call()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms))


def desc_set(_lib, data, n, dtype, on_device):
    s = _lib.DescSet()
    s.data, s.n, s.dtype, s.layout, s.on_device, s.rows, s.n_rows = data, n, dtype, _lib.LAYOUT_ND, on_device, None, 0
    return s


def throughput(a):
    import torch
    import guided_ref as gr
    from sfd2_amd import _lib
    ctx = _lib.default_context(0)
    n, k = a.n, a.pairs
    rows = []
    for kind in ("F", "H"):
        scenes = [gr.bench_scene(kind, n, i) for i in range(k)]
        d0 = scenes[0]["d0"]
        packed = []
        for d in [d0] + [sc["d1"] for sc in scenes]:
            t = torch.empty((n, 128), dtype=torch.float16, device="cuda:0")
            src = desc_set(_lib, d.ctypes.data, n, _lib.DT_F32, 0)
            _lib.check(ctx.lib.sfd2_desc_pack(ctx.h, ctypes.byref(src), 128, t.data_ptr(), 0))
            packed.append(t)
        m, s = np.empty(k * n, dtype=np.int64), np.empty(k * n, dtype=np.float32)
        for where in ("host_f32", "resident_f16"):
            res = where == "resident_f16"
            q = desc_set(_lib, packed[0].data_ptr(), n, _lib.DT_F16, 1) if res else desc_set(_lib, d0.ctypes.data, n, _lib.DT_F32, 0)
            dbs = [desc_set(_lib, packed[1 + i].data_ptr(), n, _lib.DT_F16, 1) if res else desc_set(_lib, sc["d1"].ctypes.data, n, _lib.DT_F32, 0)
                   for i, sc in enumerate(scenes)]
            db_arr = (_lib.DescSet * k)(*dbs)
            probs = (_lib.GuidedProblem * k)()
            for i, sc in enumerate(scenes):
                pr = probs[i]
                pr.d0, pr.d1 = q, dbs[i]
                pr.xy0, pr.xy1, pr.model, pr.max_error_px = sc["xy0"].ctypes.data, sc["xy1"].ctypes.data, (_lib.GUIDE_F if kind == "F" else _lib.GUIDE_H), a.max_error
                for j in range(9):
                    pr.M[j] = sc["M"].reshape(-1)[j]
            for name, (mutual, ratio, dist) in CONFS.items():
                mc = _lib.MatchConf(_lib.MATCH_HLOC, mutual, ratio, dist, _lib.SIM_F16)
                g_ms = timed(lambda: _lib.check(ctx.lib.sfd2_match_guided_batch(ctx.h, probs, k, 128, ctypes.byref(mc), m.ctypes.data, s.ctypes.data, 0)), a.reps)
                kept = int((m >= 0).sum())
                y_ms = timed(lambda: _lib.check(ctx.lib.sfd2_match_batch(ctx.h, ctypes.byref(q), db_arr, k, 128, ctypes.byref(mc), m.ctypes.data, s.ctypes.data, 0, 0)),
                             a.reps)
                row = {"guide": kind, "sets": where, "conf": name, "pairs": k, "n0": n, "n1": n, "max_error_px": a.max_error,
                       "guided": {"ms_per_batch": g_ms, "pairs_per_s": k / (g_ms / 1e3), "matches_kept": kept},
                       "sfd2_match_batch": {"ms_per_batch": y_ms, "pairs_per_s": k / (y_ms / 1e3), "matches_kept": int((m >= 0).sum())},
                       "guided_over_yardstick": g_ms / y_ms}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def twin(a):
    """The twin scene at 4096 key points in image 0: 2/3 true matches, 3/4 of them with a twin in image 1."""
    import guided_ref as gr
    from sfd2_amd import _lib, two_view
    n_true, n_extra = a.n * 2 // 3, a.n - a.n * 2 // 3
    sc = gr.twin_scene(seed=1, n_true=n_true, n_extra=n_extra, n_twin=n_true * 3 // 4, with_sim=False)
    ctx = _lib.default_context(0)
    n0, n1 = len(sc["d0"]), len(sc["d1"])
    truth = np.full(n0, -1, dtype=np.int64)
    truth[sc["rows"]] = sc["cols"]
    tw = np.zeros(n0, dtype=bool)
    tw[sc["twinned"]] = True
    out = {"n0": n0, "n1": n1, "true_matches": n_true, "twinned_rows": int(tw.sum()), "max_error_px": a.max_error}
    for name, (mutual, ratio, dist) in CONFS.items():
        mc = _lib.MatchConf(_lib.MATCH_HLOC, mutual, ratio, dist, _lib.SIM_F16)
        pm, ps = np.empty(n0, dtype=np.int64), np.empty(n0, dtype=np.float32)
        _lib.check(ctx.lib.sfd2_match(ctx.h, sc["d0"].ctypes.data, n0, sc["d1"].ctypes.data, n1, 128, _lib.DT_F32, _lib.LAYOUT_ND, 0, ctypes.byref(mc),
                                      pm.ctypes.data, ps.ctypes.data, 0))
        gm, _ = two_view.guided_matches(sc["d0"], sc["d1"], sc["xy0"], sc["xy1"], "F", sc["M"], a.max_error,
                                        {"ratio_threshold": ratio or None, "distance_threshold": dist or None, "do_mutual_check": bool(mutual)})
        def figures(m):
            ok = (m == truth) & (truth >= 0)
            return {"true_kept": int(ok.sum()), "true_kept_of_twinned": int((ok & tw).sum()), "false_kept": int(((m >= 0) & ~ok).sum())}
        out[name] = {"plain": figures(pm), "guided": figures(gm)}
        print("twin scene", name, json.dumps(out[name]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=50)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--max_error", type=float, default=4.0)
    ap.add_argument("--skip_cases", action="store_true", help="the throughput rows only (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_bench.json"))
    a = ap.parse_args()
    import torch
    rows = throughput(a)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows, "twin_scene": None if a.skip_cases else twin(a),
           "note": "wall-clock milliseconds of the synchronous calls (upload, conversion, kernels, download), median of the repetitions after one "
                   "warm-up call; both entry points run in this process on the same 50 x 4096^2 descriptor sets.  resident_f16: sets packed once by "
                   "sfd2_desc_pack and read in place by both.  sfd2_match_batch serves NNM by its single-GEMM kernel and ratio 0.8 by the two-GEMM "
                   "top-2 kernel the guided kernel is derived from.  matches_kept under a guide counts every pair's rows; the pairs share image 0's "
                   "descriptors, so only pair 0's key points belong to them and the other pairs' counts say nothing about matching quality."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
