"""The three pair selections (sfd2_amd.pairs) on a synthetic set at the scale of the reference's largest configuration: 1 000 queries
x 5 000 db images x d 4096 with k = 50 (retrieval), a 5 000-image map with ~2 000 observed points per image and tracks of ~6
(covisibility), 5 000 poses (poses).  Per stage: device milliseconds from HIP events on the library's stream around the whole call
(uploads and downloads included), and the host baseline on the same box -- torch CPU einsum + topk for retrieval, the
reference-shaped loops of tests/pairs_ref.py for the other two.  For retrieval also the call with the descriptors already on the
device and, from it, the achieved share of the 157.3 TFLOP/s f32-matrix peak.

    python tools/pairs_bench.py [--reps 3] [--baseline_images 0] [--out profiles/pairs_bench.json]

The covisibility baseline is a Python triple loop: --baseline_images N runs it on the first N images only and scales the time
linearly to all of them; 0 (the default) runs it on every image."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32_MATRIX_PEAK_TFLOPS = 157.3


def make_map(n_images, obs_per_image, track_len, window, seed):
    """CSRs of a map: every point is seen by `track_len - 2 .. track_len + 2` images drawn inside a window of the image line."""
    rs = np.random.RandomState(seed)
    n_points = n_images * obs_per_image // track_len
    start = rs.randint(0, n_images - window, n_points)
    length = rs.randint(track_len - 2, track_len + 3, n_points)
    order = np.argsort(rs.uniform(size=(n_points, window)), axis=1)
    keep = np.arange(window)[None, :] < length[:, None]
    track_image = (start[:, None] + order)[keep].astype(np.int32)
    track_offsets = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    point_of = np.repeat(np.arange(n_points, dtype=np.int32), length)
    by_image = np.argsort(track_image, kind="stable")
    obs_point = point_of[by_image]
    obs_offsets = np.concatenate([[0], np.cumsum(np.bincount(track_image, minlength=n_images))]).astype(np.int64)
    return {"obs_offsets": obs_offsets, "obs_point": obs_point, "track_offsets": track_offsets, "track_image": track_image}


def device_ms(ctx, fn, reps):
    """Median milliseconds of fn() between two HIP events on the library's stream; the first call warms up and is not counted."""
    import torch
    stream = torch.cuda.ExternalStream(ctx.stream, device=torch.device("cuda", ctx.device))
    out, times = None, []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        e1.synchronize()
        if rep:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), times, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--db", type=int, default=5000)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--obs_per_image", type=int, default=2000)
    ap.add_argument("--track_len", type=int, default=6)
    ap.add_argument("--covis_k", type=int, default=20)
    ap.add_argument("--poses", type=int, default=5000)
    ap.add_argument("--poses_k", type=int, default=20)
    ap.add_argument("--baseline_images", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pairs_ref as pr
    from sfd2_amd import _lib, pairs as P
    ctx = _lib.default_context(0)
    res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "reps": a.reps}

    # retrieval
    rs = np.random.RandomState(0)
    q = rs.standard_normal((a.queries, a.dim)).astype(np.float32)
    db = rs.standard_normal((a.db, a.dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    ms, all_ms, (idx, sim) = device_ms(ctx, lambda: P.retrieval_topk(q, db, a.k), a.reps)
    qd, dd = torch.from_numpy(q).cuda(), torch.from_numpy(db).cuda()
    ms_res, all_res, (idx_r, _) = device_ms(ctx, lambda: P.retrieval_topk(qd, dd, a.k), a.reps)
    tq, tdb = torch.from_numpy(q), torch.from_numpy(db)
    host = []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        want = torch.topk(torch.einsum("id,jd->ij", tq, tdb), a.k, dim=1)
        host.append((time.perf_counter() - t0) * 1e3)
    flop = 2.0 * a.queries * a.db * a.dim
    res["retrieval"] = {"queries": a.queries, "db": a.db, "dim": a.dim, "k": a.k, "device_ms_with_uploads": ms, "device_ms_all": all_ms,
                        "device_ms_inputs_resident": ms_res, "device_ms_inputs_resident_all": all_res,
                        "tflops_inputs_resident": flop / (ms_res * 1e-3) / 1e12,
                        "share_of_f32_matrix_peak": flop / (ms_res * 1e-3) / 1e12 / F32_MATRIX_PEAK_TFLOPS,
                        "host_ms_torch_einsum_topk": float(np.median(host[1:])), "host_over_device": float(np.median(host[1:])) / ms,
                        "rows_equal_to_host_topk": float(np.mean((idx == want.indices.numpy()).all(axis=1))),
                        "resident_equals_uploaded": bool(np.array_equal(idx, idx_r))}
    print(json.dumps(res["retrieval"]), flush=True)

    # covisibility
    m = make_map(a.images, a.obs_per_image, a.track_len, 4 * a.track_len, 1)
    covis = {}
    for name, glob in (("lds", False), ("global", True)):
        ms, all_ms, (ci, cc, cn) = device_ms(ctx, lambda: P.covisibility_topk_csr(m["obs_offsets"], m["obs_point"], m["track_offsets"], m["track_image"],
                                                                                  a.covis_k, global_counters=glob), a.reps)
        covis[name] = (ms, all_ms, ci, cn)
    nb = a.images if a.baseline_images <= 0 else min(a.baseline_images, a.images)
    sub = dict(m, obs_offsets=m["obs_offsets"][:nb + 1])
    t0 = time.perf_counter()
    loops = pr.covisibility_loops(sub, a.covis_k)
    host_ms = (time.perf_counter() - t0) * 1e3
    ci, cn = covis["lds"][2], covis["lds"][3]
    dev_pairs = [(i, int(j)) for i in range(nb) for j in ci[i, :cn[i]]]
    res["covisibility"] = {"images": a.images, "observations": int(m["obs_offsets"][-1]), "points": len(m["track_offsets"]) - 1, "k": a.covis_k,
                           "device_ms_with_uploads": covis["lds"][0], "device_ms_all": covis["lds"][1],
                           "device_ms_with_uploads_global_counters": covis["global"][0], "device_ms_global_counters_all": covis["global"][1],
                           "paths_identical": bool(np.array_equal(covis["lds"][2], covis["global"][2])),
                           "host_ms_loops_measured": host_ms, "host_images_measured": nb, "host_ms_loops_scaled_to_all_images": host_ms * a.images / nb,
                           "host_over_device": host_ms * a.images / nb / covis["lds"][0], "pairs_equal_to_host_loops": dev_pairs == loops}
    print(json.dumps(res["covisibility"]), flush=True)

    # poses
    qs, ts = [], []
    for s in range((a.poses + 299) // 300):                    # the tests' 300-pose field, repeated 12 apart along y
        q300, t300 = pr.make_poses(s, 300)
        R = np.stack([pr.qvec2rotmat(x) for x in q300])
        qs.append(q300)
        ts.append(t300 - R @ np.array([0.0, 12.0 * s, 0.0]))
    qv, tv = np.concatenate(qs)[:a.poses], np.concatenate(ts)[:a.poses]
    ms, all_ms, (pi, pd, pn) = device_ms(ctx, lambda: P.poses_topk_arrays(qv, tv, a.poses_k, 30.0), a.reps)
    t0 = time.perf_counter()
    loops = pr.poses_loops(qv, tv, a.poses_k, 30.0)
    host_ms = (time.perf_counter() - t0) * 1e3
    dev_pairs, host_pairs = {(i, int(j)) for i in range(a.poses) for j in pi[i, :pn[i]]}, set(loops)
    res["poses"] = {"poses": a.poses, "k": a.poses_k, "rotation_threshold": 30.0, "device_ms_with_uploads": ms, "device_ms_all": all_ms,
                    "host_ms_numpy_tables_and_partition": host_ms, "host_over_device": host_ms / ms,
                    "pairs": len(dev_pairs), "pairs_shared_with_host": len(dev_pairs & host_pairs), "host_pairs": len(host_pairs)}
    print(json.dumps(res["poses"]), flush=True)
    res["note"] = ("device times: HIP events on the library's stream around the whole call, uploads and downloads included, median of reps; "
                   "host baselines on the same box; the covisibility loops are measured on host_images_measured images and scaled linearly")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
