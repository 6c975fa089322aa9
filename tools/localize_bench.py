"""Times the localiser's match -> 2D-3D assembly step and the covisibility stage on synthetic data (needs a GPU).

  (a) the earlier path: StoreMatcher.match to the host, then localize.match_cluster_2D (a Python loop per key point);
  (b) StoreMatcher.match_assemble: sfd2_match_batch left on the device + sfd2_assemble_2d3d.
Per query, wall clock (transfers included) and HIP events on the context's stream, for --images x --keypoints (default 50 x 4096,
about 40 % of the key points matched per image).  Then queries/s of localize.localize_queries with and without the covisibility
stage on a small geometric scene.  Writes one JSON document (default profiles/covis_bench.json).

    python tools/localize_bench.py [--images 50] [--keypoints 4096] [--repeat 5] [--out profiles/covis_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Img:
    def __init__(self, name, qvec, tvec, point3D_ids):
        self.name, self.qvec, self.tvec, self.point3D_ids = name, qvec, tvec, point3D_ids


class _Pt:
    def __init__(self, xyz, image_ids):
        self.xyz, self.image_ids = xyz, image_ids


def _unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def assembly_set(k, n, frac=0.4, seed=0):
    """One query of n descriptors and k database images of n key points: in each image frac * n rows are noisy copies of query rows
    (their 3D point is one of three per query key point, so the de-duplication has work), the rest clutter without a 3D point
    match.  Every key point of a database image has a 3D point."""
    rs = np.random.RandomState(seed)
    Q = _unit(rs.standard_normal((n, 128)))
    store = {"query/q.jpg": {"keypoints": (rs.rand(n, 2) * [1024, 768]).astype(np.float32), "scores": rs.rand(n).astype(np.float32),
                             "descriptors": np.ascontiguousarray(Q.T)}}
    images, seen = {}, {}
    m = int(frac * n)
    for i in range(k):
        src = rs.choice(n, m, replace=False)
        d = np.concatenate([_unit(Q[src] + 0.02 * rs.standard_normal((m, 128))), _unit(rs.standard_normal((n - m, 128)))])
        ids = np.concatenate([src + n * (i % 3), 3 * n + rs.randint(0, n, n - m)]).astype(np.int64)
        order = rs.permutation(n)
        name = f"db/{i:03d}.jpg"
        images[i + 1] = _Img(name, np.array([1.0, 0, 0, 0]), np.zeros(3), ids[order])
        store[name] = {"keypoints": np.zeros((n, 2), np.float32), "scores": np.zeros(n, np.float32), "descriptors": np.ascontiguousarray(d[order].T)}
        for p in ids:
            seen.setdefault(int(p), []).append(i + 1)
    points3D = {p: _Pt(rs.rand(3) * 10, v + [0, 0, 0]) for p, v in seen.items()}
    return store, images, points3D


def _rot(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def localize_scene(n_pts=3000, n_db=16, n_q=20, seed=1):
    """A geometric scene: points in front of a base camera (PINHOLE 800 px, 1024 x 768), database and query cameras near it; key points
    are projections (1 px noise for the queries) with matching descriptors, plus clutter."""
    rs = np.random.RandomState(seed)
    cam = {"model": "PINHOLE", "width": 1024, "height": 768, "params": [800.0, 800.0, 512.0, 384.0]}
    px = np.stack([rs.uniform(20, 1004, n_pts), rs.uniform(20, 748, n_pts)], 1)
    depth = 1.0 / rs.uniform(1.0 / 60, 1.0 / 4, n_pts)
    X = np.concatenate([(px - [512.0, 384.0]) / 800.0, np.ones((n_pts, 1))], 1) * depth[:, None]
    D = _unit(rs.standard_normal((n_pts, 128)))

    def near(deg, shift):
        ax = rs.standard_normal(3)
        a = np.radians(deg) / 2
        q = np.concatenate([[np.cos(a)], np.sin(a) * ax / np.linalg.norm(ax)])
        return q, -_rot(q) @ (shift * rs.standard_normal(3))

    def view(q, t, noise):
        P = X @ _rot(q).T + t
        uv = P[:, :2] / P[:, 2:3] * 800.0 + [512.0, 384.0]
        p = np.flatnonzero((P[:, 2] > 0.5) & (uv[:, 0] > 2) & (uv[:, 0] < 1022) & (uv[:, 1] > 2) & (uv[:, 1] < 766))
        return p, uv[p] + noise * rs.standard_normal((len(p), 2)), _unit(D[p] + 0.02 * rs.standard_normal((len(p), 128)))

    store, images, seen = {}, {}, {}
    for i in range(1, n_db + 1):
        q, t = near(2.0, 0.2)
        p, uv, d = view(q, t, 0.5)
        name = f"db/{i:03d}.jpg"
        images[i] = _Img(name, q, t, (p + 1000).astype(np.int64))
        store[name] = {"keypoints": uv.astype(np.float32), "scores": np.zeros(len(p), np.float32), "descriptors": np.ascontiguousarray(d.T)}
        for pp in p:
            seen.setdefault(int(pp) + 1000, []).append(i)
    points3D = {p: _Pt(X[p - 1000], v) for p, v in seen.items()}
    queries = []
    for j in range(n_q):
        q, t = near(1.5, 0.15)
        p, uv, d = view(q, t, 1.0)
        nc = len(p) // 4
        name = f"query/{j:03d}.jpg"
        kp = np.concatenate([uv, rs.rand(nc, 2) * [1024, 768]]) - 0.5
        store[name] = {"keypoints": kp.astype(np.float32), "scores": rs.rand(len(kp)).astype(np.float32),
                       "descriptors": np.ascontiguousarray(np.concatenate([d, _unit(rs.standard_normal((nc, 128)))]).T)}
        queries.append(name)
    return cam, store, images, points3D, queries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=50)
    ap.add_argument("--keypoints", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host-repeat", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covis_bench.json"))
    args = ap.parse_args()
    import torch
    from sfd2_amd import _lib, covis, localize
    from sfd2_amd.matcher import Matcher, confs
    mt = Matcher(confs["NNM"]).eval().cuda()
    ctx = _lib.default_context(0)
    stream = torch.cuda.ExternalStream(ctx.stream, device=torch.device("cuda", 0))
    res = {"images": args.images, "keypoints": args.keypoints, "device": torch.cuda.get_device_name(0)}

    # ---- legs (a) and (b)
    store, images, points3D = assembly_set(args.images, args.keypoints)
    mi = covis.MapIndex(images, points3D).to_device(0)
    sm = localize.StoreMatcher(mt, store)
    ids = list(images)
    names, id_lists = [images[i].name for i in ids], [images[i].point3D_ids for i in ids]
    f = store["query/q.jpg"]
    job = dict(desc_q="query/q.jpg", kpq=f["keypoints"], scores=f["scores"], image_ids=ids, obs_th=3, gate=None)
    r = sm.match_assemble(mi, [job])[0]                                # warm-up: sets become resident, buffers allocated
    sm.match("query/q.jpg", names, id_lists)

    def timed(fn, n):
        wall, dev, out = [], [], None
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.sync()
            t0 = time.perf_counter()
            e0.record(stream)
            out = fn()
            e1.record(stream)
            ctx.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
            e1.synchronize()
            dev.append(e0.elapsed_time(e1))
        return float(np.median(wall)), float(np.median(dev)), out

    def leg_a():
        ml = sm.match("query/q.jpg", names, id_lists)
        return localize.match_cluster_2D(f["keypoints"], ml, id_lists, points3D, obs_th=3)

    a_wall, a_dev, a_out = timed(leg_a, args.host_repeat)
    tm = _lib.Timings()
    ctx.lib.sfd2_get_timings(ctx.h, tm)
    b_wall, b_dev, b_out = timed(lambda: sm.match_assemble(mi, [job])[0], args.repeat)
    assert b_out["query_idx"].tolist() == [int(v) for v in a_out[4]] and b_out["points2D"].tobytes() == np.ascontiguousarray(a_out[2]).tobytes()
    # the assembly alone, on matches already in HBM
    ml = sm.match("query/q.jpg", names, id_lists)
    m0 = torch.from_numpy(np.ascontiguousarray(np.stack(ml)).astype(np.int64)).cuda()
    ajob = dict(matches0=m0, images=[(i, r_) for r_, i in enumerate(ids)], kpq=f["keypoints"], scores=f["scores"], obs_th=3, gate=None)
    c_wall, c_dev, _ = timed(lambda: localize.assemble_2d3d(ctx, mi, [ajob]), args.repeat)
    gjob = dict(ajob, gate=(np.array([1.0, 0, 0, 0]), np.array([0.0, 0, 20.0]), {"model": "SIMPLE_RADIAL", "width": 1024, "height": 768,
                                                                               "params": [800.0, 512.0, 384.0, -0.05]}, 1e9))
    g_wall, g_dev, _ = timed(lambda: localize.assemble_2d3d(ctx, mi, [gjob]), args.repeat)
    b20_wall, b20_dev, _ = timed(lambda: sm.match_assemble(mi, [job] * 20), max(1, args.repeat // 2))
    res.update({"correspondences": int(b_out["m"]), "matched": int(sum(int((m >= 0).sum()) for m in ml)),
                "a_match_to_host_then_python_loop": {"wall_ms": a_wall, "stream_ms": a_dev, "match_launch_ms": float(tm.ms_match)},
                "b_match_assemble_on_device": {"wall_ms": b_wall, "stream_ms": b_dev},
                "b_batch_of_20_queries_per_query": {"wall_ms": b20_wall / 20, "stream_ms": b20_dev / 20},
                "assemble_alone": {"wall_ms": c_wall, "stream_ms": c_dev}, "assemble_alone_gated": {"wall_ms": g_wall, "stream_ms": g_dev},
                "speedup_wall_a_over_b": a_wall / b_wall})
    sm.close()

    # ---- localize_queries with and without the covisibility stage
    cam, store, images, points3D, queries = localize_scene()
    mi = covis.MapIndex(images, points3D).to_device(0)
    sm = localize.StoreMatcher(mt, store)
    cl = [images[1], images[2], images[3]]
    stages = []
    for qn in queries:
        ml = sm.match(qn, [im.name for im in cl], [im.point3D_ids for im in cl])
        stages.append(dict(kpq=store[qn]["keypoints"], clusters=[[(im, m) for im, m in zip(cl, ml)]], camera=cam, qname=qn))
    cov = localize.Covis(mi, sm, store, opt_type="clurefobs", covisibility_frame=12, iters=1, radius=30, obs_th=3, opt_th=12)
    for label, c in (("without_covis", None), ("with_covis", cov)):
        localize.localize_queries(stages, 12.0, points3D=points3D, covis=c)
        t0 = time.perf_counter()
        out = localize.localize_queries(stages, 12.0, points3D=points3D, covis=c)
        dt = time.perf_counter() - t0
        res["localize_queries_" + label] = {"queries": len(stages), "queries_per_s": len(stages) / dt, "localised": int(sum(o[2] > 0 for o in out))}
    sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
