"""Times `python -m sfd2_amd.localizer` (sfd2_amd.localizer.run) on synthetic files at the workload's size (needs a GPU): --images
retrieved database images of about --keypoints key points per query (default 50 x 4096; the scene of tools/localize_bench.py).

  * queries/s of run() for --stage1 host (the earlier stage 1: matches to the host, match_cluster_2D per cluster) and device, for
    --init_type sng and clu, with and without --do_covisible_opt; every combination --runs times, alternating; a --stage1 device window is
    --device-repeat calls of the command, so that it lasts seconds;
  * the two --do_covisible_opt rows with --stage1 device also with --frames device (key suffix _frames): the frame selection as one
    sfd2_covis_frames call per round; per run the share of the time spent in the host functions MapIndex.covisible_frames / _by_pose
    and the share of the selections the host functions decided (the fallbacks of the status protocol);
  * sfd2_covis_frames alone: 1 000 obs tasks, 50 frames each, in one call on the map of --big-images images resident on the device,
    against MapIndex.covisible_frames per task;
  * sfd2_covis_clusters (MapIndex.clusters, one call, upload included) against a plain Python search, on the scene's map and on a
    map of --big-images images, there with the image table in LDS and in global scratch.
Wall clock around calls that end in a device synchronise.  Writes one JSON document (default profiles/localizer_bench.json).

    python tools/localizer_bench.py [--images 50] [--keypoints 4096] [--queries 64] [--device-repeat 8] [--runs 2] [--out profiles/localizer_bench.json]"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from localize_bench import _Img, _Pt, localize_scene  # noqa: E402


def write_files(root, cam, store, images, points3D, queries):
    from sfd2_amd import colmap_io, feature_io
    cameras = {1: colmap_io.Camera(1, cam["model"], cam["width"], cam["height"], cam["params"])}
    ims = {i: colmap_io.Image(id=i, qvec=im.qvec, tvec=im.tvec, camera_id=1, name=im.name, xys=np.zeros((len(im.point3D_ids), 2)),
                              point3D_ids=np.asarray(im.point3D_ids, dtype=np.int64)) for i, im in images.items()}
    pts = {p: colmap_io.Point3D(id=p, xyz=pt.xyz, rgb=np.zeros(3, np.uint8), error=0.0, image_ids=np.asarray(pt.image_ids, dtype=np.int32),
                                point2D_idxs=np.zeros(len(pt.image_ids), np.int32)) for p, pt in points3D.items()}
    colmap_io.write_model(cameras, ims, pts, os.path.join(root, "model"))
    with open(os.path.join(root, "queries.txt"), "w") as f:
        for q in queries:
            f.write(" ".join([q, cam["model"], str(cam["width"]), str(cam["height"])] + [repr(float(v)) for v in cam["params"]]) + "\n")
    rs = np.random.RandomState(0)
    names = [im.name for im in images.values()]
    with open(os.path.join(root, "retrieval.txt"), "w") as f:
        for q in queries:
            for i in rs.permutation(len(names)):
                f.write(f"{q} {names[i]}\n")
    feats = os.path.join(root, "feats-bench.pack")
    st = feature_io.open_store(feats, "a")
    for name, g in store.items():
        feature_io.write_features(st, name, g)
    st.close()
    return ["--dataset", "aachen", "--db_imglist_fn", "x", "--reference_sfm", os.path.join(root, "model"), "--queries", os.path.join(root, "queries.txt"),
            "--retrieval", os.path.join(root, "retrieval.txt"), "--features", feats, "--save_root", os.path.join(root, "out"), "--with_match",
            "--ransac_thresh", "12", "--inlier_thresh", "50", "--opt_type", "clurefobs", "--covisibility_frame", "50", "--iters", "1", "--radius", "30"]


def search(frame_ids, images, points3D):
    """The clustering as a plain Python search (the reference's shape: sets per explored frame)."""
    listed, visited, clusters = set(frame_ids), set(), []
    for f in frame_ids:
        if f in visited:
            continue
        members, todo = [], [f]
        while todo:
            a = todo.pop()
            if a in visited:
                continue
            visited.add(a)
            members.append(a)
            near = set(int(j) for p in images[a].point3D_ids if p != -1 for j in points3D[int(p)].image_ids)
            todo.extend((near & listed) - visited)
        clusters.append(members)
    return sorted(clusters, key=len, reverse=True)


def big_map(n_images, obs=400, seed=2):
    """n_images cameras along a line; image i observes `obs` points of a window that moves with i, so that neighbours share points."""
    rs = np.random.RandomState(seed)
    per, seen = 60, {}
    images = {}
    for i in range(n_images):
        ids = (i * per + rs.choice(8 * per, obs, replace=False)).astype(np.int64)
        images[i + 1] = _Img(f"db/{i:06d}.jpg", np.array([1.0, 0, 0, 0]), np.zeros(3), ids)
        for p in ids:
            seen.setdefault(int(p), []).append(i + 1)
    return images, {p: _Pt(np.zeros(3), v) for p, v in seen.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=50)
    ap.add_argument("--keypoints", type=int, default=4096)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--device-repeat", type=int, default=8, help="calls of the command per timed window with --stage1 device")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--big-images", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localizer_bench.json"))
    a = ap.parse_args()
    import torch
    from sfd2_amd import _lib, covis, localizer
    res = {"images": a.images, "keypoints": a.keypoints, "queries": a.queries, "device": torch.cuda.get_device_name(0), "run": {}}
    cam, store, images, points3D, queries = localize_scene(n_pts=int(a.keypoints / 1.2), n_db=a.images, n_q=a.queries)
    res["query_keypoints_mean"] = float(np.mean([len(store[q]["keypoints"]) for q in queries]))
    res["db_keypoints_mean"] = float(np.mean([len(im.point3D_ids) for im in images.values()]))
    spent = {"t": 0.0}
    inner = covis.MapIndex.covisible_frames

    def timed_frames(self, *args, **kw):
        t0 = time.perf_counter()
        try:
            return inner(self, *args, **kw)
        finally:
            spent["t"] += time.perf_counter() - t0
    covis.MapIndex.covisible_frames = timed_frames
    inner_batch = covis.MapIndex.covisible_frames_batch
    routed = {"tasks": 0, "host": 0}

    def counted_batch(self, *args, **kw):
        before = (self.frames_tasks, self.frames_host)
        try:
            return inner_batch(self, *args, **kw)
        finally:
            routed["tasks"] += self.frames_tasks - before[0]
            routed["host"] += self.frames_host - before[1]
    covis.MapIndex.covisible_frames_batch = counted_batch
    with tempfile.TemporaryDirectory() as root:
        base = write_files(root, cam, store, images, points3D, queries)
        combos = [(s1, it, cv, fr) for it in ("sng", "clu") for cv in (False, True) for s1 in ("host", "device")
                  for fr in (("host", "device") if cv and s1 == "device" else ("host",))]
        outputs = {}
        for rep in range(a.runs + 1):                              # repetition 0 warms up: code objects, resident sets, buffers
            for s1, it, cv, fr in combos:
                argv = base + ["--stage1", s1, "--init_type", it, "--frames", fr] + (["--do_covisible_opt"] if cv else [])
                spent["t"] = 0.0
                routed["tasks"] = routed["host"] = 0
                inner_runs = a.device_repeat if s1 == "device" else 1          # a timed window of seconds, not of a fraction of one
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    for _ in range(inner_runs):
                        stem = localizer.main(argv)
                dt = (time.perf_counter() - t0) / inner_runs
                key = f"{it}_{'covis' if cv else 'plain'}_{s1}" + ("_frames" if fr == "device" else "")
                print(f"rep {rep} {key}: {dt:.2f} s per run", file=sys.stderr, flush=True)
                txt = open(stem + ".txt").read()
                assert outputs.setdefault((it, cv), txt) == txt, f"{key}: the pose file differs between the --stage1 / --frames settings"
                if rep:
                    e = res["run"].setdefault(key, {"queries_per_s": [], "covisible_frames_share": [], "window_s": []})
                    e["window_s"].append(dt * inner_runs)
                    e["queries_per_s"].append(len(queries) / dt)
                    e["covisible_frames_share"].append(spent["t"] / (dt * inner_runs) if cv else 0.0)
                    if fr == "device":
                        e.setdefault("host_fallback_share", []).append(routed["host"] / max(routed["tasks"], 1))
                        e["selections_per_run"] = routed["tasks"] // inner_runs
                    e["localised"] = len(txt.splitlines()) - len(open(stem + ".txt.failed").read().splitlines())
    covis.MapIndex.covisible_frames = inner
    covis.MapIndex.covisible_frames_batch = inner_batch
    # ---- the clustering alone
    rs = np.random.RandomState(5)
    clu = {}
    for label, (ims, pts), nq, k in (("scene_map", (images, points3D), 1000, min(a.images, 50)), ("big_map", big_map(a.big_images), 1000, 50)):
        mi = covis.MapIndex(ims, pts)
        ids = np.array(list(ims))
        lists = []
        for _ in range(nq):                                        # retrieval-like: a few runs of neighbouring images
            starts = rs.randint(0, max(1, len(ids) - 12), 5)
            li = list(dict.fromkeys(int(ids[min(s + j, len(ids) - 1)]) for s in starts for j in rs.choice(12, 10, replace=False)))
            lists.append(li[:k])
        mi.csr()
        e = {"n_images": len(ims), "queries": nq, "frames_per_query": float(np.mean([len(li) for li in lists])), "lds_ms": [], "global_ms": []}
        for rep in range(a.runs + 1):
            for key, flag in (("lds_ms", False), ("global_ms", True)):
                t0 = time.perf_counter()
                got = mi.clusters(lists, global_slots=flag)
                if rep:
                    e[key].append((time.perf_counter() - t0) * 1e3)
        n_py = 20
        t0 = time.perf_counter()
        want = [search(li, ims, pts) for li in lists[:n_py]]
        e["python_ms_per_query"] = (time.perf_counter() - t0) * 1e3 / n_py
        e["device_ms_per_query"] = [v / nq for v in e["lds_ms"]]
        assert [[len(c) for c in g] for g in got[:n_py]] == [[len(c) for c in w] for w in want]
        assert [sorted(map(sorted, g)) for g in got[:n_py]] == [sorted(map(sorted, w)) for w in want]
        e["clusters_per_query"] = float(np.mean([len(g) for g in got]))
        clu[label] = e
    res["covis_clusters"] = clu
    # ---- the frame selection alone: the big map resident on the device, 1 000 obs tasks of 50 frames in one call
    print("covis_frames", file=sys.stderr, flush=True)
    mi = mi.to_device(0)                                           # the last map of the loop above: big_map
    ids = np.array(list(mi.images))
    tasks = [dict(frame_id=int(f)) for f in ids[rs.randint(0, len(ids), 1000)]]
    e = {"n_images": len(ids), "tasks": len(tasks), "covisibility_frame": 50, "call_ms": []}
    for rep in range(a.runs + 1):
        before = mi.frames_host
        t0 = time.perf_counter()
        got = mi.covisible_frames_batch(tasks, kind="obs", covisibility_frame=50, obs_th=3)
        if rep:
            e["call_ms"].append((time.perf_counter() - t0) * 1e3)
        e["host_fallbacks"] = mi.frames_host - before
    n_py = 20
    t0 = time.perf_counter()
    want = [mi.covisible_frames(t["frame_id"], covisibility_frame=50, obs_th=3) for t in tasks[:n_py]]
    e["host_ms_per_task"] = (time.perf_counter() - t0) * 1e3 / n_py
    e["device_ms_per_task"] = [v / len(tasks) for v in e["call_ms"]]
    assert got[:n_py] == [[int(v) for v in w] for w in want]
    e["frames_per_task"] = float(np.mean([len(g) for g in got]))
    res["covis_frames"] = e
    res["frames_default"] = localizer.FRAMES_DEFAULT
    res["lds_table_bound_images"] = _lib.CLUSTER_LDS_IMAGES
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
