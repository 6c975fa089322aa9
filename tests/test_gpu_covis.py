"""The covisibility stage on the MI355X: sfd2_assemble_2d3d against the host loop (sfd2_amd.localize.match_cluster_2D), batch
independence, the reference goldens through the device assembly, StoreMatcher.match_assemble, and the stage end to end."""
import numpy as np
import pytest

import covis_ref as cr
import pose_ref as pr

pytestmark = pytest.mark.gpu

CAM = pr.camera("OPENCV")
RADIUS = 25.0


def _mods():
    import torch
    from sfd2_amd import _lib, covis, localize
    return torch, _lib, covis, localize


def _world(seed, k, n, n_pts=400, n1=96, match_p=0.4, all_matched=False, empty=(), dup=True):
    """A query of n key points against k images: a pose, points in front of it, key points near projections (so the gate splits
    them), per-image point3D_ids with -1 entries and, with dup, the same id at several key points of one image and across images;
    matches0 random (or every key point matched).  Track lengths 0..5."""
    rs = np.random.RandomState(seed)
    q, t, x, X, _ = pr.scene(rs, CAM, n_pts, offset=(30.0, 5.0, -8.0))
    points3D = {50 + 3 * p: cr.Pt(X[p], np.arange(rs.randint(0, 6))) for p in range(n_pts)}
    owner = rs.randint(0, n_pts, n)                                  # key point idx lies near the projection of point owner[idx]
    kpq = (x[owner] + rs.choice([2.0, 60.0], (n, 1)) * rs.uniform(-1, 1, (n, 2))).astype(np.float32)
    images, matches = {}, []
    pool = rs.choice(n_pts, max(8, n_pts // 4), replace=False) if dup else np.arange(n_pts)
    for i in range(k):
        if i in empty:
            ids = np.zeros(0, dtype=np.int64)
        else:
            ids = np.where(rs.rand(n1) < 0.8, 50 + 3 * rs.choice(pool, n1), -1)
        images[i + 1] = cr.Img(f"db/{i}.jpg", q, t, ids)
        if ids.size == 0:
            m = rs.randint(-1, 1, n)
        elif all_matched:
            m = rs.randint(0, n1, n)
        else:
            m = np.where(rs.rand(n) < match_p, rs.randint(0, n1, n), -1)
            hit = rs.rand(n) < 0.3                                   # often the owner's own point, so that the gate keeps some
            for idx in np.flatnonzero(hit & (m >= 0)):
                w = np.flatnonzero(ids == 50 + 3 * owner[idx])
                if len(w):
                    m[idx] = w[0]
        matches.append(m.astype(np.int64))
    scores = rs.rand(n).astype(np.float32)
    return dict(q=q, t=t, kpq=kpq, scores=scores, images=images, points3D=points3D, matches=matches)


def _host(localize, w, obs_th, gate):
    ids_list = [w["images"][i + 1].point3D_ids for i in range(len(w["matches"]))]
    info, mp3d, mkpq, ids3d, q_ids = localize.match_cluster_2D(w["kpq"], w["matches"], ids_list, w["points3D"], obs_th=obs_th, gate=gate)
    image_idx = [i for i in range(len(ids_list)) if i in info for _ in info[i]["qids"]]
    counts = [len(info[i]["qids"]) if i in info else 0 for i in range(len(ids_list))]
    return mp3d, mkpq, ids3d, q_ids, image_idx, counts


def _gate(w):
    rs = np.random.RandomState(5)
    q0 = cr.compose(cr.small_rot(rs, 0.3), w["q"])
    return (q0, -pr.qvec2rotmat(q0) @ (pr.centre(w["q"], w["t"]) + 0.01), CAM, RADIUS)


def _assert_margin(covis, w, gate):
    """No candidate's gate error within 1e-6 px of the radius (every (key point, matched point) pair, kept or not)."""
    for i, m in enumerate(w["matches"]):
        ids = w["images"][i + 1].point3D_ids
        if ids.size == 0:
            continue
        idx = np.flatnonzero(m >= 0)
        pid = ids[m[idx]]
        idx, pid = idx[pid != -1], pid[pid != -1]
        if len(idx) == 0:
            continue
        X = np.array([w["points3D"][int(p)].xyz for p in pid])
        e = np.sqrt(((w["kpq"][idx].astype(np.float64) - covis.reproject(X, gate[0], gate[1], gate[2])) ** 2).sum(1))
        assert (np.abs(e - gate[3]) > 1e-6).all()


def _job(torch, w, obs_th, gate, capacity=None):
    m = torch.from_numpy(np.ascontiguousarray(np.stack(w["matches"]))).cuda() if w["matches"] else None
    return dict(matches0=m, images=[(i + 1, i) for i in range(len(w["matches"]))], kpq=w["kpq"], scores=w["scores"], obs_th=obs_th, gate=gate,
                capacity=capacity)


def _ctx(_lib):
    return _lib.default_context(0)


def _equal(covis_mi, r, want):
    mp3d, mkpq, ids3d, q_ids, image_idx, counts = want
    assert r["m"] == len(q_ids)
    assert r["query_idx"].tolist() == [int(v) for v in q_ids]
    assert covis_mi.point_ids[r["point_row"]].tolist() == [int(v) for v in ids3d]
    assert r["image_idx"].tolist() == image_idx
    assert r["image_counts"].tolist() == counts
    assert r["points2D"].dtype == np.float64 and r["points2D"].tobytes() == np.ascontiguousarray(mkpq).tobytes()
    assert r["points3D"].tobytes() == np.ascontiguousarray(mp3d).tobytes()


CASES = {  # name: _world arguments
    "random": dict(k=7, n=1000), "all_minus_one": dict(k=5, n=300, match_p=0.0), "all_matched": dict(k=6, n=513, all_matched=True),
    "k1": dict(k=1, n=700), "k50": dict(k=50, n=640), "k130": dict(k=130, n=257), "n1": dict(k=9, n=1), "n63": dict(k=9, n=63),
    "n64": dict(k=9, n=64), "n65": dict(k=9, n=65), "n4096": dict(k=12, n=4096, n_pts=3000, n1=2048), "empty_images": dict(k=8, n=500, empty=(0, 3, 7)),
    "no_duplicates": dict(k=6, n=400, dup=False),
}


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("obs_th", [0, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_assemble_equals_host_loop(name, obs_th, gated):
    torch, _lib, covis, localize = _mods()
    w = _world(sum(map(ord, name)), **CASES[name])
    gate = _gate(w) if gated else None
    if gated:
        _assert_margin(covis, w, gate)
    mi = covis.MapIndex(w["images"], w["points3D"])
    want = _host(localize, w, obs_th, gate)
    r = localize.assemble_2d3d(_ctx(_lib), mi, [_job(torch, w, obs_th, gate)])[0]
    _equal(mi, r, want)
    assert r["score"].tobytes() == w["scores"][r["query_idx"]].tobytes()
    if name in ("random", "all_matched", "k50"):
        assert 0 < r["m"] and len(set(zip(want[3], want[2]))) == r["m"]


def test_empty_jobs_in_a_batch():
    """A query without key points and a job without images, next to an ordinary job."""
    torch, _lib, covis, localize = _mods()
    w = _world(12, k=4, n=300)
    mi = covis.MapIndex(w["images"], w["points3D"])
    want = _host(localize, w, 0, None)
    none = dict(matches0=None, images=[(1, -1), (2, -1)], kpq=np.zeros((0, 2), np.float32), scores=None, obs_th=0, gate=None)
    noimg = dict(matches0=None, images=[], kpq=w["kpq"], scores=w["scores"], obs_th=0, gate=None)
    a, b, c = localize.assemble_2d3d(_ctx(_lib), mi, [none, _job(torch, w, 0, None), noimg])
    assert a["m"] == 0 and a["image_counts"].tolist() == [0, 0] and c["m"] == 0 and len(c["image_counts"]) == 0
    _equal(mi, b, want)


@pytest.mark.parametrize("empty", ["n0_with_scores", "capacity0_k1"])
@pytest.mark.parametrize("empty_at", [0, 1])
def test_a_job_with_empty_arrays_beside_a_small_one(empty, empty_at):
    """Two jobs with host inputs and host outputs: one whose key points AND scores are empty (two empty slots of the packed input),
    or whose six output arrays have capacity 0, before or after a job of n = 8, k = 2, which is what the host loop gives."""
    torch, _lib, covis, localize = _mods()
    w = _world(21, k=2, n=8, all_matched=True, dup=False)
    mi = covis.MapIndex(w["images"], w["points3D"])
    want = _host(localize, w, 0, None)
    assert len(want[3]) > 0
    if empty == "n0_with_scores":
        e = dict(matches0=None, images=[(1, -1)], kpq=np.zeros((0, 2), np.float32), scores=np.zeros(0, np.float32), obs_th=0, gate=None)
    else:
        e = dict(matches0=None, images=[(1, -1)], kpq=w["kpq"], scores=w["scores"], obs_th=0, gate=None, capacity=0)
    jobs = [None, None]
    jobs[empty_at], jobs[1 - empty_at] = e, _job(torch, w, 0, None)
    res = localize.assemble_2d3d(_ctx(_lib), mi, jobs)
    assert res[empty_at]["m"] == 0 and res[empty_at]["image_counts"].tolist() == [0]
    _equal(mi, res[1 - empty_at], want)
    assert res[1 - empty_at]["score"].tobytes() == w["scores"][res[1 - empty_at]["query_idx"]].tobytes()


def test_gate_removes_and_keeps():
    torch, _lib, covis, localize = _mods()
    w = _world(11, k=7, n=1000)
    gate = _gate(w)
    mi = covis.MapIndex(w["images"], w["points3D"])
    a = localize.assemble_2d3d(_ctx(_lib), mi, [_job(torch, w, 0, None)])[0]["m"]
    b = localize.assemble_2d3d(_ctx(_lib), mi, [_job(torch, w, 0, gate)])[0]["m"]
    assert 0 < b < a


def test_capacity_exact_and_one_short():
    torch, _lib, covis, localize = _mods()
    w = _world(3, k=7, n=1000)
    gate = _gate(w)
    mi = covis.MapIndex(w["images"], w["points3D"])
    want = _host(localize, w, 3, gate)
    m = len(want[3])
    assert m > 10
    r = localize.assemble_2d3d(_ctx(_lib), mi, [_job(torch, w, 3, gate, capacity=m)])[0]
    _equal(mi, r, want)
    # one short: an error that reports m, and device buffers of m rows (one more than the capacity stated) stay untouched
    ctx = _ctx(_lib)
    job = _job(torch, w, 3, gate, capacity=m - 1)
    with pytest.raises(localize.AssembleError) as e:
        localize.assemble_2d3d(ctx, mi, [job])
    assert e.value.m == [m] and e.value.status == [_lib.ASM_ST_CAPACITY]
    import ctypes
    bufs = {"points2D": torch.full((m, 2), -7.0, dtype=torch.float64, device="cuda"), "points3D": torch.full((m, 3), -7.0, dtype=torch.float64, device="cuda"),
            "point_row": torch.full((m,), -7, dtype=torch.int32, device="cuda"), "query_idx": torch.full((m,), -7, dtype=torch.int32, device="cuda"),
            "image_idx": torch.full((m,), -7, dtype=torch.int32, device="cuda"), "score": torch.full((m,), -7.0, dtype=torch.float32, device="cuda")}
    k, n = len(w["matches"]), len(w["kpq"])
    imgs = (_lib.AssembleImage * k)()
    for i in range(k):
        imgs[i].point_rows, imgs[i].n1 = mi.device_rows(i + 1)
        imgs[i].match_row = i
    counts = np.zeros(k, np.int32)
    kp = np.ascontiguousarray(w["kpq"], np.float32)
    from sfd2_amd.pose import camera_model
    for cap, ok in ((m - 1, False), (m, True)):
        j = _lib.AssembleJob()
        j.matches0, j.images, j.k, j.n, j.match_rows = job["matches0"].data_ptr(), imgs, k, n, k
        j.keypoints, j.scores, j.obs_th, j.gate = kp.ctypes.data, w["scores"].ctypes.data, 3.0, 1
        j.model, params = camera_model(CAM)
        for i in range(8):
            j.params[i] = params[i]
        for i in range(4):
            j.qvec[i] = gate[0][i]
        for i in range(3):
            j.tvec[i] = gate[1][i]
        j.radius, j.capacity = RADIUS, cap
        for name, t in bufs.items():
            setattr(j, name, t.data_ptr())
        j.image_counts = counts.ctypes.data
        table = mi.point_table()
        rc = ctx.lib.sfd2_assemble_2d3d(ctx.h, ctypes.byref(table), ctypes.byref(j), 1, 1, 0)
        assert j.m == m and counts.tolist() == want[5]
        if not ok:
            assert rc != 0 and j.status == _lib.ASM_ST_CAPACITY
            assert all(bool((t == -7).all()) for t in bufs.values())          # nothing written at all, in or past the capacity
        else:
            assert rc == 0 and bufs["query_idx"].cpu().numpy().tolist() == [int(v) for v in want[3]]


def test_match_index_out_of_range_is_an_error_not_a_read():
    torch, _lib, covis, localize = _mods()
    w = _world(4, k=3, n=200)
    w["matches"][1][17] = 96                                         # n1 = 96
    mi = covis.MapIndex(w["images"], w["points3D"])
    with pytest.raises(localize.AssembleError) as e:
        localize.assemble_2d3d(_ctx(_lib), mi, [_job(torch, w, 0, None)])
    assert e.value.status == [_lib.ASM_ST_MATCH_RANGE]


def test_batch_composition_and_order_do_not_change_a_byte():
    torch, _lib, covis, localize = _mods()
    worlds = [_world(100 + i, k=3 + i % 9, n=100 + 97 * i, empty=(1,) if i % 4 == 0 else ()) for i in range(40)]
    # one map for all: shift the ids of world i
    images, points3D, jobs = {}, {}, []
    for wi, w in enumerate(worlds):
        for pid, p in w["points3D"].items():
            points3D[pid + 100000 * wi] = p
        for i, im in w["images"].items():
            images[1000 * wi + i] = cr.Img(f"{wi}/{i}", im.qvec, im.tvec, np.where(im.point3D_ids >= 0, im.point3D_ids + 100000 * wi, -1))
    mi = covis.MapIndex(images, points3D)
    for wi, w in enumerate(worlds):
        j = _job(torch, w, wi % 4, _gate(w) if wi % 2 else None)
        j["images"] = [(1000 * wi + i, r) for i, r in j["images"]]
        jobs.append(j)
    ctx = _ctx(_lib)
    batch = localize.assemble_2d3d(ctx, mi, jobs)
    rev = localize.assemble_2d3d(ctx, mi, jobs[::-1])[::-1]
    again = localize.assemble_2d3d(ctx, mi, jobs)
    fields = ("points2D", "points3D", "point_row", "query_idx", "image_idx", "score", "image_counts")
    for i in (0, 7, 20, 39):
        alone = localize.assemble_2d3d(ctx, mi, [jobs[i]])[0]
        for f in fields:
            assert alone[f].tobytes() == batch[i][f].tobytes(), (i, f)
    for i in range(40):
        for f in fields:
            assert batch[i][f].tobytes() == rev[i][f].tobytes() == again[i][f].tobytes(), (i, f)
    assert sum(b["m"] for b in batch) > 1000


class _ScriptedDeviceMatcher:
    """The scripted matches of covis_ref uploaded as sfd2_match_batch would leave them, then the device assembly."""

    def __init__(self, sc, ctx):
        self.sc, self.ctx = sc, ctx

    def match_assemble(self, map_index, queries):
        torch, _lib, covis, localize = _mods()
        jobs = []
        for q in queries:
            rows, images = [], []
            for d in q["image_ids"]:
                ids = self.sc["images"][d].point3D_ids
                if ids.size == 0 or (ids != -1).sum() <= 3:
                    images.append((d, -1))
                else:
                    images.append((d, len(rows)))
                    rows.append(self.sc["plan"][d])
            m = torch.from_numpy(np.ascontiguousarray(np.stack(rows))).cuda() if rows else None
            jobs.append(dict(matches0=m, images=images, kpq=q["kpq"], scores=q["scores"], obs_th=q["obs_th"], gate=q["gate"]))
        return localize.assemble_2d3d(self.ctx, map_index, jobs)


@pytest.mark.parametrize("name", list(cr.REFINE_CASES))
def test_golden_refinement_through_device_assembly(name):
    from test_covis_host import _run_case, check_against_golden
    torch, _lib, covis, localize = _mods()
    ci = list(cr.REFINE_CASES).index(name)
    sc = cr.refinement_scene(seed=ci)
    sc, ret, refi = _run_case(name, matcher=_ScriptedDeviceMatcher(sc, _ctx(_lib)), sc=sc)
    check_against_golden(name, sc, ret)


# ---------------------------------------------------------------------------------------------------------------- with the matcher
def _scene_with_descriptors(seed=0, n_pts=1500, n_db=14, n_q=20):
    """One world: points in front of a base camera, each with a unit descriptor; database and query cameras near the base pose see
    the points inside their image.  Database images 1 and 2 (the poor cluster) only carry points from the left third of the base
    image.  Query key points: projections with 1 px noise, plus clutter with random descriptors."""
    from sfd2_amd import synth
    rs = np.random.RandomState(seed)
    cam = pr.camera("SIMPLE_RADIAL")
    q, t, x0, X, _ = pr.scene(rs, cam, n_pts, offset=(100.0, 20.0, -30.0))
    D = synth.make_descriptors(n_pts, seed=seed + 1).astype(np.float64)
    W, H = cam["width"], cam["height"]

    def view(qv, tv, noise, keep=None):
        px, z = pr.project(cam, qv, tv, X)
        vis = (z > 0.5) & (px[:, 0] > 2) & (px[:, 0] < W - 2) & (px[:, 1] > 2) & (px[:, 1] < H - 2)
        if keep is not None:
            vis &= keep
        p = np.flatnonzero(vis)
        d = D[p] + 0.02 * rs.standard_normal((len(p), 128))
        return p, px[p] + noise * rs.standard_normal((len(p), 2)), d / np.linalg.norm(d, axis=1, keepdims=True)

    def near(deg, shift):
        qv = cr.compose(cr.small_rot(rs, deg), q)
        return qv, -pr.qvec2rotmat(qv) @ (pr.centre(q, t) + shift * rs.standard_normal(3))

    store, images, seen = {}, {}, {p: [] for p in range(n_pts)}
    for i in range(1, n_db + 1):
        qv, tv = near(2.0, 0.2)
        p, px, d = view(qv, tv, 0.5, keep=(x0[:, 0] < W / 3) if i <= 2 else None)
        n_extra = 40
        ids = np.concatenate([p + 1000, np.full(n_extra, -1)])
        clutter = synth.make_descriptors(n_extra, seed=seed + 100 + i).astype(np.float64)
        order = rs.permutation(len(ids))
        images[i] = cr.Img(f"db/{i:03d}.jpg", qv, tv, ids[order])
        store[images[i].name] = {"keypoints": np.zeros((len(ids), 2), np.float32), "scores": np.zeros(len(ids), np.float32),
                                 "descriptors": np.ascontiguousarray(np.concatenate([d, clutter])[order].T)}
        for pp in p:
            seen[int(pp)].append(i)
    points3D = {p + 1000: cr.Pt(X[p], seen[p]) for p in range(n_pts) if seen[p]}
    queries = []
    for j in range(n_q):
        qv, tv = near(1.5, 0.15)
        p, px, d = view(qv, tv, 1.0)
        n_extra = len(p) // 4
        clutter = synth.make_descriptors(n_extra, seed=seed + 500 + j).astype(np.float64)
        kp = np.concatenate([px, np.stack([rs.uniform(0, W, n_extra), rs.uniform(0, H, n_extra)], 1)]) - 0.5
        name = f"query/{j:03d}.jpg"
        store[name] = {"keypoints": kp.astype(np.float32), "scores": rs.rand(len(kp)).astype(np.float32),
                       "descriptors": np.ascontiguousarray(np.concatenate([d, clutter]).T)}
        queries.append(dict(qname=name, q=qv, t=tv))
    depth = np.median(X @ pr.qvec2rotmat(q).T[:, 2] + t[2])
    return dict(cam=cam, store=store, images=images, points3D=points3D, queries=queries, depth=depth)


@pytest.fixture(scope="module")
def scene():
    torch, _lib, covis, localize = _mods()
    from sfd2_amd.matcher import Matcher, confs as mconfs
    sc = _scene_with_descriptors()
    mt = Matcher(mconfs["NNM"]).eval().cuda()
    sm = localize.StoreMatcher(mt, sc["store"])
    mi = covis.MapIndex(sc["images"], sc["points3D"]).to_device(0)
    yield sc, sm, mi
    sm.close()


def test_match_assemble_equals_match_then_host_loop(scene):
    torch, _lib, covis, localize = _mods()
    sc, sm, mi = scene
    image_ids = list(sc["images"])
    qs = []
    for j, gate in ((0, None), (1, "g"), (2, "g")):
        qn = sc["queries"][j]
        f = sc["store"][qn["qname"]]
        q0 = cr.compose(cr.small_rot(np.random.RandomState(j), 0.3), qn["q"])
        g = None if gate is None else (q0, -pr.qvec2rotmat(q0) @ pr.centre(qn["q"], qn["t"]), sc["cam"], 30.0)
        qs.append(dict(desc_q=qn["qname"], kpq=f["keypoints"], scores=f["scores"], image_ids=image_ids, obs_th=3, gate=g))
    got = sm.match_assemble(mi, qs)
    for q, r in zip(qs, got):
        ims = [sc["images"][i] for i in image_ids]
        ml = sm.match(q["desc_q"], [im.name for im in ims], [im.point3D_ids for im in ims])
        w = dict(kpq=q["kpq"], matches=ml, images={i + 1: im for i, im in enumerate(ims)}, points3D=sc["points3D"])
        if q["gate"] is not None:
            _assert_margin(covis, w, q["gate"])
        _equal(mi, r, _host(localize, w, 3, q["gate"]))
        assert r["m"] > 200


def _first_stage(sc, sm, qn):
    cl = [sc["images"][1], sc["images"][2]]
    ml = sm.match(qn["qname"], [im.name for im in cl], [im.point3D_ids for im in cl])
    return dict(kpq=sc["store"][qn["qname"]]["keypoints"], clusters=[[(im, m) for im, m in zip(cl, ml)]], camera=sc["cam"], qname=qn["qname"])


def test_covisibility_stage_end_to_end(scene):
    torch, _lib, covis, localize = _mods()
    sc, sm, mi = scene
    cov = localize.Covis(mi, sm, sc["store"], opt_type="clurefobs", covisibility_frame=12, iters=1, radius=30, obs_th=3, opt_th=12)
    qn = sc["queries"][0]
    st = _first_stage(sc, sm, qn)
    plain = localize.pose_from_clusters(st["kpq"], st["clusters"], st["camera"], 12.0, inlier_th=20, points3D=sc["points3D"], qname=qn["qname"])
    got = localize.pose_from_clusters(st["kpq"], st["clusters"], st["camera"], 12.0, inlier_th=20, points3D=sc["points3D"], qname=qn["qname"],
                                      covis=cov)
    assert plain[2] > 0 and got[2] > 0
    assert np.degrees(pr.rot_angle(got[0], qn["q"])) <= 0.1
    assert np.linalg.norm(pr.centre(got[0], got[1]) - pr.centre(qn["q"], qn["t"])) <= 0.005 * sc["depth"]
    # the refinement saw correspondences from more images than the cluster had
    ret = localize.pose_refinement_covisibility(qn["qname"], sc["cam"], sc["store"], mi.name_to_id[plain[3]["dbname"]], mi, 12.0, sm,
                                                covisibility_frame=12, iters=1, obs_th=3, opt_th=12, qvec=plain[0], tvec=plain[1], radius=30,
                                                opt_type="clurefobs")
    assert np.array_equal(ret["qvec"], got[0]) and np.array_equal(ret["tvec"], got[1])
    assert len(ret["db_ids"]) > 2 and len(ret["mkpq"]) > sum(len(v["qids"]) for v in localize.match_cluster_2D(
        st["kpq"], [m for _, m in st["clusters"][0]], [im.point3D_ids for im, _ in st["clusters"][0]], sc["points3D"], obs_th=3)[0].values())
    f = sc["store"][qn["qname"]]
    asm = sm.match_assemble(mi, [dict(desc_q=qn["qname"], kpq=f["keypoints"], scores=f["scores"], image_ids=ret["db_ids"], obs_th=3,
                                      gate=(plain[0], plain[1], sc["cam"], 30))])[0]
    assert len(set(asm["image_idx"].tolist())) > 2


def test_localize_queries_equals_single_calls(scene):
    torch, _lib, covis, localize = _mods()
    sc, sm, mi = scene
    cov = localize.Covis(mi, sm, sc["store"], opt_type="clurefobs", covisibility_frame=12, iters=2, radius=30, obs_th=3, opt_th=12)
    stages = [_first_stage(sc, sm, qn) for qn in sc["queries"]]
    got = localize.localize_queries(stages, 12.0, inlier_th=20, points3D=sc["points3D"], covis=cov)
    for st, g, qn in zip(stages, got, sc["queries"]):
        s = localize.pose_from_clusters(st["kpq"], st["clusters"], st["camera"], 12.0, inlier_th=20, points3D=sc["points3D"], qname=st["qname"],
                                        covis=cov)
        assert np.array_equal(g[0], s[0]) and np.array_equal(g[1], s[1]) and g[2] == s[2]
    assert len(got) == 20 and any(g[2] > 0 for g in got)
