"""sfd2_covis_frames on the MI355X against MapIndex.covisible_frames / covisible_frames_by_pose, list for list: the reference's recorded
selections, seeded maps built to separate the two sides of the rule, independence of batch / order / flag / residency, more candidates
than a workgroup has threads, the status protocol at its bands and capacities, bad arguments, and the localiser with --frames device
against --frames host."""
import ctypes
import os
import re

import numpy as np
import pytest

import covis_ref as cr
import frames_ref as fr
import loc_files as lf
import pose_ref as pr
from test_gpu_localizer import files, scene  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "covis.npz"))
SENTINEL = -7


def _mods():
    from sfd2_amd import _lib, covis
    return _lib, covis


def raw(mi, tasks, cap=None, flags=0, on_device=False, frame_index=None, ref_rows=None):
    """One sfd2_covis_frames call on task dicts: (rc, idx [n, cap], n_out, status), the outputs preset to SENTINEL.  frame_index /
    ref_rows override what the first task sends (bad-argument tests)."""
    _lib, covis = _mods()
    import torch
    fc = mi.frames_csr()
    names = covis.MapIndex._FRAMES_ARRAYS
    if on_device:
        keep = {k: torch.from_numpy(fc[k] if fc[k].size else np.zeros(1, fc[k].dtype)).cuda() for k in names}
        ptrs = [keep[k].data_ptr() for k in names]
    else:
        keep, ptrs = fc, [fc[k].ctypes.data if fc[k].size else None for k in names]
    fmap = _lib.FramesMap(*ptrs, len(fc["obs_point"]), len(fc["track_image"]), len(fc["seen_image"]), len(fc["ids"]), len(mi.point_ids),
                          1 if on_device else 0, 0)
    arr = (_lib.FramesTask * len(tasks))()
    off, rows_all = np.zeros(len(tasks) + 1, np.int64), []
    for j, t in enumerate(tasks):
        a = arr[j]
        a.frame = fc["index"][t["frame_id"]] if (frame_index is None or j) else frame_index
        a.kind = _lib.FRAMES_POS if t.get("kind", "obs") == "pos" else _lib.FRAMES_OBS
        a.covisibility_frame, a.obs_th, a.q_th = int(t.get("covisibility_frame", 50)), int(t.get("obs_th", 0)), float(t.get("q_th", 5))
        if t.get("qvec") is not None:
            a.has_pose = 1
            a.qvec[:] = [float(v) for v in t["qvec"]]
            a.tvec[:] = [float(v) for v in t["tvec"]]
        rows = None
        if t.get("ref_3Dpoints") is not None:
            ref = np.asarray(t["ref_3Dpoints"], np.int64)
            rows = mi.point_rows(ref[ref != -1])
        if ref_rows is not None and j == 0:
            rows = np.asarray(ref_rows, np.int32)
        a.use_ref = 0 if rows is None else 1
        off[j + 1] = off[j] + (0 if rows is None else len(rows))
        rows_all.append(np.zeros(0, np.int32) if rows is None else rows.astype(np.int32))
    ref_pts = np.ascontiguousarray(np.concatenate(rows_all))
    if cap is None:
        cap = max(max(a.covisibility_frame, 4) if a.covisibility_frame > 0 else len(fc["ids"]) for a in arr)
    idx = np.full((len(tasks), max(cap, 1)), SENTINEL, np.int32)
    n_out, status = np.full(len(tasks), SENTINEL, np.int32), np.full(len(tasks), SENTINEL, np.int32)
    ctx = _lib.default_context(0)
    rc = ctx.lib.sfd2_covis_frames(ctx.h, ctypes.byref(fmap), arr, len(tasks), off.ctypes.data if off[-1] or any(a.use_ref for a in arr) else None,
                                   ref_pts.ctypes.data if len(ref_pts) else None, cap, idx.ctypes.data, n_out.ctypes.data, status.ctypes.data, flags)
    del keep
    return rc, idx, n_out, status


def lists(mi, idx, n_out):
    ids = mi.frames_csr()["ids"]
    return [[int(v) for v in ids[row[:n]]] for row, n in zip(idx, n_out)]


@pytest.fixture(scope="module")
def selection():
    _lib, covis = _mods()
    images, points3D = cr.selection_map()
    return images, covis.MapIndex(images, points3D)


@pytest.fixture(scope="module")
def random_case():
    """The seeded map, its 64 tasks and the host functions' lists, computed once."""
    _lib, covis = _mods()
    images, points3D = fr.random_map()
    mi = covis.MapIndex(images, points3D)
    tasks = fr.random_tasks(images, points3D)
    host = [[int(v) for v in fr.host_select(mi, t)] for t in tasks]
    return mi, tasks, host


def test_reference_goldens_in_one_call(selection):
    images, mi = selection
    tasks = fr.selection_tasks(images)
    assert all(fr.task_select(mi, t)[1] == 0 for t in tasks)                    # on the CPU first: the reference's cases stay clear of the bands
    rc, idx, n_out, status = raw(mi, tasks)
    assert rc == 0 and status.tolist() == [0] * 15
    got = lists(mi, idx, n_out)
    for c in range(15):
        assert got[c] == GOLD[f"sel{c}"].tolist(), c
        assert (idx[c, n_out[c]:] == -1).all()
    assert mi.covisible_frames_batch(tasks) == got


def test_random_map_equals_host_with_no_fallback(random_case):
    mi, tasks, host = random_case
    assert [fr.task_select(mi, t)[1] for t in tasks] == [0] * 64                # no task in a band: asserted on the CPU ...
    rc, idx, n_out, status = raw(mi, tasks)
    assert rc == 0 and status.tolist() == [0] * 64                              # ... and of the device: zero fallbacks allowed here
    assert lists(mi, idx, n_out) == host
    assert len({len(h) for h in host}) > 8 and min(len(h) for h in host) > 0


def test_result_does_not_depend_on_batch_order_flag_or_residency(random_case):
    _lib, covis = _mods()
    mi, tasks, host = random_case
    cap = len(mi.frames_csr()["ids"])
    base = raw(mi, tasks, cap=cap)
    assert base[0] == 0

    def same(other, order=None):
        assert other[0] == 0
        for a, b in zip(base[1:], other[1:]):
            assert (a if order is None else a[order]).tobytes() == b.tobytes()
    same(raw(mi, tasks[::-1], cap=cap), order=np.arange(64)[::-1])
    same(raw(mi, tasks, cap=cap, flags=_lib.FRAMES_FLAG_GLOBAL_COUNTERS))
    same(raw(mi, tasks, cap=cap, on_device=True))
    same(raw(mi, tasks, cap=cap, on_device=True, flags=_lib.FRAMES_FLAG_GLOBAL_COUNTERS))
    singles = [raw(mi, [t], cap=cap) for t in tasks]
    same((0, np.concatenate([s[1] for s in singles]), np.concatenate([s[2] for s in singles]), np.concatenate([s[3] for s in singles])))
    mi_dev = covis.MapIndex(mi.images, mi.points3D).to_device(0)                # MapIndex's own residency
    assert mi_dev.covisible_frames_batch(tasks) == host and mi_dev._dev_frames is not None and mi_dev.frames_host == 0


@pytest.mark.parametrize("cf", [0, 50])
def test_more_candidates_than_threads(cf):
    _lib, covis = _mods()
    images, points3D = fr.star_map(1500)
    mi = covis.MapIndex(images, points3D)
    t = dict(frame_id=503, kind="obs", covisibility_frame=cf)
    for flags in (0, _lib.FRAMES_FLAG_GLOBAL_COUNTERS):
        rc, idx, n_out, status = raw(mi, [t], flags=flags)
        assert rc == 0 and status[0] == 0
        got = lists(mi, idx, n_out)[0]
        assert got == [int(v) for v in fr.host_select(mi, t)]
        assert len(got) == (1500 if cf == 0 else 50)
        assert got[:3] == [503, 504, 502]                                       # the frame's own entry first, then by count
        assert got[3:] == [i for i in range(1, 1501) if i not in (502, 503, 504)][:len(got) - 3]     # equal counts by ascending index


def test_edges(selection):
    _lib, covis = _mods()
    images, mi = selection
    sc = cr.refinement_scene()
    mr = covis.MapIndex(sc["images"], sc["points3D"])
    rc, idx, n_out, status = raw(mr, [dict(frame_id=3, covisibility_frame=50), dict(frame_id=1, covisibility_frame=50, obs_th=3)])
    assert rc == 0 and n_out[0] == 0 and status.tolist() == [0, 0] and (idx[0] == -1).all()            # a frame with no 3D point
    assert lists(mr, idx, n_out)[1] == [int(v) for v in mr.covisible_frames(1, covisibility_frame=50, obs_th=3)]
    assert 3 in lists(mr, idx, n_out)[1]                                        # connected through a track, counted nowhere
    tasks = fr.selection_tasks(images)
    rc, idx, n_out, status = raw(mi, tasks[:2], cap=3)                           # cap smaller than the result
    assert rc == 0 and status.tolist() == [2, 2] and n_out.tolist() == [0, 0]
    before = mi.frames_host
    assert mi.covisible_frames_batch(tasks[:2], cap=3) == [GOLD["sel0"].tolist(), GOLD["sel1"].tolist()] and mi.frames_host == before + 2
    far = [dict(tasks[8], covisibility_frame=cf) for cf in (0, 4, 5, 50)]       # nothing passes the pose test: the <= 3 fall-back
    rc, idx, n_out, status = raw(mi, far)
    assert rc == 0 and status.tolist() == [0] * 4 and n_out.tolist() == [1, 4, 5, len(fr.host_select(mi, far[3]))]
    assert lists(mi, idx, n_out) == [[int(v) for v in fr.host_select(mi, t)] for t in far]


@pytest.mark.parametrize("ref", [None, []], ids=["own_points", "empty_ref_points"])
def test_a_host_map_without_points(ref):
    """Three images, no point: obs_point, track_image and seen_image (and, with use_ref, ref_points) are empty arrays of a host map,
    each a slot of its own in the uploaded block.  The one task selects nothing, with the restatement's status."""
    import cluster_ref as clr
    _lib, covis = _mods()
    mi = covis.MapIndex(*clr.build_map(3, []))
    fc = mi.frames_csr()
    assert len(fc["ids"]) == 3 and len(fc["obs_point"]) == len(fc["track_image"]) == len(fc["seen_image"]) == 0
    t = dict(frame_id=2, covisibility_frame=50) if ref is None else dict(frame_id=2, covisibility_frame=50, ref_3Dpoints=ref)
    want, want_status = fr.task_select(mi, t)
    assert want == [] and want_status == 0
    for flags in (0, _lib.FRAMES_FLAG_GLOBAL_COUNTERS):
        rc, idx, n_out, status = raw(mi, [t], flags=flags)
        assert rc == 0 and n_out.tolist() == [0] and status.tolist() == [want_status] and (idx == -1).all()


def test_bands_return_status_1_and_the_batch_the_host_list(selection):
    _lib, covis = _mods()
    images, _ = selection
    images = dict(images)
    images[8] = cr.Img(images[8].name, images[7].qvec, images[7].tvec, images[8].point3D_ids)          # two frames at one centre
    mi = covis.MapIndex(images, cr.selection_map()[1])
    q = images[10].qvec
    C = pr.centre(images[12].qvec, images[12].tvec) + np.array([0.0, 30.0, 0.0])                       # image 12's centre exactly 30 away
    at30 = dict(frame_id=10, kind="obs", covisibility_frame=50, qvec=q, tvec=-pr.qvec2rotmat(q) @ C)
    q7, t7 = cr.selection_pose(images, 7, "near", 5)
    tie = dict(frame_id=7, kind="pos", covisibility_frame=50, obs_th=3, q_th=10, qvec=q7, tvec=t7)
    nan = dict(at30, tvec=np.array([np.nan, 0.0, 0.0]))
    clear = dict(at30, tvec=-pr.qvec2rotmat(q) @ (C + np.array([0.0, 0.001, 0.0])))
    tasks = [at30, tie, nan, clear]
    assert [fr.task_select(mi, t)[1] for t in tasks] == [1, 1, 1, 0]
    rc, idx, n_out, status = raw(mi, tasks)
    assert rc == 0 and status.tolist() == [1, 1, 1, 0] and n_out[:3].tolist() == [0, 0, 0] and (idx[:3] == -1).all()
    host = [fr.host_select(mi, t) for t in (at30, nan, clear)]
    assert mi.covisible_frames_batch([at30, nan, clear]) == [[int(v) for v in h] for h in host]
    got = mi.covisible_frames_batch([tie])[0]                                   # numpy leaves the order of the tied pair open
    assert sorted(got) == sorted(int(v) for v in fr.host_select(mi, tie)) and len(got) > 2


def test_bad_arguments_write_nothing(selection):
    _lib, covis = _mods()
    images, mi = selection
    t = fr.selection_tasks(images)[0]
    n_images, n_points = len(images), len(mi.point_ids)
    for kw, text in ((dict(frame_index=n_images), "image index out of range"), (dict(ref_rows=[0, n_points]), "ref_points row out of range"),
                     (dict(cap=0), "cap must be at least 1")):
        for on_device in (False, True):
            rc, idx, n_out, status = raw(mi, [t, t], on_device=on_device, **kw)
            msg = _lib.load().sfd2_last_error().decode()
            assert rc == -1 and text in msg and msg.startswith("sfd2_covis_frames: ")
            assert (idx == SENTINEL).all() and (n_out == SENTINEL).all() and (status == SENTINEL).all()


@pytest.mark.parametrize("opt_type", ["clurefobs", "clurefpos"])
@pytest.mark.parametrize("init_type", ["sng", "clu"])
def test_localizer_frames_device_and_host_write_the_same_files(files, init_type, opt_type):
    from sfd2_amd import localizer
    sc, paths = files
    out = {}
    for frames in ("host", "device"):
        p = dict(paths, save_root=os.path.join(paths["save_root"], f"frames_{init_type}_{opt_type}_{frames}"))
        stem = localizer.main(lf.argv(p, dataset="aachen", db_imglist_fn="x", init_type=init_type, frames=frames, inlier_thresh=20, with_match=True,
                                      do_covisible_opt=True, opt_type=opt_type, covisibility_frame=12, iters=1, radius=30, obs_thresh=3, opt_thresh=12))
        out[frames] = {ext: open(stem + ext, "rb").read() for ext in (".txt", ".log", ".txt.failed", "_full.log")}
    for ext in (".txt", ".log", ".txt.failed"):
        assert out["device"][ext] == out["host"][ext], ext
    strip = lambda b: re.sub(rb"time\[cs/fn\]: [0-9.]+/[0-9.]+", b"", b)        # noqa: E731  the wall times are each run's own
    assert strip(out["device"]["_full.log"]) == strip(out["host"]["_full.log"])
    assert len(out["device"][".txt"].splitlines()) == 20


@pytest.mark.parametrize("opt_type", ["clurefobs", "clurefpos"])
def test_refinement_batch_frames_device_equals_host(scene, opt_type):
    from sfd2_amd import localize
    sc, sm, mi = scene
    tasks = [dict(qname=qn["qname"], cfg=sc["cam"], db_frame_id=1 + (j * 5) % 14, thresh=12.0, qvec=qn["q"], tvec=qn["t"])
             for j, qn in enumerate(sc["queries"])]
    kw = dict(covisibility_frame=12, iters=1, obs_th=3, opt_th=12, radius=30, opt_type=opt_type)
    before = (mi.frames_tasks, mi.frames_host)
    dev = localize.pose_refinement_covisibility_batch(tasks, sc["store"], mi, sm, frames="device", **kw)
    kind = "obs" if opt_type == "clurefobs" else "pos"                          # images 15 / 16 share the poses of 5 / 6: pos ties, by the rule
    banded = sum(fr.task_select(mi, dict(frame_id=t["db_frame_id"], kind=kind, covisibility_frame=12, obs_th=3, q_th=10, qvec=t["qvec"],
                                         tvec=t["tvec"]))[1] != 0 for t in tasks)
    assert (mi.frames_tasks - before[0], mi.frames_host - before[1]) == (len(tasks), banded)
    assert banded == 0 if kind == "obs" else 0 < banded < len(tasks)
    host = localize.pose_refinement_covisibility_batch(tasks, sc["store"], mi, sm, frames="host", **kw)
    for d, h in zip(dev, host):
        assert set(d) == set(h) and [int(v) for v in d["db_ids"]] == [int(v) for v in h["db_ids"]] and len(d["db_ids"]) > 0
        for k in d:
            assert np.array_equal(np.asarray(d[k]), np.asarray(h[k])), k
