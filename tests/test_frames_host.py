"""Frame selection on the device, the parts that need no GPU: the seen CSR and the excluded bytes of MapIndex.frames_csr(), the numpy
restatement of sfd2_covis_frames (tests/frames_ref.py, the header's wording) against the host functions and the reference's recorded
results, the fallback routing of MapIndex.covisible_frames_batch with a stand-in library, the binding, and the kernel's resource
metadata."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import covis_ref as cr
import frames_ref as fr
from sfd2_amd import _lib, build, covis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "covis.npz"))


@pytest.fixture(scope="module")
def selection_index():
    images, points3D = cr.selection_map()
    return images, covis.MapIndex(images, points3D)


def _check_seen(mi):
    fc = mi.frames_csr()
    ids = fc["ids"]
    assert ids.tolist() == sorted(mi.images) and fc["index"] == {int(v): i for i, v in enumerate(ids)}
    so, si = fc["seen_offsets"], fc["seen_image"]
    assert so[0] == 0 and so[-1] == len(si) and len(so) == len(mi.point_ids) + 1 and si.dtype == np.int32
    for r, pid in enumerate(mi.point_ids):
        seg = si[so[r]:so[r + 1]]
        assert (np.diff(seg) > 0).all()                                                  # distinct and ascending
        assert [int(ids[i]) for i in seg] == [i for i in sorted(mi.images) if pid in mi.images[i].point3D_ids]
    assert fc["excluded"].tolist() == [int("left" in mi.images[int(i)].name or "right" in mi.images[int(i)].name) for i in ids]
    assert mi.frames_csr() is fc
    return fc


def test_frames_csr_of_the_selection_map(selection_index):
    images, mi = selection_index
    fc = _check_seen(mi)
    assert fc["excluded"].sum() > 0
    ids5 = images[5].point3D_ids[images[5].point3D_ids != -1]
    doubled = [int(p) for p in np.unique(ids5) if (ids5 == p).sum() == 2]
    assert len(doubled) == 1                                                             # image 5 lists one id twice ...
    r = int(mi.point_rows([doubled[0]])[0])
    seg = fc["seen_image"][fc["seen_offsets"][r]:fc["seen_offsets"][r + 1]]
    assert (seg == fc["index"][5]).sum() == 1                                            # ... and is seen once
    assert len(fc["seen_image"]) == len(fc["obs_point"]) - 1


def test_frames_csr_of_the_refinement_scene():
    sc = cr.refinement_scene()
    mi = covis.MapIndex(sc["images"], sc["points3D"])
    fc = _check_seen(mi)
    i3 = fc["index"][3]
    assert (fc["track_image"] == i3).sum() == 1 and (fc["seen_image"] == i3).sum() == 0  # in a track, in no seen list
    assert fc["excluded"].sum() == 0


def test_frames_csr_orders_images_by_id():
    images, points3D = fr.random_map(seed=3, n_img=40, n_pts=700)
    assert list(images) != sorted(images)
    _check_seen(covis.MapIndex(images, points3D))


@pytest.mark.parametrize("case", range(len(cr.SELECTION_CASES)))
def test_restatement_equals_host_and_reference(selection_index, case):
    images, mi = selection_index
    t = fr.selection_tasks(images)[case]
    got, status = fr.task_select(mi, t)
    assert status == 0                                                                   # the reference's cases stay clear of the bands
    assert got == [int(v) for v in fr.host_select(mi, t)] == GOLD[f"sel{case}"].tolist()


def test_restatement_equals_host_on_the_random_tasks():
    images, points3D = fr.random_map()
    mi = covis.MapIndex(images, points3D)
    tasks = fr.random_tasks(images, points3D)
    kinds = {(t["kind"], "qvec" in t, t["covisibility_frame"], t["obs_th"], "ref_3Dpoints" in t) for t in tasks}
    assert len(tasks) == 64 and len(kinds) >= 20
    for t in tasks:
        got, status = fr.task_select(mi, t)
        assert status == 0 and got == [int(v) for v in fr.host_select(mi, t)]


def test_restatement_small_cf_and_fallback_quirk(selection_index):
    """covisibility_frame 1..3 and the `<= 3 frames` fall-back: the header's one sentence covers both."""
    images, mi = selection_index
    for c, cf in ((8, 1), (8, 2), (8, 3), (9, 0), (5, 2), (0, 3)):
        t = dict(fr.selection_tasks(images)[c], covisibility_frame=cf)
        got, status = fr.task_select(mi, t)
        assert status == 0 and got == [int(v) for v in fr.host_select(mi, t)]


def test_restatement_bands(selection_index):
    images, mi = selection_index
    im = images[12]
    import pose_ref as pr
    C = pr.centre(im.qvec, im.tvec)
    q = images[10].qvec
    at30 = dict(frame_id=10, kind="obs", covisibility_frame=50, qvec=q, tvec=-pr.qvec2rotmat(q) @ (C + np.array([0.0, 30.0, 0.0])))
    assert fr.task_select(mi, at30)[1] == 1
    assert fr.task_select(mi, dict(at30, tvec=np.array([np.nan, 0, 0])))[1] == 1
    assert fr.task_select(mi, dict(at30, tvec=-pr.qvec2rotmat(q) @ (C + np.array([0.0, 30.001, 0.0]))))[1] == 0


class StubLib:
    """Stands in for the library: writes the restatement's rows, except that `forced` maps a call's task number to a status."""

    def __init__(self, mi, forced):
        self.mi, self.forced, self.calls = mi, forced, []

    def sfd2_covis_frames(self, h, fmap, tasks, n, ref_off, ref_pts, cap, idx, n_out, status, flags):
        fc = self.mi.frames_csr()
        m = fmap._obj
        assert h is None and m.inputs_on_device == 0 and m.n_images == len(fc["ids"]) and m.n_seen == len(fc["seen_image"])
        idx = np.ctypeslib.as_array(ctypes.cast(idx, ctypes.POINTER(ctypes.c_int32)), (n, cap))
        n_out = np.ctypeslib.as_array(ctypes.cast(n_out, ctypes.POINTER(ctypes.c_int32)), (n,))
        status = np.ctypeslib.as_array(ctypes.cast(status, ctypes.POINTER(ctypes.c_int32)), (n,))
        ro = None if ref_off is None else np.ctypeslib.as_array(ctypes.cast(ref_off, ctypes.POINTER(ctypes.c_int64)), (n + 1,))
        seen = []
        for j in range(n):
            t = tasks[j]
            rows = None
            if t.use_ref:
                rows = np.ctypeslib.as_array(ctypes.cast(ref_pts, ctypes.POINTER(ctypes.c_int32)), (int(ro[-1]),))[ro[j]:ro[j + 1]] if ro[-1] else []
            got, st = fr.select(fc, t.frame, "pos" if t.kind == _lib.FRAMES_POS else "obs", t.covisibility_frame, t.obs_th, t.q_th,
                                list(t.qvec) if t.has_pose else None, list(t.tvec) if t.has_pose else None, rows, cap)
            st = self.forced.get(j, st)
            idx[j] = -1
            n_out[j], status[j] = (len(got), 0) if st == 0 else (0, st)
            idx[j, :n_out[j]] = got[:n_out[j]]
            seen.append((t.frame, t.covisibility_frame))
        self.calls.append(seen)
        return 0


def test_batch_routes_nonzero_status_and_small_cf_to_the_host(selection_index, monkeypatch):
    images, mi = selection_index
    tasks = fr.selection_tasks(images)
    tasks += [dict(tasks[8], covisibility_frame=cf) for cf in (1, 2, 3)] + [dict(tasks[0], ref_3Dpoints=[10 ** 9])]
    want = [[int(v) for v in fr.host_select(mi, t)] for t in tasks[:-1]]
    hosted = []
    for name in ("covisible_frames", "covisible_frames_by_pose"):
        orig = getattr(covis.MapIndex, name)

        def spy(self, frame_id, *a, _orig=orig, _name=name, **kw):
            hosted.append((_name, frame_id, kw.get("covisibility_frame")))
            return _orig(self, frame_id, *a, **kw)
        monkeypatch.setattr(covis.MapIndex, name, spy)
    stub = StubLib(mi, {2: 1, 11: 2})
    before = (mi.frames_tasks, mi.frames_host)
    got = mi.covisible_frames_batch(tasks[:-1], lib=stub)
    assert got == want
    assert len(stub.calls) == 1 and len(stub.calls[0]) == 15                             # one call; cf 1..3 never reach the library
    assert all(cf == 0 or cf > 3 for _, cf in stub.calls[0])
    assert hosted == [("covisible_frames", 10, 1), ("covisible_frames", 10, 2), ("covisible_frames", 10, 3),
                      ("covisible_frames", tasks[2]["frame_id"], tasks[2]["covisibility_frame"]),
                      ("covisible_frames_by_pose", tasks[11]["frame_id"], tasks[11]["covisibility_frame"])]
    assert (mi.frames_tasks - before[0], mi.frames_host - before[1]) == (18, 5)
    with pytest.raises(KeyError):                                                        # an id the map does not hold: the host's error
        mi.covisible_frames_batch(tasks[-1:], lib=stub)
    assert mi.covisible_frames_batch([], lib=stub) == []


def test_header_and_binding_agree_on_frames():
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1))  # noqa: E731
    assert re.search(r"\bint\s+sfd2_covis_frames\s*\(", hdr) and "sfd2_covis_frames" in _lib.EXPORTS
    assert hdr.index("int sfd2_covis_frames") > hdr.index("int sfd2_covis_clusters")
    assert val("SFD2_FRAMES_OBS") == _lib.FRAMES_OBS and val("SFD2_FRAMES_POS") == _lib.FRAMES_POS
    assert val("SFD2_FRAMES_MAX_CANDIDATES") == _lib.FRAMES_MAX_CANDIDATES == fr.MAX_CANDIDATES
    assert val("SFD2_FRAMES_LDS_IMAGES") == _lib.FRAMES_LDS_IMAGES
    assert val("SFD2_FRAMES_FLAG_GLOBAL_COUNTERS") == _lib.FRAMES_FLAG_GLOBAL_COUNTERS
    assert ctypes.sizeof(_lib.FramesTask) == 88 and ctypes.sizeof(_lib.FramesMap) == 9 * 8 + 3 * 8 + 4 * 4
    assert 4 * _lib.FRAMES_LDS_IMAGES + 12 * _lib.FRAMES_MAX_CANDIDATES + 4 * 1024 <= 160 * 1024    # counters beside the sort arrays
    assert "115 adds sfd2_covis_frames" in hdr
    assert "frames_kernels.hip" in build.SOURCES


def test_frames_kernel_compiles_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "frames.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "frames_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*covis_frames_kernel\S*)", meta)
    assert len(kernels) == 2                                        # counters in LDS and in global scratch
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta) == ["0"] * 2
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta) == ["0"] * 2
    assert re.findall(r"\.sgpr_spill_count:\s+(\d+)", meta) == ["0"] * 2
    assert re.findall(r"\.wavefront_size:\s+(\d+)", meta) == ["64"] * 2
    assert all(int(v) <= 12 * _lib.FRAMES_MAX_CANDIDATES + 4 * 1024 for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", meta))
