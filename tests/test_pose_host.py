"""Absolute pose, the parts that need no GPU: camera validation, no CPU fallback, the localiser glue (sfd2_amd.localize
match_cluster_2D / pose_from_clusters) against restatements of it_loc/localize_cv2.py, and the kernels' resource metadata."""
import os
import re
import subprocess

import numpy as np
import pytest

from sfd2_amd import build, localize, pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_camera_validation():
    mid, p = pose.camera_model({"model": "OPENCV", "width": 640, "height": 480, "params": [1, 2, 3, 4, 5, 6, 7, 8]})
    assert mid == 4 and list(p) == [1, 2, 3, 4, 5, 6, 7, 8]
    mid, p = pose.camera_model({"model": "SIMPLE_RADIAL", "width": 640, "height": 480, "params": [800, 320, 240, 0.1]})
    assert mid == 2 and list(p[:4]) == [800, 320, 240, 0.1] and not p[4:].any()
    with pytest.raises(ValueError, match="FULL_OPENCV"):
        pose.camera_model({"model": "FULL_OPENCV", "width": 640, "height": 480, "params": [0] * 12})
    with pytest.raises(ValueError, match="takes 3 parameters"):
        pose.camera_model({"model": "SIMPLE_PINHOLE", "width": 640, "height": 480, "params": [1, 2, 3, 4]})


def test_pose_raises_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cam = {"model": "PINHOLE", "width": 640, "height": 480, "params": [500, 500, 320, 240]}
    x, X = np.random.rand(10, 2) * 100, np.random.rand(10, 3) + [0, 0, 5]
    with pytest.raises(RuntimeError):
        pose.absolute_pose_estimation(x, X, cam, 12.0)
    with pytest.raises(RuntimeError):
        pose.pose_refinement(np.zeros(3), np.array([1.0, 0, 0, 0]), x, X, np.ones(10, bool), cam)


class _Pt:
    def __init__(self, xyz, image_ids):
        self.xyz, self.image_ids = np.asarray(xyz, float), image_ids


class _Img:
    def __init__(self, name, point3D_ids, qvec=(1.0, 0, 0, 0), tvec=(0.0, 0, 0)):
        self.name, self.point3D_ids, self.qvec, self.tvec = name, np.asarray(point3D_ids), np.asarray(qvec), np.asarray(tvec)


def _reference_cluster(kpq, matches_list, ids_list, points3D, obs_th):
    """it_loc/localize_cv2.py:593-650, line by line (without the database key points)."""
    all_mp3d, all_mkpq, all_mp3d_ids, all_q_ids = [], [], [], []
    outputs, valid_2D_3D_matches = {}, {}
    for i, (matches, points3D_ids) in enumerate(zip(matches_list, ids_list)):
        if points3D_ids.size == 0:
            continue
        mp3d_ids, q_ids, mkpq, mp3d, valid_matches = [], [], [], [], []
        for idx in range(matches.shape[0]):
            if matches[idx] == -1:
                continue
            if points3D_ids[matches[idx]] == -1:
                continue
            id_3D = points3D_ids[matches[idx]]
            if len(points3D[id_3D].image_ids) < obs_th:
                continue
            if idx in valid_2D_3D_matches.keys():
                if id_3D in valid_2D_3D_matches[idx]:
                    continue
                else:
                    valid_2D_3D_matches[idx].append(id_3D)
            else:
                valid_2D_3D_matches[idx] = [id_3D]
            mp3d.append(points3D[id_3D].xyz)
            mp3d_ids.append(id_3D)
            all_mp3d_ids.append(id_3D)
            mkpq.append(kpq[idx])
            q_ids.append(idx)
            all_q_ids.append(idx)
            all_mkpq.append(kpq[idx])
            all_mp3d.append(points3D[id_3D].xyz)
            valid_matches.append(matches[idx])
        outputs[i] = {"mkpq": mkpq, "qids": q_ids, "matches": np.array(valid_matches, dtype=int), "mp_3d_ids": mp3d_ids,
                      "mp3d": np.array(mp3d, dtype=float).reshape(-1, 3)}
    all_mp3d = np.array(all_mp3d, float).reshape(-1, 3)
    all_mkpq = np.array(all_mkpq, float).reshape(-1, 2) + 0.5
    return outputs, all_mp3d, all_mkpq, all_mp3d_ids, all_q_ids


def _synthetic_cluster(rs, nq=60, n_db=4, n_pts=40):
    points3D = {100 + i: _Pt(rs.rand(3), list(range(rs.randint(0, 6)))) for i in range(n_pts)}
    kpq = rs.rand(nq, 2) * 500
    matches_list, ids_list = [], []
    for d in range(n_db):
        m = 30
        ids = rs.choice(list(points3D) + [-1] * 10, m)          # duplicates of 3D ids and -1 entries on purpose
        if d == 2:
            ids = np.zeros(0, dtype=np.int64)                  # an image without 3D points
        matches = rs.randint(-1, m, nq) if ids.size else rs.randint(-1, 1, nq)
        matches_list.append(matches)
        ids_list.append(np.asarray(ids))
    return kpq, matches_list, ids_list, points3D


@pytest.mark.parametrize("obs_th", [0, 3])
def test_match_cluster_2D_restates_reference(obs_th):
    rs = np.random.RandomState(obs_th)
    kpq, ml, il, p3 = _synthetic_cluster(rs)
    got = localize.match_cluster_2D(kpq, ml, il, p3, obs_th=obs_th)
    want = _reference_cluster(kpq, ml, il, p3, obs_th)
    assert got[0].keys() == want[0].keys()
    for k in want[0]:
        for f in ("qids", "mp_3d_ids"):
            assert list(got[0][k][f]) == list(want[0][k][f])
        assert np.array_equal(got[0][k]["matches"], want[0][k]["matches"])
        assert np.array_equal(np.asarray(got[0][k]["mkpq"]), np.asarray(want[0][k]["mkpq"]))
        assert np.array_equal(got[0][k]["mp3d"], want[0][k]["mp3d"])
    for a, b in zip(got[1:], want[1:]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert len(got[3]) > 0 and len(set(zip(got[4], got[3]))) == len(got[3])   # no (query key point, 3D id) pair twice


def _cluster(rs, name, n, nq):
    """One db image whose matches give n distinct (query key point, 3D id) pairs, 3D ids n_offset.."""
    ids = np.arange(1000 * (name + 1), 1000 * (name + 1) + n)
    matches = np.full(nq, -1)
    q = rs.choice(nq, n, replace=False)
    matches[q] = np.arange(n)
    return _Img(f"db{name}", ids, qvec=(1.0, 0, 0, 0), tvec=(name, 0, 0)), matches


def _stub(script):
    """An estimator returning scripted (success, num_inliers) per live cluster, inliers = the first num_inliers."""
    calls = []

    def est(problems):
        calls.append(len(problems))
        out = []
        for (x, X, cam, thr), (ok, ni) in zip(problems, script):
            inl = np.zeros(len(x), bool)
            inl[:ni] = True
            out.append({"success": ok, "qvec": np.array([1.0, 0, 0, 0]), "tvec": np.array([float(ni), 0, 0]), "num_inliers": ni,
                        "inliers": inl})
        return out
    return est, calls


def _reference_loop(clusters_info, script, inlier_th=50):
    """it_loc/localize_cv2.py:705-1273 with do_covisility_opt=False, on scripted results (one db image per cluster, so best_inliers
    is num_inliers restricted to that image)."""
    best = {"num_inliers": 0, "qvec": None, "tvec": None}
    ret = None
    it = iter(script)
    for n_corr in clusters_info:
        if n_corr < 8:
            continue
        ok, ni = next(it)
        ret = {"success": ok, "qvec": np.array([1.0, 0, 0, 0]), "tvec": np.array([float(ni), 0, 0]), "num_inliers": ni}
        if not ok:
            continue
        best_inliers = ni
        keep = not (best_inliers < 8 or ni <= best["num_inliers"])
        if keep:
            best.update(ret)
        if ni < inlier_th or best_inliers < 10:
            continue
        return ret["tvec"][0], ni
    if best["num_inliers"] >= 10:
        return ret["tvec"][0], 0
    return -1.0, -1


@pytest.mark.parametrize("case", ["first", "later", "fallback", "failure"])
def test_pose_from_clusters_outcomes(case):
    rs = np.random.RandomState(7)
    nq = 400
    sizes = [100, 5, 120, 90, 80]                            # the second cluster is below the 8-correspondence floor
    script = {"first": [(True, 60), (True, 70), (True, 80), (True, 55)],
              "later": [(False, 0), (True, 30), (True, 70), (True, 20)],
              "fallback": [(True, 12), (False, 0), (True, 40), (True, 15)],
              "failure": [(False, 0), (True, 5), (True, 9), (False, 0)]}[case]
    clusters = [[_cluster(rs, i, n, nq)] for i, n in enumerate(sizes)]
    points3D = {}
    for (img, _), in clusters:
        for pid in img.point3D_ids:
            points3D[int(pid)] = _Pt(rs.rand(3), [0, 1, 2, 3])
    kpq = rs.rand(nq, 2) * 300
    est, calls = _stub(script)
    qvec, tvec, n, best = localize.pose_from_clusters(kpq, clusters, {"model": "PINHOLE", "width": 1, "height": 1, "params": [1, 1, 0, 0]},
                                                      12.0, points3D=points3D, estimator=est)
    assert calls == [4]                                       # one batch call over every live cluster
    want_t, want_n = _reference_loop(sizes, script)
    assert n == want_n
    if want_n == -1:
        assert np.array_equal(tvec, clusters[0][0][0].tvec) and best["num_inliers"] == 9
    else:
        assert tvec[0] == want_t
    assert {"first": 60, "later": 70, "fallback": 0, "failure": -1}[case] == n


def test_pose_kernel_takes_the_shared_ransac_layer():
    text = open(os.path.join(build.CSRC, "pose_kernels.hip")).read()
    # the shared layer (ransac_common.h, ransac_math.h) is the one definition of what the four RANSAC kernels share
    assert '#include "ransac_common.h"' in text
    for pat in (r"\bmix64\s*\(\s*uint64_t", r"\bvoid\s+wg_sum\s*\(", r"\bwg_best\s*\([^)]*\*", r"\bbool\s+finite_d\s*\(", r"\bsolve\d\b", r"\bsample[35]\b"):
        assert not re.search(pat, text), pat
    for helper in ("chol_solve<kNP>(", "ransac_enough(", "sample_k<3>(", "wg_best(", "wg_sum("):
        assert helper in text, helper
    for f in os.listdir(build.CSRC):        # the sampler has one name everywhere
        if f.endswith((".hip", ".h")):
            assert "sample3" not in open(os.path.join(build.CSRC, f)).read(), f


def test_pose_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "pose.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "pose_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*pose_kernel\S*)", meta)
    assert kernels
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta) and \
        all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta))
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))
