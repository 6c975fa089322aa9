"""The covisibility stage, the parts that need no GPU: frame selections and pose_refinement_covisibility against goldens recorded
from the reference (tests/golden/gen_covis_goldens.py), the two call sites in pose_from_clusters on scripted outcomes,
localize_queries against single calls, and the assembly kernels' resource metadata."""
import os
import re
import subprocess

import numpy as np
import pytest

import covis_ref as cr
from sfd2_amd import _lib, build, covis, localize
from test_pose_host import _Pt, _cluster, _reference_loop, _stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "covis.npz"))


@pytest.fixture(scope="module")
def selection_index():
    images, points3D = cr.selection_map()
    return images, covis.MapIndex(images, points3D)


@pytest.mark.parametrize("case", range(len(cr.SELECTION_CASES)))
def test_frame_selection_equals_reference(selection_index, case):
    images, mi = selection_index
    kind, frame, cf, obs_th, pose = cr.SELECTION_CASES[case]
    q, t = cr.selection_pose(images, frame, pose, case)
    if kind == "obs":
        got = mi.covisible_frames(frame, covisibility_frame=cf, obs_th=obs_th, pred_qvec=q, pred_tvec=t)
    else:
        got = mi.covisible_frames_by_pose(frame, q, t, covisibility_frame=cf, q_th=10, t_th=10, obs_th=obs_th)
    assert [int(v) for v in got] == GOLD[f"sel{case}"].tolist()
    assert len(got) > 0


def test_map_index_tables():
    images, points3D = cr.selection_map()
    mi = covis.MapIndex(images, points3D)
    assert np.array_equal(mi.point_ids, np.array(sorted(points3D)))
    for i in (1, 5, 40):
        ids, rows = images[i].point3D_ids, mi.rows(i)
        assert rows.dtype == np.int32 and np.array_equal(rows == -1, ids == -1)
        assert np.array_equal(mi.point_ids[rows[rows >= 0]], ids[ids != -1])
    p = int(mi.point_ids[7])
    assert mi.track_len[7] == len(points3D[p].image_ids) and np.array_equal(mi.xyz[7], points3D[p].xyz)
    dup = images[5].point3D_ids
    v, c = np.unique(dup[dup != -1], return_counts=True)
    assert mi.track_len[mi.point_rows(v[c == 2])[0]] == len(points3D[int(v[c == 2][0])].image_ids)   # duplicates counted, as len() does


def test_reproject_and_pose_error():
    import pose_ref as pr
    rs = np.random.RandomState(0)
    for model in covis.CAMERA_MODELS:
        cam = pr.camera(model)
        q, t, x, X, _ = pr.scene(rs, cam, 50)
        assert np.allclose(covis.reproject(X, q, t, cam), x, rtol=0, atol=1e-9)
        assert np.allclose(covis.reproject(X, 3.0 * q, t, cam), x, rtol=0, atol=1e-9)      # normalised like scipy's from_quat
    q2 = cr.compose(cr.small_rot(rs, 7.0), q)
    qe, te, _ = covis.compute_pose_error(q2, -pr.qvec2rotmat(q2) @ (pr.centre(q, t) + [3.0, 4.0, 0.0]), q, t)
    assert abs(qe - 7.0) < 1e-6 and abs(te - 5.0) < 1e-9


def _run_case(name, matcher=None, sc=None):
    ci = list(cr.REFINE_CASES).index(name)
    opt_type, iters, success, limit = cr.REFINE_CASES[name]
    sc = sc or cr.refinement_scene(seed=ci)
    q0, t0 = cr.start_pose(sc, ci)
    est, refi = cr.make_estimator(sc, ci, success, limit), cr.make_refiner(sc, ci)
    mi = covis.MapIndex(sc["images"], sc["points3D"])
    ret = localize.pose_refinement_covisibility(cr.QNAME, cr.CAMERA, cr.feature_file(sc), 1, mi, 12.0, matcher or cr.scripted_matcher(sc),
                                                covisibility_frame=cr.FRAMES, iters=iters, obs_th=cr.OBS_TH, opt_th=cr.OPT_TH, qvec=q0, tvec=t0,
                                                radius=cr.RADIUS, opt_type=opt_type, estimator=est, refiner=refi)
    return sc, ret, refi


def check_against_golden(name, sc, ret):
    assert [int(d) for d in ret["db_ids"]] == GOLD[f"{name}_db_ids"].tolist()
    for d in ret["db_ids"]:                                   # the matches the reference saw, mapped back, are the scripted plan
        if f"{name}_matches_{d}" in GOLD.files and (sc["images"][d].point3D_ids != -1).sum() > 3:
            assert np.array_equal(GOLD[f"{name}_matches_{d}"], sc["plan"][d])
    assert bool(ret["success"]) == bool(GOLD[f"{name}_success"])
    assert [int(v) for v in ret["3D_ids"]] == GOLD[f"{name}_3D_ids"].tolist()
    assert np.array_equal(np.asarray(ret["mkpq"]), GOLD[f"{name}_mkpq"]) and np.asarray(ret["mkpq"]).dtype == np.float64
    assert np.array_equal(np.asarray(ret["score_q"], dtype=np.float32), GOLD[f"{name}_score_q"])
    assert np.array_equal(np.asarray(ret["inliers"], bool), GOLD[f"{name}_inliers"])
    assert int(ret["num_inliers"]) == int(GOLD[f"{name}_num_inliers"])
    assert np.array_equal(np.asarray(ret["qvec"], float), GOLD[f"{name}_qvec"])
    assert np.array_equal(np.asarray(ret["tvec"], float), GOLD[f"{name}_tvec"])


@pytest.mark.parametrize("name", list(cr.REFINE_CASES))
def test_pose_refinement_covisibility_equals_reference(name):
    sc, ret, refi = _run_case(name)
    check_against_golden(name, sc, ret)
    assert set(ret) >= {"success", "qvec", "tvec", "inliers", "num_inliers", "mkpq", "3D_ids", "db_ids", "score_q"} and "log_info" not in ret
    assert len(refi.calls) == {"iters1": 1, "iters2": 2, "by_pose": 1}.get(name, 0)


def test_gate_blocks_later_duplicate_and_default_is_off():
    sc = cr.refinement_scene(seed=0)
    q0, t0 = cr.start_pose(sc, 0)
    ims = [sc["images"][1], sc["images"][2]]
    args = (sc["kpq"], [sc["plan"][1], sc["plan"][2]], [im.point3D_ids for im in ims], sc["points3D"])
    _, _, _, ids_off, q_off = localize.match_cluster_2D(*args, obs_th=0)
    _, _, _, ids_on, q_on = localize.match_cluster_2D(*args, obs_th=0, gate=(q0, t0, cr.CAMERA, cr.RADIUS))
    assert list(zip(q_off, ids_off)).count((0, 117)) == 1            # ungated: taken once, from the first image
    assert (0, 117) not in list(zip(q_on, ids_on))                   # gated out in image 1, and image 2's duplicate stays blocked
    assert set(zip(q_on, ids_on)) < set(zip(q_off, ids_off))


class _FakeCovis:
    """Scripted pose_refinement_covisibility outcomes, in call order."""

    def __init__(self, names, script):
        self.map_index = type("M", (), {"name_to_id": {n: i for i, n in enumerate(names)}})()
        self.script, self.requests = list(script), []

    def refine(self, requests):
        out = []
        for r in requests:
            self.requests.append(r)
            ok, ni = self.script.pop(0)
            out.append({"success": ok, "qvec": np.array([0.0, 1.0, 0, 0]) if ok else r[4], "tvec": np.array([100.0 + ni, 0, 0]) if ok else r[5],
                        "num_inliers": ni, "inliers": []})
        return out


def _clusters(rs, sizes, nq):
    clusters = [[_cluster(rs, i, n, nq)] for i, n in enumerate(sizes)]
    points3D = {}
    for (img, _), in clusters:
        for pid in img.point3D_ids:
            points3D[int(pid)] = _Pt(rs.rand(3), [0, 1, 2, 3])
    return clusters, points3D


CAM = {"model": "PINHOLE", "width": 1, "height": 1, "params": [1, 1, 0, 0]}
SIZES = [100, 5, 120, 90, 80]
SCRIPTS = {"first": [(True, 60), (True, 70), (True, 80), (True, 55)], "later": [(False, 0), (True, 30), (True, 70), (True, 20)],
           "fallback": [(True, 12), (False, 0), (True, 40), (True, 15)], "failure": [(False, 0), (True, 5), (True, 9), (False, 0)]}


@pytest.mark.parametrize("case", list(SCRIPTS))
def test_covis_none_is_the_first_stage_alone(case):
    rs = np.random.RandomState(7)
    clusters, points3D = _clusters(rs, SIZES, 400)
    kpq = rs.rand(400, 2) * 300
    est, calls = _stub(SCRIPTS[case])
    qvec, tvec, n, best = localize.pose_from_clusters(kpq, clusters, CAM, 12.0, points3D=points3D, estimator=est, covis=None)
    assert calls == [4]
    want_t, want_n = _reference_loop(SIZES, SCRIPTS[case])
    assert n == want_n and (tvec[0] == want_t if want_n != -1 else np.array_equal(tvec, clusters[0][0][0].tvec))


def test_covis_call_sites():
    rs = np.random.RandomState(7)
    clusters, points3D = _clusters(rs, SIZES, 400)
    names = [cl[0][0].name for cl in clusters]
    kpq = rs.rand(400, 2) * 300
    run = lambda script, cov: localize.pose_from_clusters(kpq, clusters, CAM, 12.0, points3D=points3D, estimator=_stub(script)[0],
                                                          covis=cov, qname="q")
    # success site: the first cluster succeeds, its refinement fails -> the next successful cluster is refined and returned
    cov = _FakeCovis(names, [(False, 0), (True, 77)])
    qvec, tvec, n, best = run(SCRIPTS["first"], cov)
    assert n == 77 and tvec[0] == 177.0 and qvec[1] == 1.0
    assert [r[2] for r in cov.requests] == [0, 2]             # db_frame_id = the cluster's best database image
    assert cov.requests[0][4][0] == 1.0 and cov.requests[0][5][0] == 60.0 and cov.requests[1][5][0] == 70.0   # refined from each cluster's own pose
    # every refinement fails -> the fallback site refines the kept pose and returns it with 0 either way; the kept pose is the LAST
    # cluster's that passed inlier_th (:960-967 overwrite best_results even when `keep` is false)
    cov = _FakeCovis(names, [(False, 0)] * 5)
    qvec, tvec, n, best = run(SCRIPTS["first"], cov)
    assert n == 0 and len(cov.requests) == 5 and cov.requests[4][5][0] == 55.0 and cov.requests[4][2] == 4 and tvec[0] == 55.0
    cov = _FakeCovis(names, [(True, 33)])
    qvec, tvec, n, best = run(SCRIPTS["fallback"], cov)        # no cluster reaches inlier_th: straight to the fallback site
    assert n == 0 and tvec[0] == 133.0 and cov.requests[0][5][0] == 40.0
    cov = _FakeCovis(names, [])
    qvec, tvec, n, best = run(SCRIPTS["failure"], cov)         # nothing to refine: the first image's pose, -1
    assert n == -1 and not cov.requests


def test_localize_queries_equals_single_calls():
    rs = np.random.RandomState(3)
    queries, singles = [], []
    keys = list(SCRIPTS)
    for i in range(8):
        clusters, points3D_i = _clusters(np.random.RandomState(7), SIZES, 400)
        queries.append({"kpq": rs.rand(400, 2) * 300, "clusters": clusters, "camera": CAM, "qname": f"q{i}"})
    _, points3D = _clusters(np.random.RandomState(7), SIZES, 400)
    names = [cl[0][0].name for cl in queries[0]["clusters"]]

    def est(problems):                                        # success and inliers from the problem alone
        out = []
        for x, X, cam, thr in problems:
            ni = int(len(x) * 0.7)
            inl = np.zeros(len(x), bool)
            inl[:ni] = True
            out.append({"success": len(x) != 90, "qvec": np.array([1.0, 0, 0, 0]), "tvec": np.array([float(ni), x[0, 0], 0]), "num_inliers": ni,
                        "inliers": inl})
        return out

    class Cov(_FakeCovis):
        def refine(self, requests):
            self.batches.append(len(requests))
            return [{"success": r[0] not in ("q2", "q5") or r[2] != 0, "qvec": r[4], "tvec": r[5] + 1.0, "num_inliers": 5, "inliers": []}
                    for r in requests]
    cov = Cov(names, [])
    cov.batches = []
    got = localize.localize_queries(queries, 12.0, points3D=points3D, estimator=est, covis=cov)
    assert cov.batches[0] == 8 and len(cov.batches) == 2      # one refinement call per round
    for q, g in zip(queries, got):
        s = localize.pose_from_clusters(q["kpq"], q["clusters"], CAM, 12.0, points3D=points3D, estimator=est, covis=cov, qname=q["qname"])
        assert np.array_equal(g[0], s[0]) and np.array_equal(g[1], s[1]) and g[2] == s[2] and g[3]["order"] == s[3]["order"]


def test_header_declares_assembly():
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    declared = set(re.findall(r"\b(sfd2_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS) and "sfd2_assemble_2d3d" in declared
    import ctypes
    assert ctypes.sizeof(_lib.AssembleImage) == 16 and ctypes.sizeof(_lib.PointTable) == 24
    assert ctypes.sizeof(_lib.AssembleJob) == 8 * 2 + 4 * 4 + 8 * 2 + 8 + 4 * 2 + 8 * 8 + 8 * 7 + 8 + 4 * 4 + 8 * 7


def test_assemble_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "assemble.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "assemble_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*assemble_\w+_kernel\S*)", meta)
    assert len(kernels) == 4
    assert len(re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)) == 4 and \
        all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta))
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))
    assert all(int(v) == 0 for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", meta))
    assert re.findall(r"\.wavefront_size:\s+(\d+)", meta) == ["64"] * 4
