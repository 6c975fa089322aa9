"""The round-based mapper (sfd2_amd.reconstruction), the parts that need no GPU: header, binding, build list
and version; the kernels' resource metadata; the command's parser; the round logic of reconstruct() driven through the numpy stand-ins
of tests/mapper_ref.py; no CPU fallback; and the restatement of the filter checked against its second formulation.

FLOORS holds the largest relative difference between the restatement's two formulations of the filter (fp64 with arccos against long
double with arctan2) over point_error and point_angle, as measured here on the CPU: 3.8e-14 on 'long_tracks', 2.5e-13 on
'busy_views'.  The GPU tolerance is 100 x the floor measured on the machine the test runs on, ceiling 1e-9 (tests/test_gpu_mapper.py).
The differences are rounding noise, so another numpy may move them: the check below allows a factor of 100.  No comparison of either
scene lies within 1e-9 (relative) of a threshold: zero banded cases."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mapper_ref as mr
import tri_ref as tr
from sfd2_amd import _lib, build, reconstruction as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("sfd2_mapper_restrict", "sfd2_mapper_filter", "sfd2_mapper_visible", "sfd2_mapper_assemble")
FLOORS = {"long_tracks": 3.8e-14, "busy_views": 2.5e-13}
KERNELS = ("restrict_count_lane", "restrict_count_wave", "restrict_scatter_lane", "restrict_scatter_wave", "filter_obs", "filter_point_lane",
           "filter_point_wave", "track_points", "visible", "assemble_count", "assemble_scatter")


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_header_binding_and_version(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in _lib.EXPORTS, name
    for k, v in (("TRACK_LANE", 1), ("TRACK_WAVE", 2)):
        assert re.search(r"#define SFD2_MAPPER_FLAG_%s %d\b" % (k, v), hdr) and getattr(_lib, "MAPPER_FLAG_" + k) == v, k
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in CALLS) and lib.sfd2_version() >= 119
    assert len(lib.sfd2_mapper_restrict.argtypes) == 15 and len(lib.sfd2_mapper_filter.argtypes) == 15
    assert len(lib.sfd2_mapper_visible.argtypes) == 11 and len(lib.sfd2_mapper_assemble.argtypes) == 19
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:      # the header is C: the compiler's own layout of the view struct the filter takes, and the flags' values
        src = tmp_path / "sizes.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfd2_hip.h"\nint main(void) { printf("%zu %zu %d %d %d\\n", sizeof(sfd2_tri_view), '
                       'offsetof(sfd2_tri_view, tvec), SFD2_MAPPER_FLAG_TRACK_LANE, SFD2_MAPPER_FLAG_TRACK_WAVE, SFD2_TRI_MAX_POINTS); return 0; }\n')
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
        got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
        assert got == [ctypes.sizeof(_lib.TriView), _lib.TriView.tvec.offset, _lib.MAPPER_FLAG_TRACK_LANE, _lib.MAPPER_FLAG_TRACK_WAVE, _lib.TRI_MAX_POINTS]


def test_sources_are_in_the_build_list():
    assert "mapper_kernels.hip" in build.SOURCES and "api_mapper.hip" in build.SOURCES
    for f in ("mapper_kernels.hip", "api_mapper.hip", "mapper.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
        assert "getenv" not in open(os.path.join(build.CSRC, f)).read()
    assert open(os.path.join(ROOT, "sfd2_amd", "build.py")).read().count('"mapper.h"') == 2      # both dependency lists


def test_mapper_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "mapper.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "mapper_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    names = re.findall(r"\.name:\s+(\S*mapper_\w+_kernel\S*)", meta)
    for k in KERNELS:
        assert any("mapper_" + k + "_kernel" in n for n in names), k
    private = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    assert len(private) >= len(names) >= len(KERNELS) and all(int(v) == 0 for v in private)
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))
    assert all(int(v) == 0 for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", meta))
    assert all(int(v) == 64 for v in re.findall(r"\.wavefront_size:\s+(\d+)", meta))


def test_command_parser():
    base = ["--sfm_dir", "s", "--image_dir", "d", "--pairs", "p", "--features", "f", "--matches", "m"]
    a = RC.parser().parse_args(base)
    assert (str(a.sfm_dir), str(a.image_dir), str(a.pairs), str(a.features), str(a.matches)) == ("s", "d", "p", "f", "m")
    assert (str(a.colmap_path), a.single_camera, a.skip_geometric_verification, a.min_match_score, a.min_num_matches) == ("colmap", False, False, None, None)
    assert (a.reference_sfm_model, a.intrinsics, a.device) == (None, [], 0)
    a = RC.parser().parse_args(base + ["--colmap_path", "c", "--single_camera", "--skip_geometric_verification", "--min_match_score", "0.2", "--min_num_matches",
                                       "20", "--reference_sfm_model", "r", "--intrinsics", "a.txt", "b.txt"])
    assert (str(a.colmap_path), a.single_camera, a.skip_geometric_verification, a.min_match_score, a.min_num_matches) == ("c", True, True, 0.2, 20)
    assert str(a.reference_sfm_model) == "r" and [str(p) for p in a.intrinsics] == ["a.txt", "b.txt"]
    for missing in range(0, 10, 2):
        with pytest.raises(SystemExit):
            RC.parser().parse_args(base[:missing] + base[missing + 2:])
    assert set(vars(a)) <= set(RC.main.__code__.co_varnames[:RC.main.__code__.co_argcount])
    assert RC.STAT_KEYS == ("mean_reproj_error", "mean_track_length", "num_observations", "num_observations_per_image", "num_reg_images",
                            "num_sparse_points", "num_input_images")


def test_prior_camera():
    c = RC.prior_camera(3, 640, 480)
    assert c["model"] == "SIMPLE_RADIAL" and (c["width"], c["height"]) == (640, 480) and c["params"].tolist() == [768.0, 320.0, 240.0, 0.0]
    assert RC.prior_camera(1, 480, 1000)["params"][0] == 1200.0


def test_read_images_takes_the_prior_from_the_feature_store(tmp_path):
    from sfd2_amd import feature_io
    feats = feature_io.open_store(str(tmp_path / "feats.h5"), "a")
    for name, size in (("b.jpg", (640, 480)), ("a.jpg", (640, 480)), ("c.jpg", (480, 1000)), ("unlisted.jpg", (640, 480))):
        feature_io.write_features(feats, name, {"keypoints": np.zeros((3, 2)), "scores": np.ones(3), "image_size": np.array(size)})
    feats.close()
    (tmp_path / "pairs.txt").write_text("b.jpg a.jpg\na.jpg c.jpg\nc.jpg missing.jpg\n")
    cams, ims = RC.read_images(tmp_path / "pairs.txt", tmp_path / "feats.h5")
    assert [ims[i].name for i in sorted(ims)] == ["a.jpg", "b.jpg", "c.jpg"] and [ims[i].camera_id for i in sorted(ims)] == [1, 2, 3]
    assert cams[1]["params"].tolist() == [768.0, 320.0, 240.0, 0.0] and cams[3]["params"].tolist() == [1200.0, 240.0, 500.0, 0.0]
    (tmp_path / "pairs2.txt").write_text("b.jpg a.jpg\n")
    cams, ims = RC.read_images(tmp_path / "pairs2.txt", tmp_path / "feats.h5", single_camera=True)
    assert sorted(cams) == [1] and [ims[i].camera_id for i in sorted(ims)] == [1, 1]
    with pytest.raises(ValueError, match="single_camera"):
        RC.read_images(tmp_path / "pairs.txt", tmp_path / "feats.h5", single_camera=True)


# ---------------------------------------------------------------------------------------------------------------- the round logic
def _scene():
    return mr.br.cached(("mapper_host_scene",), tr.make_scene)


def _run(sc=None, images=None, pair_matches=None, stages=None, **kw):
    sc = _scene() if sc is None else sc
    S = mr.RefStages(sc) if stages is None else stages
    rep = {}
    ims, pts = RC.reconstruct(sc["cameras"], sc["images"] if images is None else images, sc["keypoints"],
                              sc["pair_matches"] if pair_matches is None else pair_matches, stages=S, report=rep, **kw)
    return ims, pts, rep, S


def _first_run():
    return mr.br.cached(("mapper_host_run",), _run)


def test_reconstruct_registers_every_image_and_writes_a_consistent_model():
    sc = _scene()
    ims, pts, rep, _ = _first_run()
    assert sorted(ims) == list(range(1, 13)) and [ims[i].name for i in sorted(ims)] == sorted(im.name for im in sc["images"].values())
    assert rep["final"]["n_registered"] == 12 and len(pts) == rep["final"]["points"] > 500 and list(pts) == list(range(1, len(pts) + 1))
    assert sum(len(p.image_ids) for p in pts.values()) == rep["final"]["observations"]
    for iid, im in ims.items():
        assert np.array_equal(im.xys, sc["keypoints"][iid].astype(np.float64) + 0.5) and len(im.point3D_ids) == len(im.xys)
    for pid, p in pts.items():
        assert len(set(p.image_ids.tolist())) >= 2 and 0 <= p.error <= 4.0
        assert all(ims[int(i)].point3D_ids[int(k)] == pid for i, k in zip(p.image_ids, p.point2D_idxs))
    assert sum(int((im.point3D_ids >= 0).sum()) for im in ims.values()) == rep["final"]["observations"]
    # the initial pair has the gauge: identity and a unit baseline
    a, b = rep["initial_pair"]
    assert ims[a].qvec.tolist() == [1, 0, 0, 0] and ims[a].tvec.tolist() == [0, 0, 0] and abs(np.linalg.norm(ims[b].tvec) - 1) < 1e-12
    e = mr.model_errors(ims, pts, sc["images"])
    assert e["rotation"] < 0.02 and e["centre"] < 0.1, e        # the stand-ins are crude; the model is still the scene
    # every round's candidates obey the rule of section 15 (f), and registration is monotone
    n = 2
    for r in rep["rounds"]:
        assert r["n_registered"] == n and set(r["registered"]) <= set(r["candidates"]) and len(r["candidates"]) <= 16
        n += len(r["registered"])
    assert rep["rounds"][-1]["candidates"] == [] and n == 12


def test_initial_pair_falls_back_to_half_the_angle():
    """No pair of this scene reaches 16 degrees (measured here: the widest pairs, four images apart, see 13.7 to 14.4), so the bound is
    halved once, and the winner is the pair with the most inliers at or above 8 degrees, ties to the smaller index."""
    sc = _scene()
    _, _, rep, S = _first_run()
    _, _, counts, results = mr.RefStages(sc).two_view(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], 4.0, 15, 0)
    angles = np.array([r["tri_angle_deg"] if r["success"] else np.nan for r in results])
    assert np.nanmax(angles) < 16.0 and np.nanmax(angles) >= 8.0
    assert rep["initial_tri_angle_bound"] == 8.0
    ok = [p for p, r in enumerate(results) if r["success"] and r["tri_angle_deg"] >= 8.0]
    want = min(ok, key=lambda p: (-results[p]["num_inliers"], p))
    assert rep["initial_pair_index"] == want and rep["initial_pair"] == tuple(sc["pair_matches"][want][:2])
    # the weak pairs were dropped by the verification, and are no candidates
    for p in sc["weak_pairs"]:
        assert not results[p]["success"] and counts[p] < 15
    assert RC.select_initial_pair(results, range(len(results)), 16.0, 1.5) == (want, 8.0)
    with pytest.raises(RuntimeError, match="no initial pair"):
        RC.select_initial_pair(results, range(len(results)), 16.0, 15.0)          # 16 only: halving would fall below the floor
    nan = [dict(r, tri_angle_deg=float("nan")) for r in results]
    with pytest.raises(RuntimeError, match="no initial pair"):
        RC.select_initial_pair(nan, range(len(nan)), 16.0, 1.5)


def test_an_image_without_pairs_stays_unregistered_and_unwritten():
    sc = _scene()
    images = dict(sc["images"])
    images[13] = tr.Img(13, [1, 0, 0, 0], [0, 0, 0], 1, "db/img005b.jpg")         # sorts into the middle: ids shift behind it
    kps = dict(sc["keypoints"])
    kps[13] = sc["keypoints"][1][:50]
    sc13 = dict(sc, keypoints=kps)
    ims, pts, rep, _ = _run(sc13, images=images)
    names = sorted(im.name for im in images.values())
    assert len(ims) == 12 and names.index("db/img005b.jpg") + 1 not in ims
    assert all(ims[i].name == names[i - 1] for i in ims)
    assert all((p.image_ids != names.index("db/img005b.jpg") + 1).all() for p in pts.values())
    base = _first_run()
    assert len(pts) == len(base[1])                                               # the model is the same, under shifted ids


def test_a_view_whose_pose_always_fails_is_retired_after_three_tries():
    sc = _scene()
    base_rep = _first_run()[2]
    target = sorted(sc["images"]).index(base_rep["rounds"][0]["candidates"][0])   # the first round's best candidate, as a view index
    S = mr.RefStages(sc, fail_views=[target])
    ims, pts, rep, _ = _run(stages=S)
    asked = [target in c for c in S.calls["absolute_pose"]]
    assert sum(asked) == 3 and asked[:3] == [True, True, True]                    # exactly max_reg_trials, in consecutive rounds
    assert len(ims) == 11 and target + 1 not in ims
    assert len(rep["rounds"]) < 12 and rep["rounds"][-1]["candidates"] == []      # the loop ends; the failing view does not stall it
    ims1, _, _, S1 = _run(stages=mr.RefStages(sc, fail_views=[target]), max_reg_trials=1)
    assert sum(target in c for c in S1.calls["absolute_pose"]) == 1 and len(ims1) == 11


def test_the_gauge_is_the_first_image_and_the_pair_only_while_it_stands_alone():
    sc = _scene()
    _, _, rep, S = _first_run()
    v0, v1 = (sorted(sc["images"]).index(i) for i in rep["initial_pair"])
    assert len(S.calls["adjust"]) == len(rep["rounds"]) + 1
    for k, vc in enumerate(S.calls["adjust"]):
        n_reg = rep["rounds"][k]["n_registered"] if k < len(rep["rounds"]) else rep["final"]["n_registered"]
        free = np.flatnonzero(~vc)
        assert vc[v0] and bool(vc[v1]) == (n_reg == 2) and len(free) == n_reg - (2 if n_reg == 2 else 1)
    _, _, rep2, S2 = _run(fix_initial_pair=True)
    assert all(vc[v0] and vc[v1] for vc in S2.calls["adjust"]) and rep2["final"]["n_registered"] == 12


def test_two_runs_give_equal_results():
    a, b = _first_run(), _run()
    assert sorted(a[0]) == sorted(b[0]) and sorted(a[1]) == sorted(b[1])
    for i in a[0]:
        assert a[0][i].qvec.tobytes() == b[0][i].qvec.tobytes() and a[0][i].tvec.tobytes() == b[0][i].tvec.tobytes()
        assert a[0][i].point3D_ids.tobytes() == b[0][i].point3D_ids.tobytes()
    for p in a[1]:
        assert a[1][p].xyz.tobytes() == b[1][p].xyz.tobytes() and a[1][p].image_ids.tobytes() == b[1][p].image_ids.tobytes()


def test_skip_geometric_verification_takes_the_store_as_verified():
    sc = _scene()
    S = mr.RefStages(sc)
    m, off, _, _ = S.two_view(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], 4.0, 15, 0)
    verified = [(a, b, m[off[p]:off[p + 1]][m[off[p]:off[p + 1], 0] >= 0]) for p, (a, b, _) in enumerate(sc["pair_matches"])]
    ims, pts, rep, S2 = _run(pair_matches=verified, skip_geometric_verification=True, init_max_pairs=5)
    assert len(ims) == 12 and rep["n_eligible_pairs"] == 5                        # only the five largest pairs went through the relative pose
    sizes = [len(v[2]) for v in verified]
    top = sorted(range(len(sizes)), key=lambda p: (-sizes[p], p))[:5]
    assert rep["initial_pair_index"] in top


def test_options_and_inputs_are_checked():
    sc = _scene()
    with pytest.raises(TypeError, match="unknown options"):
        RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], stages=mr.RefStages(sc), ba_iterations=3)
    with pytest.raises(ValueError, match="two images"):
        RC.reconstruct(sc["cameras"], {1: sc["images"][1]}, sc["keypoints"], [], stages=mr.RefStages(sc))
    assert RC.select_candidates(np.array([50, 40, 100, 24, 90, 29, 100]), np.array([0, 0, 0, 0, 1, 0, 0], bool), np.array([0, 0, 0, 0, 0, 0, 3]), 3, 30, 0.5,
                                16) == [2, 0]                                     # 40 < 0.5 x 100; 24 and 29 < 30; view 4 registered; view 6 out of tries
    assert RC.select_candidates(np.array([60, 60, 60]), np.zeros(3, bool), np.zeros(3, int), 3, 30, 0.5, 2) == [0, 1]


def test_raises_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    sc = mr.table_scene("busy_views")
    with pytest.raises(RuntimeError):
        RC.restrict_tracks(sc["off"], sc["obs_view"], sc["obs_xy"], sc["registered"]["all"])
    with pytest.raises(RuntimeError):
        RC.visible_counts(sc["off"], sc["obs_view"], sc["registered"]["none"], sc["point_track"], sc["point_live"])
    s = _scene()
    with pytest.raises(RuntimeError):
        RC.reconstruct(s["cameras"], s["images"], s["keypoints"], s["pair_matches"])
    src = inspect.getsource(RC)
    for word in ("linalg", "arccos", "arctan", "np.cross", "svd", "lstsq", "tests", "mapper_ref"):
        assert word not in src, word                                              # no geometry on the host, no test helper in the product


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_of_the_integer_calls_on_a_hand_made_table():
    off = np.array([0, 3, 5, 5, 9], np.int64)                                     # tracks of 3, 2, 0 and 4 observations
    ov = np.array([0, 1, 2, 1, 1, 0, 2, 2, 3], np.int32)
    xy = np.arange(18, dtype=np.float32).reshape(9, 2)
    r = mr.restrict_ref(off, ov, xy, [1, 0, 1, 0])
    assert r["sub_track"].tolist() == [0, 3] and r["sub_offsets"].tolist() == [0, 2, 5] and r["sub_obs"].tolist() == [0, 2, 5, 6, 7]
    assert r["sub_view"].tolist() == [0, 2, 0, 2, 2] and r["sub_xy"].tolist() == xy[[0, 2, 5, 6, 7]].tolist()
    assert mr.restrict_ref(off, ov, xy, [0, 1, 0, 0])["sub_track"].tolist() == []      # track 1 has two observations, both in view 1
    pt, pl = np.array([0, 0, 3, 3, 3], np.int32), np.array([1, 1, 1, 0, 1], bool)
    assert mr.visible_ref(off, ov, [1, 0, 0, 0], pt, pl).tolist() == [0, 2, 2 + 2 + 2, 2]
    X = np.arange(15, dtype=np.float64).reshape(5, 3)
    a = mr.assemble_ref(off, ov, xy, 4, pt, pl, X, [2, 1, 2])
    assert a["offsets"].tolist() == [0, 6, 8, 14] and a["src_obs"][:8].tolist() == [2, 2, 6, 6, 7, 7, 1, 1] and a["src_point"][:8].tolist() == [0, 1, 2, 4, 2, 4, 0, 1]
    assert a["points2D"][0].tolist() == [4.5, 5.5] and a["points3D"][3].tolist() == [12.0, 13.0, 14.0]


def test_filter_floor_and_bands_are_as_recorded():
    for name in ("long_tracks", "busy_views"):
        sc, refs, second = mr.table_scene(name), mr.filter_refs(name), mr.filter_second(name)
        floor = max(mr.filter_floor(r, second) for r in refs.values())
        print(name, "floor %.2g" % floor)
        assert floor <= 100 * FLOORS[name] and 100 * floor < 1e-9, (name, floor)
        for r in list(refs.values()) + [second]:
            assert not r["banded"].any(), name                                    # zero banded cases under either formulation
            assert (r["obs_keep"] == second["obs_keep"]).all() and (r["point_live"] == second["point_live"]).all()
        r = refs[None]
        # the committed cases: an observation 60 px off (dropped, its 255-long track lives on), a point behind its first camera (dead)
        o = sc["off"][5]
        assert 59.0 < r["obs_error"][o] < 61.5 and not r["obs_keep"][o] and r["point_live"][5]
        assert r["depth"][sc["off"][12]] < 0 and not r["obs_keep"][sc["off"][12]] and not r["point_live"][12]
        assert r["point_live"].sum() >= len(r["point_live"]) - 2 and np.isfinite(r["point_angle"][r["point_live"]]).all()
        assert (refs["lane"]["point_live"] == refs["wave"]["point_live"]).all() and (refs["lane"]["point_angle"][r["point_live"]] == refs["wave"]["point_angle"][r["point_live"]]).all()
    assert np.diff(mr.table_scene("long_tracks")["off"])[:9].tolist() == list(mr.br.TRACK_LENGTHS)
    assert np.bincount(mr.table_scene("busy_views")["obs_view"], minlength=9)[:7].tolist() == list(mr.br.VIEW_COUNTS)
