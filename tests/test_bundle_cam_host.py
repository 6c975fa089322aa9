"""Bundle adjustment with camera intrinsics among the unknowns, the parts that need no GPU: the ABI of
sfd2_ba_camera, header and binding, the build list, the new kernels' resource metadata, the parsers, the Python-side validation -- the
restatement of tests/bundle_cam_ref.py checked against itself -- and the mapper's round loop with the refine options, driven through
numpy stand-ins.

FLOORS holds the two routes' disagreements (bundle_cam_ref.state_diff: radians / scene size for poses and points, relative to the
parameter's own size for camera parameters; "*_step": of the first step's norm) and RADII the near-tie radii of the runs to convergence,
as measured here on the CPU.  The GPU tolerances are 10 x the floor that bundle_cam_ref computes on the machine the test runs on,
ceiling 1e-6.  The disagreements are differences of rounding noise, so another numpy may move them: the check allows a factor of 100."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bundle_cam_ref as cr
import bundle_ref as br
import mapper_ref as mr
import pose_ref as pr
import tri_ref as tr
from sfd2_amd import _lib, build, bundle_adjustment as B, colmap_io, reconstruction as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOORS = {"shared_step_focal": 1.5e-13, "shared_step_all": 1.8e-12, "shared_focal": 7.5e-13, "shared_focal_cauchy": 1.1e-9, "per_view": 6.9e-11,
          "two_cameras_opencv": 7.4e-12, "busy_camera": 4.7e-13, "seam_255": 1.4e-13, "seam_256": 2.5e-13, "seam_257": 8.9e-13, "seam_300": 1.7e-13,
          "shared_step_focal_step": 3.0e-12, "shared_step_all_step": 3.4e-12}
RADII = {"shared_focal": 1.5e-6, "shared_focal_cauchy": 1.5e-6}
KERNELS = ("linearise", "view_cam", "cam_sum", "cam_precond", "point_apply_lane", "point_apply_wave", "view_apply", "cam_apply", "pcg_init", "pcg_step",
           "update_cams", "veto", "commit")


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_struct_layout_matches_the_header(tmp_path):
    assert ctypes.sizeof(_lib.BaCamera) == 2 * 4 + 8 * 8 and _lib.BaCamera.refine.offset == 4 and _lib.BaCamera.params.offset == 8
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    assert re.search(r"\}\s*sfd2_ba_camera\s*;", hdr)
    assert re.search(r"\bint\s+sfd2_bundle_adjust_cameras\s*\(", hdr) and "sfd2_bundle_adjust_cameras" in _lib.EXPORTS
    for k, v in (("FOCAL", 1), ("PRINCIPAL", 2), ("EXTRA", 4)):
        assert re.search(r"#define SFD2_BA_REFINE_%s %d\b" % (k, v), hdr) and getattr(_lib, "BA_REFINE_" + k) == v, k
    assert (cr.FOCAL, cr.PRINCIPAL, cr.EXTRA) == (_lib.BA_REFINE_FOCAL, _lib.BA_REFINE_PRINCIPAL, _lib.BA_REFINE_EXTRA)
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:      # the compiler's own layout of the header's struct
        src = tmp_path / "sizes.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfd2_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(sfd2_ba_camera), '
                       'offsetof(sfd2_ba_camera, model), offsetof(sfd2_ba_camera, refine), offsetof(sfd2_ba_camera, params)); return 0; }\n')
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
        got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
        assert got == [ctypes.sizeof(_lib.BaCamera), _lib.BaCamera.model.offset, _lib.BaCamera.refine.offset, _lib.BaCamera.params.offset]


def test_library_exports_the_call():
    lib = _lib.load()
    assert hasattr(lib, "sfd2_bundle_adjust_cameras") and lib.sfd2_version() >= 123
    assert len(lib.sfd2_bundle_adjust_cameras.argtypes) == len(lib.sfd2_bundle_adjust.argtypes) + 3


def test_sources_are_in_the_build_list():
    assert "bundle_cam_kernels.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "sfd2_amd", "build.py")).read()
    assert src.count('"bundle_cam.h"') == 2 and src.count('"bundle.h"') == 2                   # both dependency lists, each under its own name
    for f in ("bundle_cam_kernels.hip", "bundle_cam.h"):
        assert os.path.exists(os.path.join(build.CSRC, f)) and "getenv" not in open(os.path.join(build.CSRC, f)).read()


def test_camera_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "bundle_cam.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "bundle_cam_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    names = re.findall(r"\.name:\s+(\S*bac_\w+_kernel\S*)", meta)
    for k in KERNELS:
        assert any("bac_" + k + "_kernel" in n for n in names), k
    private = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    assert len(private) >= len(names) >= len(KERNELS) and all(int(v) == 0 for v in private)
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))
    assert all(int(v) == 0 for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", meta))
    assert all(int(v) == 64 for v in re.findall(r"\.wavefront_size:\s+(\d+)", meta))


def test_command_parsers():
    a = B.parser().parse_args(["--input_path", "m", "--output_path", "o"])
    assert (a.refine_focal_length, a.refine_principal_point, a.refine_extra_params) == (0, 0, 0)
    a = B.parser().parse_args(["--input_path", "m", "--output_path", "o", "--refine_focal_length", "1", "--refine_extra_params", "1"])
    assert (a.refine_focal_length, a.refine_principal_point, a.refine_extra_params) == (1, 0, 1)
    with pytest.raises(SystemExit):
        B.parser().parse_args(["--input_path", "m", "--output_path", "o", "--refine_focal_length", "2"])
    assert set(vars(a)) <= set(B.main.__code__.co_varnames[:B.main.__code__.co_argcount])
    base = ["--sfm_dir", "s", "--image_dir", "d", "--pairs", "p", "--features", "f", "--matches", "m"]
    a = RC.parser().parse_args(base)
    assert (a.refine_focal_length, a.refine_principal_point, a.refine_extra_params, a.intrinsics_min_views) == (0, 0, 0, None)
    a = RC.parser().parse_args(base + ["--refine_focal_length", "1", "--refine_principal_point", "1", "--refine_extra_params", "1", "--intrinsics_min_views", "5"])
    assert (a.refine_focal_length, a.refine_principal_point, a.refine_extra_params, a.intrinsics_min_views) == (1, 1, 1, 5)
    assert set(vars(a)) <= set(RC.main.__code__.co_varnames[:RC.main.__code__.co_argcount])
    d = RC.DEFAULTS
    assert (d["refine_focal_length"], d["refine_principal_point"], d["refine_extra_params"]) == (False, False, False) and d["intrinsics_min_views"] >= 2
    assert B.refine_mask() == 0 and B.refine_mask(True, False, True) == 5 and B.refine_mask(refine_principal_point=True) == 2


def _views(P):
    arr = (_lib.TriView * P.nv)()
    for i in range(P.nv):
        for k in range(4):
            arr[i].qvec[k] = P.q[i][k]
        for k in range(3):
            arr[i].tvec[k] = P.t[i][k]
    return arr


def test_input_validation_and_no_cpu_fallback():
    P = cr.scene("per_view")
    packed = [B.camera_model(c) for c in P.cam_list]
    models, params = np.array([m for m, _ in packed]), np.array([p for _, p in packed])
    args = lambda **kw: {**dict(cam_models=models, cam_params=params, cam_refine=P.refine, view_camera=P.view_camera, views=_views(P), n_views=P.nv,
                                view_constant=P.vconst, xyz=P.X, point_constant=P.pconst, point_offsets=P.off, obs_view=P.obs_view, obs_xy=P.obs_xy), **kw}
    vcam = P.view_camera.copy()
    vcam[[2, 5]] = P.ncam
    with pytest.raises(ValueError, match="view 2: camera index out of range"):
        B.adjust_cameras(**args(view_camera=vcam))
    refine = P.refine.copy()
    refine[[3, 4]] = 9
    with pytest.raises(ValueError, match="camera 3: unknown refine bits"):
        B.adjust_cameras(**args(cam_refine=refine))
    bad = params.copy()
    bad[[1, 6], 2] = np.inf
    with pytest.raises(ValueError, match="camera 1: non-finite parameters"):
        B.adjust_cameras(**args(cam_params=bad))
    with pytest.raises(ValueError, match="do not fit"):
        B.adjust_cameras(**args(view_camera=P.view_camera[:-1]))
    with pytest.raises(ValueError, match="do not fit"):
        B.adjust_cameras(**args(cam_refine=P.refine[:-1]))
    with pytest.raises(TypeError, match="unknown options"):
        B.adjust_cameras(**args(refine_focal_length=True))
    with pytest.raises(ValueError, match="observation 0: view index out of range"):
        B.adjust_cameras(**args(obs_view=np.full_like(P.obs_view, P.nv)))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            B.adjust_cameras(**args())
    assert "linalg" not in open(B.__file__).read()              # no solver on the host


def test_bundle_adjust_returns_three_values_without_a_refine_option(monkeypatch):
    """The C calls replaced by recorders: which one bundle_adjust takes, with which cameras, and what it returns."""
    cams = {7: tr.Cam(id=7, **pr.camera("SIMPLE_RADIAL")), 3: tr.Cam(id=3, **pr.camera("OPENCV")), 9: tr.Cam(id=9, **pr.camera("PINHOLE"))}
    mk = lambda i, cid, pids: colmap_io.Image(i, np.array([1.0, 0, 0, 0]), np.array([float(i), 0, 0]), cid, f"{i}.jpg", np.zeros((len(pids), 2)), np.array(pids))
    images = {1: mk(1, 7, [1, 2]), 2: mk(2, 3, [1, 2]), 4: mk(4, 7, [2, 1]), 5: mk(5, 9, [-1])}
    points = {1: colmap_io.Point3D(1, np.array([0.0, 0, 5]), np.zeros(3, np.uint8), 0.0, np.array([1, 2, 4], np.int32), np.array([0, 0, 1], np.int32)),
              2: colmap_io.Point3D(2, np.array([1.0, 0, 5]), np.zeros(3, np.uint8), 0.0, np.array([1, 2, 4], np.int32), np.array([1, 1, 0], np.int32))}
    seen = {}

    def fake_adjust(views, n_views, vc, xyz, pc, off, ov, xy, flags=0, device=0, **options):
        seen["old"] = options
        return np.asarray(xyz, float), np.zeros(len(ov)), {"status": "stand_in"}

    def fake_cameras(models, params, refine, view_camera, views, n_views, vc, xyz, pc, off, ov, xy, flags=0, device=0, **options):
        seen["new"] = (list(models), np.array(params), list(refine), list(view_camera), options)
        return np.array(params) + 1.0, np.asarray(xyz, float), np.zeros(len(ov)), {"status": "stand_in"}

    monkeypatch.setattr(B, "adjust", fake_adjust)
    monkeypatch.setattr(B, "adjust_cameras", fake_cameras)
    out = B.bundle_adjust(cams, images, points, max_iterations=3)
    assert len(out) == 3 and "new" not in seen and seen["old"] == {"max_iterations": 3} and sorted(out[0]) == [1, 2, 4, 5]
    out = B.bundle_adjust(cams, images, points, refine_focal_length=True, refine_extra_params=True, constant_cameras=[3], max_iterations=3)
    assert len(out) == 4 and sorted(out[0]) == [3, 7, 9]
    models, params, refine, vcam, options = seen["new"]
    # one camera id is one camera; the cameras of the views only (image 5 has no observation), in id order; images 1 and 4 share camera 7
    assert models == [4, 2] and refine == [0, 5] and vcam == [1, 0, 1] and options == {"max_iterations": 3}
    assert out[0][7]["params"].tolist() == (np.array(pr.camera("SIMPLE_RADIAL")["params"]) + 1).tolist() and out[0][7]["model"] == "SIMPLE_RADIAL"
    assert len(out[0][3]["params"]) == 8 and out[0][9] is cams[9]
    with pytest.raises(TypeError, match="unknown options"):
        B.bundle_adjust(cams, images, points, refine_focal=True)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_central_differences_match_the_analytic_camera_jacobians():
    for name in ("shared_step_all", "per_view", "two_cameras_opencv", "busy_camera"):
        P = cr.scene(name)
        Jf, Ja = cr.jacobians(P, P.state(), "fd"), cr.jacobians(P, P.state(), "analytic")
        assert Ja.shape[2] == 6 + cr.KMAX + 3 and np.abs(Ja[:, :, 6:6 + cr.KMAX]).max() > 0
        assert np.abs(Jf - Ja).max() <= 1e-10 * np.abs(Ja).max(), name
        dead = np.arange(cr.KMAX)[None] >= P.kcount[P.obs_cam][:, None]
        assert (np.swapaxes(Ja[:, :, 6:6 + cr.KMAX], 1, 2)[dead] == 0).all()                    # no parameter, no column


def test_directions_follow_the_model_and_the_mask():
    count = lambda m, r: len(cr.directions(m, r))
    assert [count(m, 7) for m in br.MODELS] == [3, 4, 4, 8] and [count(m, 0) for m in br.MODELS] == [0, 0, 0, 0]
    assert [count(m, cr.EXTRA) for m in br.MODELS] == [0, 0, 1, 4] and [count(m, cr.FOCAL) for m in br.MODELS] == [1, 2, 1, 2]
    assert cr.directions("SIMPLE_RADIAL", cr.FOCAL)[0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]   # the one f moves fx and fy


def test_the_two_routes_agree_and_the_floors_are_as_recorded():
    measured = {n: cr.disagreement(n) for n in cr.RUNS}
    for n in ("shared_step_focal", "shared_step_all"):
        a, b = cr.solution(n, cr.ROUTE_A), cr.solution(n, cr.ROUTE_B)
        measured[n + "_step"] = cr.step_diff(a["first_step"], b["first_step"])
        assert abs(a["initial_cost"] - b["initial_cost"]) <= 1e-12 * b["initial_cost"] and abs(a["initial_gmax"] - b["initial_gmax"]) <= 1e-9 * b["initial_gmax"]
    print({k: float("%.2g" % v) for k, v in measured.items()})
    assert set(measured) == set(FLOORS)
    for k, v in measured.items():
        assert v <= 100 * FLOORS[k] and 10 * v < 1e-6, (k, v)
    for n, want in RADII.items():
        radius = cr.near_tie_radius(cr.scene(n), cr.solution(n, cr.ROUTE_B)["state"])
        print("radius", n, float("%.2g" % radius))
        assert 0.5 * want <= radius <= 1.5 * want, (n, radius)
        assert cr.floor(n) == max(cr.disagreement(n), radius) and cr.tolerance(n) == min(10 * cr.floor(n), 1e-6)


def test_scenes_stay_inside_their_conditions():
    for name, kw in cr.RUNS.items():
        P, s = cr.scene(name), cr.solution(name)
        assert P.vconst.sum() >= 2, name
        if "max_iterations" in kw:
            assert s["accepted"] == s["iterations"] == kw["max_iterations"], name
            assert all(abs(t - c) > 1e-6 * c for c, t, _, _ in s["history"]), name          # no decision near a tie
        else:
            assert s["status"] in ("gradient_tolerance", "lambda_overflow") and s["iterations"] < 100 and s["accepted"] >= 3, (name, s["status"])
        for st in (P.state(), s["state"]):
            assert cr.residuals(P, st)[1].min() > 1.0, name
        assert (s["state"][3][~cr.active_words(P)] == P.Kc[~cr.active_words(P)]).all()       # what is not refined does not move
    # the accept / reject sequence is a property of the scene only while the decisions are far from a tie: the two routes part ways behind it
    assert cr.decisive_prefix("shared_focal") == [True] * 3 and cr.decisive_prefix("shared_focal_cauchy") == [True] * 7
    assert all(len(cr.decisive_prefix(n)) < cr.solution(n)["iterations"] for n in ("shared_focal", "shared_focal_cauchy"))
    P = cr.scene("busy_camera")
    assert np.bincount(P.obs_view, minlength=9)[:7].tolist() == list(br.VIEW_COUNTS) and P.ncam == 3 and 2 not in P.view_camera
    assert [cr.scene("seam_%d" % n).nv for n in cr.SEAM_VIEWS] == [255, 256, 257, 300]
    P = cr.scene("two_cameras_opencv")
    assert P.kcount.tolist() == [8, 0] and P.view_camera.tolist() == [0, 1] * 4
    assert cr.scene("per_view").kcount.tolist() == [1, 2, 2, 6] * 2


def test_noise_free_observations_give_back_the_true_focal_length_and_distortion():
    P = cr.scene("shared_focal_exact")
    assert P.Kc[0, [0, 4]].tolist() == [960.0, 0.0]
    for route in (cr.ROUTE_A, cr.ROUTE_B):
        s = cr.lm(P, route)
        f, k = s["state"][3][0, [0, 4]]
        assert s["cost"] < 1e-16 and abs(f - 800.0) < 1e-6 and abs(k + 0.08) < 1e-9 and s["state"][3][0, 1] == f, route
        assert br.state_diff(s["state"][:3], P.truth) < 1e-9


def test_a_bad_trial_camera_is_rejected():
    """From a focal length of 1 px the first step leaves the positive numbers (or the finite ones): rejected, lambda x 10, as a non-finite cost."""
    P = cr.scene("shared_step_focal")
    Q = cr.with_cameras(P, [cr._cam("SIMPLE_RADIAL", [1.0, 320.0, 240.0, 0.0])], P.view_camera, P.refine)
    s = cr.lm(Q, cr.ROUTE_B, max_iterations=30, initial_lambda=1e-12)
    assert (s["state"][3][:, :2] > 0).all() and np.isfinite(s["state"][3]).all()
    assert all(ok == (np.isfinite(ct) and ct < c) or not ok for c, ct, ok, _ in s["history"])


# ---------------------------------------------------------------------------------------------------------------- the mapper's loop
class CamStages(mr.RefStages):
    """mapper_ref.RefStages with an adjust_cameras that runs the restatement (route B, two steps), and a record of the cameras every
    later stage call sees."""

    def __init__(self, scene):
        super().__init__(scene)
        self.seen = []                                         # (stage, K [n_views or n_problems, 8])

    def adjust_cameras(self, cam_models, cam_params, cam_refine, view_camera, views, n_views, view_constant, xyz, point_constant, point_offsets, obs_view,
                       obs_xy, **kw):
        names = {v: k for k, v in cr.MODEL_IDS.items()}
        count = {"SIMPLE_PINHOLE": 3, "PINHOLE": 4, "SIMPLE_RADIAL": 4, "OPENCV": 8}
        cams = [cr._cam(names[int(m)], np.asarray(p)[:count[names[int(m)]]]) for m, p in zip(cam_models, cam_params)]
        K, R, t = mr._views_arrays(views, n_views)
        P = cr.CamProblem(cams, view_camera, cam_refine, np.stack([pr.rotmat2qvec(r) for r in R]), t, xyz, np.asarray(view_constant) != 0,
                          np.asarray(point_constant) != 0, point_offsets, obs_view, obs_xy, kw["loss"], kw["loss_scale"])
        s = cr.lm(P, cr.ROUTE_B, max_iterations=min(int(kw["max_iterations"]), 2))
        Rn, tn, Xn, Kn = s["state"]
        for v in np.flatnonzero(~P.vconst):
            RC._set_pose(views[v], pr.rotmat2qvec(Rn[v]), tn[v])
        out = np.zeros((len(cams), 8))
        for c, cam in enumerate(cams):
            out[c, :count[cam["model"]]] = cr.colmap_params(cam["model"], Kn[c])
        self.calls.setdefault("adjust_cameras", []).append(dict(constant=np.array(view_constant, dtype=bool), given=np.array(cam_params), returned=out.copy(),
                                                                refine=list(cam_refine), view_camera=list(view_camera), accepted=s["accepted"]))
        self.seen.append(("adjust_cameras", Kn.copy()))
        r, _ = cr.residuals(P, s["state"])
        return out, Xn, np.linalg.norm(r, axis=1), {"status": s["status"], "iterations": s["iterations"], "accepted_steps": s["accepted"]}

    def triangulate(self, views, n_views, *a, **kw):
        self.seen.append(("triangulate", mr._views_arrays(views, n_views)[0].copy()))
        return super().triangulate(views, n_views, *a, **kw)

    def filter(self, views, n_views, *a, **kw):
        self.seen.append(("filter", mr._views_arrays(views, n_views)[0].copy()))
        return super().filter(views, n_views, *a, **kw)

    def absolute_pose(self, problems, cand, *a, **kw):
        self.seen.append(("absolute_pose", np.array([pr._opencv(cam) for _, _, cam in problems], dtype=np.float64)))
        return super().absolute_pose(problems, cand, *a, **kw)


def _small_scene():
    return br.cached(("cam_mapper_scene",), lambda: tr.make_scene(n_points=400, n_clutter=40))


def _mapper_run(**kw):
    sc = _small_scene()
    S, rep = CamStages(sc), {}
    out = RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], stages=S, report=rep, **kw)
    return out, rep, S


def test_the_mapper_carries_refined_cameras_through_its_rounds():
    sc = _small_scene()
    MIN = 6
    (cams, ims, pts), rep, S = br.cached(("cam_mapper_run",), lambda: _mapper_run(refine_focal_length=True, refine_extra_params=True, intrinsics_min_views=MIN))
    order = sorted(sc["images"])
    cam_ids = sorted({sc["images"][i].camera_id for i in order})
    vcam = [cam_ids.index(sc["images"][i].camera_id) for i in order]
    prior = np.array([pr._opencv(sc["cameras"][c]) for c in cam_ids], dtype=np.float64)
    calls = S.calls["adjust_cameras"]
    reports = [r["ba"] for r in rep["rounds"]] + [rep["final"]["ba"]]
    n_reg = [r["n_registered"] for r in rep["rounds"]] + [rep["final"]["n_registered"]]
    # below intrinsics_min_views the cameras are held: stages.adjust is called; from it on stages.adjust_cameras
    assert [bool(b.get("refined_intrinsics")) for b in reports] == [n >= MIN for n in n_reg] and n_reg[0] == 2 and n_reg[-1] == 12
    assert len(S.calls["adjust"]) == sum(n < MIN for n in n_reg) > 0 and len(calls) == sum(n >= MIN for n in n_reg) > 1
    assert all(c["refine"] == [5] * len(cam_ids) and c["view_camera"] == vcam and c["accepted"] > 0 for c in calls)
    # every stage call sees the cameras the latest adjustment returned (the prior before the first), and the next adjustment is given them
    current, k = prior, 0
    for stage, K in S.seen:
        if stage == "adjust_cameras":
            given = np.array([pr._opencv(cr._cam(sc["cameras"][c]["model"], calls[k]["given"][i][:len(sc["cameras"][c]["params"])])) for i, c in enumerate(cam_ids)])
            assert np.array_equal(given, current)
            current, k = K, k + 1
        elif stage == "absolute_pose":
            assert all(any(np.array_equal(row, c) for c in current) for row in K)
        else:
            assert np.array_equal(K, current[vcam]), stage
    assert k == len(calls) and not np.array_equal(current, prior)
    moved = current != prior
    assert moved[:, :2].all() and not moved[:, 2:4].any()                                   # focal lengths refined, principal points not
    # the written model carries them
    assert sorted(cams) == cam_ids and sorted(ims) == list(range(1, 13))
    for i, c in enumerate(cam_ids):
        assert cams[c]["model"] == sc["cameras"][c]["model"] and np.array_equal(np.array(pr._opencv(cams[c]), dtype=np.float64), current[i])
    assert sc["cameras"][cam_ids[0]]["params"] == pr.camera(sc["cameras"][cam_ids[0]]["model"])["params"]      # the caller's records are not touched


def test_with_the_options_off_the_mapper_calls_adjust_as_before():
    sc = _small_scene()
    out, rep, S = _mapper_run()
    assert len(out) == 2 and "adjust_cameras" not in S.calls and not any(stage == "adjust_cameras" for stage, _ in S.seen)
    base, rep0 = mr.RefStages(sc), {}
    ims0, pts0 = RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], stages=base, report=rep0)
    assert len(S.calls["adjust"]) == len(base.calls["adjust"]) == len(rep0["rounds"]) + 1
    assert all(np.array_equal(a, b) for a, b in zip(S.calls["adjust"], base.calls["adjust"]))
    assert sorted(out[0]) == sorted(ims0) and sorted(out[1]) == sorted(pts0) and S.calls["absolute_pose"] == base.calls["absolute_pose"]
    assert all("refined_intrinsics" not in r["ba"] for r in rep["rounds"])
    # the options alone change nothing while the threshold is not reached
    out2, rep2, S2 = _mapper_run(refine_focal_length=True, intrinsics_min_views=13)
    assert len(out2) == 3 and "adjust_cameras" not in S2.calls and all(np.array_equal(a, b) for a, b in zip(S2.calls["adjust"], base.calls["adjust"]))
    assert all(np.array_equal(out2[0][c]["params"], sc["cameras"][c]["params"]) for c in out2[0])
