"""Bundle adjustment, the parts that need no GPU: the ABI of the two structs, header and binding, the build list, the kernels'
resource metadata, the command's parser, input validation, no CPU fallback -- and the restatement of tests/bundle_ref.py checked
against itself: its two dense routes agree, it recovers a noise-free scene, and the committed seeds keep every scene inside the
conditions the GPU tests rely on.

FLOORS holds the two routes' disagreements and RADII the near-tie radii (bundle_ref.floor says how the two make a scene's floor) as
measured here on the CPU; the GPU tolerances are 10 x the floor that bundle_ref computes on the machine the test runs on, ceiling
1e-6.  The disagreements are differences of rounding noise, so another numpy may move them: the check below allows a factor of 100.
The largest disagreement over all scenes is 2.1e-10 of the scene's size ('trajectory'), 2.3e-12 of the step's norm on the one-step
test; the largest near-tie radius 3.2e-7 ('trajectory').

The scenes of tests/test_gpu_bundle_edges.py are too large for a dense H: their references are bundle_ref.lm_blocks (independent clusters)
and bundle_ref.arrow_step (few views, very many points), checked here against the dense routes on small scenes.  Their floors are recorded
the same way; PCG holds what a conjugate-gradient residual of 1e-14 may do to a step of the cluster scenes, SUMS how far the fp64 sums of the
'wide' scenes are from numpy.longdouble and math.fsum.  The new scenes' references take about 20 s here, computed once (bundle_ref.cached)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bundle_ref as br
import pose_ref as pr
from sfd2_amd import _lib, build, bundle_adjustment as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# scene -> the two routes' disagreement measured on the CPU (relative to the step's norm for "arc_step", else state_diff's measure:
# radians / scene size)
FLOORS = {"arc_step": 2.3e-12, "arc": 1.1e-11, "arc_cauchy": 2.7e-14, "long_tracks": 1.6e-11, "busy_views": 3.5e-13, "trajectory": 2.1e-10,
          "views_constant": 5.6e-15, "points_constant": 2.2e-13, "one_point_constant": 8.2e-15, "mix": 3.4e-13}
# scene -> near-tie radius at the restatement's minimum (bundle_ref.near_tie_radius), same measure
RADII = {"arc": 1.2e-8, "arc_cauchy": 1.3e-8, "trajectory": 3.2e-7, "views_constant": 6.6e-9, "points_constant": 5.4e-9, "one_point_constant": 1.2e-8,
         "mix": 7.1e-9}
# the scenes of tests/test_gpu_bundle_edges.py.  "*_step": the two routes' disagreement on the first step, relative to its norm; the others
# state_diff's measure after the steps NEW_RUNS names
FLOORS.update({"clusters_step": 3.1e-12, "clusters": 2.3e-14, "clusters_point_max_step": 1.9e-12, "clusters_point_max": 3.5e-14, "wide_step": 2.2e-12,
               "short_tracks": 2.4e-14, "reject_first": 1.0e-11, "arc_function_tolerance": 1.2e-14})
NEW_RUNS = {**br.CLUSTER_RUNS, "short_tracks": dict(max_iterations=2),
            "reject_first": br.REJECT_FIRST, "arc_function_tolerance": dict(function_tolerance=1e-6, max_iterations=100)}
# scene of clusters -> what a PCG residual of 1e-14 may do to the first step (bundle_ref.pcg_allowance: of the step's norm, state_diff's measure)
PCG = {"clusters": (3.8e-12, 4.3e-13), "clusters_point_max": (5.8e-13, 2.1e-14)}
# scene -> the fp64 restatement's cost and max |g| against numpy.longdouble and math.fsum, relative (bundle_ref.sum_floors)
SUMS = {"wide": (1.5e-16, 2.1e-16), "wide_first": (1.5e-16, 4.1e-16)}
CONVERGED = ("arc", "arc_cauchy", "trajectory", "views_constant", "points_constant", "one_point_constant", "mix")
TWO_STEPS = ("long_tracks", "busy_views")


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_struct_sizes_match_the_header(tmp_path):
    assert ctypes.sizeof(_lib.BaConf) == 4 * 4 + 5 * 8 + 4 * 4
    assert ctypes.sizeof(_lib.BaResult) == 4 * 4 + 4 * 8
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    for name in ("sfd2_ba_conf", "sfd2_ba_result"):
        assert re.search(r"\}\s*" + name + r"\s*;", hdr), name
    assert re.search(r"\bint\s+sfd2_bundle_adjust\s*\(", hdr) and "sfd2_bundle_adjust" in _lib.EXPORTS
    for k, v in (("LOSS_TRIVIAL", 0), ("LOSS_CAUCHY", 1), ("ST_GRADIENT", 0), ("ST_FUNCTION", 1), ("ST_MAX_ITERATIONS", 2), ("ST_LAMBDA", 3),
                 ("ST_NONFINITE", 4), ("FLAG_POINT_LANE", 1), ("FLAG_POINT_WAVE", 2)):
        assert re.search(r"#define SFD2_BA_%s %d\b" % (k, v), hdr) and getattr(_lib, "BA_" + k) == v, k
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:      # the compiler's own layout of the header's structs
        src = tmp_path / "sizes.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfd2_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(sfd2_ba_conf), '
                       'sizeof(sfd2_ba_result), offsetof(sfd2_ba_conf, initial_lambda), offsetof(sfd2_ba_result, lambda)); return 0; }\n')
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
        got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
        assert got == [ctypes.sizeof(_lib.BaConf), ctypes.sizeof(_lib.BaResult), _lib.BaConf.initial_lambda.offset, _lib.BaResult.lambda_.offset]


def test_library_exports_the_call():
    lib = _lib.load()
    assert hasattr(lib, "sfd2_bundle_adjust") and lib.sfd2_version() >= 118


def test_sources_are_in_the_build_list():
    assert "bundle_kernels.hip" in build.SOURCES and "api_bundle.hip" in build.SOURCES
    for f in ("bundle_kernels.hip", "api_bundle.hip", "bundle.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    assert open(os.path.join(ROOT, "sfd2_amd", "build.py")).read().count('"bundle.h"') == 2      # both dependency lists
    for f in ("bundle_kernels.hip", "api_bundle.hip", "bundle.h"):
        assert "getenv" not in open(os.path.join(build.CSRC, f)).read()


def test_bundle_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "bundle.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "bundle_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    names = re.findall(r"\.name:\s+(\S*ba_\w+_kernel\S*)", meta)
    for k in ("linearise", "reduce_partial", "reduce_final", "point_build_lane", "point_build_wave", "point_apply_lane", "point_apply_wave", "point_invert",
              "view_build", "view_precond", "view_apply", "pcg_init", "pcg_step", "update_views", "update_points", "decide", "commit"):
        assert any("ba_" + k + "_kernel" in n for n in names), k
    private = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    assert len(private) >= len(names) and all(int(v) == 0 for v in private)
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))
    assert all(int(v) == 0 for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", meta))


def test_command_parser():
    a = B.parser().parse_args(["--input_path", "m", "--output_path", "o"])
    assert (str(a.input_path), str(a.output_path), a.max_num_iterations, a.loss, a.loss_scale, a.constant_images) == ("m", "o", 100, "trivial", 1.0, None)
    a = B.parser().parse_args(["--input_path", "m", "--output_path", "o", "--max_num_iterations", "7", "--loss", "cauchy", "--loss_scale", "2.5",
                               "--constant_images", "c.txt"])
    assert (a.max_num_iterations, a.loss, a.loss_scale, str(a.constant_images)) == (7, "cauchy", 2.5, "c.txt")
    with pytest.raises(SystemExit):
        B.parser().parse_args(["--input_path", "m"])
    with pytest.raises(SystemExit):
        B.parser().parse_args(["--input_path", "m", "--output_path", "o", "--loss", "huber"])
    assert set(vars(a)) <= set(B.main.__code__.co_varnames[:B.main.__code__.co_argcount])


def test_constant_image_lists(tmp_path):
    import tri_ref as tr
    images = {5: tr.Img(5, [1, 0, 0, 0], [0, 0, 0], 1, "b.jpg"), 2: tr.Img(2, [1, 0, 0, 0], [0, 0, 0], 1, "a.jpg"), 9: tr.Img(9, [1, 0, 0, 0], [0, 0, 0], 1, "c.jpg")}
    assert B.default_constant_images(images) == [2, 5]
    f = tmp_path / "const.txt"
    f.write_text("# fixed\nc.jpg\n\na.jpg\n")
    assert B.read_constant_images(f, images) == [9, 2]
    f.write_text("d.jpg\n")
    with pytest.raises(ValueError, match="d.jpg"):
        B.read_constant_images(f, images)


def _views(P):
    arr = (_lib.TriView * P.nv)()
    for i, cam in enumerate(P.cams):
        arr[i].model, params = B.camera_model(cam)
        for k in range(8):
            arr[i].params[k] = params[k]
        for k in range(4):
            arr[i].qvec[k] = P.q[i][k]
        for k in range(3):
            arr[i].tvec[k] = P.t[i][k]
    return arr


def test_input_validation():
    P = br.scene("arc")
    args = lambda **kw: {**dict(views=_views(P), n_views=P.nv, view_constant=P.vconst, xyz=P.X, point_constant=P.pconst, point_offsets=P.off,
                                obs_view=P.obs_view, obs_xy=P.obs_xy), **kw}
    off = P.off.copy()
    off[7] = off[6] - 1
    with pytest.raises(ValueError, match="point_offsets"):
        B.adjust(**args(point_offsets=off))
    with pytest.raises(ValueError, match="point_offsets"):
        B.adjust(**args(point_offsets=P.off + 1))
    with pytest.raises(ValueError, match="do not fit"):
        B.adjust(**args(point_offsets=P.off[:-1]))
    ov = P.obs_view.copy()
    ov[[31, 200]] = P.nv
    with pytest.raises(ValueError, match="observation 31: view index out of range"):
        B.adjust(**args(obs_view=ov))
    xyz = P.X.copy()
    xyz[[12, 40], 2] = np.nan
    with pytest.raises(ValueError, match="point 12: non-finite"):
        B.adjust(**args(xyz=xyz))
    xy = P.obs_xy.copy()
    xy[99, 0] = np.inf
    with pytest.raises(ValueError, match="observation 99: non-finite"):
        B.adjust(**args(obs_xy=xy))
    with pytest.raises(TypeError, match="unknown options"):
        B.adjust(**args(max_num_iterations=3))
    with pytest.raises(ValueError, match="huber"):
        B.adjust(**args(loss="huber"))
    import tri_ref as tr
    from sfd2_amd import colmap_io
    cams = {1: tr.Cam(id=1, model="FULL_OPENCV", width=640, height=480, params=[0.0] * 12)}
    images = {1: colmap_io.Image(1, np.array([1.0, 0, 0, 0]), np.zeros(3), 1, "a.jpg", np.zeros((1, 2)), np.array([1]))}
    points = {1: colmap_io.Point3D(1, np.array([0.0, 0, 5]), np.zeros(3, np.uint8), 0.0, np.array([1], np.int32), np.array([0], np.int32))}
    with pytest.raises(ValueError, match="FULL_OPENCV"):
        B.bundle_adjust(cams, images, points)


def test_pack_model_groups_observations_by_point_in_track_order():
    import tri_ref as tr
    from sfd2_amd import colmap_io
    cams = {1: tr.Cam(id=1, **pr.camera("PINHOLE"))}
    mk = lambda i, xys, pids: colmap_io.Image(i, np.array([1.0, 0, 0, 0]), np.array([float(i), 0, 0]), 1, f"{i}.jpg", np.array(xys, float), np.array(pids))
    images = {3: mk(3, [[1, 2], [3, 4], [5, 6]], [8, -1, 4]), 1: mk(1, [[7, 8], [9, 10]], [4, 8]), 2: mk(2, [[0, 0]], [-1])}
    points = {8: colmap_io.Point3D(8, np.array([0.0, 0, 5]), np.zeros(3, np.uint8), 0.0, np.array([3, 1], np.int32), np.array([0, 1], np.int32)),
              4: colmap_io.Point3D(4, np.array([1.0, 0, 5]), np.zeros(3, np.uint8), 0.0, np.array([1, 3, 3], np.int32), np.array([0, 2, 1], np.int32))}
    ids, views, pids, xyz, off, ov, xy = B.pack_model(cams, images, points)
    assert ids == [1, 3] and pids == [4, 8] and off.tolist() == [0, 2, 4]          # image 2 has no observation; (3, 1) does not name point 4
    assert ov.tolist() == [0, 1, 1, 0] and xy.tolist() == [[7, 8], [5, 6], [1, 2], [9, 10]]
    assert xyz.tolist() == [[1, 0, 5], [0, 0, 5]]


def test_raises_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    P = br.scene("arc")
    with pytest.raises(RuntimeError):
        B.adjust(_views(P), P.nv, P.vconst, P.X, P.pconst, P.off, P.obs_view, P.obs_xy)
    assert "def lm" not in open(B.__file__).read() and "linalg" not in open(B.__file__).read()      # no solver on the host


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_central_differences_match_the_analytic_jacobians():
    for name in ("arc", "arc_cauchy", "busy_views"):
        P = br.scene(name)
        Jf, Ja = br.jac_fd(P, P.state()), br.jac_analytic(P, P.state())
        assert np.abs(Jf - Ja).max() <= 1e-10 * np.abs(Ja).max(), name


def test_the_two_routes_agree_and_the_floors_are_as_recorded():
    a, b = br.solution("arc", br.ROUTE_A, max_iterations=1), br.solution("arc", br.ROUTE_B, max_iterations=1)
    measured = {"arc_step": br.step_diff(a["first_step"], b["first_step"])}
    assert abs(a["initial_cost"] - b["initial_cost"]) <= 1e-12 * b["initial_cost"] and abs(a["initial_gmax"] - b["initial_gmax"]) <= 1e-10 * b["initial_gmax"]
    measured.update({n: br.disagreement(n) for n in CONVERGED})
    measured.update({n: br.disagreement(n, max_iterations=2) for n in TWO_STEPS})
    print({k: float("%.2g" % v) for k, v in measured.items()})
    for k, v in measured.items():
        assert v <= 100 * FLOORS[k] and 10 * v < 1e-6, (k, v)
    for n in CONVERGED:                                        # the radius depends on the minimum, not on the path: it repeats closely
        radius = br.near_tie_radius(br.scene(n), br.solution(n, br.ROUTE_B)["state"])
        assert 0.5 * RADII[n] <= radius <= 1.5 * RADII[n], (n, radius)
        assert br.floor(n) == max(br.disagreement(n), radius) and br.tolerance(n) == min(10 * br.floor(n), 1e-6)
        assert br.state_diff(br.solution(n, br.ROUTE_A)["state"], br.solution(n, br.ROUTE_B)["state"]) <= br.tolerance(n)


def test_noise_free_observations_give_back_the_true_scene():
    P = br.arc_scene(noise_px=0.0, seed=31)
    assert br.state_diff(P.state(), P.truth) > 1e-2
    for route in (br.ROUTE_A, br.ROUTE_B):
        s = br.lm(P, route)
        # the two constant views fix the frame, so the minimum is the true scene itself
        assert s["cost"] < 1e-16 and br.state_diff(s["state"], P.truth) < 1e-9, route


def test_scenes_stay_inside_their_conditions():
    for name in CONVERGED:
        P, s = br.scene(name), br.solution(name)
        assert P.vconst.sum() >= 2, name
        assert s["status"] in ("gradient_tolerance", "lambda_overflow") and s["iterations"] < 100, (name, s["status"], s["iterations"])
        assert s["accepted"] >= 3 and s["cost"] < 0.5 * s["initial_cost"], name
        assert br.residuals(P, s["state"])[1].min() > 1.0, name                     # nothing behind (or near) a camera
    for name in TWO_STEPS:
        P, s = br.scene(name), br.solution(name, max_iterations=2)
        assert P.vconst.sum() >= 2 and s["accepted"] == 2, name
        for st in (P.state(), s["state"]):
            assert br.residuals(P, st)[1].min() > 1.0, name
    P = br.scene("long_tracks")
    assert np.diff(P.off)[:9].tolist() == list(br.TRACK_LENGTHS) and P.nv == 300
    P = br.scene("busy_views")
    assert np.bincount(P.obs_view, minlength=9)[:7].tolist() == list(br.VIEW_COUNTS)
    P = br.scene("arc_cauchy")
    r, _ = br.residuals(P, (P.truth[0], P.truth[1], P.truth[2]))
    assert abs((np.linalg.norm(r, axis=1) > 20).mean() - 0.1) < 0.005              # 10 % gross outliers
    assert br.solution("arc", gradient_tolerance=0.0)["status"] == "lambda_overflow"


# ---------------------------------------------------------------------------------------------------------------- the large scenes
def test_structured_solvers_match_the_dense_routes():
    for name, bound in (("arc", 100 * FLOORS["arc_step"]), ("mix", 100 * FLOORS["mix"])):
        P = br.scene(name)
        for route in (br.ROUTE_A, br.ROUTE_B):
            H, g, _ = br.normal_equations(P, P.state(), route[0])
            dense = br.split_step(P, br.solve_step(P, H, g, 1e-4, route[1]))
            d = br.step_diff(br.arrow_step(P, P.state(), 1e-4, route), dense)
            print("arrow_step", name, route, d)
            assert d <= bound, (name, route, d)
        gc, gp, c = br.gradients(P, P.state())
        assert max(np.abs(gc).max(), np.abs(gp).max()) == np.abs(g).max() and c == br.cost(P, P.state())
        assert (gc[P.vconst] == 0).all() and (gp[P.pconst] == 0).all()
    three = br.clusters("clusters")[:3]
    M = br.merge(three)
    assert (M.nv, M.np_, len(M.obs_view)) == (15, 36, 180) and M.obs_view[60:120].min() == 5 and M.off[12:25].tolist() == list(range(60, 125, 5))
    for route in (br.ROUTE_A, br.ROUTE_B):
        a, b = br.lm_blocks(three, route, max_iterations=2), br.lm(M, route, max_iterations=2)
        d = br.state_diff(a["state"], b["state"])
        print("lm_blocks", route, d)
        assert d <= 100 * FLOORS["clusters"] and a["accepted"] == b["accepted"] == 2 and abs(a["cost"] - b["cost"]) <= 1e-12 * b["cost"]
        assert br.step_diff(a["first_step"], b["first_step"]) <= 100 * FLOORS["clusters_step"]
    # one cluster: the same arithmetic as lm(), rejections and the function tolerance included
    for name, kw in (("reject_first", br.REJECT_FIRST), ("arc", dict(function_tolerance=1e-6))):
        a, b = br.lm_blocks([br.scene(name)], br.ROUTE_B, **kw), br.solution(name, br.ROUTE_B, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(a["state"], b["state"]))
        assert [a[k] for k in ("cost", "lambda", "iterations", "accepted", "status")] == [b[k] for k in ("cost", "lambda", "iterations", "accepted", "status")]


def test_the_new_scenes_floors_are_as_recorded():
    measured = {n: br.disagreement(n.replace("arc_function_tolerance", "arc"), **kw) for n, kw in NEW_RUNS.items()}
    measured.update({n + "_step": br.step_diff(*br.first_steps(n)) for n in ("clusters", "clusters_point_max", "wide")})
    print({k: float("%.2g" % v) for k, v in measured.items()})
    for k, v in measured.items():
        assert v <= 100 * FLOORS[k] and 10 * v < 1e-6, (k, v)
    for n in br.CLUSTER_SCENES:
        rel, ab = br.pcg_allowance(n)
        print("pcg allowance", n, float("%.2g" % rel), float("%.2g" % ab))
        assert PCG[n][0] / 100 <= rel <= 100 * PCG[n][0] and PCG[n][1] / 100 <= ab <= 100 * PCG[n][1]
        assert br.step_floor(n) == max(measured[n + "_step"], rel) and br.floor(n, **NEW_RUNS[n]) == max(measured[n], ab)
        assert br.step_tolerance(n) < 1e-9 and br.tolerance(n, **NEW_RUNS[n]) < 1e-10
    assert np.finfo(np.longdouble).eps < 1e-18                  # the extended figures are worth their name
    for n in ("wide", "wide_first"):
        fc, fg, mc, mg = br.sum_floors(n)
        print("sums", n, float("%.2g" % mc), float("%.2g" % mg))
        assert mc <= 100 * SUMS[n][0] and mg <= 100 * SUMS[n][1]
        assert fc == max(mc, br.SUM_DEPTH * 2.0 ** -53) and fg == max(mg, br.SUM_DEPTH * 2.0 ** -53) and max(fc, fg) < 1e-13
    # the depth of the device's largest reduction (256 strided sums per 2048-element chunk, a tree over them; 256 strided
    # sums over the partials, a tree over them) stays inside SUM_DEPTH
    no = len(br.scene("wide").obs_view)
    partials = -(-no // 2048)
    assert 2048 // 256 + 8 + -(-partials // 256) + 8 <= br.SUM_DEPTH


def test_the_new_scenes_stay_inside_their_conditions():
    for name in br.CLUSTER_SCENES:
        P, steps = br.scene(name), NEW_RUNS[name]["max_iterations"]
        assert (P.nv, P.np_, len(P.obs_view)) == (1030, 2472, 12360) and P.nv > 1024 + 5
        groups = P.vconst.reshape(-1, 5).tolist()
        assert all(g == [True, False, False, False, True] for c, g in enumerate(groups) if (name, c) != ("clusters_point_max", br.POINT_MAX_CLUSTER))
        assert not P.vconst[1026:1029].any()                                                 # variable views beyond the first 1024
        for route in (br.ROUTE_A, br.ROUTE_B):
            s = br.solution(name, route, **NEW_RUNS[name])
            assert s["accepted"] == s["iterations"] == steps and all(abs(t - c) > 1e-6 * c for c, t, _, _ in s["history"]), (name, route)
            for st in (P.state(), s["state"]):
                assert br.residuals(P, st)[1].min() > 1.0, name
        gc, gp, _ = br.gradients(P, P.state())
        gc, gp = np.abs(gc).ravel(), np.abs(gp).ravel()
        if name == "clusters":       # the largest entry: a view's, behind the first reduction chunk, in the cluster beyond view 1024
            assert gc.argmax() >= 2048 and gc.argmax() // 6 >= 1025 and gc.max() > 1.05 * np.sort(gc)[-2] and gc.max() > 10 * gp.max()
            assert 6 * P.nv > 2 * 2048 + 1 and np.sort(gc[:2048])[-1] < gc.max()
        else:                        # a point's, behind the points' first chunk; every view entry smaller
            assert gp.argmax() >= 2048 and gp.max() > 1.2 * gc.max() and gp.max() > 2 * np.sort(gp)[-2] and groups[br.POINT_MAX_CLUSTER] == [True] * 5
            assert gp.argmax() // 3 == 12 * br.POINT_MAX_CLUSTER + 11
    for name in ("wide", "wide_first"):
        P = br.scene(name)
        assert (P.nv, P.np_, len(P.obs_view)) == (3, 262145, 525290) and P.vconst.tolist() == [True, False, True]
        assert -(-len(P.obs_view) // 2048) == 257 and -(-3 * P.np_ // 2048) == 385          # one more than the final pass's 256 lanes
        lens = np.diff(P.off)
        assert (lens == 3).sum() == 1000 and (lens == 2).sum() == P.np_ - 1000 and lens[0] == lens[-1] == 2
        assert (P.obs_view[P.off[:-1]] == 0).all() and (P.obs_view[P.off[1:] - 1] == 2).all() and (P.obs_view[P.off[:-1][lens == 3] + 1] == 1).all()
        gc, gp, c = br.gradients(P, P.state())
        gp = np.abs(gp).ravel()
        want = 0 if name == "wide_first" else P.np_ - 1
        assert gp.argmax() // 3 == want and gp.max() > 2 * np.sort(gp)[-2] and gp.max() > 2 * np.abs(gc).max()
        assert (gp.argmax() // 2048 >= 256) == (name == "wide")                              # the partial that holds it: second pass or first
        assert br.residuals(P, P.state())[1].min() > 1.0
    P = br.scene("wide")
    for step in br.first_steps("wide"):
        trial = br.apply_split(P.state(), step)
        assert br.cost(P, trial) < 0.5 * br.cost(P, P.state()) and br.residuals(P, trial)[1].min() > 1.0
        assert np.abs(step[0][1]).min() > 1e-5 and (step[0][[0, 2]] == 0).all()               # the middle view moves, the outer two do not
    P, s = br.scene("short_tracks"), br.solution("short_tracks", max_iterations=2)
    assert np.diff(P.off)[list(br.SHORT_AT)].tolist() == [1, 0] * 4 and P.obs_view[P.off[:-1][list(br.SHORT_AT[::2])]].tolist() == [2, 3, 4, 5]
    assert P.np_ == 68 and (np.delete(np.diff(P.off), br.SHORT_AT) == 6).all() and s["accepted"] == 2
    assert all(np.array_equal(s["state"][2][j], P.X[j]) for j in br.SHORT_AT[1::2])          # never seen: never moved
    assert all(np.abs(s["state"][2][j] - P.X[j]).max() > 1e-3 for j in br.SHORT_AT[::2])     # seen once: moved, held by the damping
    for st in (P.state(), s["state"]):
        assert br.residuals(P, st)[1].min() > 1.0
    P = br.scene("reject_first")
    for route in (br.ROUTE_A, br.ROUTE_B):
        s = br.lm_blocks([P], route, **br.REJECT_FIRST)
        pattern = [ok for _, _, ok, _ in s["history"]]
        assert pattern == [True, False, False, False, True] and s["iterations"] == 5 and s["accepted"] == 2 and s["lambda"] == br.solution("reject_first", **br.REJECT_FIRST)["lambda"]
        assert all(abs(t - c) > 1e-6 * c for c, t, _, _ in s["history"]), [abs(t - c) / c for c, t, _, _ in s["history"]]
        assert br.residuals(P, s["state"])[1].min() > 1.0 and br.residuals(P, P.state())[1].min() > 1.0


def test_function_tolerance_decides_far_from_a_tie():
    for route in (br.ROUTE_A, br.ROUTE_B):
        s = br.lm_blocks([br.scene("arc")], route, function_tolerance=1e-6)
        assert s["status"] == "function_tolerance" and s["iterations"] == s["accepted"] == 3
        ratios = [abs(c - t) / c for c, t, ok, _ in s["history"] if ok]
        print("function tolerance", route, ratios)
        assert ratios[-1] < 1e-6 / 10 and ratios[-2] > 1e-6 * 10
