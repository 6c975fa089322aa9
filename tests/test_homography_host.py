"""Homography and the E / F / H decision, the parts that need no GPU: the ABI of the two structs, input validation, no CPU fallback, the
build list, the kernel's resource metadata, the two commands' parsers and the decision rule on hand-made result dicts."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sfd2_amd import _lib, build, geometric_verification, reconstruction, two_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_match_the_header(tmp_path):
    # n, reserved | two pointers | max_error_px
    assert ctypes.sizeof(_lib.HomographyProblem) == 2 * 4 + 2 * 8 + 8
    # success, num_inliers, num_trials, reserved | H[9]
    assert ctypes.sizeof(_lib.HomographyResult) == 4 * 4 + 9 * 8
    assert [f[0] for f in _lib.HomographyProblem._fields_] == [f[0] for f in _lib.FundamentalProblem._fields_]
    assert [f[0] for f in _lib.HomographyResult._fields_] == ["success", "num_inliers", "num_trials", "reserved", "H"]
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    for name in ("sfd2_homography_problem", "sfd2_homography_result"):
        assert re.search(r"\}\s*" + name + r"\s*;", hdr), name
    assert re.search(r"\bint\s+sfd2_homography_batch\s*\(", hdr) and "sfd2_homography_batch" in _lib.EXPORTS
    assert "121 adds sfd2_homography_batch" in hdr
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:      # the compiler's own layout of the header's structs
        src = tmp_path / "sizes.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfd2_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                       'sizeof(sfd2_homography_problem), sizeof(sfd2_homography_result), offsetof(sfd2_homography_problem, max_error_px), '
                       'offsetof(sfd2_homography_result, H)); return 0; }\n')
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
        got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
        assert got == [ctypes.sizeof(_lib.HomographyProblem), ctypes.sizeof(_lib.HomographyResult),
                       _lib.HomographyProblem.max_error_px.offset, _lib.HomographyResult.H.offset]


def test_library_version_and_export():
    core = open(os.path.join(build.CSRC, "api_core.hip")).read()
    assert int(re.search(r"sfd2_version\(void\)\s*\{\s*return\s+(\d+)", core).group(1)) >= 121
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.sfd2_version() >= 121 and hasattr(lib, "sfd2_homography_batch")


def test_input_validation():
    p = np.random.RandomState(0).uniform(0, 400, (10, 2))
    with pytest.raises(ValueError, match="10 points in image 0 for 9"):
        two_view.homography(p, p[:9])
    with pytest.raises(ValueError, match="non-finite"):
        two_view.homography(p, np.where(np.arange(20).reshape(10, 2) == 7, np.inf, p))
    with pytest.raises(ValueError, match="non-finite"):
        two_view.homography_batch([(p, p + 1), (np.where(np.arange(20).reshape(10, 2) == 0, np.nan, p), p)])
    with pytest.raises(ValueError, match="beyond the 10 key points of image 1"):
        two_view.verify_pairs_homography({0: p, 1: p}, [(0, 1, np.array([[0, 1], [2, 10]]))])
    with pytest.raises(ValueError, match="beyond the 10 key points of image 1"):
        two_view.verify_pairs_geometry({0: p, 1: p}, [(0, 1, np.array([[0, 1], [2, 10]]))])
    with pytest.raises(ValueError, match="cameras and images go together"):
        two_view.verify_pairs_geometry({0: p, 1: p}, [], cameras={})
    with pytest.raises(ValueError, match="1 camera pairs for 2 problems"):
        two_view.two_view_geometry_batch([(p, p), (p, p)], [(None, None)])
    assert two_view.homography_batch([]) == [] and two_view.two_view_geometry_batch([]) == []


def test_raises_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = np.random.RandomState(0).uniform(0, 400, (10, 2))
    m = np.stack([np.arange(10), np.arange(10)], 1)
    with pytest.raises(RuntimeError):
        two_view.homography(p, p + 1)
    with pytest.raises(RuntimeError):
        two_view.verify_pairs_homography({0: p, 1: p}, [(0, 1, m)])
    with pytest.raises(RuntimeError):
        two_view.verify_pairs_geometry({0: p, 1: p}, [(0, 1, m)])


def test_sources_are_in_the_build_list():
    assert "homography_kernels.hip" in build.SOURCES and "api_homography.hip" in build.SOURCES
    for f in ("homography_kernels.hip", "api_homography.hip", "four_point.h", "ransac_common.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    text = open(os.path.join(build.CSRC, "homography_kernels.hip")).read()
    assert '#include "ransac_common.h"' in text and '#include "four_point.h"' in text and "uint64_t mix64" not in text
    for helper in ("wg_sum(", "wg_best(", "better(", "sample_k<4>("):
        assert helper in text, helper
    assert "atomic" not in text
    # the shared layer (ransac_common.h, ransac_math.h) is the one definition of what the four RANSAC kernels share
    assert '#include "ransac_common.h"' in text
    for pat in (r"\bmix64\s*\(\s*uint64_t", r"\bvoid\s+wg_sum\s*\(", r"\bwg_best\s*\([^)]*\*", r"\bbool\s+finite_d\s*\(", r"\bsolve\d\b", r"\bsample[35]\b"):
        assert not re.search(pat, text), pat
    for helper in ("chol_solve<kNP>(", "normal_acc(", "score_lane(", "score_wg(", "publish_winner(", "ransac_enough(", "finish_matrix("):
        assert helper in text, helper
    # one packing and scratch layer for the camera-less estimators: the new entry point calls api_fundamental.hip's
    api = open(os.path.join(build.CSRC, "api_homography.hip")).read()
    assert "pairs_batch(" in api and "hipMemcpy" not in api and "Carve" not in api
    assert "four_point.h" in open(os.path.join(ROOT, "sfd2_amd", "build.py")).read()


def test_homography_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "homography.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "homography_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    assert re.findall(r"\.name:\s+(\S*homography_kernel\S*)", meta)
    private = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    assert private and all(int(v) == 0 for v in private)
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", meta)]
    assert lds and max(lds) <= 4 * 1024         # the reductions only: the solver needs no workspace


def test_command_parsers():
    base = ["--pairs", "p.txt", "--features", "f.h5", "--matches", "m.h5", "--output", "v.h5"]
    a = geometric_verification.parser().parse_args(base)
    assert a.model == "essential" and a.two_view_geometries is None
    a = geometric_verification.parser().parse_args(base + ["--model", "geometry", "--two_view_geometries", "T.txt"])
    assert a.model == "geometry" and str(a.two_view_geometries) == "T.txt" and a.reference_sfm_model is None and a.intrinsics == []
    a = geometric_verification.parser().parse_args(base + ["--model", "geometry", "--intrinsics", "q.txt"])
    assert a.model == "geometry" and [str(x) for x in a.intrinsics] == ["q.txt"]
    for model in ("essential", "fundamental"):
        with pytest.raises(ValueError, match="two_view_geometries"):
            geometric_verification.main("p", "f", "m", "o", model=model, two_view_geometries="T.txt")
    with pytest.raises(ValueError, match="relative_poses"):
        geometric_verification.main("p", "f", "m", "o", model="geometry", relative_poses="t.txt")
    with pytest.raises(ValueError, match="fundamental_matrices"):
        geometric_verification.main("p", "f", "m", "o", model="geometry", fundamental_matrices="F.txt")
    r = ["--sfm_dir", "s", "--image_dir", "d", "--pairs", "p", "--features", "f", "--matches", "m"]
    assert reconstruction.parser().parse_args(r).verification == "essential"
    assert reconstruction.parser().parse_args(r + ["--verification", "geometry"]).verification == "geometry"
    assert "verification" not in reconstruction.DEFAULTS
    assert set(two_view.NO_INITIAL_PAIR) == {"panoramic", "planar_or_panoramic", "degenerate"} and "planar" in two_view.CONFIGS


# ---------------------------------------------------------------------------------------------------------------- the decision
N = 200


def _res(k, success=True, first=0, **more):
    """A result dict with k inliers, rows first .. first + k - 1."""
    m = np.zeros(N, dtype=bool)
    m[first:first + k] = True
    return dict(success=success, num_inliers=k, inliers=m, **more)


def _E(k, small=False, success=True, first=0):
    return _res(k, success, first, small_baseline=small)


# (E, F, H) -> (config, model, kept)
DECISIONS = [
    # 1. E stands: calibrated, by the larger of the E and F masks
    ((_E(100), _res(100), _res(30)), ("calibrated", "E", 100)),
    ((_E(100), _res(104), _res(30)), ("calibrated", "F", 104)),
    ((_E(95), _res(100), _res(30)), ("calibrated", "F", 100)),            # exactly 0.95 nF: E stands
    ((_E(94), _res(100), _res(30)), ("uncalibrated", "F", 100)),          # one below
    ((_E(100), _res(0, success=False), _res(0, success=False)), ("calibrated", "E", 100)),
    # H against 0.8 nE: above it the pair is a plane or a panorama
    ((_E(100), _res(100), _res(80)), ("calibrated", "E", 100)),           # exactly 0.8 nE: not above
    ((_E(100), _res(100), _res(81)), ("planar", "E", 100)),
    ((_E(100, small=True), _res(100), _res(81)), ("panoramic", "E", 100)),
    ((_E(100), _res(100), _res(120)), ("planar", "H", 120)),              # H's mask replaces a smaller one
    ((_E(100, small=True), _res(104, first=5), _res(101, first=20)), ("panoramic", "F", 104)),
    ((_E(100, small=True), _res(103), _res(104, first=50)), ("panoramic", "H", 104)),
    ((_E(100, small=True), _res(100), _res(30)), ("calibrated", "E", 100)),   # a small baseline alone decides nothing
    # 2. E does not stand: failed its cheirality test, too few, or no cameras
    ((_E(100, success=False), _res(100), _res(30)), ("uncalibrated", "F", 100)),
    ((_E(100, success=False), _res(100), _res(81)), ("planar_or_panoramic", "F", 100)),
    ((_E(14), _res(100), _res(30)), ("uncalibrated", "F", 100)),
    ((None, _res(100), _res(30)), ("uncalibrated", "F", 100)),
    ((None, _res(100), _res(80)), ("uncalibrated", "F", 100)),            # exactly 0.8 nF
    ((None, _res(100), _res(81)), ("planar_or_panoramic", "F", 100)),
    ((None, _res(100), _res(130, first=10)), ("planar_or_panoramic", "H", 130)),
    # 3. H alone (an exact plane or rotation gives F no result)
    ((None, _res(0, success=False), _res(60, first=7)), ("planar_or_panoramic", "H", 60)),
    ((_E(14), _res(14), _res(15)), ("planar_or_panoramic", "H", 15)),
    ((_E(100, success=False), _res(9), _res(40)), ("planar_or_panoramic", "H", 40)),
    # 4. nothing
    ((None, _res(14), _res(14)), ("degenerate", None, 0)),
    ((_E(14), _res(14), _res(14)), ("degenerate", None, 0)),
    ((_E(100, success=False), _res(0, success=False), _res(0, success=False)), ("degenerate", None, 0)),
]


@pytest.mark.parametrize("k", range(len(DECISIONS)))
def test_decision_table(k):
    (E, F, H), (config, model, kept) = DECISIONS[k]
    d = two_view.decide_two_view_geometry(E, F, H)
    assert set(d) == {"config", "inliers", "num_inliers", "model"} and d["config"] in two_view.CONFIGS
    assert (d["config"], d["model"], d["num_inliers"]) == (config, model, kept)
    want = {"E": E, "F": F, "H": H}.get(model)
    assert d["inliers"].dtype == bool and len(d["inliers"]) == N and int(d["inliers"].sum()) == kept
    assert np.array_equal(d["inliers"], want["inliers"]) if want is not None else not d["inliers"].any()
    assert d["inliers"] is not (want or {}).get("inliers")                # a copy: the caller may change it


def test_decision_thresholds_are_arguments():
    E, F, H = _E(90), _res(100), _res(70)
    assert two_view.decide_two_view_geometry(E, F, H)["config"] == "uncalibrated"
    assert two_view.decide_two_view_geometry(E, F, H, min_E_F_inlier_ratio=0.9)["config"] == "calibrated"
    assert two_view.decide_two_view_geometry(E, F, H, min_E_F_inlier_ratio=0.9, max_H_inlier_ratio=0.7)["config"] == "planar"
    assert two_view.decide_two_view_geometry(E, F, H, min_num_inliers=101)["config"] == "degenerate"
    assert two_view.decide_two_view_geometry(E, F, H, min_num_inliers=95)["config"] == "uncalibrated"
    assert two_view.decide_two_view_geometry(None, F, H, min_num_inliers=95, max_H_inlier_ratio=0.0)["config"] == "uncalibrated"
