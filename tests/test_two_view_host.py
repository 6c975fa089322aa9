"""Relative pose, the parts that need no GPU: the ABI of the three structs, camera validation, no CPU fallback, the build list, the
kernel's resource metadata and the command's parser."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sfd2_amd import _lib, build, geometric_verification, two_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_match_the_header(tmp_path):
    # n, model0, model1, reserved | params0[8], params1[8] | two pointers | max_error_px
    assert ctypes.sizeof(_lib.TwoViewProblem) == 4 * 4 + 2 * 8 * 8 + 2 * 8 + 8
    assert ctypes.sizeof(_lib.TwoViewConf) == 8 + 2 * 8 + 8 + 8 + 2 * 4
    assert ctypes.sizeof(_lib.TwoViewResult) == 4 * 4 + 4 * 8 + 3 * 8 + 9 * 8
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    for name in ("sfd2_two_view_problem", "sfd2_two_view_conf", "sfd2_two_view_result"):
        assert re.search(r"\}\s*" + name + r"\s*;", hdr), name
    assert re.search(r"\bint\s+sfd2_relative_pose_batch\s*\(", hdr) and "sfd2_relative_pose_batch" in _lib.EXPORTS
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:      # the compiler's own layout of the header's structs
        src = tmp_path / "sizes.c"
        src.write_text('#include <stdio.h>\n#include "sfd2_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(sfd2_two_view_problem), '
                       'sizeof(sfd2_two_view_conf), sizeof(sfd2_two_view_result)); return 0; }\n')
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
        got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
        assert got == [ctypes.sizeof(_lib.TwoViewProblem), ctypes.sizeof(_lib.TwoViewConf), ctypes.sizeof(_lib.TwoViewResult)]


def test_camera_validation():
    p = np.random.RandomState(0).uniform(0, 400, (10, 2))
    good = {"model": "PINHOLE", "width": 640, "height": 480, "params": [500, 500, 320, 240]}
    with pytest.raises(ValueError, match="FULL_OPENCV"):
        two_view.relative_pose(p, p, good, {"model": "FULL_OPENCV", "width": 640, "height": 480, "params": [0] * 12})
    with pytest.raises(ValueError, match="takes 3 parameters"):
        two_view.relative_pose(p, p, {"model": "SIMPLE_PINHOLE", "width": 640, "height": 480, "params": [1, 2, 3, 4]}, good)
    with pytest.raises(ValueError, match="10 points in image 0 for 9"):
        two_view.relative_pose(p, p[:9], good, good)
    with pytest.raises(ValueError, match="non-finite"):
        two_view.relative_pose(p, np.where(np.arange(20).reshape(10, 2) == 7, np.inf, p), good, good)


def test_raises_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cam = {"model": "PINHOLE", "width": 640, "height": 480, "params": [500, 500, 320, 240]}
    p = np.random.RandomState(0).uniform(0, 400, (10, 2))
    with pytest.raises(RuntimeError):
        two_view.relative_pose(p, p + 1, cam, cam)


def test_sources_are_in_the_build_list():
    assert "two_view_kernels.hip" in build.SOURCES and "api_two_view.hip" in build.SOURCES
    for f in ("two_view_kernels.hip", "api_two_view.hip", "five_point.h", "ransac_common.h", "ransac_math.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    text = open(os.path.join(build.CSRC, "two_view_kernels.hip")).read()
    # the shared layer (ransac_common.h, ransac_math.h) is the one definition of what the four RANSAC kernels share
    assert '#include "ransac_common.h"' in text
    for pat in (r"\bmix64\s*\(\s*uint64_t", r"\bvoid\s+wg_sum\s*\(", r"\bwg_best\s*\([^)]*\*", r"\bbool\s+finite_d\s*\(", r"\bsolve\d\b", r"\bsample[35]\b"):
        assert not re.search(pat, text), pat
    for helper in ("chol_solve<kNP>(", "normal_acc(", "score_lane(", "score_wg(", "publish_winner(", "ransac_enough(", "sample_k<5>("):
        assert helper in text, helper


def test_two_view_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "two_view.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "two_view_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    assert re.findall(r"\.name:\s+(\S*two_view_kernel\S*)", meta)
    private = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    assert private and all(int(v) == 0 for v in private)
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))


def test_command_parser():
    a = geometric_verification.parser().parse_args(["--pairs", "p.txt", "--features", "f.h5", "--matches", "m.h5", "--output", "v.h5",
                                                    "--reference_sfm_model", "ref"])
    assert (a.max_error, a.min_num_inliers, a.relative_poses, a.intrinsics) == (4.0, 15, None, [])
    a = geometric_verification.parser().parse_args(["--pairs", "p.txt", "--features", "f.h5", "--matches", "m.h5", "--output", "v.h5",
                                                    "--intrinsics", "a.txt", "b.txt", "--max_error", "2.5", "--min_num_inliers", "30",
                                                    "--relative_poses", "t.txt"])
    assert [str(p) for p in a.intrinsics] == ["a.txt", "b.txt"] and a.reference_sfm_model is None
    assert (a.max_error, a.min_num_inliers, str(a.relative_poses)) == (2.5, 30, "t.txt")
    with pytest.raises(SystemExit):
        geometric_verification.parser().parse_args(["--pairs", "p.txt"])
    with pytest.raises(ValueError, match="no intrinsics"):
        geometric_verification.read_cameras(None, [])
