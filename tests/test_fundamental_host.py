"""Fundamental matrix, the parts that need no GPU: the ABI of the two structs, input validation, no CPU fallback, the build list,
the kernel's resource metadata and the two commands' parsers."""
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
    assert ctypes.sizeof(_lib.FundamentalProblem) == 2 * 4 + 2 * 8 + 8
    # success, num_inliers, num_trials, reserved | F[9]
    assert ctypes.sizeof(_lib.FundamentalResult) == 4 * 4 + 9 * 8
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    for name in ("sfd2_fundamental_problem", "sfd2_fundamental_result"):
        assert re.search(r"\}\s*" + name + r"\s*;", hdr), name
    assert re.search(r"\bint\s+sfd2_fundamental_batch\s*\(", hdr) and "sfd2_fundamental_batch" in _lib.EXPORTS
    assert "120 adds sfd2_fundamental_batch" in hdr
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:      # the compiler's own layout of the header's structs
        src = tmp_path / "sizes.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfd2_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                       'sizeof(sfd2_fundamental_problem), sizeof(sfd2_fundamental_result), offsetof(sfd2_fundamental_problem, max_error_px), '
                       'offsetof(sfd2_fundamental_result, F)); return 0; }\n')
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
        got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
        assert got == [ctypes.sizeof(_lib.FundamentalProblem), ctypes.sizeof(_lib.FundamentalResult),
                       _lib.FundamentalProblem.max_error_px.offset, _lib.FundamentalResult.F.offset]


def test_library_version_and_export():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.sfd2_version() >= 120 and hasattr(lib, "sfd2_fundamental_batch")


def test_input_validation():
    p = np.random.RandomState(0).uniform(0, 400, (10, 2))
    with pytest.raises(ValueError, match="10 points in image 0 for 9"):
        two_view.fundamental_matrix(p, p[:9])
    with pytest.raises(ValueError, match="non-finite"):
        two_view.fundamental_matrix(p, np.where(np.arange(20).reshape(10, 2) == 7, np.inf, p))
    with pytest.raises(ValueError, match="non-finite"):
        two_view.fundamental_matrix_batch([(p, p + 1), (np.where(np.arange(20).reshape(10, 2) == 0, np.nan, p), p)])
    with pytest.raises(ValueError, match="beyond the 10 key points of image 1"):
        two_view.verify_pairs_fundamental({0: p, 1: p}, [(0, 1, np.array([[0, 1], [2, 10]]))])
    assert two_view.fundamental_matrix_batch([]) == []


def test_raises_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = np.random.RandomState(0).uniform(0, 400, (10, 2))
    with pytest.raises(RuntimeError):
        two_view.fundamental_matrix(p, p + 1)
    with pytest.raises(RuntimeError):
        two_view.verify_pairs_fundamental({0: p, 1: p}, [(0, 1, np.stack([np.arange(10), np.arange(10)], 1))])


def test_sources_are_in_the_build_list():
    assert "fundamental_kernels.hip" in build.SOURCES and "api_fundamental.hip" in build.SOURCES
    for f in ("fundamental_kernels.hip", "api_fundamental.hip", "seven_point.h", "ransac_common.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    assert os.path.exists(os.path.join(build.CSRC, "ransac_math.h"))
    text = open(os.path.join(build.CSRC, "fundamental_kernels.hip")).read()
    assert "uint64_t mix64" not in text
    # the shared layer (ransac_common.h, ransac_math.h) is the one definition of what the four RANSAC kernels share
    assert '#include "ransac_common.h"' in text
    for pat in (r"\bmix64\s*\(\s*uint64_t", r"\bvoid\s+wg_sum\s*\(", r"\bwg_best\s*\([^)]*\*", r"\bbool\s+finite_d\s*\(", r"\bsolve\d\b", r"\bsample[35]\b"):
        assert not re.search(pat, text), pat
    for helper in ("chol_solve<kNP>(", "normal_acc(", "publish_winner(", "ransac_enough(", "finish_matrix(", "sample_k<7>("):
        assert helper in text, helper


def test_fundamental_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "fundamental.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "fundamental_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    assert re.findall(r"\.name:\s+(\S*fundamental_kernel\S*)", meta)
    private = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    assert private and all(int(v) == 0 for v in private)
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", meta)]
    assert lds and max(lds) <= 160 * 1024       # the 7 x 9 systems of 256 lanes and the reductions: one workgroup per CU


def test_command_parsers():
    base = ["--pairs", "p.txt", "--features", "f.h5", "--matches", "m.h5", "--output", "v.h5"]
    a = geometric_verification.parser().parse_args(base + ["--reference_sfm_model", "ref"])
    assert (a.max_error, a.min_num_inliers, a.relative_poses, a.intrinsics, a.model, a.fundamental_matrices) == (4.0, 15, None, [], "essential", None)
    a = geometric_verification.parser().parse_args(base + ["--model", "fundamental", "--fundamental_matrices", "F.txt"])
    assert a.model == "fundamental" and str(a.fundamental_matrices) == "F.txt" and a.reference_sfm_model is None and a.intrinsics == []
    with pytest.raises(SystemExit):
        geometric_verification.parser().parse_args(base + ["--model", "homography"])
    with pytest.raises(ValueError, match="no intrinsics"):
        geometric_verification.read_cameras(None, [])
    with pytest.raises(ValueError, match="relative_poses"):
        geometric_verification.main("p", "f", "m", "o", model="fundamental", relative_poses="t.txt")
    with pytest.raises(ValueError, match="no intrinsics"):
        geometric_verification.main("p", "f", "m", "o")
    r = ["--sfm_dir", "s", "--image_dir", "d", "--pairs", "p", "--features", "f", "--matches", "m"]
    a = reconstruction.parser().parse_args(r)
    assert a.verification == "essential" and not a.skip_geometric_verification and a.device == 0
    assert reconstruction.parser().parse_args(r + ["--verification", "fundamental"]).verification == "fundamental"
    with pytest.raises(SystemExit):
        reconstruction.parser().parse_args(r + ["--verification", "homography"])
    assert "verification" not in reconstruction.DEFAULTS
    with pytest.raises(ValueError, match="unknown verification"):
        reconstruction.reconstruct({}, {}, {}, [], verification="homography")
