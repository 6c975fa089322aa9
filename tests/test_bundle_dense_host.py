"""The dense solver of the reduced camera system, the parts that need no GPU: the solver word of sfd2_ba_conf in
header and binding, the option's way from the Python calls and the two commands to that word, the refusals raised before any call, the
mapper passing the option on only when it is asked for, the build list, the new kernels' resource metadata, and the test systems of
tests/bundle_dense_ref.py checked against what the GPU tests rely on."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bundle_dense_ref as dr
import mapper_ref as mr
import tri_ref as tr
from sfd2_amd import _lib, build, bundle_adjustment as B, reconstruction as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- header and binding
def test_header_constants_match_the_binding(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    for k, v in (("SOLVER_PCG", 0), ("SOLVER_DENSE", 1), ("DENSE_MAX_VIEWS", 2048)):
        assert re.search(r"#define SFD2_BA_%s %d\b" % (k, v), hdr) and getattr(_lib, "BA_" + k) == v, k
    assert re.search(r"\bint\s+sfd2_spd_solve\s*\(", hdr) and "sfd2_spd_solve" in _lib.EXPORTS
    assert ctypes.sizeof(_lib.BaConf) == 4 * 4 + 5 * 8 + 4 * 4                 # the struct keeps its size: the word was reserved[0]
    assert _lib.BaConf.solver.offset == 4 * 4 + 5 * 8 and _lib.BaConf.reserved.offset == _lib.BaConf.solver.offset + 4
    assert _lib.BaConf.reserved.size == 12
    assert _lib.BaConf().solver == _lib.BA_SOLVER_PCG                          # a zeroed conf is the conjugate gradients
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:      # the compiler's own layout of the header's struct
        src = tmp_path / "solver.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfd2_hip.h"\nint main(void) { printf("%zu %zu %zu %d %d %d\\n", sizeof(sfd2_ba_conf), '
                       'offsetof(sfd2_ba_conf, solver), offsetof(sfd2_ba_conf, reserved), SFD2_BA_SOLVER_PCG, SFD2_BA_SOLVER_DENSE, SFD2_BA_DENSE_MAX_VIEWS); '
                       'return 0; }\n')
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "solver")])
        got = [int(v) for v in subprocess.check_output([str(tmp_path / "solver")]).split()]
        assert got == [ctypes.sizeof(_lib.BaConf), _lib.BaConf.solver.offset, _lib.BaConf.reserved.offset, _lib.BA_SOLVER_PCG, _lib.BA_SOLVER_DENSE,
                       _lib.BA_DENSE_MAX_VIEWS]


def test_library_exports_the_solve():
    lib = _lib.load()
    assert hasattr(lib, "sfd2_spd_solve") and lib.sfd2_version() >= 124


def test_sources_are_in_the_build_list():
    assert "bundle_dense_kernels.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "bundle_dense_kernels.hip"))
    assert "getenv" not in open(os.path.join(build.CSRC, "bundle_dense_kernels.hip")).read()


def test_dense_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "bundle_dense.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "bundle_dense_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    names = re.findall(r"\.name:\s+(\S*dense_\w+_kernel\S*)", meta)
    for k in ("ba_dense_pairs", "ba_dense_block_start", "ba_dense_g", "ba_dense_form", "ba_dense_veto", "dense_pad", "dense_rhs", "dense_potrf_tile",
              "dense_trsm_tile", "dense_syrk_tile", "dense_forward", "dense_backward"):
        assert any(k + "_kernel" in n for n in names), k
    private = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    assert len(private) >= len(names) and all(int(v) == 0 for v in private)
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))
    assert all(int(v) == 0 for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", meta))
    assert all(int(v) <= 65536 for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", meta))
    assert "v_mfma_f64_16x16x4_f64" in meta                                    # the trailing update runs on the fp64 matrix instruction


# ---------------------------------------------------------------------------------------------------------------- the option's way
def test_the_option_reaches_the_conf_word():
    assert B.DEFAULTS["solver"] == "pcg" and B.SOLVERS == {"pcg": _lib.BA_SOLVER_PCG, "dense": _lib.BA_SOLVER_DENSE}
    assert B._conf({}).solver == _lib.BA_SOLVER_PCG and B._conf(dict(solver="pcg")).solver == _lib.BA_SOLVER_PCG
    conf = B._conf(dict(solver="dense", max_iterations=7))
    assert conf.solver == _lib.BA_SOLVER_DENSE and list(conf.reserved) == [0, 0, 0] and conf.max_iterations == 7
    with pytest.raises(ValueError, match="cholesky"):
        B._conf(dict(solver="cholesky"))


def test_value_errors_are_raised_before_any_call():
    views = (_lib.TriView * 2)()
    with pytest.raises(ValueError, match="dense"):
        B.adjust_cameras([1], np.zeros((1, 8)), [1], [0, 0], views, 2, [1, 0], np.zeros((1, 3)), [0], [0, 2], [0, 1], np.zeros((2, 2)), solver="dense")
    with pytest.raises(ValueError, match="solver"):
        B.adjust(views, 2, [1, 0], np.zeros((1, 3)), [0], [0, 2], [0, 1], np.zeros((2, 2)), solver="sparse")
    with pytest.raises(ValueError, match="dense"):
        B.bundle_adjust({}, {}, {}, refine_focal_length=True, solver="dense")
    sc = _scene()
    for refine in ("refine_focal_length", "refine_principal_point", "refine_extra_params"):
        with pytest.raises(ValueError, match="refine"):
            RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], stages=mr.RefStages(sc), ba_solver="dense", **{refine: True})
    with pytest.raises(ValueError, match="ba_solver"):
        RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], stages=mr.RefStages(sc), ba_solver="sparse")
    with pytest.raises(ValueError):
        B.spd_solve(np.eye(3), np.zeros(2))


def test_command_line_flags():
    a = B.parser().parse_args(["--input_path", "m", "--output_path", "o"])
    assert a.solver == "pcg"
    a = B.parser().parse_args(["--input_path", "m", "--output_path", "o", "--solver", "dense"])
    assert a.solver == "dense" and set(vars(a)) <= set(B.main.__code__.co_varnames[:B.main.__code__.co_argcount])
    with pytest.raises(SystemExit):
        B.parser().parse_args(["--input_path", "m", "--output_path", "o", "--solver", "sparse"])
    base = ["--sfm_dir", "s", "--image_dir", "d", "--pairs", "p", "--features", "f", "--matches", "m"]
    a = RC.parser().parse_args(base)
    assert a.ba_solver == "pcg" == RC.DEFAULTS["ba_solver"]
    a = RC.parser().parse_args(base + ["--ba_solver", "dense"])
    assert a.ba_solver == "dense" and set(vars(a)) <= set(RC.main.__code__.co_varnames[:RC.main.__code__.co_argcount])
    with pytest.raises(SystemExit):
        RC.parser().parse_args(base + ["--ba_solver", "sparse"])


# ---------------------------------------------------------------------------------------------------------------- the mapper
def _scene():
    return mr.br.cached(("mapper_host_scene",), tr.make_scene)


def _options_of_every_adjust_call(**kw):
    sc, rep = _scene(), {}
    S = mr.RefStages(sc)
    RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], stages=S, report=rep, **kw)
    calls = [r["ba"]["options"] for r in rep["rounds"]] + [rep["final"]["ba"]["options"]]
    assert len(calls) == len(S.calls["adjust"]) >= 2
    return calls


def test_the_mapper_passes_the_solver_on_only_when_asked():
    plain = _options_of_every_adjust_call()
    assert all(set(o) == {"max_iterations", "loss", "loss_scale"} for o in plain)           # the calls RefStages records stay as they were
    assert _options_of_every_adjust_call(ba_solver="pcg") == plain
    dense = _options_of_every_adjust_call(ba_solver="dense")
    assert len(dense) == len(plain) and all(o["solver"] == "dense" for o in dense)
    assert [{k: v for k, v in o.items() if k != "solver"} for o in dense] == plain


# ---------------------------------------------------------------------------------------------------------------- the test systems
def test_the_spd_systems_are_what_the_gpu_tests_take_them_for():
    assert dr.SPD_SIZES == (1, 5, 6, 63, 64, 65, 127, 128, 129, 258, 1000) and dr.FAIL_AT == (1, 64, 65, 200) and dr.FAIL_N == 258
    for n in (5, 65, 258):
        A, b = dr.spd_system(n, "random")
        assert (A == A.T).all() and np.linalg.eigvalsh(A).min() >= n - 1e-9 * n and len(b) == n
        assert dr.backward_error(A, np.linalg.solve(A, b) * (1 + 1e-6), b) > 1e-8               # the measure sees a wrong answer
        A, b = dr.spd_system(n, "ill")
        w = np.linalg.eigvalsh(A)
        assert (A == A.T).all() and w.min() > 0 and 0.5e10 < w.max() / w.min() < 2e10         # ten decades
        x = np.linalg.solve(A, b)
        assert dr.backward_error(A, x, b) <= dr.higham_bound(n)
    for k in dr.FAIL_AT:
        A, _ = dr.indefinite(k)
        assert (A == A.T).all() and (np.linalg.eigvalsh(A) < 0).sum() == 1
        if k > 1:
            np.linalg.cholesky(A[:k - 1, :k - 1])
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(A[:k, :k])
