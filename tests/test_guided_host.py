"""Guided matching, the parts that need no GPU: the ABI of sfd2_guided_problem, version and export, the build list, the kernels'
resource metadata, the command's new flags, input validation, the E -> F conversion, guide_of, no CPU fallback -- and the guards of
tests/guided_ref.py's own definitions (band, safe rows, the two wrong variants), which the GPU test relies on."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import guided_ref as gr
from sfd2_amd import _lib, build, geometric_verification, two_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_match_the_header(tmp_path):
    # two sfd2_desc_set (pointer, 4 ints, pointer, 2 ints) | two pointers | model, reserved | M[9] | max_error_px
    assert ctypes.sizeof(_lib.DescSet) == 8 + 4 * 4 + 8 + 2 * 4
    assert ctypes.sizeof(_lib.GuidedProblem) == 2 * ctypes.sizeof(_lib.DescSet) + 2 * 8 + 2 * 4 + 9 * 8 + 8
    assert [f[0] for f in _lib.GuidedProblem._fields_] == ["d0", "d1", "xy0", "xy1", "model", "reserved", "M", "max_error_px"]
    assert (_lib.GUIDE_F, _lib.GUIDE_H) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    assert re.search(r"\}\s*sfd2_guided_problem\s*;", hdr)
    assert re.search(r"#define\s+SFD2_GUIDE_F\s+0\b", hdr) and re.search(r"#define\s+SFD2_GUIDE_H\s+1\b", hdr)
    assert re.search(r"\bint\s+sfd2_match_guided_batch\s*\(", hdr) and "sfd2_match_guided_batch" in _lib.EXPORTS
    assert "122 adds sfd2_match_guided_batch" in hdr
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:      # the compiler's own layout of the header's struct
        fields = ["d1", "xy0", "xy1", "model", "M", "max_error_px"]
        src = tmp_path / "sizes.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfd2_hip.h"\nint main(void) { printf("%zu' + " %zu" * len(fields) + '\\n", '
                       "sizeof(sfd2_guided_problem), " + ", ".join(f"offsetof(sfd2_guided_problem, {f})" for f in fields) + "); return 0; }\n")
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
        got = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")]).split()]
        assert got == [ctypes.sizeof(_lib.GuidedProblem)] + [getattr(_lib.GuidedProblem, f).offset for f in fields]


def test_library_version_and_export():
    core = open(os.path.join(build.CSRC, "api_core.hip")).read()
    assert int(re.search(r"sfd2_version\(void\)\s*\{\s*return\s+(\d+)", core).group(1)) >= 122
    assert re.search(r"sfd2_version\(\) < (\d+)", open(os.path.join(ROOT, "sfd2_amd", "_lib.py")).read()).group(1) == "122"
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.sfd2_version() >= 122 and hasattr(lib, "sfd2_match_guided_batch")


def test_sources_are_in_the_build_list():
    assert "guided_match_kernels.hip" in build.SOURCES and "api_guided.hip" in build.SOURCES
    text = open(os.path.join(build.CSRC, "guided_match_kernels.hip")).read()
    # ONE gate: a single definition, called in the (image 0, image 1) order from both sweeps
    assert len(re.findall(r"bool\s+guided_gate\s*\(", text)) == 1
    assert "guided_gate<MODEL>(mine, cand, t2)" in text and "guided_gate<MODEL>(cand, mine, t2)" in text
    assert "atomic" not in text and "Cooperative" not in text
    api = open(os.path.join(build.CSRC, "api_guided.hip")).read()
    assert '#include "api_scratch.h"' in api and "Carve" in api and "hipMalloc" not in api
    assert "hipStreamSynchronize(c->stream)" in api and "launch_match_prep(" in api
    # the split merge is the matcher's own; the guarded decisions are a kernel of their own, the existing one keeps its text
    mk = open(os.path.join(build.CSRC, "match_kernels.hip")).read()
    fin = mk[mk.index("void launch_guided_finalize"):]
    assert "match_reduce_kernel" in fin and "guided_decide_kernel" in fin and "s1 > -INFINITY" in mk


def test_guided_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "guided.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "guided_match_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    names = re.findall(r"\.name:\s+(\S*guided_\w+_kernel\S*)", meta)
    assert any("guided_top2_kernel" in n for n in names) and any("guided_prep_kernel" in n for n in names)
    private = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    assert private and all(int(v) == 0 for v in private)
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", meta)]
    assert max(lds) == 2 * 64 * (272 + 16)      # two stages of 64 candidates: 272 B of descriptor and a 16 B record each
    assert meta.count("v_mfma_f32_32x32x16_f16") >= 16 and "s_waitcnt" in meta


def test_command_flags():
    base = ["--pairs", "p.txt", "--features", "f.h5", "--matches", "m.h5", "--output", "v.h5"]
    a = geometric_verification.parser().parse_args(base)
    assert a.guided_matching is False and a.guided_conf == "NNM"
    for model in ("essential", "fundamental", "geometry"):
        a = geometric_verification.parser().parse_args(base + ["--model", model, "--guided_matching", "--guided_conf", "NNR"])
        assert a.guided_matching is True and a.guided_conf == "NNR" and a.model == model
    with pytest.raises(SystemExit):
        geometric_verification.parser().parse_args(base + ["--guided_conf", "nope"])
    with pytest.raises(ValueError, match="guided_conf 'nope'"):
        geometric_verification.main("p", "f", "m", "o", model="fundamental", guided_matching=True, guided_conf="nope")
    import inspect
    sig = inspect.signature(geometric_verification.main).parameters
    assert sig["guided_matching"].default is False and sig["guided_conf"].default == "NNM"


def _pair(n0=5, n1=6):
    rs = np.random.RandomState(0)
    return rs.standard_normal((n0, 128)), rs.standard_normal((n1, 128)), rs.uniform(0, 100, (n0, 2)), rs.uniform(0, 100, (n1, 2))


def test_input_validation():
    d0, d1, k0, k1 = _pair()
    F = np.eye(3)
    with pytest.raises(ValueError, match=r"pair 0: descriptors must be \[n, 128\]"):
        two_view.guided_matches(d0[:, :64], d1, k0, k1, "F", F)
    with pytest.raises(ValueError, match="pair 0: 4 and 6 key points for 5 and 6 descriptors"):
        two_view.guided_matches(d0, d1, k0[:4], k1, "F", F)
    with pytest.raises(ValueError, match="pair 1: unknown guide kind 'E'"):
        two_view.guided_matches_batch([(d0, d1, k0, k1, "F", F), (d0, d1, k0, k1, "E", F)])
    with pytest.raises(ValueError, match="pair 0: the guide matrix must be 3 x 3"):
        two_view.guided_matches(d0, d1, k0, k1, "H", np.eye(4))
    with pytest.raises(ValueError, match="pair 0: non-finite key points or matrix"):
        two_view.guided_matches(d0, d1, k0, k1, "H", np.where(np.eye(3) > 0, np.nan, 0.0))
    with pytest.raises(ValueError, match="pair 0: non-finite key points or matrix"):
        two_view.guided_matches(d0, d1, np.where(np.arange(10).reshape(5, 2) == 3, np.inf, k0), k1, "H", F)
    with pytest.raises(ValueError, match="pair 0: max_error_px must be positive"):
        two_view.guided_matches(d0, d1, k0, k1, "H", F, max_error_px=0.0)
    with pytest.raises(ValueError, match="unknown matcher options"):
        two_view.guided_matches(d0, d1, k0, k1, "H", F, conf={"ratio": 0.8})
    with pytest.raises(ValueError, match="sim_mode 'f16' only"):
        two_view.guided_matches(d0, d1, k0, k1, "H", F, conf={"sim_mode": "f16x2"})
    with pytest.raises(ValueError, match="1 results for 0 pairs"):
        two_view.guided_match_pairs({}, {}, [], [{}])
    assert two_view.guided_matches_batch([]) == []
    out, off, counts, scores = two_view.guided_match_pairs({}, {}, [], [])
    assert out.shape == (0, 2) and list(off) == [0] and len(counts) == 0 and len(scores) == 0
    # pairs without a guide need no device: all -1, in verify_pairs_*'s shape
    fail = {"success": False, "F": np.zeros((3, 3)), "num_inliers": 0, "inliers": np.zeros(0, bool)}
    out, off, counts, scores = two_view.guided_match_pairs({0: k0, 1: k1}, {0: d0, 1: d1}, [(0, 1, np.zeros((0, 2))), (1, 1, np.zeros((0, 2)))],
                                                           [fail, dict(fail, success=True, F=np.eye(3))])
    assert out.dtype == np.int32 and out.shape == (5 + 6, 2) and (out == -1).all() and list(off) == [0, 5, 11] and list(counts) == [0, 0]
    assert scores.dtype == np.float32 and not scores.any()


def test_raises_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    d0, d1, k0, k1 = _pair()
    with pytest.raises(RuntimeError):
        two_view.guided_matches(d0, d1, k0, k1, "F", np.eye(3))
    ok = {"success": True, "H": np.eye(3), "num_inliers": 20, "inliers": np.ones(0, bool)}
    with pytest.raises(RuntimeError):
        two_view.guided_match_pairs({0: k0, 1: k1}, {0: d0, 1: d1}, [(0, 1, np.zeros((0, 2)))], [ok])


def test_fundamental_from_essential():
    rs = np.random.RandomState(3)
    E = rs.standard_normal((3, 3))
    cams = [{"model": "SIMPLE_PINHOLE", "params": [1400.0, 800.0, 600.0]}, {"model": "PINHOLE", "params": [900.0, 950.0, 310.0, 250.0]},
            {"model": "SIMPLE_RADIAL", "params": [700.0, 320.0, 240.0, 0.1]}, {"model": "OPENCV", "params": [800.0, 820.0, 330.0, 230.0, 0.1, 0.01, 1e-3, 1e-3]}]
    Ks = [np.array([[1400.0, 0, 800.0], [0, 1400.0, 600.0], [0, 0, 1]]), np.array([[900.0, 0, 310.0], [0, 950.0, 250.0], [0, 0, 1]]),
          np.array([[700.0, 0, 320.0], [0, 700.0, 240.0], [0, 0, 1]]), np.array([[800.0, 0, 330.0], [0, 820.0, 230.0], [0, 0, 1]])]
    for a in range(4):
        for b in range(4):
            want = np.linalg.inv(Ks[b]).T @ E @ np.linalg.inv(Ks[a])
            want /= np.linalg.norm(want)
            got = two_view.fundamental_from_essential(E, cams[a], cams[b])
            assert got.shape == (3, 3) and np.allclose(got, want, rtol=0, atol=1e-14)
    assert "istortion is ignored" in two_view.fundamental_from_essential.__doc__ or "distortion is ignored" in two_view.fundamental_from_essential.__doc__
    # a normalised correspondence on E's epipolar line lies on F's in pixels
    x0, x1n = np.array([0.1, -0.2, 1.0]), None
    l = E @ x0
    x1n = np.array([0.3, -(l[0] * 0.3 + l[2]) / l[1], 1.0])
    F = two_view.fundamental_from_essential(E, cams[0], cams[1])
    assert abs((Ks[1] @ x1n) @ F @ (Ks[0] @ x0)) < 1e-9


def test_guide_of():
    rs = np.random.RandomState(4)
    E, F, H = rs.standard_normal((3, 3)), rs.standard_normal((3, 3)), rs.standard_normal((3, 3))
    cam = {"model": "SIMPLE_PINHOLE", "params": [1000.0, 500.0, 400.0]}
    rE = {"success": True, "E": E, "qvec": np.zeros(4), "tvec": np.zeros(3), "small_baseline": False, "num_inliers": 30}
    rF = {"success": True, "F": F, "num_inliers": 30}
    rH = {"success": True, "H": H, "num_inliers": 30}
    kind, M = two_view.guide_of(rE, cam, cam)
    assert kind == "F" and np.array_equal(M, two_view.fundamental_from_essential(E, cam, cam))
    with pytest.raises(ValueError, match="cameras are needed"):
        two_view.guide_of(rE)
    assert two_view.guide_of(rF)[0] == "F" and np.array_equal(two_view.guide_of(rF)[1], F)
    assert two_view.guide_of(rH)[0] == "H" and np.array_equal(two_view.guide_of(rH)[1], H)
    for model, want in (("E", "F"), ("F", "F"), ("H", "H")):
        d = {"config": "planar", "model": model, "E": rE, "F": rF, "H": rH, "inliers": np.ones(3, bool), "num_inliers": 3}
        kind, M = two_view.guide_of(d, cam, cam)
        assert kind == want and np.array_equal(M, {"E": two_view.fundamental_from_essential(E, cam, cam), "F": F, "H": H}[model])
    assert two_view.guide_of({"config": "degenerate", "model": None, "E": None, "F": rF, "H": rH}) is None
    assert two_view.guide_of(dict(rF, success=False)) is None and two_view.guide_of(dict(rH, success=False)) is None
    with pytest.raises(ValueError, match="not a two-view result"):
        two_view.guide_of({"success": True})
    # the guide of a model estimated on key points + 0.5, for the key points as stored
    x0, x1 = np.array([10.0, 20.0, 1.0]), np.array([30.0, 5.0, 1.0])
    s = np.array([0.5, 0.5, 0.0])
    assert np.isclose((x1 + s) @ F @ (x0 + s), x1 @ two_view._guide_for_stored("F", F) @ x0, rtol=1e-12, atol=1e-12)
    p, q = H @ (x0 + s), two_view._guide_for_stored("H", H) @ x0
    assert np.allclose(p[:2] / p[2] - 0.5, q[:2] / q[2], rtol=1e-12, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------- the restatement's guards
def test_band_is_the_measured_one():
    got = gr.measured_band()
    print("8 x the largest relative float32 / fp64 difference:", got)
    for kind in ("F", "H"):
        assert 0.5 * gr.BAND_MEASURED[kind] <= got[kind] <= gr.BAND_MEASURED[kind] <= gr.BAND <= 1e-2
    assert 10 * gr.BAND <= gr.OUTSIDE


@pytest.mark.parametrize("kind", ["F", "H"])
def test_float32_gate_differs_only_on_banded_pairs(kind):
    for n0, n1 in gr.SIZES:
        sc = gr.scene(kind, n0, n1)
        e, p = gr.gate64(kind, sc["M"], sc["xy0"], sc["xy1"])
        _, p32 = gr.gate32(kind, sc["M"], sc["xy0"], sc["xy1"])
        banded = np.abs(e - gr.MAX_ERROR ** 2) <= gr.BAND * gr.MAX_ERROR ** 2
        assert not ((p != p32) & ~banded).any()
        assert 0 < p.mean() < 0.05


@pytest.mark.parametrize("kind", ["F", "H"])
@pytest.mark.parametrize("conf", list(gr.CONFS))
def test_most_rows_are_safe(kind, conf):
    for n0, n1 in gr.GUARD_SIZES:
        sc = gr.scene(kind, n0, n1)
        e, _ = gr.gate64(kind, sc["M"], sc["xy0"], sc["xy1"])
        frac = gr.safe_rows(sc["sim"], e, **gr.CONFS[conf]).mean()
        print(kind, conf, n0, n1, f"safe {frac:.3f}")
        assert frac >= 0.9


def test_dropping_the_gate_changes_the_twin_scene():
    sc = gr.twin_scene()
    e, p = gr.gate64("F", sc["M"], sc["xy0"], sc["xy1"])
    assert 0.005 < p.mean() < 0.02                        # the gate lets through about one pair in a hundred
    c = gr.CONFS["RATIO"]
    safe = gr.safe_rows(sc["sim"], e, **c)
    m, _ = gr.hloc_masked(sc["sim"], p, **c)
    w, _ = gr.hloc_no_gate(sc["sim"], **c)
    changed = (m != w)[safe].mean()
    print(f"twin scene: guided keeps {(m >= 0).sum()}, plain {(w >= 0).sum()} of 200; {changed:.2f} of the safe rows change; safe {safe.mean():.3f}")
    assert safe.mean() >= 0.9 and changed >= 0.2
    tw = sc["twinned"]
    # (a twin within 0.02 cosine leaves the ratio test at 0.8 a chance only where 1 - c < 0.02 / 0.36: the top 2 % of U(0.7, 0.95))
    assert (m[tw] >= 0).sum() >= 140 and (w[tw] >= 0).sum() <= 10 and (m >= 0).sum() >= 190 and (w >= 0).sum() <= 60


def test_transposed_reverse_changes_the_h_scene():
    sc = gr.scene("H", 257, 300)
    e, p = gr.gate64("H", sc["M"], sc["xy0"], sc["xy1"])
    c = gr.CONFS["NNM"]
    safe = gr.safe_rows(sc["sim"], e, **c)
    m, _ = gr.hloc_masked(sc["sim"], p, **c)
    w, _ = gr.hloc_transposed_reverse(sc["sim"], "H", sc["M"], sc["xy0"], sc["xy1"])
    assert (m != w)[safe].sum() >= 1


def test_masked_rule_edge_cases():
    sim = np.array([[0.9, 0.8, 0.1], [0.5, 0.6, 0.2], [0.3, 0.2, 0.1]])
    none = np.zeros((3, 3), dtype=bool)
    for mutual in (False, True):                          # nothing gated, row 0 and column 0 empty too: no match anywhere, score 0
        m, s = gr.hloc_masked(sim, none, ratio=0.8, mutual=mutual)
        assert (m == -1).all() and not s.any()
    one = none.copy()
    one[1, 2] = True                                      # one gated candidate: s2 = -inf, the ratio test passes
    m, s = gr.hloc_masked(sim, one, ratio=0.8, mutual=True)
    assert list(m) == [-1, 2, -1] and s[1] == (0.2 + 1) / 2 and s[0] == 0 and s[2] == 0
    dup = np.array([[0.7, 0.7, 0.1]])                     # a duplicated maximum inside the gate: first index, no ratio below 1 passes
    m, _ = gr.hloc_masked(dup, np.ones((1, 3), bool), ratio=None, mutual=False)
    assert list(m) == [0]
    m, _ = gr.hloc_masked(dup, np.ones((1, 3), bool), ratio=0.999, mutual=False)
    assert list(m) == [-1]
    m, _ = gr.hloc_masked(dup, np.array([[True, False, True]]), ratio=0.8, mutual=False)      # ... outside the gate it does not count
    assert list(m) == [0]
    assert gr.hloc_masked(np.zeros((2, 0)), np.zeros((2, 0), bool))[0].tolist() == [-1, -1]
    assert gr.splits(1, 2049) == 8 and gr.splits(1, 300) == 8 and gr.splits(50, 4096) == 2 and gr.splits(1, 33) == 2 and gr.chunk(2049, 8) == 288


@pytest.mark.parametrize("kind", ["F", "H"])
def test_forced_scenes_are_what_they_say(kind):
    for n0, n1 in ((300, 300), (300, 2049)):
        c, pairs = gr.forced_pairs(n1)
        assert c == gr.chunk(n1, gr.splits(1, max(n0, n1)))
        sc = gr.forced_scene(kind, n0, n1, pairs)
        e, p = gr.gate64(kind, sc["M"], sc["xy0"], sc["xy1"])
        q, j1, j2 = sc["q"], sc["j1"], sc["j2"]
        assert p[q, j1].all() and not p[q, j2].any() and (sc["sim"][q, j2] > sc["sim"][q, j1] + 0.05).all()
        assert (e[q, j2] / gr.MAX_ERROR ** 2 - 1 >= 10 * gr.BAND).all() and (e[q, j2] / gr.MAX_ERROR ** 2 - 1 <= 2 * gr.OUTSIDE).all()
        for conf in gr.CONFS.values():
            safe = gr.safe_rows(sc["sim"], e, **conf)
            m, _ = gr.hloc_masked(sc["sim"], p, **conf)
            w, _ = gr.hloc_no_gate(sc["sim"], ratio=None, dist=None, mutual=False)
            assert safe[q].all() and (m[q] == j1).all() and (w[q] == j2).all()
