"""Absolute pose with an unknown focal length, the parts that need no GPU: the restatement of tests/pose_focal_ref.py checked on its
own (ground truth, its two LM formulations, the growing masks, broken rules that must show), the new kernels' resource metadata, the
ABI and the argument checks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pose_focal_ref as fr
import pose_ref as pr
from sfd2_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(sc, **kw):
    x, X, cam, prior, q, t, thr = fr.make_scene(*sc)
    return fr.focal_pose_ref(x, X, prior, thr, key=sc, **kw, **fr.CONF), cam, q, t


def test_factor_set():
    a = fr.factors()
    assert len(a) == 31 and a[0] == 0.2 and a[30] == 5.0 and (np.diff(a) > 0).all()
    assert a[15] == 0.2 + 4.8 * 0.25                          # from the integer index, not by accumulation
    assert fr.factors(1, 0.5, 2.0).tolist() == [0.5, 2.0]
    cam = fr.scaled_camera(pr.camera("OPENCV"), 2.0)
    assert cam["params"][:2] == [1610.0, 1590.0] and cam["params"][2:] == pr.PARAMS["OPENCV"][2:]
    assert fr.scaled_camera(pr.camera("SIMPLE_RADIAL"), 0.5)["params"] == [400.0, 320.0, 240.0, -0.08]


@pytest.mark.parametrize("sc", fr.SWEEP_SCENES, ids=lambda s: s[0])
def test_the_sweep_peaks_and_the_restatement_finds_the_truth(sc):
    r, cam, q, t = _run(sc, estimate=True, refine_focal=True)
    cnt = sorted((s["cnt"] for s in r["sweep"]), reverse=True)
    assert r["success"] and not r["banded"] and cnt[0] > cnt[1]
    true_factor = sc[5]
    a = fr.factors()
    assert abs(np.argmin(np.abs(a - true_factor)) - r["focal_sample"]) <= 1
    assert fr.focal_error(r["camera"], cam) <= 0.01 and np.degrees(pr.rot_angle(r["qvec"], q)) <= 0.25
    assert r["num_inliers"] >= r["ransac_num_inliers"]


def test_mask_sizes_grow_between_two_samples():
    """24 -> 37 -> 40 (PINHOLE, seed 13, ratio 1.035) and 26 -> 45 -> 56 (SIMPLE_PINHOLE, seed 14, ratio 0.4267): the winner holds part
    of the inliers, refining and re-scoring recovers all of them (40 and 56 of 80 are the scenes' inliers)."""
    sizes = []
    for sc in fr.MIDGAP_SCENES:
        r, cam, q, t = _run(sc, estimate=True, refine_focal=True)
        sizes.append(r["sizes"])
        assert fr.focal_error(r["camera"], cam) <= 0.003 and np.degrees(pr.rot_angle(r["qvec"], q)) <= 0.1
        assert r["num_inliers"] == r["sizes"][-1] == int(r["inliers"].sum())
    assert sizes[0] == [24, 37, 40]
    assert sizes[1] == [26, 45, 56]            # (the issue's 47 in the middle came from a scene whose size it does not give)


def test_two_lm_formulations_agree():
    for sc in (fr.MIDGAP_SCENES[0], fr.SWEEP_SCENES[2]):
        extra = sc[0] == "OPENCV"
        a, cam, q, t = _run(sc, estimate=True, refine_focal=True, refine_extra=extra)
        b, *_ = _run(sc, estimate=True, refine_focal=True, refine_extra=extra, jac="numeric")
        nf = fr.N_FOCAL[sc[0]]
        pa, pb = np.array(a["camera"]["params"]), np.array(b["camera"]["params"])
        assert np.abs(pa[:nf] / pb[:nf] - 1).max() <= 1e-7 and np.abs(pa[nf:] - pb[nf:]).max() <= 1e-6
        assert pr.rot_angle(a["qvec"], b["qvec"]) <= 1e-7 and np.array_equal(a["inliers"], b["inliers"])
        assert pa[nf:nf + 2].tolist() == cam["params"][nf:nf + 2]          # the principal point is never refined


def test_broken_rules_show():
    sc = fr.MIDGAP_SCENES[0]
    good, *_ = _run(sc, estimate=True, refine_focal=True)
    once, *_ = _run(sc, estimate=True, refine_focal=True, rounds=1)          # no re-scoring
    assert once["num_inliers"] == good["sizes"][0] < good["num_inliers"]
    # the sweep cap ignored: a sample's trial count changes
    x, X, cam, prior, q, t, thr = fr.make_scene(*fr.SWEEP_SCENES[3])
    conf = dict(min_num_trials=2000, confidence=0.9999)
    a = fr.sweep_ref(x, X, prior, thr, S=4, **conf)
    b = fr.sweep_ref(x, X, prior, thr, S=4, ignore_cap=True, **conf)
    assert all(s["num_trials"] == 1024 for s in a) and any(s["num_trials"] != 1024 for s in b)
    # selection on the sum in normalised units: between samples of equal count the larger focal wins the normalised sum.  None of the
    # committed scenes has a count tie between its two best samples (asserted), so the rule is shown on two hand-made records
    for c in fr.SWEEP_SCENES + fr.MIDGAP_SCENES:
        sweep = _run(c, estimate=True)[0]["sweep"]
        w, r = fr.select_ref(sweep)
        assert sweep[w]["cnt"] > sweep[r]["cnt"] and fr.select_ref(sweep, "sum")[0] == w
    sw = [{"cnt": 10, "sum": np.float32(1e-4), "sum_px": np.float32(1e-4 * 400 ** 2), "banded": False},
          {"cnt": 10, "sum": np.float32(0.5e-4), "sum_px": np.float32(0.5e-4 * 800 ** 2), "banded": False}]
    assert fr.select_ref(sw)[0] == 0 and fr.select_ref(sw, "sum")[0] == 1


def test_focal_kernels_compile_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "pose_focal.s"
    src = os.path.join(build.CSRC, "pose_focal_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    names = " ".join(re.findall(r"\.name:\s+(\S+)", meta))
    for kernel in ("pose_sweep_kernel", "pose_focal_select_kernel", "pose_cam_refine_kernel"):
        assert kernel in names
    assert "11pose_kernel" not in names                                    # the solver's kernel stays in its own translation unit
    priv = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    assert len(priv) == 3 and all(int(v) == 0 for v in priv)
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta))


def test_no_second_copy_of_the_solver():
    text = open(os.path.join(build.CSRC, "pose_focal_kernels.hip")).read()
    assert '#include "pose_kernels.hip"' in text and "#define SFD2_POSE_KERNEL_HEAD" in text and "#define SFD2_POSE_AFTER_RANSAC" in text
    for pat in (r"\bvoid\s+p3p\s*\(", r"\beval_f32\s*\([^;]*\)\s*\{", r"sample_k<3>", r"ransac_enough\("):
        assert not re.search(pat, text), pat
    assert "pose_focal_kernels.hip" in build.SOURCES


def test_abi():
    lib = _lib.load()
    assert lib.sfd2_version() >= 125
    assert hasattr(lib, "sfd2_absolute_pose_focal_batch") and hasattr(lib, "sfd2_pose_refine_camera_batch")
    assert ctypes.sizeof(_lib.PoseFocalConf) == 56 and ctypes.sizeof(_lib.PoseFocalResult) == 152 and ctypes.sizeof(_lib.PoseSweepRecord) == 16
    header = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    assert "absolute pose, unknown focal" in header


def _call(fc_kw=None, conf_kw=None, model=1, params=(500.0, 500.0, 320.0, 240.0), n=6, bad_point=False, refine=False):
    """The entry points on a context that is never touched: every check comes before the first use of the device."""
    lib = _lib.load()
    lib.sfd2_last_error.restype = ctypes.c_char_p
    ctx = ctypes.create_string_buffer(1 << 16)
    x, X = np.random.RandomState(0).rand(n, 2) * 100, np.random.RandomState(1).rand(n, 3) + [0, 0, 5]
    if bad_point:
        X[2, 1] = np.nan
    p = _lib.PoseProblem()
    p.n, p.model, p.points2D, p.points3D, p.max_error_px = n, model, x.ctypes.data, X.ctypes.data, 12.0
    for i, v in enumerate(params):
        p.params[i] = v
    conf = _lib.PoseConf(0.01, 0, 1000, 0.9999, 0)
    for k, v in (conf_kw or {}).items():
        setattr(conf, k, v)
    fc = _lib.PoseFocalConf(1, 1, 0, 30, 0.2, 5.0, 1024)
    for k, v in (fc_kw or {}).items():
        if k == "reserved":
            fc.reserved[1] = v
        else:
            setattr(fc, k, v)
    res = (_lib.PoseFocalResult * 1)()
    mask = np.zeros(n, np.uint8)
    if refine:
        qt = np.array([1.0, 0, 0, 0, 0, 0, 0])
        rc = lib.sfd2_pose_refine_camera_batch(ctypes.addressof(ctx), (_lib.PoseProblem * 1)(p), 1, qt.ctypes.data, mask.ctypes.data, ctypes.byref(fc), res, 0)
    else:
        rc = lib.sfd2_absolute_pose_focal_batch(ctypes.addressof(ctx), (_lib.PoseProblem * 1)(p), 1, ctypes.byref(conf), ctypes.byref(fc), res,
                                                mask.ctypes.data, None, 0)
    return rc, lib.sfd2_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(fc_kw={"num_focal_length_samples": 0}), "num_focal_length_samples"),
    (dict(fc_kw={"num_focal_length_samples": 65}), "num_focal_length_samples"),
    (dict(fc_kw={"min_focal_length_ratio": 0.0}), "ratio"),
    (dict(fc_kw={"min_focal_length_ratio": 2.0, "max_focal_length_ratio": 1.0}), "ratio"),
    (dict(fc_kw={"max_focal_length_ratio": float("inf")}), "ratio"),
    (dict(fc_kw={"min_focal_length_ratio": float("nan")}), "ratio"),
    (dict(fc_kw={"sweep_max_num_trials": 0}), "sweep_max_num_trials"),
    (dict(fc_kw={"reserved": 7}), "reserved"),
    (dict(conf_kw={"confidence": 1.5}), "confidence"),
    (dict(conf_kw={"max_num_trials": 0}), "trial limits"),
    (dict(model=6, params=(1.0,) * 8), "FULL_OPENCV"),
    (dict(params=(500.0, float("nan"), 320.0, 240.0)), "non-finite camera"),
    (dict(params=(500.0, -1.0, 320.0, 240.0)), "positive"),
    (dict(bad_point=True), "non-finite points"),
    (dict(refine=True, fc_kw={"reserved": 1}), "reserved"),
    (dict(refine=True, fc_kw={"max_focal_length_ratio": 0.1}), "ratio"),
    (dict(refine=True, bad_point=True), "non-finite points"),
])
def test_bad_arguments_are_errors_with_a_message(kw, word):
    rc, msg = _call(**kw)
    assert rc == -1 and word in msg, msg
    assert ("sfd2_pose_refine_camera_batch" if kw.get("refine") else "sfd2_absolute_pose_focal_batch") in msg


def test_python_passes_the_old_call_through_unchanged():
    """Without a GPU both forms raise; the signature keeps the old positional order and the new arguments are keyword-only."""
    import inspect
    from sfd2_amd import pose
    sig = inspect.signature(pose.absolute_pose_estimation_batch)
    names = list(sig.parameters)
    assert names[:8] == ["problems", "max_error_px", "min_inlier_ratio", "min_num_trials", "max_num_trials", "confidence", "seed", "device"]
    for k, d in dict(estimate_focal_length=False, refine_focal_length=False, refine_extra_params=False, num_focal_length_samples=30,
                     min_focal_length_ratio=0.2, max_focal_length_ratio=5.0, sweep_max_num_trials=1024, return_sweep=False).items():
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == d
    rsig = inspect.signature(pose.pose_refinement_batch)
    assert rsig.parameters["refine_focal_length"].kind is inspect.Parameter.KEYWORD_ONLY and not rsig.parameters["refine_extra_params"].default
