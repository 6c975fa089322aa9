"""Absolute pose on the device (include/sfd2_hip.h sfd2_absolute_pose_batch / sfd2_pose_refine_batch): the two pycolmap calls of
the localiser, pycolmap.absolute_pose_estimation (it_loc/localize_cv2.py:731, :390) and pycolmap.pose_refinement (:451), with the
reference's call signatures and the dicts it reads (:731-742, :930-964).

Conventions (COLMAP's, it_loc/common.py:225-236): qvec = (w, x, y, z), unit, world to camera, x_cam = R(qvec) X + tvec.  points2D are
pixel coordinates taken as given (the localiser adds its +0.5 itself, :647).  camera is the dict of :684-689 -- model, width, height,
params in COLMAP's order -- for SIMPLE_PINHOLE (f, cx, cy), PINHOLE (fx, fy, cx, cy), SIMPLE_RADIAL (f, cx, cy, k) and OPENCV
(fx, fy, cx, cy, k1, k2, p1, p2).  Inputs and returned poses are fp64.

RANSAC defaults (this project's choice; pycolmap is not available to compare against): min_inlier_ratio 0.01, min_num_trials 1000,
max_num_trials 100000, confidence 0.9999, seed 0.  The result depends on the problem and the seed only.  Nothing here computes on
the CPU: without a GPU the calls raise.

Unknown focal length (sfd2_absolute_pose_focal_batch / sfd2_pose_refine_camera_batch): pycolmap's estimate_focal_length,
refine_focal_length and refine_extra_params as keyword-only arguments.  With all three False the calls above run and their dicts come
back unchanged."""
import ctypes

import numpy as np

try:        # torch's HIP runtime first (see sfd2_amd/jpeg.py)
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    pass

from . import _lib

CAMERA_MODELS = {"SIMPLE_PINHOLE": (0, 3), "PINHOLE": (1, 4), "SIMPLE_RADIAL": (2, 4), "OPENCV": (4, 8)}
DEFAULTS = dict(min_inlier_ratio=0.01, min_num_trials=1000, max_num_trials=100000, confidence=0.9999, seed=0)
FOCAL_DEFAULTS = dict(num_focal_length_samples=30, min_focal_length_ratio=0.2, max_focal_length_ratio=5.0, sweep_max_num_trials=1024)


SWEEP_DTYPE = np.dtype([("cnt", np.int32), ("num_trials", np.int32), ("sum_px", np.float32), ("pad", np.int32)])   # sfd2_pose_sweep_record


def camera_model(camera):
    """(model id, params as float64 [8]) of a camera dict; ValueError naming the model when it is not one of CAMERA_MODELS."""
    model = camera["model"]
    if not isinstance(model, str):
        model = getattr(model, "name", str(model))
    if model not in CAMERA_MODELS:
        raise ValueError(f"camera model {model!r} is not supported (one of {', '.join(CAMERA_MODELS)})")
    mid, n = CAMERA_MODELS[model]
    params = np.asarray(camera["params"], dtype=np.float64).reshape(-1)
    if params.size != n:
        raise ValueError(f"camera model {model} takes {n} parameters, got {params.size}")
    out = np.zeros(8, dtype=np.float64)
    out[:n] = params
    return mid, out


def _problem(points2D, points3D, camera, max_error_px, keep):
    p2 = np.ascontiguousarray(points2D, dtype=np.float64).reshape(-1, 2)
    p3 = np.ascontiguousarray(points3D, dtype=np.float64).reshape(-1, 3)
    if p2.shape[0] != p3.shape[0]:
        raise ValueError(f"{p2.shape[0]} 2D points for {p3.shape[0]} 3D points")
    if not (np.isfinite(p2).all() and np.isfinite(p3).all()):
        raise ValueError("non-finite correspondences")
    mid, params = camera_model(camera)
    keep += [p2, p3]
    pr = _lib.PoseProblem()
    pr.n = p2.shape[0]
    pr.model = mid
    pr.points2D = p2.ctypes.data if p2.size else None
    pr.points3D = p3.ctypes.data if p3.size else None
    for i in range(8):
        pr.params[i] = params[i]
    pr.width = int(camera.get("width", 0))
    pr.height = int(camera.get("height", 0))
    pr.max_error_px = float(max_error_px)
    return pr


def _result(r, mask=None):
    out = {"success": bool(r.success), "qvec": np.array(r.qvec[:], dtype=np.float64), "tvec": np.array(r.tvec[:], dtype=np.float64)}
    if mask is not None:
        out["num_inliers"] = int(r.num_inliers)
        out["inliers"] = mask.astype(bool)
        out["num_trials"] = int(r.num_trials)
    return out


def _focal_conf(estimate_focal_length, refine_focal_length, refine_extra_params, num_focal_length_samples, min_focal_length_ratio,
                max_focal_length_ratio, sweep_max_num_trials):
    fc = _lib.PoseFocalConf()
    fc.estimate_focal_length, fc.refine_focal_length, fc.refine_extra_params = int(bool(estimate_focal_length)), int(bool(refine_focal_length)), \
        int(bool(refine_extra_params))
    fc.num_focal_length_samples = int(num_focal_length_samples)
    fc.min_focal_length_ratio, fc.max_focal_length_ratio = float(min_focal_length_ratio), float(max_focal_length_ratio)
    fc.sweep_max_num_trials = int(sweep_max_num_trials)
    return fc


def _focal_result(r, camera, mask=None):
    """_result, with the camera (a copy of the given dict with the returned params) and the sweep's choice."""
    out = _result(r, mask)
    cam = dict(camera)
    mid = camera_model(camera)[0]
    n = next(cnt for m, cnt in CAMERA_MODELS.values() if m == mid)
    cam["params"] = [float(v) for v in r.params[:n]]
    out["camera"] = cam
    if mask is not None:
        out["focal_sample"] = int(r.focal_sample)
        out["focal_factor"] = float(r.focal_factor)
        out["ransac_num_inliers"] = int(r.ransac_num_inliers)
    return out


def absolute_pose_estimation_batch(problems, max_error_px=12.0, min_inlier_ratio=DEFAULTS["min_inlier_ratio"],
                                   min_num_trials=DEFAULTS["min_num_trials"], max_num_trials=DEFAULTS["max_num_trials"],
                                   confidence=DEFAULTS["confidence"], seed=DEFAULTS["seed"], device=0, *, estimate_focal_length=False,
                                   refine_focal_length=False, refine_extra_params=False,
                                   num_focal_length_samples=FOCAL_DEFAULTS["num_focal_length_samples"],
                                   min_focal_length_ratio=FOCAL_DEFAULTS["min_focal_length_ratio"],
                                   max_focal_length_ratio=FOCAL_DEFAULTS["max_focal_length_ratio"],
                                   sweep_max_num_trials=FOCAL_DEFAULTS["sweep_max_num_trials"], return_sweep=False):
    """problems: a list of (points2D [n,2], points3D [n,3], camera) or (points2D, points3D, camera, max_error_px).  One device call;
    returns one dict per problem, as absolute_pose_estimation does."""
    keep, probs = [], []
    for p in problems:
        thr = p[3] if len(p) > 3 else max_error_px
        probs.append(_problem(p[0], p[1], p[2], thr, keep))
    k = len(probs)
    if k == 0:
        return []
    ctx = _lib.default_context(device)
    arr = (_lib.PoseProblem * k)(*probs)
    conf = _lib.PoseConf(float(min_inlier_ratio), int(min_num_trials), int(max_num_trials), float(confidence), int(seed) & (2 ** 64 - 1))
    if estimate_focal_length or refine_focal_length or refine_extra_params:
        fc = _focal_conf(estimate_focal_length, refine_focal_length, refine_extra_params, num_focal_length_samples, min_focal_length_ratio,
                         max_focal_length_ratio, sweep_max_num_trials)
        res = (_lib.PoseFocalResult * k)()
        total = sum(pr.n for pr in probs)
        mask = np.zeros(max(total, 1), dtype=np.uint8)
        want_sweep = bool(return_sweep and estimate_focal_length)
        ns = max(fc.num_focal_length_samples, 0) + 1
        sweep = np.zeros((k, ns), dtype=SWEEP_DTYPE) if want_sweep else None
        _lib.check(ctx.lib.sfd2_absolute_pose_focal_batch(ctx.h, arr, k, ctypes.byref(conf), ctypes.byref(fc), res, mask.ctypes.data,
                                                          sweep.ctypes.data if want_sweep else None, 0))
        out, o = [], 0
        for i, pr in enumerate(probs):
            out.append(_focal_result(res[i], problems[i][2], mask[o:o + pr.n].copy()))
            if want_sweep:
                out[-1]["sweep"] = sweep[i].copy()
            o += pr.n
        return out
    res = (_lib.PoseResult * k)()
    total = sum(pr.n for pr in probs)
    mask = np.zeros(max(total, 1), dtype=np.uint8)
    _lib.check(ctx.lib.sfd2_absolute_pose_batch(ctx.h, arr, k, ctypes.byref(conf), res, mask.ctypes.data, 0))
    out, o = [], 0
    for i, pr in enumerate(probs):
        out.append(_result(res[i], mask[o:o + pr.n].copy()))
        o += pr.n
    return out


def absolute_pose_estimation(points2D, points3D, camera, max_error_px=12.0, min_inlier_ratio=DEFAULTS["min_inlier_ratio"],
                             min_num_trials=DEFAULTS["min_num_trials"], max_num_trials=DEFAULTS["max_num_trials"],
                             confidence=DEFAULTS["confidence"], seed=DEFAULTS["seed"], device=0, **focal):
    """pycolmap.absolute_pose_estimation(points2D, points3D, camera, max_error_px) (localize_cv2.py:731): LO-RANSAC over P3P, then
    the Cauchy refinement in pixels.  Returns {'success', 'qvec', 'tvec', 'num_inliers', 'inliers' (bool [n]), 'num_trials'};
    num_inliers and inliers are the RANSAC winner's, the pose the refined one.  Fewer than 4 correspondences: success False.
    **focal: absolute_pose_estimation_batch's keyword-only arguments (estimate_focal_length, refine_focal_length, refine_extra_params,
    num_focal_length_samples, min_focal_length_ratio, max_focal_length_ratio, sweep_max_num_trials, return_sweep).  With one of the
    first three the dict adds 'camera' (the given dict with the estimated params), 'focal_sample', 'focal_factor' and
    'ransac_num_inliers' ('sweep' on request: [S + 1] records cnt / num_trials / sum_px); num_inliers and inliers are then those of
    the mask the returned pose and camera were refined over."""
    return absolute_pose_estimation_batch([(points2D, points3D, camera)], max_error_px, min_inlier_ratio, min_num_trials,
                                          max_num_trials, confidence, seed, device, **focal)[0]


def pose_refinement_batch(problems, device=0, *, refine_focal_length=False, refine_extra_params=False,
                          min_focal_length_ratio=FOCAL_DEFAULTS["min_focal_length_ratio"],
                          max_focal_length_ratio=FOCAL_DEFAULTS["max_focal_length_ratio"]):
    """problems: a list of (tvec, qvec, points2D, points3D, inlier_mask, camera).  One device call; a list of pose_refinement's dicts.
    With a refine flag the camera's focal and / or extra parameters are refined with the pose and each dict adds 'camera'."""
    keep, probs, qt, masks = [], [], [], []
    for tvec, qvec, p2, p3, m, cam in problems:
        pr = _problem(p2, p3, cam, 1.0, keep)
        m = np.asarray(m).reshape(-1)
        if m.size != pr.n:
            raise ValueError(f"inlier mask of {m.size} for {pr.n} correspondences")
        probs.append(pr)
        masks.append(m.astype(bool).astype(np.uint8))
        qt.append(np.concatenate([np.asarray(qvec, dtype=np.float64).reshape(4), np.asarray(tvec, dtype=np.float64).reshape(3)]))
    k = len(probs)
    if k == 0:
        return []
    qt = np.ascontiguousarray(qt, dtype=np.float64)
    if not np.isfinite(qt).all():
        raise ValueError("non-finite start pose")
    mask = np.ascontiguousarray(np.concatenate(masks + [np.zeros(1, np.uint8)]))
    ctx = _lib.default_context(device)
    arr = (_lib.PoseProblem * k)(*probs)
    if refine_focal_length or refine_extra_params:
        fc = _focal_conf(False, refine_focal_length, refine_extra_params, FOCAL_DEFAULTS["num_focal_length_samples"], min_focal_length_ratio,
                         max_focal_length_ratio, FOCAL_DEFAULTS["sweep_max_num_trials"])
        fres = (_lib.PoseFocalResult * k)()
        _lib.check(ctx.lib.sfd2_pose_refine_camera_batch(ctx.h, arr, k, qt.ctypes.data, mask.ctypes.data, ctypes.byref(fc), fres, 0))
        return [_focal_result(fres[i], problems[i][5]) for i in range(k)]
    res = (_lib.PoseResult * k)()
    _lib.check(ctx.lib.sfd2_pose_refine_batch(ctx.h, arr, k, qt.ctypes.data, mask.ctypes.data, res, 0))
    return [_result(res[i]) for i in range(k)]


def pose_refinement(tvec, qvec, points2D, points3D, inlier_mask, camera, device=0, **focal):
    """pycolmap.pose_refinement(tvec, qvec, points2D, points3D, inlier_mask, camera) (localize_cv2.py:451): the refinement of
    absolute_pose_estimation alone, started from the given pose, over the correspondences the mask selects (intrinsics fixed).
    Returns {'success', 'qvec', 'tvec'}; with refine_focal_length / refine_extra_params (**focal, see pose_refinement_batch) also
    'camera'."""
    return pose_refinement_batch([(tvec, qvec, points2D, points3D, inlier_mask, camera)], device, **focal)[0]
