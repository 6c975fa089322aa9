"""Relative pose on the device (include/sfd2_hip.h sfd2_relative_pose_batch): the calibrated two-view geometry COLMAP estimates inside
`colmap matches_importer` (hloc/triangulation.py:114, hloc/reconstruction.py:145) -- five-point LO-RANSAC on the squared Sampson error,
a refinement over the inliers and the cheirality choice.  Essential matrix only; a rotation-only pair is reported
through the triangulation angle (`small_baseline`); the homography and the label of a pair are at the end of this file.  That holds
for a rotation with noise on the points; correspondences that are a rotation exactly have no isolated solution and give no result
(no inliers, success False, `small_baseline` False): a caller takes `success`, not `small_baseline` alone, for "this pair has a pose".

Conventions: qvec = (w, x, y, z), camera 0 to camera 1, x1 = R(qvec) x0 + tvec with |tvec| = 1; E = [tvec]x R.  points2D are pixel
coordinates taken as given; a camera is the dict of sfd2_amd.pose (model, params in COLMAP's order).  RANSAC defaults are COLMAP's
two-view ones: max_error 4 px, confidence 0.999, max_num_trials 10000, min_num_trials 0, min_inlier_ratio 0.25, min_num_inliers 15.
The result depends on the pair and the seed only.  Nothing here computes on the CPU: without a GPU the calls raise.

Without cameras: fundamental_matrix(_batch) and verify_pairs_fundamental at the end of this file
estimate the fundamental matrix instead -- seven-point LO-RANSAC on the squared Sampson error in pixels, x1^T F x0 = 0, what COLMAP
runs for a pair without a trusted focal length.  Same RANSAC keywords and defaults; no pose, no angles.

The homography and the decision: homography(_batch) and verify_pairs_homography estimate H with
x1 ~ H x0 in pixels -- closed-form four-point LO-RANSAC on the one-sided squared transfer error in image 1 -- with the same keywords.
decide_two_view_geometry(E, F, H) is a pure host function on three result dicts that labels the pair calibrated, uncalibrated, planar,
panoramic, planar_or_panoramic or degenerate and names the mask to keep, modelled on COLMAP's EstimateCalibrated / EstimateUncalibrated;
two_view_geometry_batch and verify_pairs_geometry make the two (F, H) or three (E too, with cameras) device calls with one threshold
and seed and decide per pair.

Guided matching: guided_matches(_batch) match a pair's descriptors again with only those
candidates allowed whose key points agree with the pair's F or H; guide_of takes (kind, matrix) from any result above (E through
fundamental_from_essential), guided_match_pairs does it for all pairs of a verify_pairs_* call."""
import ctypes

import numpy as np

try:        # torch's HIP runtime first (see sfd2_amd/jpeg.py)
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    pass

from . import _lib
from .pose import camera_model

DEFAULTS = dict(min_inlier_ratio=0.25, min_num_trials=0, max_num_trials=10000, confidence=0.999, seed=0, min_num_inliers=15,
                min_tri_angle=1.5)


def _problem(points2D0, points2D1, camera0, camera1, max_error_px, keep):
    p0 = np.ascontiguousarray(points2D0, dtype=np.float64).reshape(-1, 2)
    p1 = np.ascontiguousarray(points2D1, dtype=np.float64).reshape(-1, 2)
    if p0.shape[0] != p1.shape[0]:
        raise ValueError(f"{p0.shape[0]} points in image 0 for {p1.shape[0]} in image 1")
    if not (np.isfinite(p0).all() and np.isfinite(p1).all()):
        raise ValueError("non-finite correspondences")
    (m0, q0), (m1, q1) = camera_model(camera0), camera_model(camera1)
    keep += [p0, p1]
    pr = _lib.TwoViewProblem()
    pr.n = p0.shape[0]
    pr.model0, pr.model1 = m0, m1
    for i in range(8):
        pr.params0[i] = q0[i]
        pr.params1[i] = q1[i]
    pr.points2D_0 = p0.ctypes.data if p0.size else None
    pr.points2D_1 = p1.ctypes.data if p1.size else None
    pr.max_error_px = float(max_error_px)
    return pr


def relative_pose_batch(problems, max_error_px=4.0, min_inlier_ratio=DEFAULTS["min_inlier_ratio"], min_num_trials=DEFAULTS["min_num_trials"],
                        max_num_trials=DEFAULTS["max_num_trials"], confidence=DEFAULTS["confidence"], seed=DEFAULTS["seed"],
                        min_num_inliers=DEFAULTS["min_num_inliers"], min_tri_angle=DEFAULTS["min_tri_angle"], device=0):
    """problems: a list of (points2D0 [n,2], points2D1 [n,2], camera0, camera1) or (..., max_error_px).  One device call; returns one
    dict per pair, as relative_pose does."""
    keep, probs = [], []
    for p in problems:
        probs.append(_problem(p[0], p[1], p[2], p[3], p[4] if len(p) > 4 else max_error_px, keep))
    k = len(probs)
    if k == 0:
        return []
    ctx = _lib.default_context(device)
    arr = (_lib.TwoViewProblem * k)(*probs)
    conf = _lib.TwoViewConf(float(min_inlier_ratio), int(min_num_trials), int(max_num_trials), float(confidence), int(seed) & (2 ** 64 - 1),
                            int(min_num_inliers), 0)
    res = (_lib.TwoViewResult * k)()
    total = sum(pr.n for pr in probs)
    mask = np.zeros(max(total, 1), dtype=np.uint8)
    angle = np.full(max(total, 1), np.nan, dtype=np.float64)
    _lib.check(ctx.lib.sfd2_relative_pose_batch(ctx.h, arr, k, ctypes.byref(conf), res, mask.ctypes.data, angle.ctypes.data, 0))
    out, o = [], 0
    for i, pr in enumerate(probs):
        r, m, a = res[i], mask[o:o + pr.n].astype(bool), angle[o:o + pr.n].copy()
        o += pr.n
        fin = a[m & np.isfinite(a)]
        med = float(np.median(fin)) if fin.size else float("nan")
        out.append({"success": bool(r.success), "qvec": np.array(r.qvec[:], dtype=np.float64), "tvec": np.array(r.tvec[:], dtype=np.float64),
                    "E": np.array(r.E[:], dtype=np.float64).reshape(3, 3), "num_inliers": int(r.num_inliers), "inliers": m,
                    "num_trials": int(r.num_trials), "tri_angles_deg": a, "tri_angle_deg": med, "small_baseline": bool(med < min_tri_angle)})
    return out


def relative_pose(points2D0, points2D1, camera0, camera1, max_error_px=4.0, **ransac):
    """The relative pose of one matched pair.  Returns {'success', 'qvec', 'tvec', 'E' [3,3], 'num_inliers', 'inliers' (bool [n]),
    'num_trials', 'tri_angle_deg' (the median over the inliers with a finite angle, NaN when there are none), 'tri_angles_deg' [n],
    'small_baseline' (tri_angle_deg < min_tri_angle, default 1.5)}; **ransac: relative_pose_batch's keywords.  Fewer than 5
    correspondences: success False."""
    return relative_pose_batch([(points2D0, points2D1, camera0, camera1)], max_error_px, **ransac)[0]


def verify_pairs_two_view(cameras, images, keypoints, pair_matches, max_error=4.0, min_num_inliers=DEFAULTS["min_num_inliers"], device=0,
                          **ransac):
    """triangulation.verify_pairs without poses: every pair's relative pose is estimated from its matches (the poses in `images` are
    ignored), the RANSAC inliers stay.  pair_matches: [(image id 0, image id 1, matches [m, 2])].  Returns (matches int32 [M, 2] of all
    pairs concatenated with the rejected rows (-1, -1), offsets int64 [n_pairs + 1], counts int32 [n_pairs] = inliers of a pair before
    the min_num_inliers rule, the pairs' relative_pose dicts).  Rows that come in negative stay rejected, a pair of an image with
    itself and a pair below min_num_inliers (or without success) lose all; an index beyond an image's key points raises.  Key points
    are taken as float32 plus COLMAP's +0.5, as verify_pairs takes them."""
    kps = {}
    problems, rows_of, ms = [], [], []
    off = np.zeros(len(pair_matches) + 1, dtype=np.int64)
    for p, (i0, i1, m) in enumerate(pair_matches):
        m = np.asarray(m).reshape(-1, 2).astype(np.int32)
        ms.append(m)
        off[p + 1] = off[p] + len(m)
        for i in (i0, i1):
            if i not in kps:
                kps[i] = np.asarray(keypoints[i], dtype=np.float32).reshape(-1, 2).astype(np.float64) + 0.5
        live = np.flatnonzero((m[:, 0] >= 0) & (m[:, 1] >= 0))
        for col, i in ((0, i0), (1, i1)):
            if live.size and m[live, col].max() >= len(kps[i]):
                raise ValueError(f"pair {p}: match index {int(m[live, col].max())} beyond the {len(kps[i])} key points of image {i}")
        if i0 == i1:
            live = live[:0]
        rows_of.append(live)
        problems.append((kps[i0][m[live, 0]], kps[i1][m[live, 1]], cameras[images[i0].camera_id], cameras[images[i1].camera_id]))
    results = relative_pose_batch(problems, max_error, min_num_inliers=min_num_inliers, device=device, **ransac)
    out = np.full((int(off[-1]), 2), -1, dtype=np.int32)
    counts = np.zeros(len(pair_matches), dtype=np.int32)
    for p, (live, r) in enumerate(zip(rows_of, results)):
        counts[p] = r["num_inliers"]
        if r["success"] and r["num_inliers"] >= min_num_inliers:
            keep = live[r["inliers"]]
            out[off[p] + keep] = ms[p][keep]
    return out, off, counts, results


# ------------------------------------------------------------------------------------------------ without cameras
def _fundamental_problem(points2D0, points2D1, max_error_px, keep, struct=None):
    """A sfd2_fundamental_problem, or with struct = _lib.HomographyProblem a sfd2_homography_problem (the same fields)."""
    p0 = np.ascontiguousarray(points2D0, dtype=np.float64).reshape(-1, 2)
    p1 = np.ascontiguousarray(points2D1, dtype=np.float64).reshape(-1, 2)
    if p0.shape[0] != p1.shape[0]:
        raise ValueError(f"{p0.shape[0]} points in image 0 for {p1.shape[0]} in image 1")
    if not (np.isfinite(p0).all() and np.isfinite(p1).all()):
        raise ValueError("non-finite correspondences")
    keep += [p0, p1]
    pr = (struct or _lib.FundamentalProblem)()
    pr.n = p0.shape[0]
    pr.points2D_0 = p0.ctypes.data if p0.size else None
    pr.points2D_1 = p1.ctypes.data if p1.size else None
    pr.max_error_px = float(max_error_px)
    return pr


def _camera_less_batch(entry, Problem, Result, key, problems, max_error_px, min_inlier_ratio, min_num_trials, max_num_trials, confidence, seed,
                       min_num_inliers, device):
    """One call of the library's `entry` (sfd2_fundamental_batch or sfd2_homography_batch: the same arguments) on (points2D0, points2D1) or
    (..., max_error_px) problems; the matrix goes under `key`."""
    keep, probs = [], []
    for p in problems:
        probs.append(_fundamental_problem(p[0], p[1], p[2] if len(p) > 2 else max_error_px, keep, Problem))
    k = len(probs)
    if k == 0:
        return []
    ctx = _lib.default_context(device)
    arr = (Problem * k)(*probs)
    conf = _lib.TwoViewConf(float(min_inlier_ratio), int(min_num_trials), int(max_num_trials), float(confidence), int(seed) & (2 ** 64 - 1),
                            int(min_num_inliers), 0)
    res = (Result * k)()
    total = sum(pr.n for pr in probs)
    mask = np.zeros(max(total, 1), dtype=np.uint8)
    _lib.check(getattr(ctx.lib, entry)(ctx.h, arr, k, ctypes.byref(conf), res, mask.ctypes.data, 0))
    out, o = [], 0
    for i, pr in enumerate(probs):
        r, m = res[i], mask[o:o + pr.n].astype(bool)
        o += pr.n
        out.append({"success": bool(r.success), key: np.array(getattr(r, key)[:], dtype=np.float64).reshape(3, 3), "num_inliers": int(r.num_inliers),
                    "inliers": m, "num_trials": int(r.num_trials)})
    return out


def fundamental_matrix_batch(problems, max_error_px=4.0, min_inlier_ratio=DEFAULTS["min_inlier_ratio"], min_num_trials=DEFAULTS["min_num_trials"],
                             max_num_trials=DEFAULTS["max_num_trials"], confidence=DEFAULTS["confidence"], seed=DEFAULTS["seed"],
                             min_num_inliers=DEFAULTS["min_num_inliers"], device=0):
    """problems: a list of (points2D0 [n,2], points2D1 [n,2]) or (..., max_error_px).  One device call (sfd2_fundamental_batch: seven-point
    LO-RANSAC, no camera); returns one dict per pair, as fundamental_matrix does."""
    return _camera_less_batch("sfd2_fundamental_batch", _lib.FundamentalProblem, _lib.FundamentalResult, "F", problems, max_error_px,
                              min_inlier_ratio, min_num_trials, max_num_trials, confidence, seed, min_num_inliers, device)


def fundamental_matrix(points2D0, points2D1, max_error_px=4.0, **ransac):
    """The fundamental matrix of one matched pair, no camera needed.  Returns {'success', 'F' [3,3] (x1^T F x0 = 0 in pixels, rank 2,
    unit Frobenius norm), 'num_inliers', 'inliers' (bool [n]), 'num_trials'}; **ransac: fundamental_matrix_batch's keywords.  Fewer
    than 7 correspondences: success False, F = 0."""
    return fundamental_matrix_batch([(points2D0, points2D1)], max_error_px, **ransac)[0]


def verify_pairs_fundamental(keypoints, pair_matches, max_error=4.0, min_num_inliers=DEFAULTS["min_num_inliers"], device=0, **ransac):
    """verify_pairs_two_view without cameras: every pair's fundamental matrix is estimated from its matches, the RANSAC inliers stay.
    The return shape and the rules are verify_pairs_two_view's (the results are fundamental_matrix dicts): rows that come in negative
    stay rejected, a pair of an image with itself and a pair below min_num_inliers lose all; an index beyond an image's key points
    raises.  Key points are taken as float32 plus COLMAP's +0.5."""
    problems, rows_of, ms, off = _pair_problems(keypoints, pair_matches)
    results = fundamental_matrix_batch(problems, max_error, min_num_inliers=min_num_inliers, device=device, **ransac)
    out, counts = _keep_rows(rows_of, ms, off, results,
                             lambda r: r["inliers"] if r["success"] and r["num_inliers"] >= min_num_inliers else None)
    return out, off, counts, results


# ------------------------------------------------------------------------------------------------ homography
def homography_batch(problems, max_error_px=4.0, min_inlier_ratio=DEFAULTS["min_inlier_ratio"], min_num_trials=DEFAULTS["min_num_trials"],
                     max_num_trials=DEFAULTS["max_num_trials"], confidence=DEFAULTS["confidence"], seed=DEFAULTS["seed"],
                     min_num_inliers=DEFAULTS["min_num_inliers"], device=0):
    """problems: a list of (points2D0 [n,2], points2D1 [n,2]) or (..., max_error_px).  One device call (sfd2_homography_batch: four-point
    LO-RANSAC, no camera); returns one dict per pair, as homography does."""
    return _camera_less_batch("sfd2_homography_batch", _lib.HomographyProblem, _lib.HomographyResult, "H", problems, max_error_px,
                              min_inlier_ratio, min_num_trials, max_num_trials, confidence, seed, min_num_inliers, device)


def homography(points2D0, points2D1, max_error_px=4.0, **ransac):
    """The homography of one matched pair, no camera needed.  Returns {'success', 'H' [3,3] (x1 ~ H x0 in pixels, unit Frobenius norm),
    'num_inliers', 'inliers' (bool [n]), 'num_trials'}; **ransac: homography_batch's keywords.  Fewer than 4 correspondences: success
    False, H = 0."""
    return homography_batch([(points2D0, points2D1)], max_error_px, **ransac)[0]


def _pair_problems(keypoints, pair_matches):
    """What the camera-less verify_pairs_* functions share: (problems [(p0, p1)] of the live rows, those rows per pair, the pairs' matches
    as int32, offsets), by the rules in verify_pairs_fundamental's text."""
    kps = {}
    problems, rows_of, ms = [], [], []
    off = np.zeros(len(pair_matches) + 1, dtype=np.int64)
    for p, (i0, i1, m) in enumerate(pair_matches):
        m = np.asarray(m).reshape(-1, 2).astype(np.int32)
        ms.append(m)
        off[p + 1] = off[p] + len(m)
        for i in (i0, i1):
            if i not in kps:
                kps[i] = np.asarray(keypoints[i], dtype=np.float32).reshape(-1, 2).astype(np.float64) + 0.5
        live = np.flatnonzero((m[:, 0] >= 0) & (m[:, 1] >= 0))
        for col, i in ((0, i0), (1, i1)):
            if live.size and m[live, col].max() >= len(kps[i]):
                raise ValueError(f"pair {p}: match index {int(m[live, col].max())} beyond the {len(kps[i])} key points of image {i}")
        if i0 == i1:
            live = live[:0]
        rows_of.append(live)
        problems.append((kps[i0][m[live, 0]], kps[i1][m[live, 1]]))
    return problems, rows_of, ms, off


def _keep_rows(rows_of, ms, off, results, kept):
    """(matches with the rejected rows (-1, -1), counts): kept(r) is the mask over a pair's live rows that stays, or None."""
    out = np.full((int(off[-1]), 2), -1, dtype=np.int32)
    counts = np.zeros(len(ms), dtype=np.int32)
    for p, (live, r) in enumerate(zip(rows_of, results)):
        counts[p] = r["num_inliers"]
        m = kept(r)
        if m is not None:
            keep = live[m]
            out[off[p] + keep] = ms[p][keep]
    return out, counts


def verify_pairs_homography(keypoints, pair_matches, max_error=4.0, min_num_inliers=DEFAULTS["min_num_inliers"], device=0, **ransac):
    """verify_pairs_fundamental with the homography: every pair's H is estimated from its matches, the RANSAC inliers stay.  The return
    shape and the rules are verify_pairs_fundamental's (the results are homography dicts)."""
    problems, rows_of, ms, off = _pair_problems(keypoints, pair_matches)
    results = homography_batch(problems, max_error, min_num_inliers=min_num_inliers, device=device, **ransac)
    out, counts = _keep_rows(rows_of, ms, off, results,
                             lambda r: r["inliers"] if r["success"] and r["num_inliers"] >= min_num_inliers else None)
    return out, off, counts, results


# ------------------------------------------------------------------------------------------------ the decision between E, F and H
CONFIGS = ("calibrated", "uncalibrated", "planar", "panoramic", "planar_or_panoramic", "degenerate")
NO_INITIAL_PAIR = ("panoramic", "planar_or_panoramic", "degenerate")      # configs without a baseline a reconstruction can start from


def decide_two_view_geometry(E, F, H, min_num_inliers=DEFAULTS["min_num_inliers"], min_E_F_inlier_ratio=0.95, max_H_inlier_ratio=0.8):
    """The project's rule between the three models of one pair, modelled on COLMAP's EstimateCalibrated / EstimateUncalibrated; a pure
    host function on the result dicts of relative_pose (E, or None without cameras), fundamental_matrix (F) and homography (H).
    Returns {'config' (one of CONFIGS), 'inliers' (bool [n]), 'num_inliers', 'model' ('E', 'F', 'H' or None: whose mask it is)}.

    nX is the model's num_inliers when at least min_num_inliers, else 0; E's call must also have succeeded.
    1. nE > 0 and nE >= min_E_F_inlier_ratio nF: the mask is E's when nE >= nF, else F's; with nH > max_H_inlier_ratio nE the config is
       'panoramic' when E's small_baseline is set, else 'planar', and the mask becomes H's when nH exceeds the mask's count; otherwise
       'calibrated'.
    2. else nF > 0: with nH > max_H_inlier_ratio nF 'planar_or_panoramic' (H's mask when larger), otherwise 'uncalibrated'.
    3. else nH > 0: 'planar_or_panoramic' with H's mask.
    4. else 'degenerate' with an empty mask."""
    def count(r, need_success):
        if r is None or (need_success and not r["success"]):
            return 0
        return int(r["num_inliers"]) if int(r["num_inliers"]) >= min_num_inliers else 0
    nE, nF, nH = count(E, True), count(F, False), count(H, False)
    n = len((H if H is not None else F)["inliers"])

    def out(config, model, r):
        m = np.zeros(n, dtype=bool) if r is None else np.asarray(r["inliers"], dtype=bool).copy()
        return {"config": config, "inliers": m, "num_inliers": int(m.sum()), "model": model}

    def larger(model, r, count_):
        return ("H", H) if nH > count_ else (model, r)
    if nE > 0 and nE >= min_E_F_inlier_ratio * nF:
        model, r, c = ("E", E, nE) if nE >= nF else ("F", F, nF)
        if nH > max_H_inlier_ratio * nE:
            return out("panoramic" if E["small_baseline"] else "planar", *larger(model, r, c))
        return out("calibrated", model, r)
    if nF > 0:
        if nH > max_H_inlier_ratio * nF:
            return out("planar_or_panoramic", *larger("F", F, nF))
        return out("uncalibrated", "F", F)
    if nH > 0:
        return out("planar_or_panoramic", "H", H)
    return out("degenerate", None, None)


def two_view_geometry_batch(problems, cameras=None, max_error_px=4.0, min_num_inliers=DEFAULTS["min_num_inliers"], min_E_F_inlier_ratio=0.95,
                            max_H_inlier_ratio=0.8, device=0, **ransac):
    """problems: a list of (points2D0 [n,2], points2D1 [n,2]); cameras: None, or one (camera0, camera1) per problem.  Two device calls
    (F and H) or three (E too, with cameras), each with the same threshold and seed, then decide_two_view_geometry per pair.  Returns
    one decision dict per pair, with the three models' result dicts under 'E' (None without cameras), 'F' and 'H'."""
    problems = [(p[0], p[1]) for p in problems]
    if cameras is not None and len(cameras) != len(problems):
        raise ValueError(f"{len(cameras)} camera pairs for {len(problems)} problems")
    kw = dict(min_num_inliers=min_num_inliers, device=device, **ransac)
    Es = [None] * len(problems)
    if cameras is not None:
        Es = relative_pose_batch([(p0, p1, c0, c1) for (p0, p1), (c0, c1) in zip(problems, cameras)], max_error_px, **kw)
    kw.pop("min_tri_angle", None)
    Fs = fundamental_matrix_batch(problems, max_error_px, **kw)
    Hs = homography_batch(problems, max_error_px, **kw)
    out = []
    for E, F, H in zip(Es, Fs, Hs):
        d = decide_two_view_geometry(E, F, H, min_num_inliers, min_E_F_inlier_ratio, max_H_inlier_ratio)
        d.update(E=E, F=F, H=H)
        out.append(d)
    return out


def verify_pairs_geometry(keypoints, pair_matches, cameras=None, images=None, max_error=4.0, min_num_inliers=DEFAULTS["min_num_inliers"],
                          min_E_F_inlier_ratio=0.95, max_H_inlier_ratio=0.8, device=0, **ransac):
    """verify_pairs_fundamental with the decision: E (with cameras and images, as verify_pairs_two_view takes them), F and H are estimated
    for every pair and decide_two_view_geometry's mask stays.  The return shape is verify_pairs_fundamental's; the results are
    two_view_geometry_batch's decision dicts and counts are the kept masks' sizes (0 for 'degenerate')."""
    if (cameras is None) != (images is None):
        raise ValueError("cameras and images go together")
    problems, rows_of, ms, off = _pair_problems(keypoints, pair_matches)
    cams = None
    if cameras is not None:
        cams = [(cameras[images[i0].camera_id], cameras[images[i1].camera_id]) for i0, i1, _ in pair_matches]
    results = two_view_geometry_batch(problems, cams, max_error, min_num_inliers, min_E_F_inlier_ratio, max_H_inlier_ratio, device, **ransac)
    out, counts = _keep_rows(rows_of, ms, off, results, lambda r: r["inliers"] if r["config"] != "degenerate" else None)
    return out, off, counts, results


# ------------------------------------------------------------------------------------------------ guided matching
GUIDED_CONF = {"ratio_threshold": None, "distance_threshold": None, "do_mutual_check": True}      # match_features.confs["NNM"]'s rule


def fundamental_from_essential(E, camera0, camera1):
    """F = K1^-T E K0^-1 in pixels (x1^T F x0 = 0), unit Frobenius norm, from the cameras' focal lengths and principal points ONLY:
    distortion is ignored, so for a SIMPLE_RADIAL or OPENCV camera the epipolar lines are those of the undistorted image and a guide
    made from F is off by the distortion at the key point."""
    def K_inv(camera):
        model, q = camera_model(camera)
        fx, fy, cx, cy = (q[0], q[0], q[1], q[2]) if model in (0, 2) else (q[0], q[1], q[2], q[3])
        return np.array([[1.0 / fx, 0.0, -cx / fx], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]])
    F = K_inv(camera1).T @ np.asarray(E, dtype=np.float64).reshape(3, 3) @ K_inv(camera0)
    n = np.linalg.norm(F)
    return F / n if n > 0 else F


def guide_of(result, camera0=None, camera1=None):
    """(kind, matrix) of the model whose mask a result kept, kind 'F' or 'H', or None where there is nothing to guide by (no success,
    a 'degenerate' decision).  result: a relative_pose dict (E -> F through fundamental_from_essential, which needs the two cameras), a
    fundamental_matrix dict, a homography dict, or a decision dict of two_view_geometry_batch (the model its 'model' key names)."""
    if "config" in result:
        if result["config"] == "degenerate" or result["model"] is None:
            return None
        return guide_of(result[result["model"]], camera0, camera1)
    if not result["success"]:
        return None
    if "E" in result:
        if camera0 is None or camera1 is None:
            raise ValueError("an essential matrix guides through F: the two cameras are needed")
        return "F", fundamental_from_essential(result["E"], camera0, camera1)
    if "F" in result:
        return "F", np.asarray(result["F"], dtype=np.float64).reshape(3, 3)
    if "H" in result:
        return "H", np.asarray(result["H"], dtype=np.float64).reshape(3, 3)
    raise ValueError("not a two-view result: none of the keys 'E', 'F', 'H', 'config'")


def _match_conf(conf):
    conf = dict(GUIDED_CONF, **(conf.get("model", conf) if conf else {}))
    unknown = set(conf) - set(GUIDED_CONF) - {"name", "sim_mode"}
    if unknown:
        raise ValueError(f"unknown matcher options {sorted(unknown)}")
    if conf.get("sim_mode", "f16") != "f16":
        raise ValueError("guided matching supports sim_mode 'f16' only")
    return _lib.MatchConf(_lib.MATCH_HLOC, int(bool(conf["do_mutual_check"])), float(conf["ratio_threshold"] or 0.0),
                          float(conf["distance_threshold"] or 0.0), _lib.SIM_F16)


def guided_matches_batch(problems, max_error_px=4.0, conf=None, device=0):
    """problems: a list of (desc0 [n0,128], desc1 [n1,128], kp0 [n0,2], kp1 [n1,2], kind 'F' | 'H', matrix [3,3]) or (..., max_error_px).
    One device call (sfd2_match_guided_batch): every pair's descriptors are matched again with only those candidates allowed whose key
    points agree with the model within max_error_px -- F: the Sampson error, x1^T F x0 = 0; H: the transfer error in image 1, x1 ~ H x0
    -- under the NearestNeighbor rule of `conf` (a match_features.confs entry, its 'model' dict, or None = mutual nearest neighbours:
    ratio_threshold, distance_threshold, do_mutual_check).  Key points and matrix must share one pixel frame.  Returns one
    (matches0 int64 [n0], scores0 float32 [n0]) per pair; a row without an allowed candidate gets -1 and score 0."""
    mc = _match_conf(conf)
    keep, probs = [], []
    for i, p in enumerate(problems):
        d0 = np.ascontiguousarray(p[0], dtype=np.float32)
        d1 = np.ascontiguousarray(p[1], dtype=np.float32)
        k0 = np.ascontiguousarray(p[2], dtype=np.float32).reshape(-1, 2)
        k1 = np.ascontiguousarray(p[3], dtype=np.float32).reshape(-1, 2)
        if d0.ndim != 2 or d1.ndim != 2 or d0.shape[1] != 128 or d1.shape[1] != 128:
            raise ValueError(f"pair {i}: descriptors must be [n, 128], got {d0.shape} and {d1.shape}")
        if len(k0) != len(d0) or len(k1) != len(d1):
            raise ValueError(f"pair {i}: {len(k0)} and {len(k1)} key points for {len(d0)} and {len(d1)} descriptors")
        if p[4] not in ("F", "H"):
            raise ValueError(f"pair {i}: unknown guide kind {p[4]!r} (one of 'F', 'H')")
        M = np.ascontiguousarray(p[5], dtype=np.float64).reshape(-1)
        if M.size != 9:
            raise ValueError(f"pair {i}: the guide matrix must be 3 x 3")
        if not (np.isfinite(k0).all() and np.isfinite(k1).all() and np.isfinite(M).all()):
            raise ValueError(f"pair {i}: non-finite key points or matrix")
        err = float(p[6] if len(p) > 6 else max_error_px)
        if not (np.isfinite(err) and err > 0):
            raise ValueError(f"pair {i}: max_error_px must be positive")
        keep += [d0, d1, k0, k1]
        pr = _lib.GuidedProblem()
        for s, d in ((pr.d0, d0), (pr.d1, d1)):
            s.data, s.n, s.dtype, s.layout, s.on_device, s.rows, s.n_rows = (d.ctypes.data if d.size else None), len(d), _lib.DT_F32, _lib.LAYOUT_ND, 0, None, 0
        pr.xy0, pr.xy1 = (k0.ctypes.data if k0.size else None), (k1.ctypes.data if k1.size else None)
        pr.model = _lib.GUIDE_F if p[4] == "F" else _lib.GUIDE_H
        for j in range(9):
            pr.M[j] = M[j]
        pr.max_error_px = err
        probs.append(pr)
    k = len(probs)
    if k == 0:
        return []
    ctx = _lib.default_context(device)
    total = sum(pr.d0.n for pr in probs)
    m = np.full(max(total, 1), -1, dtype=np.int64)
    s = np.zeros(max(total, 1), dtype=np.float32)
    _lib.check(ctx.lib.sfd2_match_guided_batch(ctx.h, (_lib.GuidedProblem * k)(*probs), k, 128, ctypes.byref(mc), m.ctypes.data, s.ctypes.data, 0))
    out, o = [], 0
    for pr in probs:
        out.append((m[o:o + pr.d0.n].copy(), s[o:o + pr.d0.n].copy()))
        o += pr.d0.n
    return out


def guided_matches(desc0, desc1, kp0, kp1, kind, matrix, max_error_px=4.0, conf=None, device=0):
    """One pair of guided_matches_batch: (matches0 int64 [n0], scores0 float32 [n0])."""
    return guided_matches_batch([(desc0, desc1, kp0, kp1, kind, matrix)], max_error_px, conf, device)[0]


def _guide_for_stored(kind, M):
    """The guide of a model estimated on key points + 0.5 (verify_pairs_*), for the key points as stored: with T the shift by +0.5,
    F' = T^T F T and H' = T^-1 H T, exact in fp64 up to rounding -- the stored float32 coordinates stay as they are."""
    T = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])
    return T.T @ M @ T if kind == "F" else np.linalg.inv(T) @ M @ T


def guided_match_pairs(keypoints, descriptors, pair_matches, results, max_error=4.0, conf=None, cameras=None, images=None, device=0):
    """The step after verify_pairs_*: every pair is matched again under the model its verification kept.  keypoints / descriptors: image
    id -> [n,2] as stored / [n,128]; pair_matches: [(image id 0, image id 1, matches [m,2])] as verify_pairs_* took them (only the
    image ids and, for the shape of the output, m are used); results: the dicts verify_pairs_* returned; cameras and images: as
    verify_pairs_two_view takes them, needed where a result's guide is an essential matrix.  Returns (matches int32 [M,2], offsets int64
    [n_pairs + 1], counts int32 [n_pairs], scores float32 [M]) in verify_pairs_*'s shape with m = the key points of image 0: row r of a
    pair is (r, its guided match) or (-1, -1), counts the matched rows.  A pair whose result failed or is 'degenerate', and a pair of an
    image with itself, keeps all -1."""
    if len(results) != len(pair_matches):
        raise ValueError(f"{len(results)} results for {len(pair_matches)} pairs")
    off = np.zeros(len(pair_matches) + 1, dtype=np.int64)
    problems, where = [], []
    for p, ((i0, i1, _), r) in enumerate(zip(pair_matches, results)):
        n0 = len(np.asarray(keypoints[i0]).reshape(-1, 2))
        off[p + 1] = off[p] + n0
        cams = (cameras[images[i0].camera_id], cameras[images[i1].camera_id]) if cameras is not None else (None, None)
        g = None if i0 == i1 else guide_of(r, *cams)
        if g is None:
            continue
        where.append(p)
        problems.append((descriptors[i0], descriptors[i1], keypoints[i0], keypoints[i1], g[0], _guide_for_stored(*g)))
    out = np.full((int(off[-1]), 2), -1, dtype=np.int32)
    scores = np.zeros(int(off[-1]), dtype=np.float32)
    counts = np.zeros(len(pair_matches), dtype=np.int32)
    for p, (m, s) in zip(where, guided_matches_batch(problems, max_error, conf, device)):
        rows = np.flatnonzero(m >= 0)
        out[off[p] + rows, 0] = rows
        out[off[p] + rows, 1] = m[rows]
        scores[off[p]:off[p + 1]] = s
        counts[p] = len(rows)
    return out, off, counts, scores
