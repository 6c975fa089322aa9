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
and seed and decide per pair."""
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
