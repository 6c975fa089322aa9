"""Reconstruction without poses: hloc/reconstruction.py (`colmap mapper`) on the device.  From a feature store and a match store to
sfm_dir/models/0/{cameras,images,points3D}.bin, the map sfd2_amd.covis.MapIndex, sfd2_amd.localize, sfd2_amd.bundle_adjustment and
sfd2_amd.pairs_from_covisibility read.  A round-based incremental mapper: the tracks are built once from the
verified matches; the points are a function of the registered views and their poses, rebuilt every round.

  two_view         two_view.verify_pairs_two_view: the matches verified without poses, every pair's relative pose.
  build_tracks     triangulation.build_tracks: connected components of the verified matches.
  a round          restrict_tracks (sfd2_mapper_restrict)  the tracks seen by two registered views
                   triangulation.triangulate               their points at the current poses
                   bundle_adjustment.adjust                poses and points together, the gauge held by the initial pair (below)
                   filter_points (sfd2_mapper_filter)      reprojection error, depth and triangulation angle
                   visible_counts (sfd2_mapper_visible)    what every unregistered view sees of the live points
                   assemble_problems (sfd2_mapper_assemble) the 2D-3D problems of the round's candidates
                   pose.absolute_pose_estimation_batch     their poses

  python -m sfd2_amd.reconstruction --sfm_dir S --image_dir D --pairs P --features F --matches M
         [--reference_sfm_model R | --intrinsics LIST...] [--single_camera] [--skip_geometric_verification]
         [--min_match_score X] [--min_num_matches N] [--verification essential|fundamental|geometry]
         [--refine_focal_length 0|1] [--refine_principal_point 0|1] [--refine_extra_params 0|1] [--intrinsics_min_views N]
         [--abs_pose_estimate_focal_length 0|1]
         [--ba_solver pcg|dense]

The refine options (default off) let every round's adjustment, from intrinsics_min_views registered views on, refine the cameras'
intrinsics with the poses and points (bundle_adjustment.adjust_cameras): the next round triangulates, filters and
registers with the refined cameras, and the written model carries them.  --ba_solver dense (option ba_solver, default "pcg") runs every
adjustment with the dense solver of the reduced camera system (bundle_adjustment.adjust(solver="dense")); it holds
the intrinsics constant, so together with a refine option it is refused.

--verification fundamental (reconstruct(..., verification="fundamental")): for cameras nobody trusts, i.e. the focal-length prior.  Step 1
verifies every pair by its fundamental matrix (two_view.verify_pairs_fundamental) and continues as
--skip_geometric_verification does on the verified matches; the init_max_pairs pairs with the most survivors get a relative pose.
--verification geometry verifies every pair by E, F and H and keeps the matches of the decision between them (two_view.verify_pairs_geometry,
DESIGN.md section 17): a planar or rotation-only pair keeps its matches, and a pair labelled panoramic, planar_or_panoramic or
degenerate is not taken as the initial pair.

Deviations from COLMAP: one model; intrinsics are refined only on request (without the refine options a map built from the focal-length
prior is only as good as that prior); the gauge is held by whole views: the first image of the initial pair is constant in every
adjustment, the second only until a third image is registered (option fix_initial_pair keeps it constant throughout), after which the
scale is left to the damping; no local bundle adjustment, no track merging or re-triangulation beyond the per-round triangulation; no
database.db, no EXIF.  The host takes the decisions on arrays of
length n_views or n_pairs and regroups index arrays; nothing here computes geometry on the CPU: without a GPU the stages raise."""
import argparse
import ctypes
import logging
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

try:        # torch's HIP runtime first (see sfd2_amd/jpeg.py)
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    pass

from . import _lib, bundle_adjustment, colmap_io, feature_io, geometric_verification, pose, triangulation, two_view
from .pose import camera_model

INTRINSICS_MIN_VIEWS = 4              # registered views from which a round's adjustment refines the intrinsics
DEFAULTS = dict(max_error=4.0, min_num_matches=15, init_max_pairs=50, init_min_tri_angle=16.0, min_tri_angle=1.5, create_max_angle_error=2.0,
                max_reproj_error=4.0, ba_round_iterations=25, ba_final_iterations=100, ba_loss_scale=1.0, max_reg_trials=3,
                abs_pose_min_num_inliers=30, abs_pose_min_inlier_ratio=0.25, abs_pose_max_error=12.0, round_ratio=0.5, max_images_per_round=16,
                seed=0, max_refine_iterations=50, max_rounds=64, fix_initial_pair=False, refine_focal_length=False, refine_principal_point=False,
                refine_extra_params=False, intrinsics_min_views=INTRINSICS_MIN_VIEWS, ba_solver="pcg", abs_pose_estimate_focal_length=False)
STAT_KEYS = triangulation.STAT_KEYS + ("num_input_images",)


# ---------------------------------------------------------------------------------------------------------------- the four new calls
def restrict_tracks(track_offsets, obs_view, obs_xy, registered, flags=0, device=0):
    """The tracks with observations in at least two distinct registered views, in track order, each with its registered observations in
    observation order.  Returns {'sub_track' int32 [T'], 'sub_offsets' int64 [T' + 1], 'sub_obs' int32 [O'] (source observation),
    'sub_view' int32 [O'], 'sub_xy' float32 [O', 2]}."""
    off = np.ascontiguousarray(track_offsets, dtype=np.int64).reshape(-1)
    ov = np.ascontiguousarray(obs_view, dtype=np.int32).reshape(-1)
    xy = np.ascontiguousarray(np.asarray(obs_xy, dtype=np.float32).reshape(-1, 2))
    reg = np.ascontiguousarray(np.asarray(registered).reshape(-1) != 0, dtype=np.uint8)
    T = len(off) - 1
    if T < 0 or len(ov) != len(xy) or (T > 0 and off[-1] != len(ov)) or (T == 0 and len(ov)):
        raise ValueError("track_offsets and the observation arrays do not fit together")
    st, so = np.zeros(max(T, 1), np.int32), np.zeros(T + 1, np.int64)
    sb, sv, sx = np.zeros(max(len(ov), 1), np.int32), np.zeros(max(len(ov), 1), np.int32), np.zeros((max(len(ov), 1), 2), np.float32)
    nt, no = ctypes.c_int64(0), ctypes.c_int64(0)
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_mapper_restrict(ctx.h, off.ctypes.data, T, ov.ctypes.data, xy.ctypes.data, reg.ctypes.data, len(reg), st.ctypes.data,
                                            so.ctypes.data, sb.ctypes.data, sv.ctypes.data, sx.ctypes.data, ctypes.byref(nt), ctypes.byref(no), int(flags)))
    return {"sub_track": st[:nt.value].copy(), "sub_offsets": so[:nt.value + 1].copy(), "sub_obs": sb[:no.value].copy(),
            "sub_view": sv[:no.value].copy(), "sub_xy": sx[:no.value].copy()}


def filter_points(views, n_views, xyz, point_offsets, obs_view, obs_xy, max_reproj_error=DEFAULTS["max_reproj_error"],
                  min_tri_angle=DEFAULTS["min_tri_angle"], flags=0, device=0):
    """views: triangulation.make_views()'s array; point p holds the observations point_offsets[p] .. point_offsets[p + 1] of (obs_view,
    obs_xy in pixels as bundle_adjustment.adjust takes them).  Returns {'obs_keep' bool [N], 'point_live' bool [P], 'point_error' [P],
    'point_angle' [P] (degrees, NaN below two kept observations)}."""
    pts = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    off = np.ascontiguousarray(point_offsets, dtype=np.int64).reshape(-1)
    ov = np.ascontiguousarray(obs_view, dtype=np.int32).reshape(-1)
    xy = np.ascontiguousarray(np.asarray(obs_xy, dtype=np.float64).reshape(-1, 2))
    P = len(pts)
    if len(off) != P + 1 or len(ov) != len(xy) or off[-1] != len(ov):
        raise ValueError("the point, offset and observation arrays do not fit together")
    keep, live = np.zeros(max(len(ov), 1), np.uint8), np.zeros(max(P, 1), np.uint8)
    err, ang = np.zeros(max(P, 1)), np.zeros(max(P, 1))
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_mapper_filter(ctx.h, views, int(n_views), pts.ctypes.data, P, off.ctypes.data, ov.ctypes.data, xy.ctypes.data,
                                          float(max_reproj_error), float(min_tri_angle), keep.ctypes.data, live.ctypes.data, err.ctypes.data,
                                          ang.ctypes.data, int(flags)))
    return {"obs_keep": keep[:len(ov)].astype(bool), "point_live": live[:P].astype(bool), "point_error": err[:P], "point_angle": ang[:P]}


def _tables(track_offsets, obs_view, point_track, point_live):
    off = np.ascontiguousarray(track_offsets, dtype=np.int64).reshape(-1)
    ov = np.ascontiguousarray(obs_view, dtype=np.int32).reshape(-1)
    pt = np.ascontiguousarray(point_track, dtype=np.int32).reshape(-1)
    pl = np.ascontiguousarray(np.asarray(point_live).reshape(-1) != 0, dtype=np.uint8)
    if len(off) < 1 or len(pt) != len(pl) or (len(off) > 1 and off[-1] != len(ov)) or (len(off) == 1 and len(ov)):
        raise ValueError("the track table and the point arrays do not fit together")
    return off, ov, pt, pl


def visible_counts(track_offsets, obs_view, registered, point_track, point_live, device=0):
    """counts int64 [n_views]: per unregistered view the sum, over its observations, of the live points of the observation's track; 0
    for a registered view.  point_track [P]: the track of every point, ascending."""
    off, ov, pt, pl = _tables(track_offsets, obs_view, point_track, point_live)
    reg = np.ascontiguousarray(np.asarray(registered).reshape(-1) != 0, dtype=np.uint8)
    counts = np.zeros(max(len(reg), 1), np.int64)
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_mapper_visible(ctx.h, off.ctypes.data, len(off) - 1, ov.ctypes.data, reg.ctypes.data, len(reg), pt.ctypes.data,
                                           pl.ctypes.data, len(pt), counts.ctypes.data, 0))
    return counts[:len(reg)]


def assemble_problems(track_offsets, obs_view, obs_xy, n_views, point_track, point_live, xyz, cand, capacity, device=0):
    """The 2D-3D problems of the views cand: {'offsets' int64 [k + 1], 'points2D' [m, 2] (stored xy + 0.5), 'points3D' [m, 3], 'src_obs'
    int32 [m], 'src_point' int32 [m]}, a candidate's rows ordered by observation and then by point.  capacity: the sum of
    visible_counts over the candidates."""
    off, ov, pt, pl = _tables(track_offsets, obs_view, point_track, point_live)
    xy = np.ascontiguousarray(np.asarray(obs_xy, dtype=np.float32).reshape(-1, 2))
    pts = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    cd = np.ascontiguousarray(cand, dtype=np.int32).reshape(-1)
    if len(xy) != len(ov) or len(pts) != len(pt):
        raise ValueError("the observation and point arrays do not fit together")
    cap = int(capacity)
    offsets = np.zeros(len(cd) + 1, np.int64)
    p2, p3 = np.zeros((max(cap, 1), 2)), np.zeros((max(cap, 1), 3))
    so, sp = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_mapper_assemble(ctx.h, off.ctypes.data, len(off) - 1, ov.ctypes.data, xy.ctypes.data, int(n_views), pt.ctypes.data,
                                            pl.ctypes.data, pts.ctypes.data, len(pt), cd.ctypes.data, len(cd), cap, offsets.ctypes.data, p2.ctypes.data,
                                            p3.ctypes.data, so.ctypes.data, sp.ctypes.data, 0))
    m = int(offsets[-1])
    return {"offsets": offsets, "points2D": p2[:m], "points3D": p3[:m], "src_obs": so[:m], "src_point": sp[:m]}


class DeviceStages:
    """The stage calls of reconstruct() on the device: two set-up calls (two_view, build_tracks) and the seven of a round."""

    def __init__(self, device=0):
        self.device = device

    def two_view(self, cameras, images, keypoints, pair_matches, max_error, min_num_inliers, seed):
        return two_view.verify_pairs_two_view(cameras, images, keypoints, pair_matches, max_error, min_num_inliers, self.device, seed=seed)

    def fundamental(self, keypoints, pair_matches, max_error, min_num_inliers, seed):
        return two_view.verify_pairs_fundamental(keypoints, pair_matches, max_error, min_num_inliers, self.device, seed=seed)

    def geometry(self, cameras, images, keypoints, pair_matches, max_error, min_num_inliers, seed):
        return two_view.verify_pairs_geometry(keypoints, pair_matches, cameras, images, max_error, min_num_inliers, device=self.device, seed=seed)

    def build_tracks(self, n_nodes, edges, max_rounds):
        return triangulation.build_tracks(n_nodes, edges, max_rounds, self.device)

    def restrict(self, track_offsets, obs_view, obs_xy, registered):
        return restrict_tracks(track_offsets, obs_view, obs_xy, registered, device=self.device)

    def triangulate(self, views, n_views, track_offsets, track_labels, obs_view, obs_xy, **kw):
        return triangulation.triangulate(views, n_views, track_offsets, track_labels, obs_view, obs_xy, device=self.device, **kw)

    def adjust(self, views, n_views, view_constant, xyz, point_constant, point_offsets, obs_view, obs_xy, **kw):
        return bundle_adjustment.adjust(views, n_views, view_constant, xyz, point_constant, point_offsets, obs_view, obs_xy, device=self.device, **kw)

    def adjust_cameras(self, cam_models, cam_params, cam_refine, view_camera, views, n_views, view_constant, xyz, point_constant, point_offsets, obs_view,
                       obs_xy, **kw):
        return bundle_adjustment.adjust_cameras(cam_models, cam_params, cam_refine, view_camera, views, n_views, view_constant, xyz, point_constant,
                                                point_offsets, obs_view, obs_xy, device=self.device, **kw)

    def filter(self, views, n_views, xyz, point_offsets, obs_view, obs_xy, max_reproj_error, min_tri_angle):
        return filter_points(views, n_views, xyz, point_offsets, obs_view, obs_xy, max_reproj_error, min_tri_angle, device=self.device)

    def visible(self, track_offsets, obs_view, registered, point_track, point_live):
        return visible_counts(track_offsets, obs_view, registered, point_track, point_live, self.device)

    def assemble(self, track_offsets, obs_view, obs_xy, n_views, point_track, point_live, xyz, cand, capacity):
        return assemble_problems(track_offsets, obs_view, obs_xy, n_views, point_track, point_live, xyz, cand, capacity, self.device)

    def absolute_pose(self, problems, cand, max_error_px, min_inlier_ratio, seed):
        """cand: the view index of every problem (the device call does not need it)."""
        return pose.absolute_pose_estimation_batch(problems, max_error_px, min_inlier_ratio=min_inlier_ratio, seed=seed, device=self.device)

    def absolute_pose_focal(self, problems, cand, max_error_px, min_inlier_ratio, seed):
        """absolute_pose for views of a camera nobody has seen yet: the focal length is swept and refined, the extras
        stay as given; each result carries 'camera'."""
        from . import pose
        return pose.absolute_pose_estimation_batch(problems, max_error_px, min_inlier_ratio=min_inlier_ratio, seed=seed, device=self.device,
                                                   estimate_focal_length=True, refine_focal_length=True)


# ---------------------------------------------------------------------------------------------------------------- the mapper
def _blank_views(cameras, cam_ids):
    arr = (_lib.TriView * max(len(cam_ids), 1))()
    for k, cid in enumerate(cam_ids):
        mid, params = camera_model(cameras[cid])
        arr[k].model = mid
        for i in range(8):
            arr[k].params[i] = params[i]
        arr[k].qvec[0] = 1.0
    return arr


def _set_pose(view, qvec, tvec):
    for i in range(4):
        view.qvec[i] = float(qvec[i])
    for i in range(3):
        view.tvec[i] = float(tvec[i])


def select_initial_pair(results, eligible, init_min_tri_angle, min_tri_angle):
    """The first pair, by more inliers and then by smaller index, among the eligible pairs with success whose tri_angle_deg reaches the
    bound; the bound starts at init_min_tri_angle and is halved while it stays >= min_tri_angle.  Returns (pair index, bound used)."""
    cands = sorted((p for p in eligible if results[p]["success"]), key=lambda p: (-int(results[p]["num_inliers"]), p))
    angle = float(init_min_tri_angle)
    while angle >= min_tri_angle:
        for p in cands:
            if results[p]["tri_angle_deg"] >= angle:          # a NaN angle never qualifies
                return p, angle
        angle *= 0.5
    raise RuntimeError(f"no initial pair: none of the {len(cands)} pairs with a relative pose reaches a triangulation angle of "
                       f"{min_tri_angle} degrees")


def select_candidates(counts, registered, tries, max_reg_trials, min_count, round_ratio, max_images):
    """Unregistered views with tries left and count >= min_count, by larger count and then by smaller index; those within round_ratio of
    the best, at most max_images."""
    idx = [v for v in range(len(counts)) if not registered[v] and tries[v] < max_reg_trials and counts[v] >= min_count]
    idx.sort(key=lambda v: (-int(counts[v]), v))
    if not idx:
        return []
    best = int(counts[idx[0]])
    return [v for v in idx if counts[v] >= round_ratio * best][:max_images]


def reconstruct(cameras, images, keypoints, pair_matches, skip_geometric_verification=False, device=0, stages=None, report=None,
                verification="essential", **options):
    """cameras: id -> camera dict; images: id -> record with .name and .camera_id; keypoints: image id -> [n, 2] as the feature store holds
    them; pair_matches: [(image id 0, image id 1, matches [m, 2])].  options: DEFAULTS.  stages: the stage calls (DeviceStages).  report:
    a dict that receives 'initial_pair', 'rounds' (per round: candidates, registered, points, observations, the adjustment's report, seconds
    per stage) and 'final'.  Returns (images, points3D) as colmap_io writes them: image ids 1..n in sorted-name order, registered images
    only; point ids 1-based in (track, slot) order.  verification "fundamental": for cameras nobody trusts (the prior focal length), the
    matches are verified by every pair's fundamental matrix instead of an essential matrix at those cameras; the map then
    starts as with skip_geometric_verification on the verified matches.  verification "geometry": E, F and H are estimated for every pair and
    the matches of two_view.decide_two_view_geometry's choice stay, so a planar or rotation-only pair keeps its matches
    through H; a pair labelled panoramic, planar_or_panoramic or degenerate is no initial pair (planar is: the five-point pose holds on a
    plane).  The map then starts as with "fundamental".  With one of the options refine_focal_length, refine_principal_point,
    refine_extra_params set the return is (cameras, images, points3D): the camera records with the refined intrinsics first.  Option
    abs_pose_estimate_focal_length: a candidate whose camera id has no registered view is registered through
    stages.absolute_pose_focal, and on registration the camera record and every view of that camera id take the returned parameters; of
    several candidates of a round that share such a camera the first to register sets it, the others wait for the next round without
    losing a try.  The return then is (cameras, images, points3D) as well."""
    if verification not in ("essential", "fundamental", "geometry"):
        raise ValueError(f"unknown verification {verification!r}")
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown options {sorted(unknown)}")
    o = dict(DEFAULTS, **options)
    S = DeviceStages(device) if stages is None else stages
    mask = bundle_adjustment.refine_mask(o["refine_focal_length"], o["refine_principal_point"], o["refine_extra_params"])
    if o["ba_solver"] not in bundle_adjustment.SOLVERS:
        raise ValueError(f"ba_solver {o['ba_solver']!r} is not supported (one of {', '.join(bundle_adjustment.SOLVERS)})")
    if mask and o["ba_solver"] != DEFAULTS["ba_solver"]:
        raise ValueError('ba_solver "dense" does not go with a refine option: the dense solver holds the intrinsics constant (DESIGN.md section 21)')
    ba_options = {} if o["ba_solver"] == DEFAULTS["ba_solver"] else {"solver": o["ba_solver"]}     # the default's calls stay as they were
    focal = bool(o["abs_pose_estimate_focal_length"])
    if mask or focal:
        cameras = dict(cameras)                                                   # the refined records replace the given ones, round by round
    rep = {} if report is None else report
    order = sorted(images, key=lambda i: (images[i].name, i))                    # view k <-> input id order[k] <-> output id k + 1
    index = {iid: k for k, iid in enumerate(order)}
    nv = len(order)
    if nv < 2:
        raise ValueError("a reconstruction needs at least two images")
    kp_off, kp = triangulation.keypoint_table(order, keypoints)
    pair_matches = [(a, b, np.asarray(m).reshape(-1, 2).astype(np.int32)) for a, b, m in pair_matches]
    clock = time.perf_counter

    # 1. verification and the pairs' relative poses
    t0 = clock()
    n_pairs = len(pair_matches)
    if verification == "fundamental" and not skip_geometric_verification:
        m_all, off, _, _ = S.fundamental(keypoints, pair_matches, o["max_error"], o["min_num_matches"], o["seed"])
        pair_matches = [(a, b, m_all[off[p]:off[p + 1]]) for p, (a, b, _) in enumerate(pair_matches)]
    barred = set()                                                               # pairs without a baseline to start from
    if verification == "geometry" and not skip_geometric_verification:
        m_all, off, _, decisions = S.geometry(cameras, images, keypoints, pair_matches, o["max_error"], o["min_num_matches"], o["seed"])
        pair_matches = [(a, b, m_all[off[p]:off[p + 1]]) for p, (a, b, _) in enumerate(pair_matches)]
        barred = {p for p, d in enumerate(decisions) if d["config"] in two_view.NO_INITIAL_PAIR}
        rep["two_view_configs"] = [d["config"] for d in decisions]
    if skip_geometric_verification or verification in ("fundamental", "geometry"):
        sizes = [int(((m[:, 0] >= 0) & (m[:, 1] >= 0)).sum()) for _, _, m in pair_matches]
        for p, (a, b, m) in enumerate(pair_matches):
            if len(m) and (m[:, 0].max() >= kp_off[index[a] + 1] - kp_off[index[a]] or m[:, 1].max() >= kp_off[index[b] + 1] - kp_off[index[b]]):
                raise ValueError(f"pair {p}: a match index beyond its image's key points")
        top = sorted((p for p in range(n_pairs) if sizes[p] >= o["min_num_matches"] and p not in barred), key=lambda p: (-sizes[p], p))[:o["init_max_pairs"]]
        _, _, _, res = S.two_view(cameras, images, keypoints, [pair_matches[p] for p in top], o["max_error"], o["min_num_matches"], o["seed"])
        results = {p: r for p, r in zip(top, res)}
        eligible = list(top)
        matches = [np.where(((m[:, 0] >= 0) & (m[:, 1] >= 0))[:, None], m, -1) if sizes[p] >= o["min_num_matches"] else np.full_like(m, -1)
                   for p, (_, _, m) in enumerate(pair_matches)]
    else:
        m_all, off, counts, res = S.two_view(cameras, images, keypoints, pair_matches, o["max_error"], o["min_num_matches"], o["seed"])
        results = dict(enumerate(res))
        eligible = [p for p in range(n_pairs) if counts[p] >= o["min_num_matches"]]
        matches = [m_all[off[p]:off[p + 1]] for p in range(n_pairs)]
    t1 = clock()

    # the tracks, once
    rows = []
    for p, (a, b, _) in enumerate(pair_matches):
        m = matches[p]
        m = m[(m[:, 0] >= 0) & (m[:, 1] >= 0)].astype(np.int64)
        rows.append(np.stack([kp_off[index[a]] + m[:, 0], kp_off[index[b]] + m[:, 1]], 1))
    edges = np.concatenate(rows) if rows else np.zeros((0, 2), np.int64)
    _, t_off, t_nodes = S.build_tracks(int(kp_off[-1]), edges, o["max_rounds"])
    t_off = np.asarray(t_off, dtype=np.int64)
    nodes = np.asarray(t_nodes, dtype=np.int64)
    obs_view = (np.searchsorted(kp_off, nodes, side="right") - 1).astype(np.int32)
    obs_xy = np.ascontiguousarray(kp[nodes]).reshape(-1, 2)
    t_label = nodes[t_off[:-1]] if len(t_off) > 1 else np.zeros(0, np.int64)
    t2 = clock()

    # 2. the initial pair
    p0, angle = select_initial_pair(results, eligible, o["init_min_tri_angle"], o["min_tri_angle"])
    v0, v1 = index[pair_matches[p0][0]], index[pair_matches[p0][1]]
    views = _blank_views(cameras, [images[i].camera_id for i in order])
    _set_pose(views[v0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    _set_pose(views[v1], results[p0]["qvec"], results[p0]["tvec"])
    registered = np.zeros(nv, dtype=bool)
    registered[[v0, v1]] = True
    cam_ids = sorted({images[i].camera_id for i in order})
    cam_index = {cid: k for k, cid in enumerate(cam_ids)}
    view_camera = np.array([cam_index[images[i].camera_id] for i in order], dtype=np.int32)
    constant = np.ones(nv, dtype=np.uint8)                                        # an unregistered view has no observation; it stays as it is
    tries = np.zeros(nv, dtype=np.int64)
    rep.update(initial_pair=(order[v0], order[v1]), initial_pair_index=int(p0), initial_tri_angle_bound=angle, n_pairs=n_pairs,
               n_eligible_pairs=len(eligible), n_tracks=len(t_off) - 1, verify_s=t1 - t0, tracks_s=t2 - t1, rounds=[])

    def build(iterations):
        """(a)-(d): the map of the registered views at the current poses, adjusted and filtered."""
        tm = {}
        t = clock()
        sub = S.restrict(t_off, obs_view, obs_xy, registered)
        tm["restrict_s"] = clock() - t
        t = clock()
        tri = S.triangulate(views, nv, sub["sub_offsets"], t_label[sub["sub_track"]], sub["sub_view"], sub["sub_xy"], min_tri_angle=o["min_tri_angle"],
                            create_max_angle_error=o["create_max_angle_error"], filter_max_reproj_error=o["max_reproj_error"], seed=o["seed"],
                            max_refine_iterations=o["max_refine_iterations"])
        tm["triangulate_s"] = clock() - t
        # the live slots in (track, slot) order and their observations in observation order: index regrouping, no arithmetic
        P = _lib.TRI_MAX_POINTS
        slot_live = np.asarray(tri["n_obs"]).reshape(-1) > 0
        slots = np.flatnonzero(slot_live)
        slot_row = np.full(len(slot_live), -1, dtype=np.int64)
        slot_row[slots] = np.arange(len(slots))
        obs_sub_track = np.repeat(np.arange(len(sub["sub_track"]), dtype=np.int64), np.diff(sub["sub_offsets"]))
        taken = np.flatnonzero(np.asarray(tri["obs_point"]) >= 0)
        row = slot_row[obs_sub_track[taken] * P + np.asarray(tri["obs_point"])[taken].astype(np.int64)]
        taken, row = taken[row >= 0], row[row >= 0]
        by_point = np.argsort(row, kind="stable")
        p_src = taken[by_point]                                                   # index into the restricted observations
        p_off = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=len(slots)))]).astype(np.int64)
        p_view = sub["sub_view"][p_src]
        p_xy = sub["sub_xy"][p_src].astype(np.float64) + 0.5
        point_track = sub["sub_track"][slots // P].astype(np.int32)
        xyz = np.asarray(tri["xyz"]).reshape(-1, 3)[slots]
        t = clock()
        vc = constant.copy()
        vc[registered] = 0
        vc[v0] = 1
        if o["fix_initial_pair"] or registered.sum() == 2:    # the pair's relative pose is held only while nothing else can correct it
            vc[v1] = 1
        if mask and registered.sum() >= o["intrinsics_min_views"]:
            packed = [camera_model(cameras[cid]) for cid in cam_ids]
            cam_params, xyz, _, ba = S.adjust_cameras([m for m, _ in packed], [p for _, p in packed], [mask] * len(cam_ids), view_camera, views, nv, vc, xyz,
                                                      np.zeros(len(xyz), np.uint8), p_off, p_view, p_xy, max_iterations=int(iterations), loss="cauchy",
                                                      loss_scale=o["ba_loss_scale"])
            for c, cid in enumerate(cam_ids):                 # the records and the views: what the next stage calls read
                cam = cameras[cid]
                cameras[cid] = colmap_io.Camera(cam["id"], cam["model"], cam["width"], cam["height"], cam_params[c][:len(cam["params"])])
            for k in range(nv):
                for i in range(8):
                    views[k].params[i] = float(cam_params[view_camera[k]][i])
            ba = dict(ba, refined_intrinsics=True)
        else:
            xyz, _, ba = S.adjust(views, nv, vc, xyz, np.zeros(len(xyz), np.uint8), p_off, p_view, p_xy, max_iterations=int(iterations), loss="cauchy",
                                  loss_scale=o["ba_loss_scale"], **ba_options)
        tm["adjust_s"] = clock() - t
        t = clock()
        flt = S.filter(views, nv, xyz, p_off, p_view, p_xy, o["max_reproj_error"], o["min_tri_angle"])
        tm["filter_s"] = clock() - t
        return dict(point_track=point_track, xyz=xyz, p_off=p_off, p_obs=sub["sub_obs"][p_src], filt=flt, ba=ba, seconds=tm)

    # 3. the rounds
    while True:
        M = build(o["ba_round_iterations"])
        live = M["filt"]["point_live"]
        t = clock()
        counts = np.asarray(S.visible(t_off, obs_view, registered, M["point_track"], live))
        M["seconds"]["visible_s"] = clock() - t
        cand = select_candidates(counts, registered, tries, o["max_reg_trials"], o["abs_pose_min_num_inliers"], o["round_ratio"],
                                 o["max_images_per_round"])
        rnd = dict(candidates=[order[v] for v in cand], registered=[], points=int(live.sum()), observations=int(M["filt"]["obs_keep"].sum()),
                   n_registered=int(registered.sum()), ba={k: v for k, v in M["ba"].items() if not isinstance(v, np.ndarray)}, seconds=M["seconds"])
        rep["rounds"].append(rnd)
        if not cand:
            break
        t = clock()
        prob = S.assemble(t_off, obs_view, obs_xy, nv, M["point_track"], live, M["xyz"], cand, int(counts[cand].sum()))
        rnd["seconds"]["assemble_s"] = clock() - t
        po = prob["offsets"]
        problems = [(prob["points2D"][po[c]:po[c + 1]], prob["points3D"][po[c]:po[c + 1]], cameras[images[order[v]].camera_id])
                    for c, v in enumerate(cand)]
        t = clock()
        unseen = []                                                               # candidates of a camera no registered view has: its focal length is a prior
        if focal:
            seen = {images[order[k]].camera_id for k in np.flatnonzero(registered)}
            unseen = [c for c, v in enumerate(cand) if images[order[v]].camera_id not in seen]
        if unseen:
            known = [c for c in range(len(cand)) if c not in set(unseen)]
            res = [None] * len(cand)
            if known:
                for c, r in zip(known, S.absolute_pose([problems[c] for c in known], [cand[c] for c in known], o["abs_pose_max_error"],
                                                       o["abs_pose_min_inlier_ratio"], o["seed"])):
                    res[c] = r
            for c, r in zip(unseen, S.absolute_pose_focal([problems[c] for c in unseen], [cand[c] for c in unseen], o["abs_pose_max_error"],
                                                          o["abs_pose_min_inlier_ratio"], o["seed"])):
                res[c] = r
            rnd["focal_candidates"] = [order[cand[c]] for c in unseen]
        else:
            res = S.absolute_pose(problems, list(cand), o["abs_pose_max_error"], o["abs_pose_min_inlier_ratio"], o["seed"])
        rnd["seconds"]["absolute_pose_s"] = clock() - t
        set_now = set()                                                           # cameras a candidate of this round has set
        for c, (v, r) in enumerate(zip(cand, res)):
            n = int(po[c + 1] - po[c])
            cid = images[order[v]].camera_id
            if c in unseen and cid in set_now:                                    # estimated at the prior another candidate has replaced: next round
                continue
            if r["success"] and r["num_inliers"] >= o["abs_pose_min_num_inliers"] and n > 0 and r["num_inliers"] / n >= o["abs_pose_min_inlier_ratio"]:
                _set_pose(views[v], r["qvec"], r["tvec"])
                registered[v] = True
                rnd["registered"].append(order[v])
                if c in unseen:                                                   # the record and the views, as the adjustment's path does
                    cam = cameras[cid]
                    params = camera_model(r["camera"])[1]
                    cameras[cid] = colmap_io.Camera(cam["id"], cam["model"], cam["width"], cam["height"], params[:len(cam["params"])])
                    for k in np.flatnonzero(view_camera == cam_index[cid]):
                        for i in range(8):
                            views[k].params[i] = float(params[i])
                    set_now.add(cid)
            else:
                tries[v] += 1

    # 4. the final map
    M = build(o["ba_final_iterations"])
    flt = M["filt"]
    rep["final"] = dict(points=int(flt["point_live"].sum()), observations=int((flt["obs_keep"] & np.repeat(flt["point_live"], np.diff(M["p_off"]))).sum()),
                        n_registered=int(registered.sum()), ba={k: v for k, v in M["ba"].items() if not isinstance(v, np.ndarray)}, seconds=M["seconds"])
    live_rows = np.flatnonzero(flt["point_live"])
    pid_of_row = np.full(len(flt["point_live"]), -1, dtype=np.int64)
    pid_of_row[live_rows] = np.arange(1, len(live_rows) + 1)
    obs_row = np.repeat(np.arange(len(M["p_off"]) - 1, dtype=np.int64), np.diff(M["p_off"]))
    kept = flt["obs_keep"] & flt["point_live"][obs_row]
    node = nodes[M["p_obs"][kept]]
    node_pid = np.full(int(kp_off[-1]), -1, dtype=np.int64)
    node_pid[node] = pid_of_row[obs_row[kept]]
    out_images = {}
    for k in np.flatnonzero(registered):
        im = images[order[k]]
        lo, hi = int(kp_off[k]), int(kp_off[k + 1])
        out_images[int(k) + 1] = colmap_io.Image(int(k) + 1, np.array(views[k].qvec[:], dtype=np.float64), np.array(views[k].tvec[:], dtype=np.float64),
                                                 im.camera_id, im.name, kp[lo:hi].astype(np.float64) + 0.5, node_pid[lo:hi].copy())
    k_off = np.concatenate([[0], np.cumsum(np.bincount(obs_row[kept], minlength=len(M["p_off"]) - 1))]).astype(np.int64)
    node_view = obs_view[M["p_obs"][kept]].astype(np.int64)
    node_idx = node - kp_off[node_view]
    points3D = {}
    for r in live_rows:
        a, b = k_off[r], k_off[r + 1]
        pid = int(pid_of_row[r])
        points3D[pid] = colmap_io.Point3D(pid, M["xyz"][r].copy(), np.zeros(3, np.uint8), float(flt["point_error"][r]), (node_view[a:b] + 1).astype(np.int32),
                                          node_idx[a:b].astype(np.int32))
    if mask or focal:
        return cameras, out_images, points3D
    return out_images, points3D


# ---------------------------------------------------------------------------------------------------------------- the command
def prior_camera(cam_id, width, height):
    """COLMAP's prior without EXIF: SIMPLE_RADIAL, f = 1.2 max(w, h), the principal point at the centre, k = 0."""
    return colmap_io.Camera(cam_id, "SIMPLE_RADIAL", int(width), int(height), [1.2 * max(int(width), int(height)), 0.5 * int(width), 0.5 * int(height), 0.0])


def read_images(pairs_path, features_path, single_camera=False, reference_sfm_model=None, intrinsics=()):
    """(cameras, images) of the names the pair list mentions and the feature store holds, in sorted-name order with ids 1..n.
    Intrinsics from geometric_verification.read_cameras when a model or lists are given (a name without intrinsics is left out), else
    the prior from the feature store's image_size (width, height)."""
    with open(str(pairs_path), "r") as f:
        names = sorted({n for line in f for n in line.split()[:2]})
    given = geometric_verification.read_cameras(reference_sfm_model, intrinsics) if (reference_sfm_model is not None or intrinsics) else None
    cameras, images = {}, {}
    feats = feature_io.open_store(features_path, "r")
    try:
        for name in names:
            if name not in feats or (given is not None and name not in given):
                continue
            iid = len(images) + 1
            if given is not None:
                c = given[name]
                cam = colmap_io.Camera(iid, c["model"] if isinstance(c["model"], str) else c["model"].name, c["width"], c["height"], c["params"])
            else:
                w, h = (int(v) for v in np.asarray(feats[name]["image_size"].__array__()).reshape(-1)[:2])
                if single_camera and cameras:
                    first = cameras[1]
                    if (first["width"], first["height"]) != (w, h):
                        raise ValueError(f"--single_camera: {name} is {w}x{h}, the first image {first['width']}x{first['height']}")
                    images[iid] = SimpleNamespace(name=name, camera_id=1)
                    continue
                cam = prior_camera(iid, w, h)
            cameras[iid] = cam
            images[iid] = SimpleNamespace(name=name, camera_id=iid)
    finally:
        feats.close()
    return cameras, images


def main(sfm_dir, image_dir, pairs, features, matches, colmap_path=None, single_camera=False, skip_geometric_verification=False,
         min_match_score=None, min_num_matches=None, reference_sfm_model=None, intrinsics=(), device=0, verification="essential",
         refine_focal_length=0, refine_principal_point=0, refine_extra_params=0, intrinsics_min_views=None, ba_solver=None,
         abs_pose_estimate_focal_length=0, **options):
    """hloc/reconstruction.py main(): image_dir and colmap_path are accepted and unused.  Writes sfm_dir/models/0/{cameras,images,
    points3D}.bin and sfm_dir/stats.txt (one `key: value` per line; the reference writes the same keys without the newline); returns
    the statistics.  With a refine option set cameras.bin holds the refined intrinsics."""
    sfm_dir = Path(sfm_dir)
    assert Path(pairs).exists(), pairs
    assert Path(features).exists(), features
    assert Path(matches).exists(), matches
    if min_num_matches is not None:
        options["min_num_matches"] = int(min_num_matches)
    for key, value in (("refine_focal_length", refine_focal_length), ("refine_principal_point", refine_principal_point),
                       ("refine_extra_params", refine_extra_params), ("abs_pose_estimate_focal_length", abs_pose_estimate_focal_length)):
        if value:
            options[key] = True
    if intrinsics_min_views is not None:
        options["intrinsics_min_views"] = int(intrinsics_min_views)
    if ba_solver is not None:
        options["ba_solver"] = ba_solver
    cameras, images = read_images(pairs, features, single_camera, reference_sfm_model, intrinsics)
    keypoints, pair_matches = triangulation.read_inputs(images, pairs, features, matches, min_match_score)
    logging.info("Reconstructing from %d pairs over %d images...", len(pair_matches), len(images))
    report = {}
    out = reconstruct(cameras, images, keypoints, pair_matches, skip_geometric_verification, device=device, report=report, verification=verification,
                      **options)
    if len(out) == 3:
        cameras = out[0]
    out_images, points3D = out[-2:]
    model = sfm_dir / "models" / "0"
    model.mkdir(parents=True, exist_ok=True)
    used = {im.camera_id for im in out_images.values()}
    colmap_io.write_model({i: c for i, c in cameras.items() if i in used}, out_images, points3D, model)
    stats = triangulation.model_statistics(out_images, points3D)
    stats["num_input_images"] = len(images)
    with open(sfm_dir / "stats.txt", "w") as f:
        for k in STAT_KEYS:
            f.write(f"{k}: {stats[k]}\n")
    logging.info("Statistics: %s (%d rounds)", stats, len(report["rounds"]))
    return stats


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sfm_dir", type=Path, required=True)
    ap.add_argument("--image_dir", type=Path, required=True)
    ap.add_argument("--pairs", type=Path, required=True)
    ap.add_argument("--features", type=Path, required=True)
    ap.add_argument("--matches", type=Path, required=True)
    ap.add_argument("--colmap_path", type=Path, default="colmap")
    ap.add_argument("--single_camera", action="store_true")
    ap.add_argument("--skip_geometric_verification", action="store_true")
    ap.add_argument("--min_match_score", type=float)
    ap.add_argument("--min_num_matches", type=int)
    ap.add_argument("--reference_sfm_model", type=Path)
    ap.add_argument("--intrinsics", type=Path, nargs="+", default=[])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--verification", choices=("essential", "fundamental", "geometry"), default="essential")
    ap.add_argument("--refine_focal_length", type=int, choices=(0, 1), default=0)
    ap.add_argument("--refine_principal_point", type=int, choices=(0, 1), default=0)
    ap.add_argument("--refine_extra_params", type=int, choices=(0, 1), default=0)
    ap.add_argument("--intrinsics_min_views", type=int, default=None)
    ap.add_argument("--abs_pose_estimate_focal_length", type=int, choices=(0, 1), default=0)
    ap.add_argument("--ba_solver", choices=sorted(bundle_adjustment.SOLVERS), default=DEFAULTS["ba_solver"])
    return ap


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main(**parser().parse_args().__dict__)
