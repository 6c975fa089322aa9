"""Bundle adjustment with camera intrinsics among the unknowns on the MI355X (sfd2_bundle_adjust_cameras) against
the numpy restatement and the scenes of tests/bundle_cam_ref.py.

Tolerances follow section 14's rule: 10 x the floor of the restatement on the same scene, computed where the test runs, ceiling 1e-6;
poses and points in bundle_ref.state_diff's measure, camera parameters relative to the parameter's own size (bundle_cam_ref.cam_diff).
The floor is the disagreement of the restatement's two routes, for a run to convergence the larger of that and the near-tie radius.
The restatement is the yardstick, never the device.  The floors as measured on the CPU are listed in tests/test_bundle_cam_host.py
(FLOORS, RADII).

Measured on the MI355X (the larger of the pose / point and the camera difference, the tolerance in brackets): one step, focal group alone
2.9e-12 of the step's norm (3.0e-11), all three groups 1.5e-13 (1.8e-11); 'shared_focal' 7.1e-13, 'shared_focal_cauchy' 7.0e-11 (1e-6: the
near-tie radius is 1.5e-6); 'per_view' 6.7e-11 (6.9e-10); 'two_cameras_opencv' 7.2e-12 (7.3e-11); one camera shared by 255 / 256 / 257 / 300
views 4.0e-13 / 3.9e-14 / 2.1e-12 / 9.0e-13 (5.8e-12 / 2.6e-13 / 3.5e-10 / 1.1e-11); 'busy_camera' 3.9e-13 (4.7e-12) under every mapping.
The final cost is printed beside them and not asserted: the floor above is the state's, not the cost's (the two routes' costs differ by
8.0e-12 on the one-step scene, the device's from route A's by 7.9e-12)."""
import numpy as np
import pytest

import bundle_cam_ref as cr
import bundle_ref as br
import pose_ref as pr

pytestmark = pytest.mark.gpu

TIGHT = dict(pcg_tolerance=br.PCG_TOLERANCE, pcg_max_iterations=2000)


def _B():
    from sfd2_amd import bundle_adjustment
    return bundle_adjustment


def _views(P, junk=False):
    """P's poses; the views' own camera words are not read by the new call (junk: filled with what would be an error if they were)."""
    from sfd2_amd import _lib
    arr = (_lib.TriView * P.nv)()
    for i, cam in enumerate(P.cams):
        mid, params = _B().camera_model(cam)
        arr[i].model = 77 if junk else mid
        for k in range(8):
            arr[i].params[k] = np.nan if junk else params[k]
        for k in range(4):
            arr[i].qvec[k] = P.q[i][k]
        for k in range(3):
            arr[i].tvec[k] = P.t[i][k]
    return arr


def _cam_arrays(P):
    packed = [_B().camera_model(c) for c in P.cam_list]
    return np.array([m for m, _ in packed], np.int32), np.array([p for _, p in packed], np.float64)


def _opencv(P, params):
    return np.array([pr._opencv(dict(c, params=params[i][:len(c["params"])])) for i, c in enumerate(P.cam_list)], dtype=np.float64).reshape(-1, 8)


def run(P, flags=0, junk=True, refine=None, **options):
    """The device's result for a CamProblem: state (R, t, X, Kc), the words as returned, the report."""
    views = _views(P, junk)
    models, params = _cam_arrays(P)
    opts = dict(loss=P.loss, loss_scale=P.loss_scale)
    opts.update(options)
    cams, xyz, err, report = _B().adjust_cameras(models, params, P.refine if refine is None else refine, P.view_camera, views, P.nv, P.vconst, P.X, P.pconst,
                                                 P.off, P.obs_view, P.obs_xy, flags=flags, **opts)
    words = np.array([list(views[i].qvec) + list(views[i].tvec) for i in range(P.nv)], dtype=np.float64)
    vcams = np.array([[views[i].model] + list(views[i].params) for i in range(P.nv)], dtype=np.float64)
    R = np.stack([pr.qvec2rotmat(w[:4]) for w in words])
    return {"state": (R, words[:, 4:].copy(), xyz, _opencv(P, cams)), "words": words, "xyz": xyz, "err": err, "cams": cams, "view_cams": vcams,
            "report": report}


def _same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("words", "xyz", "err", "cams", "view_cams")) and a["report"] == b["report"]


def _checks(P, out):
    """Constants come back bit for bit; every view leaves with its camera's words; obs_error is the residual norm of the returned state."""
    words0 = np.concatenate([P.q, P.t], 1)
    assert out["words"][P.vconst].tobytes() == words0[P.vconst].tobytes()
    assert out["xyz"][P.pconst].tobytes() == P.X[P.pconst].tobytes()
    models, params = _cam_arrays(P)
    held = P.refine == 0
    assert out["cams"][held].tobytes() == params[held].tobytes()
    inactive = ~cr.active_words(P)
    assert (out["state"][3][inactive] == P.Kc[inactive]).all()
    assert (out["view_cams"][:, 0] == models[P.view_camera]).all() and out["view_cams"][:, 1:].tobytes() == out["cams"][P.view_camera].tobytes()
    r, _ = cr.residuals(P, out["state"])
    assert np.abs(np.linalg.norm(r, axis=1) - out["err"]).max() <= 1e-9


def _compare(name, out, **kw):
    P, ref, tol = cr.scene(name), cr.solution(name), cr.tolerance(name)
    fig = {"tol": tol, "pose_point": br.state_diff(out["state"][:3], ref["state"][:3]), "camera": cr.cam_diff(P, out["state"][3], ref["state"][3]),
           "cost": abs(out["report"]["final_cost"] - ref["cost"]) / ref["cost"]}
    print(name, kw, {k: float("%.3g" % v) for k, v in fig.items()}, out["report"])        # the cost is printed, not asserted: its floor is another one
    return fig


# ---------------------------------------------------------------------------------------------------------------- 1. one step
@pytest.mark.parametrize("name", ["shared_step_focal", "shared_step_all"])
def test_one_step_matches_the_dense_solve(name):
    P = cr.scene(name)
    a, b = cr.solution(name, cr.ROUTE_A), cr.solution(name, cr.ROUTE_B)
    tol = min(10 * cr.step_diff(a["first_step"], b["first_step"]), 1e-6)
    out = run(P, max_iterations=1, **TIGHT)
    rep = out["report"]
    assert rep["iterations"] == 1 and rep["accepted_steps"] == 1
    dv, dp = br.step_between(P, out["state"][:3])
    dK = out["state"][3] - P.Kc
    dk = np.einsum("ci,cki->ck", dK, P.dirs) / np.maximum((P.dirs ** 2).sum(2), 1.0)
    gmax = run(P, max_iterations=0)["report"]["gradient_max"]
    fig = {"tol": tol, "step": cr.step_diff((dv, dp, dk), a["first_step"]), "cost": abs(rep["initial_cost"] - a["initial_cost"]) / a["initial_cost"],
           "gmax": abs(gmax - a["initial_gmax"]) / a["initial_gmax"], "pcg": rep["pcg_iterations"]}
    print(name, fig)
    assert fig["step"] <= tol and fig["cost"] <= tol and fig["gmax"] <= tol
    f = _compare(name, out)
    assert f["pose_point"] <= f["tol"] and f["camera"] <= f["tol"]
    assert (dk != 0).sum() == P.kcount.sum()
    _checks(P, out)
    assert _same_bytes(out, run(P, max_iterations=1, **TIGHT))


# ---------------------------------------------------------------------------------------------------------------- 2. converged
@pytest.mark.parametrize("name", ["shared_focal", "shared_focal_cauchy"])
def test_converged_focal_length_and_distortion(name):
    """Truth f = 800, k = -0.08, start f = 960, k = 0.  The accept / reject sequence: neither the restatement's length nor one accepted step
    fewer can be asserted for the whole run, because the restatement has no single length: near the minimum every decision compares two
    costs that agree to rounding, and its two routes part ways there.  Measured: trivial loss, route A 7 accepted in 30 steps, route B 10 in
    36, the MI355X 9 in 34; Cauchy, 17 in 50, 15 in 46, the MI355X 17 in 50 (equal to route A).  Asserted instead, step by step, is the
    sequence for as long as both routes take every decision alike and at least 1e-6 (relative) from a tie: 3 and 7 steps, all accepted.
    The totals are printed."""
    P, ref = cr.scene(name), cr.solution(name)
    out = run(P, pcg_tolerance=1e-10, pcg_max_iterations=500)
    rep = out["report"]
    f = _compare(name, out)
    print(name, "device iterations / accepted", rep["iterations"], rep["accepted_steps"], "restatement", ref["iterations"], ref["accepted"],
          "route B", cr.solution(name, cr.ROUTE_B)["iterations"], cr.solution(name, cr.ROUTE_B)["accepted"], "f, k", out["state"][3][0, [0, 4]])
    assert rep["status"] in ("gradient_tolerance", "lambda_overflow")
    assert f["pose_point"] <= f["tol"] and f["camera"] <= f["tol"]
    # the accept / reject sequence: the same as the restatement's for as long as the restatement has one (bundle_cam_ref.decisive_prefix)
    prefix = cr.decisive_prefix(name)
    for k in range(1, len(prefix) + 1):
        r = run(P, max_iterations=k, pcg_tolerance=1e-10, pcg_max_iterations=500)["report"]
        assert (r["iterations"], r["accepted_steps"]) == (k, sum(prefix[:k])), (k, prefix, r)
    assert abs(out["state"][3][0, 0] - 800.0) < 0.01 * 800.0 and abs(out["state"][3][0, 4] + 0.08) < 0.02
    _checks(P, out)
    assert _same_bytes(out, run(P, pcg_tolerance=1e-10, pcg_max_iterations=500))


# ---------------------------------------------------------------------------------------------------------------- 3. several cameras
@pytest.mark.parametrize("name", ["per_view", "two_cameras_opencv"])
def test_two_steps_with_several_cameras(name):
    P, ref = cr.scene(name), cr.solution(name)
    out = run(P, max_iterations=2, **TIGHT)
    f = _compare(name, out)
    assert out["report"]["accepted_steps"] == ref["accepted"] == 2
    assert f["pose_point"] <= f["tol"] and f["camera"] <= f["tol"]
    _checks(P, out)
    if name == "two_cameras_opencv":
        assert P.refine.tolist() == [7, 0] and P.kcount.tolist() == [8, 0]
        assert (out["cams"][0] != _cam_arrays(P)[1][0]).all()                            # all eight moved
    else:
        assert P.kcount.tolist() == [1, 2, 2, 6] * 2
    assert _same_bytes(out, run(P, max_iterations=2, **TIGHT))


# ---------------------------------------------------------------------------------------------------------------- 4. seams
@pytest.mark.parametrize("n_views", cr.SEAM_VIEWS)
def test_one_camera_shared_by_many_views(n_views):
    name = "seam_%d" % n_views
    P, ref = cr.scene(name), cr.solution(name)
    assert P.nv == n_views and P.ncam == 1
    out = run(P, max_iterations=2, **TIGHT)
    f = _compare(name, out)
    assert out["report"]["accepted_steps"] == ref["accepted"] == 2
    assert f["pose_point"] <= f["tol"] and f["camera"] <= f["tol"]
    _checks(P, out)
    assert _same_bytes(out, run(P, max_iterations=2, **TIGHT))


@pytest.mark.parametrize("flags", [0, 1, 2], ids=["by_length", "lane", "wave"])
def test_camera_of_views_with_few_and_many_observations(flags):
    P, ref = cr.scene("busy_camera"), cr.solution("busy_camera")
    assert np.bincount(P.obs_view, minlength=9)[:7].tolist() == list(br.VIEW_COUNTS) and (P.view_camera != 2).all()
    out = run(P, flags=flags, max_iterations=2, **TIGHT)
    f = _compare("busy_camera", out, flags=flags)
    assert out["report"]["accepted_steps"] == ref["accepted"] == 2
    assert f["pose_point"] <= f["tol"] and f["camera"] <= f["tol"]
    _checks(P, out)
    assert out["cams"][2].tobytes() == _cam_arrays(P)[1][2].tobytes()                    # the camera no view uses: bit for bit
    assert out["cams"][1][0] != _cam_arrays(P)[1][1][0]                                  # the constant views' camera moves
    assert _same_bytes(out, run(P, flags=flags, max_iterations=2, **TIGHT))


def test_unobserved_camera_and_rejected_run_come_back_bit_for_bit():
    P = cr.scene("busy_camera")
    vcam = P.view_camera.copy()
    vcam[0] = 2                                                                         # view 0 has no observation: camera 2 has views, but none observed
    Q = cr.with_cameras(P, P.cam_list, vcam, P.refine)
    out = run(Q, max_iterations=1, **TIGHT)
    assert out["report"]["accepted_steps"] == 1 and out["cams"][2].tobytes() == _cam_arrays(P)[1][2].tobytes()
    out = run(P, max_iterations=0)
    assert out["cams"].tobytes() == _cam_arrays(P)[1].tobytes() and out["report"]["accepted_steps"] == 0


# ---------------------------------------------------------------------------------------------------------------- 5. the old call
@pytest.mark.parametrize("name", ["arc", "long_tracks"])
def test_constant_cameras_give_the_old_calls_bytes(name):
    import test_gpu_bundle as old
    P = br.scene(name)
    opts = dict(max_iterations=3, pcg_tolerance=1e-10, pcg_max_iterations=60)
    a, b = old.run(P, **opts), old.run(P, **opts)
    assert old._same_bytes(a, b) and a["report"]["accepted_steps"] >= 2                 # sfd2_bundle_adjust itself: still byte-equal
    out = run(cr.constant_cameras(name), junk=True, **opts)
    assert all(out[k].tobytes() == a[k].tobytes() for k in ("words", "xyz", "err")) and out["report"] == a["report"]
    # the same cameras shared (one per model) instead of one per view
    C = cr.constant_cameras(name)
    S = cr.with_cameras(P, C.cam_list[:4], np.arange(P.nv, dtype=np.int32) % 4, [0] * 4)
    assert [c["model"] for c in S.cams] == [c["model"] for c in P.cams]
    out = run(S, **opts)
    assert all(out[k].tobytes() == a[k].tobytes() for k in ("words", "xyz", "err")) and out["report"] == a["report"]


def test_pcg_batch_length_changes_nothing():
    P = cr.scene("per_view")
    opts = dict(max_iterations=3, pcg_tolerance=1e-10, pcg_max_iterations=60)
    base = run(P, pcg_batch=16, **opts)
    assert base["report"]["pcg_iterations"] > 3
    for batch in (1, 7, 64):
        assert _same_bytes(base, run(P, pcg_batch=batch, **opts)), batch


# ---------------------------------------------------------------------------------------------------------------- 6. errors
def test_bad_arguments_return_minus_one_with_the_first_offending_index():
    import ctypes
    from sfd2_amd import _lib
    P = cr.scene("per_view")
    ctx = _lib.default_context(0)

    def call(edit):
        models, params = _cam_arrays(P)
        cams = (_lib.BaCamera * P.ncam)()
        for i in range(P.ncam):
            cams[i].model, cams[i].refine = int(models[i]), int(P.refine[i])
            cams[i].params[:] = params[i].tolist()
        vcam = P.view_camera.copy()
        edit(cams, vcam)
        views, conf, res = _views(P), _B()._conf({}), _lib.BaResult()
        vc, pc = P.vconst.astype(np.uint8), P.pconst.astype(np.uint8)
        xyz, err = P.X.copy(), np.zeros(len(P.obs_view))
        rc = ctx.lib.sfd2_bundle_adjust_cameras(ctx.h, cams, P.ncam, vcam.ctypes.data, views, P.nv, vc.ctypes.data, xyz.ctypes.data, P.np_, pc.ctypes.data,
                                                P.off.ctypes.data, P.obs_view.ctypes.data, P.obs_xy.ctypes.data, ctypes.byref(conf), ctypes.byref(res),
                                                err.ctypes.data, 0)
        return rc, ctx.lib.sfd2_last_error().decode()

    def set_vcam(cams, vcam):
        vcam[[3, 6]] = P.ncam

    def set_refine(cams, vcam):
        cams[2].refine = cams[5].refine = 8

    def set_model(cams, vcam):
        cams[4].model = cams[7].model = 3

    def set_nan(cams, vcam):
        cams[1].params[0] = cams[6].params[0] = float("nan")

    for edit, msg in ((set_vcam, "view 3: camera index out of range"), (set_refine, "camera 2: unknown refine bits"), (set_model, "camera 4: camera model 3"),
                      (set_nan, "camera 1: non-finite camera parameters")):
        rc, text = call(edit)
        assert rc == -1 and text.startswith("sfd2_bundle_adjust_cameras: ") and msg in text, (msg, text)
    assert call(lambda cams, vcam: None)[0] == 0


# ---------------------------------------------------------------------------------------------------------------- 7. end to end
TRUE_F = 0.8 * 768.0                                          # 20 % below the prior of a 640 x 480 image (1.2 x 640)


def e2e_scene():
    """The 12-image scene of tests/test_gpu_mapper.py (tri_ref.make_scene) taken by one SIMPLE_RADIAL camera with f = TRUE_F, k = -0.08."""
    import tri_ref as tr

    def make():
        models, params = tr.MODELS, pr.PARAMS["SIMPLE_RADIAL"]
        tr.MODELS, pr.PARAMS["SIMPLE_RADIAL"] = ["SIMPLE_RADIAL"] * 4, [TRUE_F, 320.0, 240.0, -0.08]
        try:
            sc = tr.make_scene()
        finally:
            tr.MODELS, pr.PARAMS["SIMPLE_RADIAL"] = models, params
        for im in sc["images"].values():
            im.camera_id = 1
        sc["cameras"] = {1: sc["cameras"][1]}
        return sc
    return br.cached(("cam_e2e_scene",), make)


def e2e_run(**options):
    """reconstruct() from matches alone with the prior camera: (cameras, images, points3D, report)."""
    from sfd2_amd import reconstruction as RC
    sc, rep = e2e_scene(), {}
    out = RC.reconstruct({1: RC.prior_camera(1, 640, 480)}, sc["images"], sc["keypoints"], sc["pair_matches"], verification="fundamental", report=rep, **options)
    return ((out[0],) if len(out) == 3 else ({1: RC.prior_camera(1, 640, 480)},)) + tuple(out[-2:]) + (rep,)


def test_reconstruction_with_a_wrong_prior_refines_the_shared_camera():
    """The 12-image scene of section 15's test taken by one SIMPLE_RADIAL camera with f = 614.4 (20 % below the prior 768), k = -0.08, built
    from matches alone (fundamental verification, single camera, focal and extra refined) against the project's own pieces from the truth:
    the map triangulated at the true poses with the true camera, then adjusted with the same refine flags from the same prior camera,
    which the adjustment has to bring back.  Measured on the MI355X: the mapper registers 12 of 12 images, 839 points, mean reprojection
    error 1.011 px, rotation 0.0023 rad, centre 0.0076, f = 612.03 (0.39 % off), k = -0.0797; the yardstick 839 points, 1.021 px, 0.0017 rad,
    0.0072, f = 612.40 (0.33 % off), k = -0.0799.  Ratios: points 1.00 (>= 0.9), mean reprojection error 0.99 (<= 1.5), rotation 1.41 and
    centre 1.07 (<= 3), focal error 1.18 (<= 3).  With refinement off: 12 images, 839 points, 1.046 px, rotation 0.109 rad, centre 0.157,
    focal error 25 %.
    The yardstick is not triangulated with the prior camera: at a focal length 25 % too long the known-pose triangulation splits tracks
    (measured: 1199 points of mean track 3.4 for 791 distinct true points, where the mapper's 839 points of mean track 6.6 stand for 829;
    the scene holds 912), the adjustment cannot join them again and ends at f = 641.85, 4.5 % off.  Nine tenths of that count is more
    points than the scene has."""
    import mapper_ref as mr
    from sfd2_amd import reconstruction as RC, triangulation as T
    sc = e2e_scene()
    assert sc["cameras"][1]["params"][0] == TRUE_F and abs(RC.prior_camera(1, 640, 480)["params"][0] - 1.25 * TRUE_F) < 1e-9
    flags = dict(refine_focal_length=True, refine_extra_params=True)
    cams, ims, pts, rep = e2e_run(**flags)
    prior = {1: RC.prior_camera(1, 640, 480)}
    y_ims, y_pts = T.triangulate_model(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"])
    y_cams, y_ims, y_pts, _ = _B().bundle_adjust(prior, y_ims, y_pts, constant_images=list(rep["initial_pair"]), max_iterations=100, loss="cauchy", loss_scale=1.0,
                                                 **flags)
    f_err = lambda c: abs(c[1]["params"][0] - TRUE_F) / TRUE_F
    got, want = mr.model_errors(ims, pts, sc["images"]), mr.model_errors(y_ims, y_pts, sc["images"])
    got["focal"], want["focal"] = f_err(cams), f_err(y_cams)
    ratios = {k: got[k] / want[k] for k in ("points", "mean_reproj", "rotation", "centre", "focal")}
    print("mapper", got, cams[1]["params"], "yardstick", want, y_cams[1]["params"], "ratios", {k: round(v, 3) for k, v in ratios.items()}, "rounds", len(rep["rounds"]))
    _, ims0, pts0, rep0 = e2e_run()
    off = mr.model_errors(ims0, pts0, sc["images"])
    print("refinement off", off, "registered", rep0["final"]["n_registered"], "focal error", 0.25)
    assert sorted(ims) == list(range(1, 13)) and rep["final"]["n_registered"] == 12
    assert ratios["points"] >= 0.9 and ratios["mean_reproj"] <= 1.5 and ratios["rotation"] <= 3.0 and ratios["centre"] <= 3.0 and ratios["focal"] <= 3.0, ratios
    assert got["mean_reproj"] < off["mean_reproj"]
    assert cams[1]["params"][1:3].tolist() == [320.0, 240.0] and cams[1]["model"] == "SIMPLE_RADIAL"      # the principal point was not refined
