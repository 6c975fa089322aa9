"""The dense solver of the reduced camera system on the MI355X (solver="dense") against the numpy restatement and
the scenes of tests/bundle_ref.py, and sfd2_spd_solve against numpy.linalg.solve.

The tolerance rule is tests/test_gpu_bundle.py's, unchanged: 10 x the floor bundle_ref computes where the test runs, ceiling 1e-6.  The
restatement solves every damped step densely, so a dense step on the device is compared with what it restates; the floors of the scenes
of clusters still hold bundle_ref.pcg_allowance, which only makes them no smaller than the two routes' disagreement.  Iteration counts of
converged runs are printed, never asserted.

sfd2_spd_solve is judged by the normwise backward error |A x - b| / (|A| |x| + |b|) (2-norms, the residual in numpy.longdouble): at most
10 x what numpy.linalg.solve reaches on the same system where the test runs, and never above Higham's bound n (3 n + 1) 2^-53 of a
Cholesky solve.  The measured figures are printed by the test and recorded in DESIGN.md section 21."""
import ctypes

import numpy as np
import pytest

import bundle_dense_ref as dr
import bundle_ref as br
from test_gpu_bundle import _B, _constants_untouched, _same_bytes, _views, run
from test_gpu_bundle_edges import _check_step, _rel

pytestmark = pytest.mark.gpu

DENSE = dict(solver="dense")


def _dense(P, flags=0, **kw):
    out = run(P, flags=flags, **DENSE, **kw)
    assert out["report"]["solver"] == "dense" and out["report"]["pcg_iterations"] == 0
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. one step
def test_one_dense_step_matches_the_dense_solve():
    P = br.scene("arc")
    a, b = br.solution("arc", br.ROUTE_A, max_iterations=1), br.solution("arc", br.ROUTE_B, max_iterations=1)
    tol = min(10 * br.step_diff(a["first_step"], b["first_step"]), 1e-6)
    out = _dense(P, max_iterations=1, initial_lambda=1e-4)
    rep = out["report"]
    assert rep["iterations"] == 1 and rep["accepted_steps"] == 1
    step = br.step_between(P, out["state"])
    figures = {"tol": tol, "cost": abs(rep["initial_cost"] - a["initial_cost"]) / a["initial_cost"],
               "gmax": abs(_dense(P, max_iterations=0)["report"]["gradient_max"] - a["initial_gmax"]) / a["initial_gmax"],
               "step": br.step_diff(step, a["first_step"])}
    print("one dense step:", figures)
    assert figures["cost"] <= tol and figures["gmax"] <= tol
    norm = np.sqrt((a["first_step"][0] ** 2).sum() + (a["first_step"][1] ** 2).sum())
    assert np.abs(step[0] - a["first_step"][0]).max() <= tol * norm and np.abs(step[1] - a["first_step"][1]).max() <= tol * norm
    assert figures["step"] <= tol
    _constants_untouched(P, out)


# ---------------------------------------------------------------------------------------------------------------- 2. seams of forming S
@pytest.mark.parametrize("flags", [0, 1, 2], ids=["by_length", "lane", "wave"])
def test_long_tracks_make_many_pairs_of_one_point(flags):
    P, ref, tol = br.scene("long_tracks"), br.solution("long_tracks", max_iterations=2), br.tolerance("long_tracks", max_iterations=2)
    assert sorted(set(np.diff(P.off)[:9].tolist())) == sorted(br.TRACK_LENGTHS)
    out = _dense(P, flags=flags, max_iterations=2)
    figures = {"tol": tol, "state": br.state_diff(out["state"], ref["state"]), "cost": abs(out["report"]["final_cost"] - ref["cost"]) / ref["cost"]}
    print("dense, long tracks", flags, figures, out["report"])
    assert out["report"]["accepted_steps"] == ref["accepted"] == 2
    assert figures["state"] <= tol and figures["cost"] <= tol
    _constants_untouched(P, out)


def test_views_with_few_and_many_observations_make_block_lists_of_every_length():
    P, ref, tol = br.scene("busy_views"), br.solution("busy_views", max_iterations=2), br.tolerance("busy_views", max_iterations=2)
    assert np.bincount(P.obs_view, minlength=9)[:7].tolist() == list(br.VIEW_COUNTS)
    out = _dense(P, max_iterations=2)
    figures = {"tol": tol, "state": br.state_diff(out["state"], ref["state"]), "cost": abs(out["report"]["final_cost"] - ref["cost"]) / ref["cost"]}
    print("dense, busy views", figures, out["report"])
    assert out["report"]["accepted_steps"] == ref["accepted"] == 2
    assert out["words"][0].tobytes() == np.concatenate([P.q[0], P.t[0]]).tobytes()      # no observation (a zero row, a damped pivot): bit for bit
    for v in (1, 2):                                                                    # held by the damping
        assert br.state_diff((out["state"][0][v:v + 1], out["state"][1][v:v + 1], P.X[:0]), (ref["state"][0][v:v + 1], ref["state"][1][v:v + 1], P.X[:0])) <= tol
    assert figures["state"] <= tol and figures["cost"] <= tol
    _constants_untouched(P, out)


# ---------------------------------------------------------------------------------------------------------------- 3. seams of the factorisation
@pytest.mark.parametrize("steps", [1, 2])
def test_more_than_1024_views_many_tile_steps_and_a_ragged_last_tile(steps):
    name = "clusters"
    P, ref = br.scene(name), br.solution(name, br.ROUTE_A, **br.CLUSTER_RUNS[name])
    tol = br.step_tolerance(name)
    assert P.nv == 1030 and (6 * P.nv) % 64 != 0
    out = _dense(P, max_iterations=steps, initial_lambda=1e-4)
    rep = out["report"]
    gmax = _dense(P, max_iterations=0)["report"]["gradient_max"]
    figures = {"tol": tol, "cost": _rel(rep["initial_cost"], ref["initial_cost"]), "gmax": _rel(gmax, ref["initial_gmax"])}
    print("dense", name, steps, figures, rep)
    assert rep["iterations"] == rep["accepted_steps"] == steps <= ref["accepted"]
    assert figures["cost"] <= tol and figures["gmax"] <= tol
    _constants_untouched(P, out)
    if steps == 1:
        _check_step(P, out, ref["first_step"], tol)
        trial = ref["history"][0][1]
        print("final cost:", _rel(rep["final_cost"], trial))
        assert _rel(rep["final_cost"], trial) <= tol
    else:
        stol = br.tolerance(name, **br.CLUSTER_RUNS[name])
        figures = {"tol": stol, "state": br.state_diff(out["state"], ref["state"]), "cost": _rel(rep["final_cost"], ref["cost"])}
        print("two steps:", figures)
        assert steps == ref["accepted"] == ref["iterations"] and figures["state"] <= stol and figures["cost"] <= stol


# ---------------------------------------------------------------------------------------------------------------- 4. a rejected step
def test_rejected_dense_steps_follow_the_restatement():
    P, ref, tol = br.scene("reject_first"), br.solution("reject_first", **br.REJECT_FIRST), br.tolerance("reject_first", **br.REJECT_FIRST)
    out = _dense(P, **br.REJECT_FIRST)
    rep = out["report"]
    figures = {"tol": tol, "state": br.state_diff(out["state"], ref["state"]), "cost": _rel(rep["final_cost"], ref["cost"])}
    print("dense, rejections", figures, rep)
    assert (rep["iterations"], rep["accepted_steps"], rep["lambda"], rep["status"]) == (ref["iterations"], ref["accepted"], ref["lambda"], "max_iterations")
    assert rep["iterations"] == 5 and rep["accepted_steps"] == 2
    assert figures["state"] <= tol and figures["cost"] <= tol
    r, _ = br.residuals(P, out["state"])
    assert np.abs(np.linalg.norm(r, axis=1) - out["err"]).max() <= 1e-9       # the records behind a rejected step are the accepted state's
    _constants_untouched(P, out)


# ---------------------------------------------------------------------------------------------------------------- 5. converged runs
@pytest.mark.parametrize("name", ["arc", "arc_cauchy", "views_constant", "points_constant", "one_point_constant", "mix"])
def test_converged_dense_runs_match_the_restatement(name):
    P, ref, tol = br.scene(name), br.solution(name), br.tolerance(name)
    out = _dense(P)
    rep = out["report"]
    figures = {"tol": tol, "state": br.state_diff(out["state"], ref["state"]), "cost": abs(rep["final_cost"] - ref["cost"]) / ref["cost"],
               "status": rep["status"], "iterations": rep["iterations"], "restatement": ref["iterations"], "gmax": rep["gradient_max"]}
    print("dense", name, figures)
    assert rep["status"] in ("gradient_tolerance", "lambda_overflow")
    assert figures["state"] <= tol and figures["cost"] <= tol
    _constants_untouched(P, out)


# ---------------------------------------------------------------------------------------------------------------- 6. bytes
@pytest.mark.parametrize("name,kw", [("arc", {}), ("long_tracks", dict(max_iterations=2)), ("clusters", dict(max_iterations=1))])
def test_two_dense_runs_give_the_same_bytes(name, kw):
    P = br.scene(name)
    assert _same_bytes(_dense(P, **kw), _dense(P, **kw))


def test_the_pcg_solver_by_name_is_the_call_without_the_option():
    P = br.scene("arc")
    kw = dict(max_iterations=3, pcg_tolerance=1e-10, pcg_max_iterations=40)
    plain, named = run(P, **kw), run(P, solver="pcg", **kw)
    assert plain["report"]["solver"] == "pcg" and plain["report"]["pcg_iterations"] > 0
    assert _same_bytes(plain, named)


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def _raw(P, views, n_views, solver):
    from sfd2_amd import _lib
    xyz, ov, xy, off = np.array(P.X), np.ascontiguousarray(P.obs_view, np.int32), np.ascontiguousarray(P.obs_xy), np.ascontiguousarray(P.off, np.int64)
    vc, pc = np.zeros(n_views, np.uint8), P.pconst.astype(np.uint8)
    vc[:P.nv] = P.vconst
    err = np.full(len(ov), -1.0)
    conf, res = _B()._conf(dict(max_iterations=1)), _lib.BaResult()
    conf.solver = solver
    ctx = _lib.default_context(0)
    rc = ctx.lib.sfd2_bundle_adjust(ctx.h, views, n_views, vc.ctypes.data, xyz.ctypes.data, len(xyz), pc.ctypes.data, off.ctypes.data, ov.ctypes.data,
                                    xy.ctypes.data, ctypes.byref(conf), ctypes.byref(res), err.ctypes.data, 0)
    return rc, ctx.lib.sfd2_last_error().decode(), xyz, err


def test_refusals_say_why():
    from sfd2_amd import _lib
    B, P = _B(), br.scene("arc")
    rc, msg, xyz, err = _raw(P, _views(P), P.nv, 7)
    assert rc == -1 and "solver must be" in msg and xyz.tobytes() == P.X.tobytes() and (err == -1.0).all()
    with pytest.raises(ValueError, match="solver"):
        run(P, solver="cholesky")
    # one view too many: the six of 'arc' and unobserved ones up to the limit + 1
    n = _lib.BA_DENSE_MAX_VIEWS + 1
    views, few = (_lib.TriView * n)(), _views(P)
    for i in range(n):
        ctypes.memmove(ctypes.byref(views[i]), ctypes.byref(few[min(i, P.nv - 1)]), ctypes.sizeof(_lib.TriView))
    rc, msg, xyz, err = _raw(P, views, n, _lib.BA_SOLVER_DENSE)
    assert rc == -1 and "SFD2_BA_DENSE_MAX_VIEWS" in msg and str(n) in msg and xyz.tobytes() == P.X.tobytes() and (err == -1.0).all()
    rc, msg = _raw(P, views, n, _lib.BA_SOLVER_PCG)[:2]                      # the limit is the dense solver's alone
    assert rc == 0, msg
    # a pair list beyond 2^31 - 1 entries: one point seen 46 341 times by one view makes 46 341^2 ordered pairs; refused before it is built
    m = 46341
    assert m * m > 2 ** 31 - 1 > (m - 1) * (m - 1)
    conf, res = B._conf(dict(max_iterations=1)), _lib.BaResult()
    conf.solver = _lib.BA_SOLVER_DENSE
    one, ov, xy, off = np.array(P.X[:1]), np.zeros(m, np.int32), np.ascontiguousarray(np.repeat(P.obs_xy[:1], m, 0)), np.array([0, m], np.int64)
    vc, pc, err = np.array([1, 0], np.uint8), np.zeros(1, np.uint8), np.full(m, -1.0)
    ctx = _lib.default_context(0)
    args = (ctx.h, _views(P), 2, vc.ctypes.data, one.ctypes.data, 1, pc.ctypes.data, off.ctypes.data, ov.ctypes.data, xy.ctypes.data, ctypes.byref(conf),
            ctypes.byref(res), err.ctypes.data, 0)
    rc = ctx.lib.sfd2_bundle_adjust(*args)
    msg = ctx.lib.sfd2_last_error().decode()
    assert rc == -1 and "pair list" in msg and str(m * m) in msg and one.tobytes() == P.X[:1].tobytes() and (err == -1.0).all()
    conf.solver = _lib.BA_SOLVER_PCG                                         # the limit is the dense solver's alone
    assert ctx.lib.sfd2_bundle_adjust(*args) == 0, ctx.lib.sfd2_last_error().decode()
    # intrinsics among the unknowns: refused by the binding and by the library
    cams = [B.camera_model(c) for c in P.cams]
    with pytest.raises(ValueError, match="dense"):
        B.adjust_cameras([m for m, _ in cams], [p for _, p in cams], [_lib.BA_REFINE_FOCAL] * P.nv, np.arange(P.nv), _views(P), P.nv, P.vconst, P.X, P.pconst,
                         P.off, P.obs_view, P.obs_xy, solver="dense")
    arr = (_lib.BaCamera * P.nv)()
    for i, (m, p) in enumerate(cams):
        arr[i].model, arr[i].refine = int(m), _lib.BA_REFINE_FOCAL
        arr[i].params[:] = [float(v) for v in p]
    conf, res = B._conf({}), _lib.BaResult()
    conf.solver = _lib.BA_SOLVER_DENSE
    xyz, ov, xy, off = np.array(P.X), np.ascontiguousarray(P.obs_view, np.int32), np.ascontiguousarray(P.obs_xy), np.ascontiguousarray(P.off, np.int64)
    vc, pc, vcam, err = P.vconst.astype(np.uint8), P.pconst.astype(np.uint8), np.arange(P.nv, dtype=np.int32), np.full(len(ov), -1.0)
    ctx = _lib.default_context(0)
    rc = ctx.lib.sfd2_bundle_adjust_cameras(ctx.h, arr, P.nv, vcam.ctypes.data, _views(P), P.nv, vc.ctypes.data, xyz.ctypes.data, len(xyz), pc.ctypes.data,
                                            off.ctypes.data, ov.ctypes.data, xy.ctypes.data, ctypes.byref(conf), ctypes.byref(res), err.ctypes.data, 0)
    msg = ctx.lib.sfd2_last_error().decode()
    assert rc == -1 and "dense solver" in msg and "intrinsics" in msg and xyz.tobytes() == P.X.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 8. spd_solve
def _spd_raw(A, b, x):
    from sfd2_amd import _lib
    A, b = np.ascontiguousarray(A, np.float64), np.ascontiguousarray(b, np.float64)
    info = ctypes.c_int32(-5)
    ctx = _lib.default_context(0)
    rc = ctx.lib.sfd2_spd_solve(ctx.h, A.ctypes.data, len(b), b.ctypes.data, x.ctypes.data, ctypes.byref(info))
    return rc, info.value, ctx.lib.sfd2_last_error().decode()


@pytest.mark.parametrize("family", ["random", "ill"])
@pytest.mark.parametrize("n", dr.SPD_SIZES)
def test_spd_solve_is_as_backward_stable_as_numpy(n, family):
    A, b = dr.spd_system(n, family)
    x, info = _B().spd_solve(A, b)
    assert info == 0 and x.shape == (n,) and np.isfinite(x).all()
    got, want = dr.backward_error(A, x, b), dr.backward_error(A, np.linalg.solve(A, b), b)
    tol = min(10 * want, dr.higham_bound(n))
    print("spd_solve", family, n, "device %.3g numpy %.3g tolerance %.3g cond %.3g" % (got, want, tol, np.linalg.cond(A)))
    assert got <= tol
    lower = np.tril(A) + np.triu(np.full((n, n), np.nan), 1)                  # only the lower triangle is read
    again, info = _B().spd_solve(lower, b)
    assert info == 0 and again.tobytes() == x.tobytes()                        # and two calls give the same bytes


@pytest.mark.parametrize("k", dr.FAIL_AT)
def test_spd_solve_names_the_first_pivot_that_is_not_positive(k):
    A, b = dr.indefinite(k)
    assert (np.linalg.eigvalsh(A) < 0).sum() == 1
    if k > 1:
        np.linalg.cholesky(A[:k - 1, :k - 1])
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(A[:k, :k])
    x = np.full(dr.FAIL_N, 123.5)
    rc, info, _ = _spd_raw(A, b, x)
    assert rc == 0 and info == k and (x == 123.5).all()
    got, info = _B().spd_solve(A, b)
    assert got is None and info == k
    good, gb = dr.spd_system(dr.FAIL_N, "random")                              # the raised word does not outlive the call
    x, info = _B().spd_solve(good, gb)
    assert info == 0 and dr.backward_error(good, x, gb) <= dr.higham_bound(dr.FAIL_N)


def test_spd_solve_refuses_what_is_not_finite():
    A, b = dr.spd_system(65, "random")
    x = np.full(65, 123.5)
    for r, c in ((0, 0), (64, 3), (40, 40)):
        bad = A.copy()
        bad[r, c] = np.nan
        rc, info, msg = _spd_raw(bad, b, x)
        assert rc == -1 and "row %d" % r in msg and (x == 123.5).all()
    bb = b.copy()
    bb[7] = np.inf
    rc, info, msg = _spd_raw(A, bb, x)
    assert rc == -1 and "right-hand side" in msg and (x == 123.5).all()
    with pytest.raises(RuntimeError, match="non-finite"):
        _B().spd_solve(bad, b)
    with pytest.raises(ValueError):
        _B().spd_solve(A[:, :5], b)


# ---------------------------------------------------------------------------------------------------------------- 9. end to end
def test_reconstruction_with_the_dense_solver_against_the_pieces_started_from_the_truth():
    import mapper_ref as mr
    from sfd2_amd import bundle_adjustment as B, reconstruction as RC, triangulation as T
    from test_gpu_mapper import _scene
    sc, rep = _scene(), {}
    ims, pts = RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], report=rep, ba_solver="dense")
    assert sorted(ims) == list(range(1, 13)) and rep["final"]["n_registered"] == 12
    assert all(r["ba"]["solver"] == "dense" and r["ba"]["pcg_iterations"] == 0 for r in rep["rounds"]) and rep["final"]["ba"]["solver"] == "dense"
    y_ims, y_pts = T.triangulate_model(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"])
    y_ims, y_pts, _ = B.bundle_adjust(sc["cameras"], y_ims, y_pts, constant_images=list(rep["initial_pair"]), max_iterations=100, loss="cauchy",
                                      loss_scale=1.0)
    got, want = mr.model_errors(ims, pts, sc["images"]), mr.model_errors(y_ims, y_pts, sc["images"])
    ratios = {"points": got["points"] / want["points"], "mean_reproj": got["mean_reproj"] / want["mean_reproj"],
              "rotation": got["rotation"] / want["rotation"], "centre": got["centre"] / want["centre"]}
    print("mapper, dense", got, "yardstick", want, "ratios", {k: round(v, 3) for k, v in ratios.items()}, "rounds", len(rep["rounds"]),
          "final adjustment", rep["final"]["ba"])
    assert ratios["points"] >= 0.9 and ratios["mean_reproj"] <= 1.5 and ratios["rotation"] <= 3.0 and ratios["centre"] <= 3.0, ratios
