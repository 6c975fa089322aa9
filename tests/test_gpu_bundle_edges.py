"""Bundle adjustment on the MI355X, the seams of its launch decomposition: more than 1024 views (the second pass of the one-workgroup PCG
kernels, a second partial of the view gradient's reduction), more than 2^19 observations (the second pass of the final reduction), the
function tolerance, runs that accept nothing, tracks of 0 and 1 observations, a fixed pattern of rejected steps, scratch reuse.

The scenes, the two structured reference solvers (bundle_ref.lm_blocks, bundle_ref.arrow_step) and every floor are in tests/bundle_ref.py,
measured and checked on the CPU by tests/test_bundle_host.py (FLOORS, PCG, SUMS).  Tolerances are 10 x the floor, ceiling 1e-6, as in
tests/test_gpu_bundle.py; two kinds of floor are new.  For the scenes of clusters the floor is the larger of the two routes' disagreement
and of what a PCG residual of 1e-14 does to the restatement's step (bundle_ref.pcg_allowance).  For the cost and the gradient maximum of
the 'wide' scenes it is the larger of the fp64 restatement's distance from numpy.longdouble / math.fsum and 32 x 2^-53, the bound of a
summation tree as deep as the device's (bundle_ref.sum_floors).

Measured on the MI355X against them (the device's figure, then the tolerance):
  'clusters', one step         step 3.1e-12 of its norm (3.8e-11), largest entry 3.1e-13; cost 1.7e-16, max |g| 2.6e-13; 27 PCG iterations
  'clusters', two steps        state 2.3e-14 of the scene's size (4.3e-12), final cost 1.3e-16
  'clusters_point_max'         step 1.9e-12 (1.9e-11), max |g| 9.9e-14, final cost 5.6e-14
  'wide', 'wide_first'         cost 0 and 1.5e-16, max |g| 2.1e-16 and 0 (3.6e-14 both); step 2.2e-12 (2.2e-11), final cost 4.4e-15
  function tolerance           state 1.2e-14 (1.2e-13), cost 5.7e-15; 3 iterations on both sides
  'short_tracks'               state 3.5e-14, forced wave mapping 3.8e-14 (2.4e-13)
  'reject_first'               state 1.1e-11 (1.0e-10), cost 1.7e-12; accept, three rejections, accept on both sides, lambda equal
Wall time per test on the MI355X with the shared references computed once: the 'wide' step 3.4 s and the first 'clusters' case 2.8 s (the
references: arrow_step by both routes, lm_blocks by both routes), the two 'wide' starts 1.2 s each, everything else under 0.1 s; the file
10 s.  No defect was found: every test passed against the unmodified library at once.

Mutation check (three in-bounds mutants of the library, built apart and never committed; tests/test_gpu_bundle.py passes all three):
  ba_pcg_step_kernel's view loop as a single pass    test_more_than_1024_views[clusters-1], [clusters-2] fail
  ba_reduce_final_kernel reads 256 partials only     both test_more_than_2_19_observations_at_the_start cases and ..._one_step fail
  SFD2_BA_ST_FUNCTION never set                      test_function_tolerance_stops_where_the_restatement_stops fails
"""
import numpy as np
import pytest

import bundle_ref as br
from test_gpu_bundle import TIGHT, _B, _constants_untouched, _pose_words, _same_bytes, _views, run

pytestmark = pytest.mark.gpu

CONVERGED = dict(pcg_tolerance=1e-6, pcg_max_iterations=500)


def _rel(a, b):
    return abs(a - b) / abs(b)


def _words(P):
    return np.concatenate([P.q, P.t], 1)


def _norm(step):
    return np.sqrt((step[0] ** 2).sum() + (step[1] ** 2).sum())


def _check_step(P, out, want, tol):
    """The device's step against the restatement's: every entry within tol of the step's norm, and the whole in norm."""
    step = br.step_between(P, out["state"])
    figures = {"entry": max(np.abs(step[0] - want[0]).max(), np.abs(step[1] - want[1]).max()) / _norm(want), "norm": br.step_diff(step, want)}
    print("step:", figures, "tol", tol)
    assert figures["entry"] <= tol and figures["norm"] <= tol


# ---------------------------------------------------------------------------------------------------------------- 1. more than 1024 views
@pytest.mark.parametrize("name,steps", [("clusters", 1), ("clusters", 2), ("clusters_point_max", 0), ("clusters_point_max", 1)])
def test_more_than_1024_views(name, steps):
    P, ref = br.scene(name), br.solution(name, br.ROUTE_A, **br.CLUSTER_RUNS[name])
    tol = br.step_tolerance(name)
    assert P.nv == 1030
    out = run(P, max_iterations=steps, initial_lambda=1e-4, **TIGHT)
    rep = out["report"]
    gmax = rep["gradient_max"] if steps == 0 else run(P, max_iterations=0)["report"]["gradient_max"]
    figures = {"tol": tol, "cost": _rel(rep["initial_cost"], ref["initial_cost"]), "gmax": _rel(gmax, ref["initial_gmax"]), "pcg": rep["pcg_iterations"]}
    print(name, steps, figures, rep)
    assert rep["iterations"] == rep["accepted_steps"] == steps <= ref["accepted"]
    assert figures["cost"] <= tol and figures["gmax"] <= tol
    _constants_untouched(P, out)
    if steps == 0:
        assert out["words"].tobytes() == _words(P).tobytes() and out["xyz"].tobytes() == P.X.tobytes() and rep["final_cost"] == rep["initial_cost"]
    elif steps == 1:
        _check_step(P, out, ref["first_step"], tol)
        trial = ref["history"][0][1]
        print("final cost:", _rel(rep["final_cost"], trial))
        assert _rel(rep["final_cost"], trial) <= tol
    else:
        stol = br.tolerance(name, **br.CLUSTER_RUNS[name])
        figures = {"tol": stol, "state": br.state_diff(out["state"], ref["state"]), "cost": _rel(rep["final_cost"], ref["cost"])}
        print("two steps:", figures)
        assert steps == ref["accepted"] == ref["iterations"] and figures["state"] <= stol and figures["cost"] <= stol


# ---------------------------------------------------------------------------------------------------------------- 2. more than 2^19 observations
@pytest.mark.parametrize("name", ["wide", "wide_first"])
def test_more_than_2_19_observations_at_the_start(name):
    P = br.scene(name)
    cost, gmax = br.start(name)
    fc, fg = br.sum_floors(name)[:2]
    out = run(P, max_iterations=0)
    rep = out["report"]
    figures = {"cost": _rel(rep["initial_cost"], cost), "tol_cost": 10 * fc, "gmax": _rel(rep["gradient_max"], gmax), "tol_gmax": 10 * fg}
    print(name, figures, rep)
    assert len(P.obs_view) > 256 * 2048 and rep["iterations"] == rep["accepted_steps"] == 0 and rep["final_cost"] == rep["initial_cost"]
    assert figures["cost"] <= 10 * fc and figures["gmax"] <= 10 * fg
    r, _ = br.residuals(P, P.state())
    assert np.abs(np.linalg.norm(r, axis=1) - out["err"]).max() <= 1e-9
    assert out["xyz"].tobytes() == P.X.tobytes() and out["words"].tobytes() == _words(P).tobytes()


def test_more_than_2_19_observations_one_step():
    P, tol = br.scene("wide"), br.step_tolerance("wide")
    want = br.first_steps("wide")[0]
    out = run(P, max_iterations=1, initial_lambda=1e-4, **TIGHT)
    rep = out["report"]
    trial = br.cost(P, br.apply_split(P.state(), want))
    figures = {"tol": tol, "cost": _rel(rep["initial_cost"], br.start("wide")[0]), "final": _rel(rep["final_cost"], trial), "pcg": rep["pcg_iterations"]}
    print("wide", figures, rep)
    assert rep["iterations"] == rep["accepted_steps"] == 1
    _check_step(P, out, want, tol)
    assert figures["final"] <= tol and figures["cost"] <= 10 * br.sum_floors("wide")[0]
    _constants_untouched(P, out)


# ---------------------------------------------------------------------------------------------------------------- 3. function tolerance
def test_function_tolerance_stops_where_the_restatement_stops():
    kw = dict(function_tolerance=1e-6, max_iterations=100)     # a fixed number of steps (test_bundle_host.py: no decision is close): no near-tie radius
    P, ref, tol = br.scene("arc"), br.solution("arc", **kw), br.tolerance("arc", **kw)
    out = run(P, function_tolerance=1e-6, **TIGHT)
    rep = out["report"]
    figures = {"tol": tol, "state": br.state_diff(out["state"], ref["state"]), "cost": _rel(rep["final_cost"], ref["cost"])}
    print("function tolerance", figures, rep)
    assert ref["status"] == "function_tolerance" and rep["status"] == "function_tolerance"
    assert rep["iterations"] == ref["iterations"] == 3 and rep["accepted_steps"] == ref["accepted"] == 3
    assert figures["state"] <= tol and figures["cost"] <= tol
    _constants_untouched(P, out)


# ---------------------------------------------------------------------------------------------------------------- 4. nothing accepted
def _run_with_quaternions(P, q, **options):
    views = _views(P, q=q)
    xyz, err, report = _B().adjust(views, P.nv, P.vconst, P.X, P.pconst, P.off, P.obs_view, P.obs_xy, **options)
    return {"words": _pose_words(views, P.nv), "xyz": xyz, "err": err, "report": report}


def test_nothing_accepted_nothing_changed():
    P = br.scene("arc")
    unit, twice = _run_with_quaternions(P, P.q, max_iterations=0), _run_with_quaternions(P, 2 * P.q, max_iterations=0)
    assert unit["report"]["iterations"] == unit["report"]["accepted_steps"] == 0 and unit["report"]["status"] == "max_iterations"
    assert unit["words"].tobytes() == _words(P).tobytes() and unit["xyz"].tobytes() == P.X.tobytes()
    # a non-unit quaternion is normalised for the computation (the division by 2 is exact) and returned as it came
    assert twice["words"].tobytes() == np.concatenate([2 * P.q, P.t], 1).tobytes() and twice["xyz"].tobytes() == P.X.tobytes()
    assert twice["report"] == unit["report"] and twice["err"].tobytes() == unit["err"].tobytes()
    unit, twice = _run_with_quaternions(P, P.q, max_iterations=1, **TIGHT), _run_with_quaternions(P, 2 * P.q, max_iterations=1, **TIGHT)
    assert unit["report"]["accepted_steps"] == 1 and twice["report"] == unit["report"]
    assert twice["xyz"].tobytes() == unit["xyz"].tobytes() and twice["err"].tobytes() == unit["err"].tobytes()
    assert twice["words"][~P.vconst].tobytes() == unit["words"][~P.vconst].tobytes()              # an adjusted view: unit words
    assert np.abs(np.linalg.norm(unit["words"][~P.vconst, :4], axis=1) - 1).max() < 1e-12
    assert twice["words"][P.vconst].tobytes() == np.concatenate([2 * P.q, P.t], 1)[P.vconst].tobytes()      # a constant one: as it came
    assert unit["words"][~P.vconst].tobytes() != _words(P)[~P.vconst].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 5. short tracks
@pytest.mark.parametrize("flags", [0, 1, 2], ids=["by_length", "lane", "wave"])
def test_tracks_of_no_and_one_observation(flags):
    """bundle_adjustment.adjust accepts repeated offsets, so the scene goes through the ordinary call."""
    P, ref, tol = br.scene("short_tracks"), br.solution("short_tracks", max_iterations=2), br.tolerance("short_tracks", max_iterations=2)
    assert np.diff(P.off)[list(br.SHORT_AT)].tolist() == [1, 0] * 4
    out = run(P, flags=flags, max_iterations=2, **TIGHT)
    rep = out["report"]
    figures = {"tol": tol, "state": br.state_diff(out["state"], ref["state"]), "cost": _rel(rep["final_cost"], ref["cost"])}
    print("short tracks", flags, figures, rep)
    assert rep["accepted_steps"] == ref["accepted"] == 2
    assert figures["state"] <= tol and figures["cost"] <= tol
    never, once = list(br.SHORT_AT[1::2]), list(br.SHORT_AT[::2])
    assert out["xyz"][never].tobytes() == P.X[never].tobytes()
    assert np.abs(out["xyz"][once] - ref["state"][2][once]).max() <= tol * br.SCALE and np.abs(out["xyz"][once] - P.X[once]).max() > 1e-3
    _constants_untouched(P, out)


# ---------------------------------------------------------------------------------------------------------------- 6. rejections
def test_rejected_steps_follow_the_restatement():
    P, ref, tol = br.scene("reject_first"), br.solution("reject_first", **br.REJECT_FIRST), br.tolerance("reject_first", **br.REJECT_FIRST)
    assert [ok for _, _, ok, _ in br.lm_blocks([P], br.ROUTE_A, **br.REJECT_FIRST)["history"]] == [True, False, False, False, True]
    out = run(P, **br.REJECT_FIRST, **TIGHT)
    rep = out["report"]
    figures = {"tol": tol, "state": br.state_diff(out["state"], ref["state"]), "cost": _rel(rep["final_cost"], ref["cost"])}
    print("rejections", figures, rep)
    assert (rep["iterations"], rep["accepted_steps"], rep["lambda"], rep["status"]) == (ref["iterations"], ref["accepted"], ref["lambda"], "max_iterations")
    assert rep["iterations"] == 5 and rep["accepted_steps"] == 2
    assert figures["state"] <= tol and figures["cost"] <= tol
    r, _ = br.residuals(P, out["state"])
    assert np.abs(np.linalg.norm(r, axis=1) - out["err"]).max() <= 1e-9       # the records behind a rejected step are the accepted state's
    _constants_untouched(P, out)
    for batch in (1, 64):
        assert _same_bytes(out, run(P, pcg_batch=batch, **br.REJECT_FIRST, **TIGHT)), batch


# ---------------------------------------------------------------------------------------------------------------- 7. scratch reuse
def test_a_small_problem_after_a_large_one_gives_the_same_bytes():
    arc, clusters, wide = br.scene("arc"), br.scene("clusters"), br.scene("wide")
    first = [run(arc, **CONVERGED), run(clusters, max_iterations=1, **TIGHT), run(wide, max_iterations=0)]
    again = [run(arc, **CONVERGED), run(clusters, max_iterations=1, **TIGHT), run(wide, max_iterations=0)]
    assert first[0]["report"]["accepted_steps"] >= 3
    for a, b, name in zip(first, again, ("arc", "clusters", "wide")):
        assert _same_bytes(a, b), name
