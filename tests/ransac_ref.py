"""What the numpy restatements of the four RANSAC estimators share (pose_ref, two_view_ref, fundamental_ref, homography_ref; for the
tests only, never imported by the product), as the device side shares ransac_math.h and ransac_common.h: the sampling on integers,
COLMAP's trial count and trial limits, the damped solve of the normal equations, the accept / reject skeleton of the final
Levenberg-Marquardt, and the one LO-RANSAC round loop of the two-view estimators E, F and H.  pose_ref.lo_ransac_ref stays a loop
of its own (fp32 scoring, hypotheses keyed by trial * 4 + root, its own records); it takes the sampler and the trial rule from here.

What an estimator adds to the round loop is a Model (below).  Three of its fields record differences between the E, F and H loops
as they were found when the loops were merged, and are NOT endorsed by being written down here: `exact_needs_all` (E calls a winner
exact only when it holds all n points), `carries_exact` (H keeps exact fits across rounds in 'either' where E and F report a "tie")
and `near_any_sample` (H reports "near" once per round for any sample, E and F for the winner's sample only).  Whether E and F should
follow H is a question of behaviour for a change of its own."""
import contextlib
from typing import Callable, NamedTuple

import numpy as np

ROUND = 256                  # trials per round
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------------ sampling
def mix64(z):
    """splitmix64's output function on a Python int (mod 2^64)."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _mix64v(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sample_k(seed, trial, n, k):
    """k distinct indices in [0, n) from (seed, trial) only, on Python ints: h_0 = mix64(seed ^ mix64(trial)), h_i = mix64(h_i-1);
    draw i is h_i mod (n - i), stepped over the earlier indices in ascending order."""
    h = mix64((seed & _M64) ^ mix64(trial & _M64))
    out = []
    for i in range(k):
        if i:
            h = mix64(h)
        v = h % (n - i)
        for c in sorted(out):
            if v >= c:
                v += 1
        out.append(v)
    return tuple(out)


def sample_kv(seed, trials, n, k):
    """sample_k for an array of trials (np.uint64 arithmetic): int64 [T, k]."""
    t = np.asarray(trials, dtype=np.int64).astype(np.uint64)
    h = _mix64v(np.uint64(seed & _M64) ^ _mix64v(t))
    cols = []
    for i in range(k):
        if i:
            h = _mix64v(h)
        v = (h % np.uint64(n - i)).astype(np.int64)
        if cols:
            srt = np.sort(np.stack(cols, 1), axis=1)
            for p in range(i):
                v = v + (v >= srt[:, p])
        cols.append(v)
    return np.stack(cols, 1)


# ------------------------------------------------------------------------------------------------------------ the trial rule
def num_trials_needed(inlier_ratio, confidence, sample_size, multiplier=3.0):
    """COLMAP's ComputeNumTrials: ceil(multiplier * log(1 - confidence) / log(1 - ratio^sample_size))."""
    nom = 1.0 - confidence
    if nom <= 0:
        return np.inf
    den = 1.0 - inlier_ratio ** sample_size
    if den <= 0:
        return 1.0
    if den == 1.0 or abs(np.log(den)) < 1e-16:
        return np.inf
    return float(np.ceil(np.log(nom) / np.log(den) * multiplier))


def trial_limits(min_inlier_ratio, min_num_trials, max_num_trials, confidence, sample_size, multiplier=3.0):
    """(min_trials, max_trials): max_num_trials limited by the trial count of min_inlier_ratio floored to 1e-5 steps (COLMAP's
    RANSAC), at least 1; min_num_trials clamped to it."""
    dyn = num_trials_needed(np.floor(min_inlier_ratio * 100000) / 100000.0, confidence, sample_size, multiplier)
    mx = int(max(1, min(float(max_num_trials), dyn)))
    return min(int(min_num_trials), mx), mx


def trial_rule(sample_size):
    """(num_trials_needed, trial_limits) of one sample size, with the signatures the estimators' modules have always had."""
    return (lambda inlier_ratio, confidence, multiplier=3.0: num_trials_needed(inlier_ratio, confidence, sample_size, multiplier),
            lambda min_inlier_ratio, min_num_trials, max_num_trials, confidence, multiplier=3.0:
            trial_limits(min_inlier_ratio, min_num_trials, max_num_trials, confidence, sample_size, multiplier))


def make_cached():
    """A module's memo: cached(key, make) calls make() once per key."""
    cache = {}

    def cached(key, make):
        if key not in cache:
            cache[key] = make()
        return cache[key]
    return cached


# ------------------------------------------------------------------------------------------------------------ refinement
def damped_solve(H, g, lam=0.0):
    """d of (H + lam diag H + 1e-15 max diag H) d = -g, and whether the system was positive definite and finite."""
    dg = np.diag(H)
    if not (np.isfinite(H).all() and np.isfinite(g).all() and dg.max() > 0):
        return np.zeros(len(g)), False
    A = H + np.diag(lam * dg + 1e-15 * dg.max())
    if not np.linalg.eigvalsh(A)[0] > 0:
        return np.zeros(len(g)), False
    d = -np.linalg.solve(A, g)
    return d, bool(np.isfinite(d).all())


def levenberg_marquardt(state, normal_equations, solve, apply_update, iters):
    """The final refinement's accept / reject loop: lambda from 1e-4, x 0.1 (down to 1e-12) after a step that does not raise the cost,
    x 10 after one that does; it ends after iters steps, when a system cannot be solved, when lambda passes 1e12 or when a step is
    shorter than 1e-13.  normal_equations(state) -> (J^T J, J^T r, r^T r), solve(H, g, lam) -> (d, ok), apply_update(state, d) -> state.
    Returns (state, H, g) at the end point."""
    H, g, c = normal_equations(state)
    lam = 1e-4
    for _ in range(iters):
        d, ok = solve(H, g, lam)
        if not ok:
            break
        new = apply_update(state, d)
        Hn, gn, cn = normal_equations(new)
        step = float(np.sum(d * d))
        if np.isfinite(cn) and cn <= c:
            state, H, g, c = new, Hn, gn, cn
            lam = max(lam * 0.1, 1e-12)
            if step < 1e-26:
                break
        else:
            lam *= 10.0
            if lam > 1e12 or step < 1e-26:
                break
    return state, H, g


# ------------------------------------------------------------------------------------------------------------ LO-RANSAC
class Model(NamedTuple):
    """What a two-view estimator adds to lo_ransac.  M stands for its 3 x 3 matrix, x0 / x1 [n, 2] for the normalised points."""
    name: str                    # the key of the best matrix in the result: 'E', 'F' or 'H'
    sample_size: int
    solver: Callable             # (x0 [T, k, 2], x1 [T, k, 2]) -> (M [K, 3, 3], owner [K] = row of the sample, near [T], ...); takes
    #                              drop_root=True where the estimator's host test breaks that rule
    support: Callable            # (M [..., 3, 3], x0, x1, th2) -> (count, sum of the inliers' errors, ..., errors): E and F give the mask third
    error: Callable              # (M, x0, x1) -> squared errors [n]
    distinct: Callable           # (Ma, Mb) -> two contenders are not the same hypothesis
    band: float                  # the module's BAND: relative half-width around the threshold, and of "equal" sums
    exact_sum: float             # the module's EXACT_SUM: a sum below it is an exact fit's (rounding only)
    lo_steps: int                # re-estimations per improvement
    lo_start: Callable           # (M) -> what the local optimisation carries from step to step, made once when a hypothesis wins: E
    #                              decomposes here and carries (R, t); F and H carry nothing and build a chart from the best at every step
    lo_step: Callable            # (carried, M best, weights [n] 0 / 1, x0, x1) -> (carried, M re-estimated), None when a system fails
    rule_breaks: tuple = ()      # which of drop_root / dead_lanes the estimator's host test uses (dead_lanes: E only)
    nan_errors: bool = False     # H: an error may be NaN (a point on the vanishing line), and is then no inlier and in no band
    # the three differences recorded as found (module docstring)
    exact_needs_all: bool = False    # E: a winner is exact only with cnt == n as well as sum < exact_sum; F and H: the sum alone
    carries_exact: bool = False      # H: an exact best replaced by an exact winner of as many points stays in 'either', and later
    #                                  rounds' exact fits of as many points join it; E and F: "tie"
    near_any_sample: bool = False    # H: "near" once per round when any sample is near; E and F: for the winner's sample only


def lo_ransac(model, x0, x1, th2, min_inlier_ratio=0.25, min_num_trials=0, max_num_trials=10000, confidence=0.999, seed=0, multiplier=3.0,
              lo=True, smaller_sum=True, drop_root=False, dead_lanes=False, solver=None):
    """The rounds on normalised points.  Returns {model.name: the best matrix (None without a hypothesis), 'cnt', 'sum', 'trials',
    'banded', 'why' (the reasons), 'either' (the other matrices that fit their points to rounding as the best one does)}.
    multiplier, lo, smaller_sum, drop_root, dead_lanes (a partial round runs all its 256 trials): the rule breaks of the host tests;
    solver: another route to the same hypotheses."""
    for name, on in (("drop_root", drop_root), ("dead_lanes", dead_lanes)):
        if on and name not in model.rule_breaks:
            raise TypeError(f"lo_ransac: the {model.name} estimator has no rule break {name!r}")
    solver = solver or model.solver
    quiet = (lambda: np.errstate(invalid="ignore")) if model.nan_errors else contextlib.nullcontext

    def in_band(e, rel=model.band):
        with quiet():
            return bool(np.any(np.abs(e - th2) <= rel * th2))

    def close(a, b):
        """Two sums of squared errors are too close to order: within the band of each other, or both an exact fit's."""
        return abs(a - b) <= model.band * max(abs(a), abs(b)) or max(abs(a), abs(b)) < model.exact_sum

    n = len(x0)
    mn, mx = trial_limits(min_inlier_ratio, min_num_trials, max_num_trials, confidence, model.sample_size, multiplier)
    best, bM, why, trials, rnd = (-1, 0.0, np.inf), None, [], 0, 0
    either = []
    sg = 1.0 if smaller_sum else -1.0
    while True:
        tr = np.arange(rnd * ROUND, (rnd + 1) * ROUND if dead_lanes else min((rnd + 1) * ROUND, mx))
        idx = sample_kv(seed, tr, n, model.sample_size)
        Ms, owner, near = (solver(x0[idx], x1[idx], drop_root=True) if drop_root else solver(x0[idx], x1[idx]))[:3]
        if model.near_any_sample and near.any():       # a sample too close to a degeneracy threshold may or may not give a hypothesis
            why.append("near")
        if len(Ms):
            cnt, sm, *_, err = model.support(Ms, x0, x1, th2)
            # np.lexsort is stable: the last key changes nothing, it says so
            order = np.lexsort((np.arange(len(Ms)), tr[owner], sg * sm, -cnt))
            w = order[0]
            win = (int(cnt[w]), float(sm[w]), int(tr[owner[w]]))
            if (win[0], -sg * win[1], -win[2]) > (best[0], -sg * best[1], -best[2]):
                rivals = [k for k in order[1:] if cnt[k] == cnt[w] and close(sm[k], sm[w]) and model.distinct(Ms[k], Ms[w])]
                # A winner that fits its points to rounding (n = sample size: each of the sample's solutions does; one wrong match
                # more: every sample without it does; E on a planar scene: both plane-consistent matrices do) is ordered among its
                # like by rounding alone.  Those rivals are not a reason to leave the case out: they are reported, and any one of
                # them is a right answer.  carries_exact: the same across rounds, for an exact best that an exact winner replaces.
                exact = win[1] < model.exact_sum and (win[0] == n or not model.exact_needs_all)
                carried = model.carries_exact and exact and best[0] == win[0] and best[1] < model.exact_sum
                either = [Mo for Mo in [bM] + either if model.distinct(Mo, Ms[w])] if carried else []
                for k in rivals if exact else []:
                    if all(model.distinct(Ms[k], Mo) for Mo in either):
                        either.append(Ms[k])
                why += ["rival"] * int(bool(rivals) and not exact) + ["threshold"] * int(in_band(err[w]))
                why += ["near"] * int(not model.near_any_sample and near[owner[w]])
                why += ["tie"] * int(best[0] == win[0] and close(best[1], win[1]) and not carried)
                best, bM = win, Ms[w]
                carry = model.lo_start(bM) if lo else None
                for _ in range(model.lo_steps if lo else 0):
                    with quiet():
                        inl = (model.error(bM, x0, x1) <= th2).astype(np.float64)
                    step = model.lo_step(carry, bM, inl, x0, x1)
                    if step is None:
                        break
                    carry, Mn = step
                    c, s, *_, e = model.support(Mn, x0, x1, th2)
                    # A re-estimate that ties with its predecessor (the local optimisation has converged: same count, sums within the
                    # band) may be accepted or not; the two matrices differ by the last step only, which matters when a point is
                    # within 1e-3 of the threshold.
                    tie = int(c) == best[0] and close(float(s), best[1]) and model.distinct(Mn, bM) and in_band(e, 1e-3)
                    why += ["lo threshold"] * int(in_band(e)) + ["lo tie"] * int(tie)
                    if not (c > best[0] or (c == best[0] and sg * s < sg * best[1])):
                        break
                    best, bM = (int(c), float(s), best[2]), Mn
            elif win[0] == best[0] and close(win[1], best[1]) and model.distinct(Ms[w], bM):
                if model.carries_exact and win[1] < model.exact_sum and best[1] < model.exact_sum:
                    for k in order:                    # exact fits of as many points in a later round
                        if cnt[k] == cnt[w] and sm[k] < model.exact_sum and all(model.distinct(Ms[k], Mo) for Mo in [bM] + either):
                            either.append(Ms[k])
                else:
                    why.append("tie")
        trials = min((rnd + 1) * ROUND, mx)
        if trials >= mx:
            break
        if trials >= mn and best[0] > 0 and trials >= num_trials_needed(best[0] / n, confidence, model.sample_size, multiplier):
            break
        rnd += 1
    return {model.name: bM, "cnt": best[0], "sum": best[1], "trials": trials, "banded": bool(why), "why": why, "either": either}
