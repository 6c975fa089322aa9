"""What the four restatements share (tests/ransac_ref.py) on its own, on the CPU: the sampling on integers at every sample size, through
the names the estimators' modules bind it to (pose_ref.sample3, homography_ref.sample_k, two_view_ref.sample5, fundamental_ref.sample_k),
the trial rule in closed form at every sample size, the damped solve and the accept / reject loop.  The trial counts worked by hand
stay with each estimator's own host test, next to the committed cases they decide."""
import math

import numpy as np
import pytest

import fundamental_ref as fr
import homography_ref as hr
import pose_ref as pr
import ransac_ref as rr
import two_view_ref as tv

# sample size -> the scalar and the vectorised sampler as the estimator's module names them
BOUND = {3: (pr.sample3, pr.sample3v), 4: (hr.sample_k, hr.sample_kv), 5: (tv.sample5, tv.sample5v), 7: (fr.sample_k, fr.sample_kv)}
SIZES = sorted(BOUND)


def test_mix64_is_splitmix64():
    assert rr.mix64(0) == 0xE220A8397B1DCDAF and rr.mix64(1) == 0x910A2DEC89025CC1      # splitmix64's first outputs
    assert pr.mix64 is rr.mix64 and tv.mix64 is rr.mix64 and pr._mix64v is rr._mix64v
    z = [0, 1, 2 ** 63, 2 ** 64 - 1, 0xDEADBEEFCAFEF00D]
    assert rr._mix64v(np.array(z, dtype=np.uint64)).tolist() == [rr.mix64(v) for v in z]


@pytest.mark.parametrize("k", SIZES)
def test_sampling_on_integers(k):
    one, many = BOUND[k]
    for n in (k, k + 1, k + 2, 40, 300, 2 ** 31 - 1):
        for trial in (0, 1, 255, 256, 10 ** 9):
            s = one(12345, trial, n)
            assert s == rr.sample_k(12345, trial, n, k)
            assert len(set(s)) == k and all(0 <= i < n for i in s)
            assert tuple(many(12345, [trial], n)[0]) == s
    assert sorted(one(0, 0, k)) == list(range(k))
    assert one(0, 0, 40) != one(1, 0, 40) and one(0, 0, 40) != one(0, 1, 40)
    # every index is drawn about equally often: 20000 samples of k out of 2 k, 10000 each
    hist = np.bincount(many(3, np.arange(20000), 2 * k).ravel(), minlength=2 * k)
    assert hist.min() > 9500 and hist.max() < 10500


@pytest.mark.parametrize("k", SIZES)
def test_sampling_of_many_trials(k):
    one, many = BOUND[k]
    for n in (k, k + 1, k + 2, 257):
        for seed in (0, 0xDEADBEEFCAFEF00D):
            v = many(seed, np.arange(10000), n)
            assert v.dtype == np.int64 and v.shape == (10000, k) and v.min() >= 0 and v.max() < n
            assert all((v[:, a] != v[:, b]).all() for a in range(k) for b in range(a + 1, k))
            for i in range(0, 10000, 997):
                assert tuple(v[i]) == one(seed, i, n)
            if n > k:
                assert len({tuple(r) for r in v}) > min(1000, math.perm(n, k) // 2)       # and they do vary
    assert not np.array_equal(many(0, np.arange(64), 257), many(1, np.arange(64), 257))


def test_one_scheme_for_every_sample_size():
    """The first draws of a larger sample are the smaller sample: pose_ref.sample3, homography_ref.sample_k, two_view_ref.sample5 and
    fundamental_ref.sample_k are one sampler at four sizes."""
    assert fr.sample_k(3, 17, 40)[:5] == tv.sample5(3, 17, 40)
    assert tv.sample5(3, 17, 40)[:4] == hr.sample_k(3, 17, 40)
    assert hr.sample_k(3, 17, 40)[:3] == pr.sample3(3, 17, 40)
    assert fr.sample_k(3, 17, 40, 4) == hr.sample_k(3, 17, 40) and np.array_equal(fr.sample_kv(3, [17], 40, 4), hr.sample_kv(3, [17], 40))


@pytest.mark.parametrize("k", SIZES)
def test_seeds_are_64_bits_without_a_sign(k):
    one, many = BOUND[k]
    for n in (k, 60, 4096):
        for trial in (0, 255, 256, 10 ** 9):
            for seed in tv.SEED_RUNS:
                assert tuple(many(seed, [trial], n)[0]) == one(seed, trial, n)
            assert one(-1, trial, n) == one(2 ** 64 - 1, trial, n) == tuple(many(-1, [trial], n)[0])
    # the top bit reaches the draw
    assert one(2 ** 63, 0, 60) != one(0, 0, 60) and one(2 ** 64 - 1, 0, 60) != one(2 ** 63 - 1, 0, 60)


@pytest.mark.parametrize("k,mod", [(3, pr), (4, hr), (5, tv), (7, fr)])
def test_trial_rule_in_closed_form(k, mod):
    for ratio in (0.2, 0.3, 0.5, 0.7):
        for conf in (0.5, 0.99, 0.999, 0.9999):
            for mult in (3.0, 2.0):
                want = np.ceil(np.log(1 - conf) / np.log(1 - ratio ** k) * mult)
                assert rr.num_trials_needed(ratio, conf, k, mult) == mod.num_trials_needed(ratio, conf, mult) == want
            assert mod.num_trials_needed(ratio, conf) == rr.num_trials_needed(ratio, conf, k)
    # an inlier ratio of 1: one trial; of 0, or a confidence of 1: no number of trials is enough
    assert rr.num_trials_needed(1.0, 0.999, k) == 1.0 and rr.num_trials_needed(0.0, 0.999, k) == np.inf
    assert rr.num_trials_needed(0.5, 1.0, k) == np.inf and rr.num_trials_needed(1e-6, 0.999, k) == np.inf
    need = int(rr.num_trials_needed(0.5, 0.99, k))
    assert rr.trial_limits(0.5, 0, 10 ** 6, 0.99, k) == mod.trial_limits(0.5, 0, 10 ** 6, 0.99) == (0, need)
    assert rr.trial_limits(0.5000099, 0, 10 ** 6, 0.99, k) == (0, need)                  # floored to 1e-5 steps
    assert rr.trial_limits(0.50001, 0, 10 ** 6, 0.99, k)[1] <= need
    assert rr.trial_limits(0.5, 10 ** 6, 10 ** 6, 0.99, k) == (need, need)               # min_num_trials clamped to the limit
    assert rr.trial_limits(0.5, 7, need - 1, 0.99, k) == (7, need - 1)
    assert rr.trial_limits(0.0, 0, 10000, 0.999, k) == (0, 10000) and rr.trial_limits(0.5, 0, 10000, 1.0, k) == (0, 10000)
    assert rr.trial_limits(1.0, 5, 10000, 0.999, k) == (1, 1) and rr.trial_limits(0.5, 0, 10000, 0.0, k) == (0, 1)
    assert rr.trial_limits(0.5, 0, 10 ** 6, 0.99, k, 2.0) == (0, int(rr.num_trials_needed(0.5, 0.99, k, 2.0)))


def test_damped_solve_and_the_accept_reject_loop():
    rs = np.random.RandomState(3)
    for n in (5, 7, 8):
        J = rs.standard_normal((3 * n, n))
        H, g = J.T @ J, rs.standard_normal(n)
        for lam in (0.0, 1e-4, 10.0):
            d, ok = rr.damped_solve(H, g, lam)
            A = H + np.diag(lam * np.diag(H) + 1e-15 * np.diag(H).max())
            assert ok and d.shape == (n,) and np.allclose(A @ d, -g, rtol=0, atol=1e-10)
        bad = H.copy()
        bad[0, 0] = np.nan
        for Hb, gb in ((bad, g), (np.zeros((n, n)), g), (-H, g), (H, g * np.inf)):
            d, ok = rr.damped_solve(Hb, gb)
            assert not ok and d.shape == (n,) and not d.any()
    # a linear least-squares problem: the loop ends at its solution, with the system it stands on
    A, b = rs.standard_normal((12, 4)), rs.standard_normal(12)

    def system(x):
        r = A @ x - b
        return A.T @ A, A.T @ r, float(r @ r)
    x, H, g = rr.levenberg_marquardt(np.zeros(4), system, rr.damped_solve, lambda x, d: x + d, 50)
    assert np.allclose(x, np.linalg.lstsq(A, b, rcond=None)[0], rtol=0, atol=1e-9) and np.array_equal(H, A.T @ A)
    assert np.array_equal(g, A.T @ (A @ x - b)) and np.linalg.norm(g) <= 1e-9
    # no step that raises the cost is taken, and a system that cannot be solved ends the loop where it stands
    x0 = np.ones(4)
    assert rr.levenberg_marquardt(x0, system, lambda H, g, lam: (np.full(4, 1e3), True), lambda x, d: x + d, 50)[0] is x0
    assert rr.levenberg_marquardt(x0, system, lambda H, g, lam: (np.zeros(4), False), lambda x, d: x + d, 50)[0] is x0
