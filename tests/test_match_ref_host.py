"""tests/match_ref.py checked on its own, without a GPU and without the library: against the oracle on the planted sets,
against every matcher entry of the committed reference results, and the guard conditions of tests/test_gpu_match_top2.py
(share of safe rows, share of planted rows that depend on the second best) for every size that file uses."""
import os

import numpy as np
import pytest

import match_ref as mr
import test_gpu_match_top2 as cases
from oracle import oracle as orc

HLOC_CONFS = {          # the configurations behind tests/golden/matchers.npz (tests/test_gpu_parity.py)
    "NNM": ("hloc", None, None, True),
    "ONN": ("hloc", None, None, False),
    "NNR": ("hloc", None, 0.9, True),
    "RATIO": ("hloc", 0.8, None, True),
    "RATIO_DIST": ("hloc", 0.9, 0.7, False),
}
ITLOC_CONFS = {"NNM": ("nnm", None, None, True), "NNR": ("nnr", 0.9, None, True)}


def _oracle(mode, d0, d1):
    kind, ratio, dist, mutual = mode
    if kind == "hloc":
        return orc.hloc_nearest_neighbor(d0, d1, ratio_threshold=ratio, distance_threshold=dist, do_mutual_check=mutual)
    return orc.itloc_matcher(d0, d1, kind, ratio if ratio else 0.9)


@pytest.mark.parametrize("n0,n1", cases.STRADDLE_SIZES)
def test_match_ref_equals_the_oracle_on_the_planted_sets(n0, n1):
    """The oracle's hloc matcher works on fp32 similarities (1e-7), its it_loc matcher on fp64 ones: rows decided by more
    than 1e-6 are identical, scores agree to 1e-6."""
    for swap in (False, True):
        d0, d1, rows, sim = cases.straddle_set(n0, n1, swap)
        modes = dict(cases.STRADDLE_MODES, NNM=HLOC_CONFS["NNM"], ONN=HLOC_CONFS["ONN"], it_nnm=ITLOC_CONFS["NNM"])
        for name, mode in modes.items():
            m, s = cases.ref(mode, d0, d1, sim=sim)
            want = _oracle(mode, d0, d1)
            safe = cases.safe_rows(mode, d0, d1, 1e-6, sim=sim)
            assert safe.mean() > 0.99
            np.testing.assert_array_equal(m[safe], want["matches0"][safe], err_msg=name)
            same = m == want["matches0"]
            np.testing.assert_allclose(s[same], want["matching_scores0"][same], atol=1e-6, err_msg=name)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_match_ref_equals_the_reference_results(golden_dir, tag):
    """tests/golden/matchers.npz: results of the reference's own matchers (fp32 similarities).  Exact on the rows that
    margins calls safe at 1e-6."""
    g = np.load(os.path.join(golden_dir, "matchers.npz"), allow_pickle=False)
    d0, d1 = g[f"{tag}/d0"], g[f"{tag}/d1"]
    sim = mr.similarity(d0, d1)
    n = 0
    for fam, confs in (("hloc", HLOC_CONFS), ("itloc", ITLOC_CONFS)):
        for name, mode in confs.items():
            gm, gs = g[f"{tag}/{fam}/{name}/matches0"], g[f"{tag}/{fam}/{name}/scores0"]
            m, s = cases.ref(mode, d0, d1, sim=sim)
            safe = cases.safe_rows(mode, d0, d1, 1e-6, sim=sim)
            assert safe.mean() > 0.99, (fam, name)
            np.testing.assert_array_equal(m[safe], gm[safe], err_msg=f"{fam}/{name}")
            same = m == gm
            np.testing.assert_allclose(s[same], gs[same], atol=1e-6, err_msg=f"{fam}/{name}")
            n += 1
    # the label-aware matcher: a cascade of mutual nearest neighbours, exact on these sets (smallest gap >> 1e-6)
    m, s = mr.itloc_with_label(d0, g[f"{tag}/labels0"], d1, g[f"{tag}/labels1"])
    np.testing.assert_array_equal(m, g[f"{tag}/itloc/NNML/matches0"])
    np.testing.assert_allclose(s, g[f"{tag}/itloc/NNML/scores0"], atol=1e-6)
    n += 1
    assert n == len([k for k in g.files if k.startswith(f"{tag}/") and k.endswith("/matches0")])       # every matcher entry


def test_tie_and_duplicate_rules():
    d0 = np.eye(4, 8)
    d1 = 0.9 * np.stack([d0[1], d0[0], d0[0], 0.6 * d0[2] + 0.8 * d0[3], d0[2]])
    m, s = mr.hloc(d0, d1, mutual=False)
    assert m.tolist() == [1, 0, 4, 3] and np.allclose(s, [0.95, 0.95, 0.95, 0.86])          # first index on the exact tie of row 0
    m, s = mr.hloc(d0, d1, ratio=0.99, mutual=False)
    assert m[0] == -1 and s[0] == 0.0                                                     # duplicated best: s2 == s1
    m, s = mr.itloc(d0, d1, "nnr", 0.99)
    assert m[0] == -1 and s[0] == 0.9
    with pytest.raises(ValueError):
        mr.hloc(d0, d1[:1], ratio=0.8)                                                    # topk(2) of one candidate
    assert mr.hloc(d0, d1[:0])[0].tolist() == [-1] * 4


def test_margins_bound_what_a_perturbation_can_change():
    """Similarities moved by less than eps (all entries, random signs) never change a row that margins calls safe."""
    d0, d1, rows, sim = cases.straddle_set(257, 300, False)
    rs = np.random.RandomState(0)
    for name, mode in cases.STRADDLE_MODES.items():
        for eps in (1e-3, 1e-5):
            safe = cases.safe_rows(mode, d0, d1, eps, sim=sim)
            want, _ = cases.ref(mode, d0, d1, sim=sim)
            changed = np.zeros(len(want), dtype=bool)
            for _ in range(20):
                got, _ = cases.ref(mode, d0, d1, sim=sim + eps * rs.uniform(-1, 1, sim.shape))
                changed |= got != want
            assert not (changed & safe).any(), name
            assert eps < 1e-4 or changed.any()           # ... and the perturbation does reach the unsafe ones


@pytest.mark.parametrize("n0,n1", cases.STRADDLE_SIZES)
def test_generator_guards_hold_for_the_gpu_sizes(n0, n1):
    for swap in (False, True):
        d0, d1, rows, sim = cases.straddle_set(n0, n1, swap)
        assert d0.shape == ((n1, 128) if swap else (n0, 128)) and len(rows) == min(n0, n1 // 2)
        assert np.array_equal(d0, d0.astype(np.float16).astype(np.float32))               # fp16-representable
        assert np.abs(np.linalg.norm(d0, axis=1) - 1).max() < 2e-3
        for name, mode in cases.STRADDLE_MODES.items():
            for sim_mode in cases.SIM_MODES:
                share, dep, *_ = cases.straddle_guards(n0, n1, swap, mode, mr.EPS[sim_mode])
                print(n0, n1, "swapped" if swap else "as built", name, sim_mode, "safe %.3f  s2-dependent planted %.3f" % (share, dep))
                assert share >= cases.MIN_SAFE
                if cases.s2_guard(mode, swap) is not None:
                    assert dep >= cases.s2_guard(mode, swap)


@pytest.mark.parametrize("n0,n1", cases.FORCED_N)
def test_forced_positions_are_decided_as_designed(n0, n1):
    chunk, groups = cases.forced_pairs(n1)
    for group in range(len(groups)):
        for duplicate in (False, True):
            for swap in (False, True):
                d0, d1, rows, sim = cases.forced_set(n0, n1, group, duplicate, swap)
                for kind, _, mutual in cases.FORCED_MODES:
                    if swap and not mutual:
                        continue
                    for ratio in (0.6, 0.8, 0.99):
                        mode = (kind, ratio, None, mutual)
                        m, _ = cases.ref(mode, d0, d1, sim=sim)
                        safe = cases.safe_rows(mode, d0, d1, 1e-3, sim=sim)
                        if duplicate:
                            assert (m[rows] == -1).all()
                        elif ratio < 0.99:
                            assert safe[rows].all() and ((m[rows] >= 0) == (ratio == 0.8)).all()


@pytest.mark.parametrize("dim", cases.DIM_CASES)
def test_small_dimensions_keep_enough_safe_rows(dim):
    d0, d1, rows, sim = cases.dim_set(dim)
    assert d0.shape == (257, dim)
    for name, mode in cases.DIM_MODES.items():
        assert cases.safe_rows(mode, d0, d1, 1e-3, sim=sim).mean() >= cases.MIN_SAFE


def test_negative_sets_are_negative_and_tied():
    ties = 0
    for d0, d1 in cases.negative_sets():
        sim = mr.similarity(d0, d1)
        assert (sim < 0).all() and 1 <= min(sim.shape) <= 5 and 3 <= max(sim.shape) <= 300
        ties += int(((sim == sim.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        ties += int(((sim == sim.max(axis=0, keepdims=True)).sum(axis=0) > 1).sum())
    assert ties >= 8
