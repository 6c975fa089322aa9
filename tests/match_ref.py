"""Plain fp64 NumPy restatement of the two matchers (hloc/matchers/nearest_neighbor.py:6-57, it_loc/matcher.py:91-194, as
oracle/orc_post.c states them), the margins that say which rows a similarity error of eps cannot change, and the
descriptor sets whose second-best similarity decides the result.  Imports neither the library's matcher wrappers nor the
oracle: tests/test_match_ref_host.py checks it against the oracle and the committed reference results, the GPU tests of
tests/test_gpu_match_top2.py check the kernels against it.

Rules restated: the similarity matrix is d0 . d1^T; per row (and, for the mutual check, per column) s1 is the largest
value, taken at the FIRST index on an exact tie (torch.max / topk), and s2 the second largest WITH multiplicity, so
s2 == s1 when the maximum is duplicated.  `rank` (2 by default) names the order statistic used as "second best":
rank=3 is the deliberately wrong matcher that lost the true second best, rank=1 the one that counted the best twice; the
tests use them to show that a case depends on s2 at all."""
import numpy as np

from sfd2_amd import synth

EPS = {"f16": 1e-3, "f16x2": 1e-5}        # similarity error per sim_mode (header of tests/test_gpu_parity.py)


def similarity(d0, d1):
    return np.asarray(d0, dtype=np.float64) @ np.asarray(d1, dtype=np.float64).T


def _top(sim, rank):
    """Per row: arg-max (first on ties), s1, and the rank-th largest value (multiplicity counted)."""
    n, m = sim.shape
    i1 = np.argmax(sim, axis=1)
    s1 = sim[np.arange(n), i1]
    if rank == 1:
        return i1, s1, s1.copy()
    if m < rank:
        raise ValueError(f"top-{rank} of {m} candidates (the reference's topk raises)")
    s2 = np.partition(sim, m - rank, axis=1)[:, m - rank]
    return i1, s1, s2


def _hloc_mask(s1, s2, ratio, dist):
    d0, d1 = 2.0 * (1.0 - s1), 2.0 * (1.0 - s2)       # find_nn: dist_nn = 2 * (1 - sim_nn)
    ok = np.ones(s1.shape, dtype=bool)
    if ratio:
        ok &= d0 <= ratio * ratio * d1
    if dist:
        ok &= d0 <= dist * dist
    return ok


def hloc(d0, d1, ratio=None, dist=None, mutual=True, rank=2, sim=None):
    """NearestNeighbor._forward: (matches0 int64 [n0], scores0 float64 [n0])."""
    sim = similarity(d0, d1) if sim is None else sim
    n0, n1 = sim.shape
    if n1 == 0:
        return np.full(n0, -1, dtype=np.int64), np.zeros(n0)
    j, s1, s2 = _top(sim, rank if ratio else 1)
    ok = _hloc_mask(s1, s2, ratio, dist)
    m0 = np.where(ok, j, -1).astype(np.int64)
    sc = np.where(ok, (s1 + 1.0) / 2.0, 0.0)
    if mutual:
        i, t1, t2 = _top(sim.T, rank if ratio else 1)
        m1 = np.where(_hloc_mask(t1, t2, ratio, dist), i, -1)
        keep = (m0 >= 0) & (m1[np.maximum(m0, 0)] == np.arange(n0))
        m0 = np.where(keep, m0, -1)
    return m0, sc


def _lowe(s1, s2):
    with np.errstate(invalid="ignore"):                # sim > 1 -> NaN -> "no match", as the reference
        return np.sqrt(2.0 - 2.0 * s1) / (np.sqrt(2.0 - 2.0 * s2) + 1e-8)


def itloc(d0, d1, mode="nnm", ratio=0.9, rank=2, sim=None):
    """Matcher.forward with mutual_nn_matcher ('nnm') or mutual_nn_ratio_matcher ('nnr'): (matches0, scores0 = s1)."""
    sim = similarity(d0, d1) if sim is None else sim
    n0, n1 = sim.shape
    if n1 == 0:
        return np.full(n0, -1, dtype=np.int64), np.zeros(n0)
    nnr = mode == "nnr"
    j, s1, s2 = _top(sim, rank if nnr else 1)
    i, t1, t2 = _top(sim.T, rank if nnr else 1)
    ok = i[j] == np.arange(n0)
    if nnr:
        with np.errstate(invalid="ignore"):
            ok &= (_lowe(s1, s2) <= ratio) & (_lowe(t1, t2)[j] <= ratio)
    return np.where(ok, j, -1).astype(np.int64), s1


def itloc_with_label(d0, labels0, d1, labels1):
    """Matcher.forward with mode 'nnml' (matcher_with_label, it_loc/matcher.py:239-297): mutual nearest neighbours inside
    every label > 0 that both sets carry, then among the rows still unmatched; scores0 = s1 over all of d1."""
    d0, d1 = np.asarray(d0, dtype=np.float64), np.asarray(d1, dtype=np.float64)
    labels0, labels1 = np.asarray(labels0).reshape(-1), np.asarray(labels1).reshape(-1)
    out = np.full(len(d0), -1, dtype=np.int64)
    used = np.zeros(len(d1), dtype=bool)
    for u in np.intersect1d(np.unique(labels0), np.unique(labels1)):
        if u <= 0:
            continue
        i0, i1 = np.flatnonzero(labels0 == u), np.flatnonzero(labels1 == u)
        m, _ = itloc(d0[i0], d1[i1], "nnm")
        out[i0[m >= 0]] = i1[m[m >= 0]]
        used[i1[m[m >= 0]]] = True
    i0, i1 = np.flatnonzero(out < 0), np.flatnonzero(~used)
    if len(i0) and len(i1):
        m, _ = itloc(d0[i0], d1[i1], "nnm")
        out[i0[m >= 0]] = i1[m[m >= 0]]
    return out, similarity(d0, d1).max(axis=1)


# ------------------------------------------------------------------------------------------ margins
def _dir_margins(sim, kind, ratio, dist, eps):
    """One direction: per row, True where every comparison behind that row's own decision keeps its sign when every
    similarity moves by at most eps.  The k-th largest value of a row moves by at most eps too (order statistics are
    1-Lipschitz in the maximum norm), so s1 and s2 each carry eps and d = 2 (1 - s) carries de = 2 eps."""
    n, m = sim.shape
    de = 2.0 * eps
    if m < 2:
        return np.ones(n, dtype=bool)
    srt = np.partition(sim, m - 2, axis=1)
    s1, s2 = srt[:, m - 1], srt[:, m - 2]
    ok = (s1 - s2) > 2.0 * eps                          # own arg-max
    d0, d1 = 2.0 * (1.0 - s1), 2.0 * (1.0 - s2)
    if kind == "hloc":
        if ratio:                                       # d0 <= r^2 d1: the two sides move by de and r^2 de
            ok &= np.abs(d0 - ratio * ratio * d1) > (1.0 + ratio * ratio) * de
        if dist:                                        # d0 <= dist^2: only the left side moves
            ok &= np.abs(d0 - dist * dist) > de
    elif kind == "nnr":
        # sqrt(d0) / (sqrt(d1) + 1e-8) <= ratio  <=>  sqrt(d0) <= ratio (sqrt(d1) + 1e-8), the left side increasing in d0
        # and the right side in d1.  With d0' in [d0 - de, d0 + de] and d1' in [d1 - de, d1 + de] (clamped at 0) the test
        # surely passes iff sqrt(d0 + de) <= ratio (sqrt(d1 - de) + 1e-8) and surely fails iff
        # sqrt(d0 - de) > ratio (sqrt(d1 + de) + 1e-8): interval evaluation is exact for a monotone comparison.  A best
        # similarity that can reach 1 (d0 - de <= 0) is left out: the reference's sqrt of a negative number is NaN.
        lo = lambda d: np.sqrt(np.maximum(d - de, 0.0))
        hi = lambda d: np.sqrt(d + de)
        sure_pass = hi(d0) <= ratio * (lo(d1) + 1e-8)
        sure_fail = lo(d0) > ratio * (hi(d1) + 1e-8)
        ok &= (sure_pass | sure_fail) & (d0 - de > 0.0)
    return ok


def margins(d0, d1, kind, ratio=None, dist=None, mutual=True, eps=1e-3, sim=None):
    """Per query row: is its result decided by more than a similarity error of eps?  kind: 'hloc', 'nnm' or 'nnr'
    (the it_loc modes are always mutual).  With the mutual check the column of the row's arg-max must be decided too."""
    sim = similarity(d0, d1) if sim is None else sim
    n0, n1 = sim.shape
    if n1 == 0:
        return np.ones(n0, dtype=bool)
    safe = _dir_margins(sim, kind, ratio, dist, eps)
    if mutual or kind != "hloc":
        safe &= _dir_margins(sim.T, kind, ratio, dist, eps)[np.argmax(sim, axis=1)]
    return safe


# ------------------------------------------------------------------------------------------ generators
def _fp16(a):
    return a.astype(np.float16).astype(np.float32)


def _at_cosine(q, c, rs):
    """Unit vectors at cosine c[i] to the unit vectors q[i]: c q + sqrt(1 - c^2) u with u orthogonal to q."""
    u = rs.standard_normal(q.shape)
    u -= (u * q).sum(axis=1, keepdims=True) * q
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return c[:, None] * q + np.sqrt(1.0 - c * c)[:, None] * u


def planted_straddle(n0, n1, seed, dim=128):
    """Two descriptor sets (float32 holding fp16-representable values) in which k = min(n0, n1 // 2) queries have their
    best and second-best candidate planted at cosines c1 ~ U(0.6, 0.95) and c2 = 1 - (1 - c1) / rho, rho ~ U(0.3, 1): the
    hloc ratio statistic d0 / d1 of those rows is rho, spread over both sides of r^2 = 0.64.  Returns (d0, d1, info) with
    info = {'q': rows, 'j1': best, 'j2': second best}."""
    rs = np.random.RandomState(seed)
    d0 = synth.make_descriptors(n0, dim=dim, seed=seed).astype(np.float64)
    d1 = synth.make_descriptors(n1, dim=dim, seed=seed + 1).astype(np.float64)
    k = min(n0, n1 // 2)
    q = rs.permutation(n0)[:k]
    pos = rs.permutation(n1)[:2 * k]
    c1 = rs.uniform(0.6, 0.95, k)
    rho = rs.uniform(0.3, 1.0, k)
    c2 = 1.0 - (1.0 - c1) / rho
    d1[pos[:k]] = _at_cosine(d0[q], c1, rs)
    d1[pos[k:]] = _at_cosine(d0[q], c2, rs)
    return _fp16(d0), _fp16(d1), {"q": q, "j1": pos[:k], "j2": pos[k:]}


def planted_at(n0, n1, seed, pairs, c1=0.8, c2=0.6, duplicate=False, dim=128):
    """As planted_straddle, with the best / second-best candidate of query qs[p] forced to positions pairs[p] = (j1, j2)
    (all positions distinct).  c1 = 0.8, c2 = 0.6 give d0 / d1 = 0.5: the hloc ratio test fails at r = 0.6 (r^2 = 0.36)
    and passes at r = 0.8 (0.64); with the third best (random, < 0.5) in place of s2 it passes at 0.6, with s1 in place
    of s2 it fails at 0.8.  duplicate=True: d1[j2] = d1[j1] bit for bit.  The queries are spread over the query tiles."""
    rs = np.random.RandomState(seed)
    d0 = synth.make_descriptors(n0, dim=dim, seed=seed).astype(np.float64)
    d1 = synth.make_descriptors(n1, dim=dim, seed=seed + 1).astype(np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    assert len(np.unique(pairs)) == pairs.size and pairs.min() >= 0 and pairs.max() < n1
    k = len(pairs)
    qs = np.unique(np.linspace(0, n0 - 1, k).astype(np.int64))
    assert len(qs) == k
    d1[pairs[:, 0]] = _at_cosine(d0[qs], np.full(k, c1), rs)
    d1[pairs[:, 1]] = _at_cosine(d0[qs], np.full(k, c2), rs)
    d0, d1 = _fp16(d0), _fp16(d1)
    if duplicate:
        d1[pairs[:, 1]] = d1[pairs[:, 0]]
    return d0, d1, {"q": qs, "j1": pairs[:, 0], "j2": pairs[:, 1]}
