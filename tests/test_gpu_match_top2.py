"""The second-best similarity behind the ratio tests (pytest -m gpu): match_top2_v2_kernel<true> (fp16 operands),
match_top2_kernel<USE_LO> (f16x2) and match_reduce_kernel against tests/match_ref.py, on descriptor sets in which the
second best decides the result, plus the smaller gaps of the same files: dim < 128, row selection with a top-2 mode,
more than 8 candidate splits, maxima that are negative.

Every comparison is made on the rows that match_ref.margins calls safe at the similarity error of the mode (1e-3 for
'f16', 1e-5 for 'f16x2': header of tests/test_gpu_parity.py); the share of safe rows is itself asserted (>= 90 %), and so
is the share of planted rows whose result changes when the third best stands in for the second best (>= 20 %): a test
that would still pass with a lost second best fails on its own guard.  tests/test_match_ref_host.py checks the same
guards without a GPU.  The case definitions up to the first fixture need no GPU and no library."""
import ctypes
import functools

import numpy as np
import pytest

import match_ref as mr
from sfd2_amd import _lib, synth

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------ cases (CPU side)
# (a) sizes: the 32-row sub-tile, the 64-row stage, the 256-query block, 2 splits (min(n) = 33) and 8 splits (n >= 256)
STRADDLE_SIZES = [(3, 33), (65, 64), (257, 300), (300, 257), (1000, 37), (33, 1025), (700, 2049)]
STRADDLE_SEED = {(3, 33): 1, (65, 64): 2, (257, 300): 3, (300, 257): 4, (1000, 37): 5, (33, 1025): 6, (700, 2049): 7}
# mode = (kind, ratio, dist, mutual)
STRADDLE_MODES = {
    "hloc_r0.8": ("hloc", 0.8, None, False),
    "hloc_r0.8_mutual": ("hloc", 0.8, None, True),
    "hloc_r0.9_d0.7": ("hloc", 0.9, 0.7, False),
    "nnr_0.8": ("nnr", 0.8, None, True),
}
SIM_MODES = ("f16", "f16x2")
MIN_SAFE = 0.90           # share of all rows that must be safe
# Share of planted rows that are safe AND change with the third best in place of s2, at r = 0.8: the generator spreads d0 / d1
# = rho over U(0.3, 1), so 51 % of the planted rows lie above r^2 = 0.64 and pass only because of the third best.  At r = 0.9
# with distance 0.7 a row must also pass d0 <= 0.49 (c1 >= 0.755): P(rho > 0.81) P(c1 >= 0.755) = 0.27 x 0.56 = 15 % in
# expectation, below 20 % whatever the seed -- that mode must have at least one such row.
MIN_S2_DEPENDENT = 0.20


def ref(mode, d0, d1, rank=2, sim=None):
    kind, ratio, dist, mutual = mode
    if kind == "hloc":
        return mr.hloc(d0, d1, ratio, dist, mutual, rank=rank, sim=sim)
    return mr.itloc(d0, d1, kind, ratio, rank=rank, sim=sim)


def safe_rows(mode, d0, d1, eps, sim=None):
    kind, ratio, dist, mutual = mode
    return mr.margins(d0, d1, kind, ratio, dist, mutual, eps=eps, sim=sim)


@functools.lru_cache(maxsize=None)
def straddle_set(n0, n1, swap):
    """planted_straddle(n0, n1) as built, or with the two sets swapped: the planted pairs then sit in the columns and
    the rows that depend on them are the best candidates j1.  Returns (d0, d1, planted rows, fp64 similarities)."""
    d0, d1, info = mr.planted_straddle(n0, n1, STRADDLE_SEED[(n0, n1)])
    rows = info["q"]
    if swap:
        d0, d1, rows = d1, d0, info["j1"]
    sim = mr.similarity(d0, d1)
    for a in (d0, d1, rows, sim):
        a.setflags(write=False)
    return d0, d1, rows, sim


def straddle_guards(n0, n1, swap, mode, eps):
    """(share of safe rows, share of planted rows that are safe and depend on s2, reference matches, scores, safe)."""
    d0, d1, rows, sim = straddle_set(n0, n1, swap)
    m, s = ref(mode, d0, d1, sim=sim)
    m3, _ = ref(mode, d0, d1, rank=3, sim=sim)
    safe = safe_rows(mode, d0, d1, eps, sim=sim)
    dep = safe[rows] & (m[rows] != m3[rows])
    return safe.mean(), dep.mean(), m, s, safe


def s2_guard(mode, swap):
    """The least share of s2-dependent planted rows (None: no guard).  Swapped, the planted pairs are a column's top two:
    only the modes with a mutual check read them."""
    if swap and not mode[3]:
        return None
    return MIN_S2_DEPENDENT if mode[2] is None else 1e-9


def forced_pairs(n1):
    """(b): two groups of (best, second best) positions with distinct entries.  chunk = the candidates per split at
    8 splits (n1 >= 256): ceil(n1 / 8) rounded up to 32."""
    chunk = ((n1 + 7) // 8 + 31) & ~31
    b = chunk                                            # second split, first stage
    g0 = [(0, n1 - 1), (31, 32), (63, 64),
          (b + 2, b + 6),                                # same register, the two half-waves
          (b + 9, b + 10),                               # neighbouring registers of one lane
          (b + 17, b + 49),                              # the two 32-row sub-tiles of one stage
          (10, 10 + 2 * chunk + 5)]                      # two splits apart, best first
    g1 = [(n1 - 1, n1 - 2),
          (20 + 3 * chunk, 20),                          # ... and second best first
          (chunk - 1, chunk)]                            # either side of a split boundary
    return chunk, [g0, g1]


FORCED_N = [(300, 300), (300, 2049)]
FORCED_MODES = [("hloc", None, False), ("hloc", None, True), ("nnr", None, True)]      # ratio filled in per run


@functools.lru_cache(maxsize=None)
def forced_set(n0, n1, group, duplicate, swap):
    _, groups = forced_pairs(n1)
    d0, d1, info = mr.planted_at(n0, n1, 100 + group, groups[group], duplicate=duplicate)
    rows = info["q"]
    if swap:
        d0, d1, rows = d1, d0, np.concatenate([info["j1"], info["j2"]]) if duplicate else info["j1"]
    sim = mr.similarity(d0, d1)
    for a in (d0, d1, rows, sim):
        a.setflags(write=False)
    return d0, d1, rows, sim


DIM_CASES = [17, 64, 127]
DIM_MODES = {"NNM": ("hloc", None, None, True), "RATIO": ("hloc", 0.8, None, True)}


@functools.lru_cache(maxsize=None)
def dim_set(dim):
    d0, d1, info = mr.planted_straddle(257, 300, 40 + dim, dim=dim)
    sim = mr.similarity(d0, d1)
    for a in (d0, d1, sim):
        a.setflags(write=False)
    return d0, d1, info["q"], sim


# ------------------------------------------------------------------------------------------ device side
@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no MI355X visible: GPU tests cannot run (there is no CPU fallback)")
    return _lib.default_context(0)


_DT = {np.dtype(np.float32): _lib.DT_F32, np.dtype(np.float64): _lib.DT_F64, np.dtype(np.float16): _lib.DT_F16}


def conf_of(mode, sim_mode):
    kind, ratio, dist, mutual = mode
    sm = _lib.SIM_F16X2 if sim_mode == "f16x2" else _lib.SIM_F16
    if kind == "hloc":
        return _lib.MatchConf(_lib.MATCH_HLOC, int(mutual), float(ratio or 0.0), float(dist or 0.0), sm)
    return _lib.MatchConf(_lib.MATCH_ITLOC_NNR if kind == "nnr" else _lib.MATCH_ITLOC_NNM, 1, float(ratio or 0.0), 0.0, sm)


def gpu_match(ctx, d0, d1, mode, sim_mode, layout=_lib.LAYOUT_ND, device=False):
    """sfd2_match on [n][dim] arrays of one dtype; layout DN passes their transposes, device=True torch tensors."""
    n0, dim = d0.shape
    n1 = d1.shape[0]
    a0, a1 = (d0, d1) if layout == _lib.LAYOUT_ND else (d0.T, d1.T)
    a0, a1 = np.ascontiguousarray(a0), np.ascontiguousarray(a1)
    keep = (a0, a1)
    if device:
        import torch
        keep = (torch.from_numpy(a0).cuda(), torch.from_numpy(a1).cuda())
        torch.cuda.synchronize()
    m = np.full((n0,), -7, dtype=np.int64)
    s = np.full((n0,), np.nan, dtype=np.float32)
    conf = conf_of(mode, sim_mode)
    _lib.check(ctx.lib.sfd2_match(ctx.h, _lib.ptr(keep[0]), n0, _lib.ptr(keep[1]), n1, dim, _DT[a0.dtype], layout, int(device),
                                  ctypes.byref(conf), m.ctypes.data, s.ctypes.data, 0))
    return m, s


def check_against_ref(got, want, safe, eps, what):
    m, s = got
    wm, ws = want
    bad = np.flatnonzero(safe & (m != wm))
    assert len(bad) == 0, (what, "rows", bad[:10], "got", m[bad[:10]], "want", wm[bad[:10]])
    same = m == wm
    err = np.abs(s[same] - ws[same]).max() if same.any() else 0.0
    assert err <= eps, (what, "score error", err)


# ------------------------------------------------------------------------------------------ (a) straddling decisions
@pytest.mark.parametrize("n0,n1", STRADDLE_SIZES)
def test_ratio_decisions_straddling_the_threshold(ctx, n0, n1):
    """Rows whose ratio statistic spreads over both sides of the threshold, every ratio mode, both operand kernels, as
    built and with the sets swapped (the column direction then reads the planted pairs).  Smallest share of safe rows
    over the modes and both orientations for these seeds, f16 (eps = 1e-3): (3, 33) 1.000, (65, 64) 0.938, (257, 300) 0.930,
    (300, 257) 0.937, (1000, 37) 0.964, (33, 1025) 0.960, (700, 2049) 0.923; f16x2 (1e-5): 0.993 or more everywhere.
    Planted rows that are safe and depend on s2 at r = 0.8: 0.33, 0.47, 0.47, 0.41, 0.33, 0.42, 0.52 (each line is printed)."""
    for swap in (False, True):
        d0, d1, rows, sim = straddle_set(n0, n1, swap)
        for name, mode in STRADDLE_MODES.items():
            for sim_mode in SIM_MODES:
                eps = mr.EPS[sim_mode]
                share, dep, wm, ws, safe = straddle_guards(n0, n1, swap, mode, eps)
                what = (n0, n1, "swapped" if swap else "as built", name, sim_mode)
                print(what, "safe %.3f  s2-dependent planted %.3f" % (share, dep))
                assert share >= MIN_SAFE, what
                if s2_guard(mode, swap) is not None:
                    assert dep >= s2_guard(mode, swap), what
                check_against_ref(gpu_match(ctx, d0, d1, mode, sim_mode), (wm, ws), safe, eps, what)


# ------------------------------------------------------------------------------------------ (b) forced positions
@pytest.mark.parametrize("n0,n1", FORCED_N)
def test_second_best_at_forced_positions(ctx, n0, n1):
    """Best and second best at the two ends, across the 32-row and 64-row boundaries, in the two half-waves, in one lane,
    in the two sub-tiles of a stage and in different splits (both orders).  d0 / d1 = 0.5: 'fail' at r = 0.6, 'pass' at
    r = 0.8; a lost second best turns the first into 'pass', a best counted twice the second into 'fail'."""
    chunk, groups = forced_pairs(n1)
    assert all(abs(a - b) > chunk for g in groups for a, b in g if abs(a - b) > 64)       # 'far' pairs are in different splits
    for group in range(len(groups)):
        for swap in (False, True):
            d0, d1, rows, sim = forced_set(n0, n1, group, False, swap)
            for kind, _, mutual in FORCED_MODES:
                if swap and not mutual:
                    continue
                for ratio in (0.6, 0.8):
                    mode = (kind, ratio, None, mutual)
                    wm, ws = ref(mode, d0, d1, sim=sim)
                    lost, _ = ref(mode, d0, d1, rank=3, sim=sim)
                    twice, _ = ref(mode, d0, d1, rank=1, sim=sim)
                    # the test's own guard: every planted row is decided as designed and each mutation flips one threshold
                    assert ((wm[rows] >= 0) == (ratio == 0.8)).all(), (group, swap, mode)
                    assert ((lost[rows] >= 0) != (wm[rows] >= 0)).all() if ratio == 0.6 else ((twice[rows] >= 0) != (wm[rows] >= 0)).all()
                    for sim_mode in SIM_MODES:
                        eps = mr.EPS[sim_mode]
                        safe = safe_rows(mode, d0, d1, eps, sim=sim)
                        what = (n0, n1, "group", group, "swapped" if swap else "as built", mode, sim_mode)
                        assert safe[rows].all(), what
                        check_against_ref(gpu_match(ctx, d0, d1, mode, sim_mode), (wm, ws), safe, eps, what)


# ------------------------------------------------------------------------------------------ (c) duplicated best
@pytest.mark.parametrize("n0,n1", FORCED_N)
def test_duplicated_best_never_passes_a_ratio_test(ctx, n0, n1):
    """d1[j2] = d1[j1] bit for bit at the positions of (b): s2 == s1, so d0 <= r^2 d0 is false for every r < 1.  As built
    the planted queries get no match, score 0 (hloc) or s1 (it_loc); swapped, both copies lose their query to the
    column's ratio test.  Every safe row equals the reference, and so do the planted rows, whose top-1 gap is zero."""
    _, groups = forced_pairs(n1)
    for group in range(len(groups)):
        for swap in (False, True):
            d0, d1, rows, sim = forced_set(n0, n1, group, True, swap)
            for kind, _, mutual in FORCED_MODES:
                if swap and not mutual:
                    continue
                for ratio in (0.8, 0.99):
                    mode = (kind, ratio, None, mutual)
                    wm, ws = ref(mode, d0, d1, sim=sim)
                    assert (wm[rows] == -1).all()
                    for sim_mode in SIM_MODES:
                        eps = mr.EPS[sim_mode]
                        safe = safe_rows(mode, d0, d1, eps, sim=sim)
                        what = (n0, n1, "group", group, "swapped" if swap else "as built", mode, sim_mode)
                        m, s = gpu_match(ctx, d0, d1, mode, sim_mode)
                        check_against_ref((m, s), (wm, ws), safe, eps, what)
                        assert (m[rows] == -1).all(), (what, m[rows])
                        if not swap:
                            want_s = np.zeros(len(rows)) if kind == "hloc" else sim[rows].max(axis=1)
                            assert np.abs(s[rows] - want_s).max() <= (0.0 if kind == "hloc" else eps), what


# ------------------------------------------------------------------------------------------ (d) dim < 128
@pytest.mark.parametrize("dim", DIM_CASES)
def test_descriptor_dimension_below_128(ctx, dim):
    """match_prep_kernel zero-fills columns dim..127: every dtype, both layouts, host and device inputs, a top-1 mode
    (single-GEMM kernel) and a ratio mode (top-2 kernel), at (257, 300).  The values are fp16-representable, so all
    three dtypes carry the same numbers."""
    d0, d1, rows, sim = dim_set(dim)
    eps = mr.EPS["f16"]
    for name, mode in DIM_MODES.items():
        wm, ws = ref(mode, d0, d1, sim=sim)
        safe = safe_rows(mode, d0, d1, eps, sim=sim)
        print(dim, name, "safe %.3f" % safe.mean())
        assert safe.mean() >= MIN_SAFE, (dim, name)
        for dt in (np.float32, np.float64, np.float16):
            for layout in (_lib.LAYOUT_ND, _lib.LAYOUT_DN):
                for device in (False, True):
                    got = gpu_match(ctx, d0.astype(dt), d1.astype(dt), mode, "f16", layout, device)
                    check_against_ref(got, (wm, ws), safe, eps, (dim, name, np.dtype(dt).name, layout, device))


# ------------------------------------------------------------------------------------------ (e) rows with a top-2 mode
@pytest.mark.parametrize("sim_mode", SIM_MODES)
def test_row_selection_with_a_ratio_mode(ctx, sim_mode):
    """sfd2_desc_set.rows (a permuted subset of a [dim][n] fp32 set) under the ratio modes, k = 3: a subset, an empty
    selection and a single selected row.  A single candidate has no second best: s2 = -inf, the forward ratio test
    passes (include/sfd2_hip.h, sfd2_match); the column direction has its n0 queries and is tested as usual."""
    n0, n1 = 257, 300
    d0, d1, info = mr.planted_straddle(n0, n1, 3)
    eps = mr.EPS[sim_mode]
    rs = np.random.RandomState(5)
    # the subset keeps every planted candidate and drops a third of the rest, in permuted order
    planted = np.concatenate([info["j1"], info["j2"]])
    rest = np.setdiff1d(np.arange(n1), planted)
    sub = rs.permutation(np.concatenate([planted, rs.permutation(rest)[:len(rest) * 2 // 3]])).astype(np.int32)
    one = np.array([info["j1"][0]], dtype=np.int32)
    none = np.zeros((0,), dtype=np.int32)
    dn = np.ascontiguousarray(d1.T)                                         # [dim][n]
    q = _lib.DescSet(d0.ctypes.data, n0, _lib.DT_F32, _lib.LAYOUT_ND, 0, None, 0, 0)
    sel = [sub, none, one]
    db = (_lib.DescSet * 3)(*[_lib.DescSet(dn.ctypes.data, n1, _lib.DT_F32, _lib.LAYOUT_DN, 0, r.ctypes.data, len(r), 0) for r in sel])
    for name in ("hloc_r0.8_mutual", "hloc_r0.9_d0.7", "nnr_0.8"):
        mode = STRADDLE_MODES[name]
        kind, ratio, dist, mutual = mode
        conf = conf_of(mode, sim_mode)
        m = np.full((3, n0), -7, dtype=np.int64)
        s = np.full((3, n0), np.nan, dtype=np.float32)
        _lib.check(ctx.lib.sfd2_match_batch(ctx.h, ctypes.byref(q), db, 3, 128, ctypes.byref(conf), m.ctypes.data, s.ctypes.data, 0, 0))
        # the subset: the reference on d1[rows], indices mapped back through rows
        wm, ws = ref(mode, d0, d1[sub])
        safe = safe_rows(mode, d0, d1[sub], eps)
        assert safe.mean() >= MIN_SAFE, name
        wm = np.where(wm >= 0, sub[np.maximum(wm, 0)], -1)
        check_against_ref((m[0], s[0]), (wm, ws), safe, eps, (name, sim_mode, "subset"))
        # the empty selection: no match, score 0
        assert (m[1] == -1).all() and (s[1] == 0).all(), name
        # one candidate: s2 = -inf forward; the column's own top two decide the mutual direction
        col = mr.similarity(d0, d1[one])[:, 0]
        d_fwd = 2.0 * (1.0 - col)
        fwd_ok = np.ones(n0, dtype=bool) if not dist else d_fwd <= dist * dist
        fwd_safe = np.ones(n0, dtype=bool) if not dist else np.abs(d_fwd - dist * dist) > 2.0 * eps
        want = np.where(fwd_ok, int(one[0]), -1)
        want_s = np.where(fwd_ok, (col + 1.0) / 2.0, 0.0) if kind == "hloc" else col
        if mutual:
            # the column's top two over the queries: a planted pair's best candidate, so the best query wins by a wide margin
            i1 = int(np.argmax(col))
            t = np.sort(col)
            c_d0, c_d1 = 2.0 * (1.0 - t[-1]), 2.0 * (1.0 - t[-2])
            if kind == "hloc":
                c_ok = c_d0 <= ratio * ratio * c_d1
                assert abs(c_d0 - ratio * ratio * c_d1) > 2.0 * (1.0 + ratio * ratio) * eps and t[-1] - t[-2] > 2.0 * eps
            else:
                c_ok = np.sqrt(c_d0) / (np.sqrt(c_d1) + 1e-8) <= ratio
                assert abs(np.sqrt(c_d0) - ratio * np.sqrt(c_d1)) > 0.05 and t[-1] - t[-2] > 2.0 * eps
            keep = np.zeros(n0, dtype=bool)
            keep[i1] = bool(c_ok)
            want = np.where(keep, want, -1)
        np.testing.assert_array_equal(m[2][fwd_safe], want[fwd_safe], err_msg=f"{name} {sim_mode} single row")
        assert np.abs(s[2] - want_s)[fwd_safe].max() <= eps, name


# ------------------------------------------------------------------------------------------ (f) more than 8 splits
def test_single_gemm_kernel_with_more_than_eight_splits(ctx):
    """n1 = 33000 > 8 * 4096: the tile id must fit 7 bits, so the single-GEMM kernel takes 9 candidate splits.  NNM and
    ONN in f16 against the reference by the gap rule of test_matcher_vs_oracle_sizes (own and partner's arg-max clear
    by 1e-3)."""
    n0, n1 = 300, 33000
    eps = mr.EPS["f16"]
    d0 = synth.make_descriptors(n0, seed=n0 + 7)
    d1 = synth.make_descriptors(n1, seed=n1 + 8)
    rs = np.random.RandomState(9)
    k = 150
    src, dst = rs.permutation(n0)[:k], rs.permutation(n1)[:k]
    dst[:4] = [0, n1 - 1, 8 * 4096 - 1, 8 * 4096]                       # the ends and either side of candidate 32768
    noisy = d0[src] + (0.02 + 0.1 * rs.random_sample((k, 1))).astype(np.float32) * rs.standard_normal((k, 128)).astype(np.float32)
    d1[dst] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
    sim = mr.similarity(d0, d1)
    for mutual in (True, False):
        mode = ("hloc", None, None, mutual)
        wm, ws = ref(mode, d0, d1, sim=sim)
        safe = safe_rows(mode, d0, d1, eps / 2, sim=sim)                 # margins tests gap > 2 eps: the gap rule is gap > 1e-3
        assert safe.mean() >= MIN_SAFE
        assert (wm[src[:4]] == dst[:4]).all() or not mutual
        check_against_ref(gpu_match(ctx, d0, d1, mode, "f16"), (wm, ws), safe, eps, ("9 splits", mutual))


# ------------------------------------------------------------------------------------------ (g) negative maxima
# (g) n0, n1, seed, position the best candidate of query 0 is moved to, positions of its bit-equal copies
NEGATIVE_CASES = [(1, 3, 1, 0, (2,)),              # one tile
                  (2, 33, 2, 1, (32,)),            # the two 32-row tiles of one stage
                  (5, 70, 3, 3, (7, 67)),          # one tile and the next stage
                  (4, 70, 4, 5, (40,)),
                  (3, 70, 5, 2, (66,)),            # the next stage only
                  (2, 300, 6, 3, (35,))]           # beyond 256 candidates a split holds two tiles: the forward tile ids decide


def negative_sets():
    """Small sets whose similarities are all negative: queries near a direction b, candidates near -b.  The best candidate of
    query 0 is duplicated bit for bit (same 32-row tile, the other tile, the next stage), and with four or more queries the
    last query duplicates query 1, a tie in every column.  Each set also comes transposed (3 to 300 queries, 1 to 5
    candidates): the duplicated rows then tie on the query side, up to different waves (queries 3 and 67).  Up to 256
    candidates every split is one 32-row tile and the splits merge by value, first split first; the last case is there for
    the tile ids inside a split."""
    out = []
    for n0, n1, seed, first, copies in NEGATIVE_CASES:
        rs = np.random.RandomState(seed)
        b = rs.standard_normal(128)
        b /= np.linalg.norm(b)
        unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
        d0 = unit(b + 0.06 * rs.standard_normal((n0, 128)))
        d1 = -unit(b + 0.06 * rs.standard_normal((n1, 128)))
        d0, d1 = d0.astype(np.float16).astype(np.float32), d1.astype(np.float16).astype(np.float32)
        j0 = int(np.argmax(mr.similarity(d0[:1], d1)[0]))
        d1[[first, j0]] = d1[[j0, first]]
        for c in copies:
            d1[c] = d1[first]
        if n0 >= 4:
            d0[n0 - 1] = d0[1]
        out.append((d0, d1))
        out.append((d1.copy(), d0.copy()))
    return out


def test_negative_maxima_and_their_ties(ctx):
    """Whole rows and columns of negative similarities (very small sets).  The single-GEMM kernel packs id codes into the
    low mantissa bits so that the larger code wins the maximum; for a negative value a larger mantissa is a SMALLER value,
    so among negative maxima that are equal after truncation the higher index can win (file header of
    match_mutual_kernel.hip).  Asserted: rows without a tie equal the reference; at a tie the reported partner's
    similarity is bit-equal to the maximum of the row (and, with the mutual check, of the column)."""
    eps = mr.EPS["f16"]
    first = other = 0
    for d0, d1 in negative_sets():
        sim = mr.similarity(d0, d1)
        assert (sim < 0).all()
        n0, n1 = sim.shape
        for mutual in (True, False):
            mode = ("hloc", None, None, mutual)
            wm, ws = ref(mode, d0, d1, sim=sim)
            safe = safe_rows(mode, d0, d1, eps, sim=sim)
            m, s = gpu_match(ctx, d0, d1, mode, "f16")
            bad = np.flatnonzero(safe & (m != wm))
            assert len(bad) == 0, ((n0, n1), mutual, bad, m[bad], wm[bad])
            assert np.abs(s - ws).max() <= eps                          # the score is the row maximum either way
            rmax, cmax = sim.max(axis=1), sim.max(axis=0)
            row_tie = (sim == rmax[:, None]).sum(axis=1) > 1
            col_tie = (sim == cmax[None, :]).sum(axis=0) > 1
            for i in np.flatnonzero(~safe):
                tie = row_tie[i] or (mutual and col_tie[np.argmax(sim[i])])
                if not tie:
                    continue                                            # a near tie within eps: nothing is claimed
                if m[i] >= 0:
                    assert sim[i, m[i]] == rmax[i], ((n0, n1), mutual, i, m[i])
                    if mutual:
                        assert sim[i, m[i]] == cmax[m[i]], ((n0, n1), mutual, i, m[i])
                if m[i] == wm[i]:
                    first += 1
                else:
                    other += 1
                    print("negative tie", (n0, n1), "mutual" if mutual else "one-way", "row", i, "got", m[i], "reference", wm[i])
            if mutual:
                # whoever won a tie, the reported pairs are a partial bijection and every column maximum that is also
                # its row's maximum is reported for exactly one of the tied rows
                mm = m[m >= 0]
                assert len(np.unique(mm)) == len(mm)
                assert (m >= 0).sum() == (wm >= 0).sum(), ((n0, n1), m, wm)
    print("negative-maximum ties: first index %d, another index %d" % (first, other))
    assert first + other > 0
