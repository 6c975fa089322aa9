"""Plain NumPy restatement of guided matching (include/sfd2_hip.h sfd2_match_guided_batch), independent of the library's
wrappers: the gate in fp64, the gate again in float32 in the kernel's stated operation order, the masked NearestNeighbor rule through
tests/match_ref.py, two deliberately wrong variants, the scenes of the tests and the rule that says which rows a comparison may use.
tests/test_guided_host.py asserts the guards of these definitions on the CPU; tests/test_gpu_guided.py imports the same definitions.

The gate.  F: l = F (x0, y0, 1), m = F^T (x1, y1, 1), r = x1 l0 + y1 l1 + l2, e = r^2 / (l0^2 + l1^2 + m0^2 + m1^2); the pair passes iff
r^2 <= t^2 (l0^2 + l1^2 + m0^2 + m1^2).  H: p = pi(H (x0, y0, 1)), e = |x1 - p|^2; it passes iff p is finite and e <= t^2.

Safe rows.  A pair is BANDED when |e - t^2| <= BAND t^2: the float32 gate of the device may decide it either way.  A row is safe when no
pair of it is banded, when match_ref's margin reasoning holds on its gated candidates with EPS["f16"] = 1e-3 (a row without a candidate
is decided -- no match; a row with one candidate has no second best to come close to), and, with the mutual check, when the same is
true of the column of its arg-max.

BAND is measured, not chosen: 8 x the largest relative difference between the float32 and the fp64 gate error over the pairs with e in
[t^2 / 4, 4 t^2] on the scenes of SIZES, both kinds (measured_band below; the factor 8 because numpy does not contract to fmaf as the
device does), with a ceiling of 1e-2.  BAND_MEASURED holds what these scenes gave; BAND is that figure rounded up to one digit, and
test_guided_host.py asserts that the measurement has not moved above it."""
import functools

import numpy as np

import match_ref as mr
from sfd2_amd import synth

BAND_MEASURED = {"F": 7.4e-4, "H": 3.5e-4}  # 8 x the largest relative difference per kind, as measured_band() gave it (9.2e-5 and 4.3e-5 x 8)
BAND = 1e-3
EPS = mr.EPS["f16"]
SIZES = [(3, 33), (65, 64), (257, 300), (300, 257), (1000, 37), (33, 1025), (700, 2049)]
GUARD_SIZES = [(3, 33), (65, 64), (257, 300), (300, 257), (33, 1025), (700, 2049)]        # the sizes whose safe fraction is guarded
CONFS = {"NNM": dict(ratio=None, dist=None, mutual=True), "RATIO": dict(ratio=0.8, dist=None, mutual=True),
         "ONEWAY": dict(ratio=0.9, dist=0.7, mutual=False)}
MAX_ERROR = 4.0
OUTSIDE = 0.05                            # forced scenes: the better-scoring candidate's e is t^2 (1 + OUTSIDE), >= 10 BAND outside the gate
FOCAL, CX, CY = 1400.0, 800.0, 600.0      # a 1600 x 1200 image


# ------------------------------------------------------------------------------------------ the gate
def _hom(xy):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    return np.concatenate([xy, np.ones((len(xy), 1))], 1)


def gate64(kind, M, xy0, xy1, t=MAX_ERROR):
    """fp64: (e [n0, n1], passes [n0, n1]).  H: a row whose projection is not finite has e = inf and passes nowhere."""
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    a, b = _hom(xy0), _hom(xy1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "F":
            l, m = a @ M.T, b @ M                                 # l_i = F x0_i, m_j = F^T x1_j
            r = l @ b.T
            n = (l[:, 0] ** 2 + l[:, 1] ** 2)[:, None] + (m[:, 0] ** 2 + m[:, 1] ** 2)[None, :]
            return r * r / n, r * r <= t * t * n
        p = a @ M.T
        p = p[:, :2] / p[:, 2:3]
        valid = np.isfinite(p.astype(np.float32)).all(axis=1)
        d = b[None, :, :2] - np.where(valid[:, None], p, 0.0)[:, None, :]
        e = np.where(valid[:, None], (d * d).sum(axis=2), np.inf)
    return e, e <= t * t


def gate32(kind, M, xy0, xy1, t=MAX_ERROR):
    """The gate as the device states it: the per-point records in fp64 from the double matrix, rounded to float32; the test in float32
    in the kernel's order, r = x1 l0 + (y1 l1 + l2) and dx dx + dy dy (numpy rounds where the device fuses).  (e, passes) in float32."""
    f = np.float32
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    a, b = _hom(np.asarray(xy0, dtype=f)), _hom(np.asarray(xy1, dtype=f))
    t2 = f(t * t)
    x1, y1 = b[:, 0].astype(f)[None, :], b[:, 1].astype(f)[None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "F":
            l, m = a @ M.T, b @ M
            l0, l1, l2 = (l[:, c].astype(f)[:, None] for c in range(3))
            nl = (l[:, 0] ** 2 + l[:, 1] ** 2).astype(f)[:, None]
            nm = (m[:, 0] ** 2 + m[:, 1] ** 2).astype(f)[None, :]
            r = x1 * l0 + (y1 * l1 + l2)
            n = nl + nm
            return r * r / n, r * r <= t2 * n
        p = a @ M.T
        p = (p[:, :2] / p[:, 2:3]).astype(f)
        valid = np.isfinite(p).all(axis=1)[:, None]
        dx, dy = x1 - np.where(valid, p[:, 0:1], f(0)), y1 - np.where(valid, p[:, 1:2], f(0))
        e = dx * dx + dy * dy
        return np.where(valid, e, f(np.inf)), valid & (e <= t2)


def measured_band(t=MAX_ERROR):
    """{kind: 8 x the largest relative difference between gate32's and gate64's error over the pairs with e in [t^2 / 4, 4 t^2]} on
    the scenes of SIZES."""
    out = {}
    for kind in ("F", "H"):
        worst = 0.0
        for n0, n1 in SIZES:
            sc = scene(kind, n0, n1)
            e64, _ = gate64(kind, sc["M"], sc["xy0"], sc["xy1"], t)
            e32, _ = gate32(kind, sc["M"], sc["xy0"], sc["xy1"], t)
            near = (e64 >= t * t / 4) & (e64 <= 4 * t * t)
            if near.any():
                worst = max(worst, float(np.max(np.abs(e32.astype(np.float64)[near] - e64[near]) / e64[near])))
        out[kind] = 8.0 * worst
    return out


# ------------------------------------------------------------------------------------------ the rule
def _padded(sim):
    """sim with one more row and column of -inf: changes no arg-max, no second best and no decision of the others, and lets
    match_ref.hloc take its top-2 of a matrix with a single row or column."""
    out = np.full((sim.shape[0] + 1, sim.shape[1] + 1), -np.inf)
    out[:-1, :-1] = sim
    return out


def hloc_masked(sim, passes, ratio=None, dist=None, mutual=True, rank=2):
    """match_ref.hloc on the masked matrix with the two additions: a row without a gated candidate gives -1 and score 0 (with them the
    empty row 0 / empty column 0 pair cannot match), and s2 = -inf passes the ratio test (2 (1 - s2) = inf, match_ref's arithmetic as it
    is).  (matches0 int64 [n0], scores0 float64 [n0])."""
    n0, n1 = sim.shape
    if n0 == 0 or n1 == 0:
        return np.full(n0, -1, dtype=np.int64), np.zeros(n0)
    masked = np.where(passes, sim, -np.inf)
    with np.errstate(invalid="ignore"):
        m0, sc = mr.hloc(None, None, ratio, dist, mutual, rank, sim=_padded(masked))
    m0, sc = m0[:-1].copy(), sc[:-1].copy()
    empty = ~passes.any(axis=1)
    m0[empty] = -1
    sc[empty] = 0.0
    assert (m0 < n1).all()
    return m0, sc


def hloc_no_gate(sim, ratio=None, dist=None, mutual=True):
    """Deliberately wrong: the gate dropped."""
    return hloc_masked(sim, np.ones(sim.shape, dtype=bool), ratio, dist, mutual)


def hloc_transposed_reverse(sim, kind, M, xy0, xy1, t=MAX_ERROR, ratio=None, dist=None):
    """Deliberately wrong: the reverse direction of the mutual check gates with the TRANSPOSED guide (a gate written a second time for
    the other orientation, with the matrix the wrong way round); the forward direction is right."""
    fwd = gate64(kind, M, xy0, xy1, t)[1]
    rev = gate64(kind, np.asarray(M, dtype=np.float64).reshape(3, 3).T, xy0, xy1, t)[1]
    m0, sc = hloc_masked(sim, fwd, ratio, dist, mutual=False)
    m1, _ = hloc_masked(sim.T, rev.T, ratio, dist, mutual=False)
    keep = (m0 >= 0) & (m1[np.maximum(m0, 0)] == np.arange(len(m0)))
    return np.where(keep, m0, -1), sc


def _dir_safe(masked, ratio, dist, eps):
    n, m = masked.shape
    if m == 0:
        return np.ones(n, dtype=bool)
    cnt = np.isfinite(masked).sum(axis=1)
    pad = np.concatenate([masked, np.full((n, 1), -np.inf)], 1)           # (so that one candidate has a second best of -inf)
    with np.errstate(invalid="ignore"):
        ok = mr._dir_margins(pad, "hloc", ratio, dist, eps)
    ok[cnt == 0] = True                                                   # no candidate: decided
    return ok


def safe_rows(sim, e, ratio=None, dist=None, mutual=True, t=MAX_ERROR, band=BAND, eps=EPS):
    """Per row: may the device's float32 gate and fp16 similarities not change this row's result?  (The rule in this file's text.)"""
    t2 = t * t
    with np.errstate(invalid="ignore"):
        banded = np.abs(e - t2) <= band * t2
    passes = e <= t2
    masked = np.where(passes, sim, -np.inf)
    safe = ~banded.any(axis=1) & _dir_safe(masked, ratio, dist, eps)
    if mutual and sim.shape[1] > 0:
        col = ~banded.any(axis=0) & _dir_safe(masked.T, ratio, dist, eps)
        safe &= np.where(passes.any(axis=1), col[np.argmax(masked, axis=1)], True)
    return safe


def splits(k, max_n):
    """The candidate splits of a batch of k pairs whose largest set has max_n rows, as include/sfd2_hip.h states them; a direction's
    n candidates are swept in chunks of chunk(n, splits)."""
    blocks = (max_n + 127) // 128
    s = (768 * 6 + 2 * k * blocks - 1) // (2 * k * blocks)
    return max(1, min(s, 8, (max_n + 31) // 32))


def chunk(n, s):
    return ((n + s - 1) // s + 31) & ~31


# ------------------------------------------------------------------------------------------ scenes
def _geometry():
    K = np.array([[FOCAL, 0.0, CX], [0.0, FOCAL, CY], [0.0, 0.0, 1.0]])
    a = 0.15
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    return K, R, np.array([-1.0, 0.05, 0.1])


def _model(kind):
    """(M with unit Frobenius norm, depth(u0 [n,2]) -> z or None)."""
    K, R, t = _geometry()
    Ki = np.linalg.inv(K)
    if kind == "F":
        tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
        M = Ki.T @ tx @ R @ Ki
        return M / np.linalg.norm(M), None
    n, d = np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0]), 8.0      # the plane n . X = d in camera 0
    M = K @ (R + np.outer(t, n) / d) @ Ki
    return M / np.linalg.norm(M), lambda u0: d / (_hom(u0) @ Ki.T @ n)


def _project(u0, z):
    K, R, t = _geometry()
    X = (_hom(u0) @ np.linalg.inv(K).T) * z[:, None]
    x = (X @ R.T + t) @ K.T
    return x[:, :2] / x[:, 2:3]


def _fresh(a):
    a.setflags(write=False)
    return a


def _finish(sc):
    sc["sim"] = mr.similarity(sc["d0"], sc["d1"])
    for v in sc.values():
        if isinstance(v, np.ndarray):
            _fresh(v)
    return sc


def _base(kind, n0, n1, seed, n_true, noise=0.5):
    rs = np.random.RandomState(7000 + seed)
    M, depth = _model(kind)
    d0 = synth.make_descriptors(n0, seed=300 + seed).astype(np.float64)
    d1 = synth.make_descriptors(n1, seed=400 + seed).astype(np.float64)
    xy0 = rs.uniform([0.0, 0.0], [2 * CX, 2 * CY], (n0, 2))
    xy1 = rs.uniform([0.0, 0.0], [2 * CX, 2 * CY], (n1, 2))
    rows, cols = rs.permutation(n0)[:n_true], rs.permutation(n1)[:n_true]
    z = depth(xy0[rows]) if depth else rs.uniform(5.0, 12.0, n_true)
    true1 = _project(xy0[rows], z)
    xy1[cols] = true1 + rs.normal(0.0, noise, (n_true, 2))
    cos = rs.uniform(0.7, 0.95, n_true)
    if n_true:
        d1[cols] = mr._at_cosine(d0[rows], cos, rs)
    return dict(kind=kind, M=M, d0=d0, d1=d1, xy0=xy0, xy1=xy1, rows=rows, cols=cols, cos=cos, true1=true1, rs=rs)


def _stored(sc, with_sim=True):
    """Descriptors as fp16-representable float32 (the device's conversion is then exact), key points as float32."""
    sc.pop("rs")
    sc.pop("true1")
    sc["d0"], sc["d1"] = mr._fp16(sc["d0"]), mr._fp16(sc["d1"])
    sc["xy0"], sc["xy1"] = sc["xy0"].astype(np.float32), sc["xy1"].astype(np.float32)
    if not with_sim:
        return sc
    return _finish(sc)


@functools.lru_cache(maxsize=None)
def scene(kind, n0, n1, seed=0):
    """kind 'F': a 0.15 rad rotation about y with t = (-1, 0.05, 0.1), depths 5 - 12; 'H': the same motion in front of a tilted plane.
    min(n0, n1) * 2 // 3 true matches at cosine U(0.7, 0.95) with 0.5 px noise, in no spatial order; the rest of both sides are points
    anywhere with random descriptors.  Read-only arrays: d0, d1 (float32), xy0, xy1 (float32), M, sim (fp64), rows / cols (the true pairs)."""
    return _stored(_base(kind, n0, n1, seed + 17 * n0 + n1, min(n0, n1) * 2 // 3))


def bench_scene(kind, n, seed):
    """scene(kind, n, n) without the fp64 similarity matrix (tools/guided_bench.py: 50 pairs of 4096 x 4096)."""
    return _stored(_base(kind, n, n, 10000 + seed, n * 2 // 3), with_sim=False)


def _off_model(kind, M, x0, x1, e_target, sign=1.0):
    """The point next to x1 (on the model of x0) whose gate error with x0 is e_target: moved along the epipolar line's normal (F) or
    along x (H), the distance by bisection on gate64."""
    if kind == "F":
        l = np.asarray(M).reshape(3, 3) @ np.array([x0[0], x0[1], 1.0])
        u = sign * l[:2] / np.linalg.norm(l[:2])
    else:
        u = np.array([sign, 0.0])
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if gate64(kind, M, x0[None], (x1 + mid * u)[None], 1.0)[0][0, 0] < e_target:
            lo = mid
        else:
            hi = mid
    return x1 + hi * u


@functools.lru_cache(maxsize=None)
def twin_scene(seed=0, n_true=200, n_extra=100, n_twin=150, kind="F", with_sim=True):
    """n_true true matches plus n_extra points per side; n_twin of the true rows have a TWIN in image 1: a descriptor within +- 0.02
    cosine of the true one, 40 - 120 px off the epipolar line.  The twins are the last n_twin columns; 'twinned': their rows."""
    n0, n1 = n_true + n_extra, n_true + n_extra + n_twin
    sc = _base(kind, n0, n1 - n_twin, 900 + seed, n_true)
    rs = sc["rs"]
    pick = rs.permutation(n_true)[:n_twin]
    rows = sc["rows"][pick]
    cos = np.clip(sc["cos"][pick] + rs.uniform(-0.02, 0.02, n_twin), 0.0, 0.99)
    twins_d = mr._at_cosine(sc["d0"][rows], cos, rs)
    dist = rs.uniform(40.0, 120.0, n_twin) * rs.choice([-1.0, 1.0], n_twin)
    twins_xy = np.empty((n_twin, 2))
    for k, r in enumerate(rows):
        if kind == "F":
            l = sc["M"] @ np.array([sc["xy0"][r, 0], sc["xy0"][r, 1], 1.0])
            u = l[:2] / np.linalg.norm(l[:2])
        else:
            u = np.array([1.0, 0.0])
        twins_xy[k] = sc["true1"][pick[k]] + dist[k] * u
    sc["d1"] = np.concatenate([sc["d1"], twins_d])
    sc["xy1"] = np.concatenate([sc["xy1"], twins_xy])
    sc["twinned"] = rows
    return _stored(sc, with_sim)


@functools.lru_cache(maxsize=None)
def forced_scene(kind, n0, n1, pairs, seed=0):
    """No true matches; query qs[p] (spread over the query tiles) gets its gated best -- cosine 0.8, on the model -- at column
    pairs[p][0] and a BETTER-scoring candidate -- cosine 0.9 -- just outside the gate, at e = t^2 (1 + OUTSIDE), at column pairs[p][1].
    'q', 'j1', 'j2' name them."""
    sc = _base(kind, n0, n1, 500 + seed, 0)
    rs = sc["rs"]
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    assert len(np.unique(pairs)) == pairs.size and pairs.min() >= 0 and pairs.max() < n1
    k = len(pairs)
    qs = np.unique(np.linspace(0, n0 - 1, k).astype(np.int64))
    assert len(qs) == k
    _, depth = _model(kind)
    x0 = sc["xy0"][qs].astype(np.float32).astype(np.float64)          # as the device will see them
    on = _project(x0, depth(x0) if depth else rs.uniform(5.0, 12.0, k))
    for p in range(k):
        sc["xy1"][pairs[p, 0]] = _off_model(kind, sc["M"], x0[p], on[p], 0.25)                                   # half a pixel off: clearly inside
        sc["xy1"][pairs[p, 1]] = _off_model(kind, sc["M"], x0[p], on[p], MAX_ERROR ** 2 * (1.0 + OUTSIDE), -1.0)
    sc["d1"][pairs[:, 0]] = mr._at_cosine(sc["d0"][qs], np.full(k, 0.8), rs)
    sc["d1"][pairs[:, 1]] = mr._at_cosine(sc["d0"][qs], np.full(k, 0.9), rs)
    sc.update(q=qs, j1=pairs[:, 0].copy(), j2=pairs[:, 1].copy())
    return _stored(sc)


def _distinct(*pairs):
    """The pairs without those that name a column an earlier pair took (at small n1 two placements can coincide)."""
    seen, out = set(), []
    for a, b in pairs:
        if a not in seen and b not in seen:
            out.append((a, b))
            seen |= {a, b}
    return tuple(out)


def forced_pairs(n1):
    """(gated best, better candidate outside the gate) column pairs, placed as tests/test_gpu_match_top2.py's forced_pairs places its
    (best, second best): relative to the 16 accumulator registers of a lane, the two half-waves, the two 32-row sub-tiles of a stage
    and the split boundaries.  chunk: the candidates per split at 8 splits."""
    c = chunk(n1, 8)
    b = c                                                # second split, first stage
    return c, _distinct((0, n1 - 1), (31, 32), (63, 64),
               (b + 2, b + 6),                           # same register, the two half-waves
               (b + 9, b + 10),                          # neighbouring registers of one lane
               (b + 17, b + 49),                         # the two 32-row sub-tiles of one stage
               (10, 10 + 2 * c + 5),                     # two splits apart, best first
               (20 + 3 * c, 20),                         # ... and the candidate outside the gate first
               (c - 1, c),                               # either side of a split boundary
               (2 * c, 2 * c - 1))                       # ... and the other way round
