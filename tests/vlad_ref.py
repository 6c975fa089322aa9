"""Numpy restatement of the VLAD stages (sfd2_amd/vlad.py; include/sfd2_hip.h, "global descriptors"), the input families the tests
run them on, and the rows where two correct implementations may differ ("banded").  There is no reference implementation to match:
the arithmetic below IS the interface, restated from the header.

Arithmetic
  h_j, dot_j     fp32 fmaf chains over ascending e.  fmaf(a, b, c) is restated as float32(float64(a) * float64(b) + float64(c)): the
                 product of two fp32 values is exact in fp64, so this is the fused result up to a double rounding that needs the
                 fp64 sum to land exactly between two fp32 values (not met in 1e8 operations of these tests; it would show as a
                 failure, not pass silently).
  s_j            float32(dot_j) - float32(h_j), the argument of the arg-max; a tie goes to the smaller j.
  sums           in-order fp32: np.cumsum over float32 is a strictly sequential accumulation, 0 + v = v exactly.
  norms, update  fp64 from the fp32 sums, rounded to fp32 once.

Families
  exact   rows and centroids on a 2^-7 grid, row norm <= 1.1: products are multiples of 2^-14 and every partial sum stays below 2,
          so every partial sum of every chain is exact in fp32 (chains_exact checks it) and the fp64 scores ARE the kernel's bits:
          the rounding bound is 0, no row is banded, and the designed ties (a duplicated centroid; a row that scores the same
          against two centroids) are decided by the index rule alone.
  float   unit-norm rows around cluster centres, centroids = means of rows.  A row is banded when its two largest exact (fp64)
          scores lie within twice the rounding bound of an fp32 score, (128 + 2) 2^-24 (|x| |c_j| + h_j), the largest over j:
          gamma_n of a chain of 128 multiply-adds plus the subtraction, the argument of tests/pairs_ref.py's retrieval band.
  edge    (tests/test_gpu_vlad_edges.py) covering: row i near centroid i, so every centroid wins; lane ties: all the centroids
          16 nt + lc of a lane equal; all equal: k-way and 16-way ties; negative: centroids times 4, every score below 0.  The
          exact-type ones keep exact chains (tests/test_vlad_host.py checks each at every K it is used with).
"""
import numpy as np

DIM = 128
CHUNK = 4096
EPS24 = 2.0 ** -24
F32, F64 = np.float32, np.float64

ASSIGN_NS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)
ASSIGN_KS = (1, 2, 15, 16, 17, 64, 100, 256)
AGG_LENGTHS = (0, 0, 1, 2, 0, 31, 32, 33, 4096, 0, 4097, 0)      # empty images at the front, in the middle and at the end
AGG_KS = (1, 17, 64, 256)
KMEANS_SEPARATED = ((2, 3000, 8), (2, 5000, 8))                # (seed, n, K): the second crosses a chunk seam
KMEANS_OVERLAP = (5, 3000, 16)
SCENE_SEED, SCENE_K, SCENE_ITERS, SCENE_TOP = 1, 16, 15, 5

# tests/test_gpu_vlad_edges.py: the shapes the cases above do not reach
EDGE_KS = (32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 192, 193, 255)   # both sides of every seam between two accumulator counts, and 255
EDGE_NS = (63, 65, 257)
LANE_TIE_KS = (35, 48, 97, 193)
NEGATIVE_KS = (1, 15, 17, 33, 100, 193, 255)
LARGE_NS = (65665, 131073)             # 1 027 and 2 049 tiles on 1 024 blocks: a second and a third tile per block, the last with one live row
KMEANS_LARGE = (7, 65665, 8)           # 17 chunks, two tiles in three of the assignment blocks (seed 2 has a banded row in iteration 1)
# (seed, n, K, the centroid whose start row is tripled so that no row ever chooses it, or None)
KMEANS_WIDE = ((2, 4097 + 33, 33, None), (2, 4097 + 255, 255, None), (2, 4098, 1, None), (29, 2 * 4096 + 10, 9, 4))
AGG_SEAM_LENGTHS = (31, 64, 33, 0, 65, 1)                        # images start at the rows 0, 31, 95, 128, 128, 193
AGG_SEAM_KS = (33, 34, 255)


# ---------------------------------------------------------------------------------------------------------------- restatement
def half_norms(c):
    c = np.asarray(c, dtype=F32)
    h = np.zeros(len(c), dtype=F32)
    for e in range(DIM):
        h = (c[:, e].astype(F64) * c[:, e].astype(F64) + h.astype(F64)).astype(F32)
    return (F32(0.5) * h).astype(F32)


def dots32(x, c):
    """[n, K] fp32: the fmaf chain over ascending e."""
    x, c = np.asarray(x, dtype=F32), np.asarray(c, dtype=F32)
    acc = np.zeros((len(x), len(c)), dtype=F32)
    x64, c64 = x.astype(F64), c.astype(F64)
    for e in range(DIM):
        acc = (x64[:, e, None] * c64[None, :, e] + acc.astype(F64)).astype(F32)
    return acc


def scores32(x, c):
    return (dots32(x, c) - half_norms(c)[None, :]).astype(F32)


def assign32(x, c):
    """(assign int32 [n], score float32 [n]) as the kernel computes them; np.argmax takes the first of equal maxima."""
    s = scores32(x, c)
    a = np.argmax(s, axis=1).astype(np.int32)
    return a, s[np.arange(len(s)), a]


def scores64(x, c):
    x64, c64 = np.asarray(x, dtype=F32).astype(F64), np.asarray(c, dtype=F32).astype(F64)
    return x64 @ c64.T - 0.5 * (c64 * c64).sum(1)[None, :]


def chains_exact(x, c):
    """Every partial sum of every chain is exact in fp32: the fp32 chain and the fp64 chain agree at every step."""
    x64, c64 = np.asarray(x, dtype=F32).astype(F64), np.asarray(c, dtype=F32).astype(F64)
    acc, h = np.zeros((len(x64), len(c64))), np.zeros(len(c64))
    for e in range(DIM):
        acc = x64[:, e, None] * c64[None, :, e] + acc
        h = c64[:, e] * c64[:, e] + h
        if (acc.astype(F32).astype(F64) != acc).any() or (h.astype(F32).astype(F64) != h).any():
            return False
    s = acc - 0.5 * h[None, :]
    return bool((s.astype(F32).astype(F64) == s).all())


def banded(x, c):
    """bool [n] of the float family's band (module docstring); K = 1 has no second score."""
    x64, c64 = np.asarray(x, dtype=F32).astype(F64), np.asarray(c, dtype=F32).astype(F64)
    if len(c64) < 2:
        return np.zeros(len(x64), dtype=bool)
    s = np.sort(scores64(x, c), axis=1)
    cn = np.sqrt((c64 * c64).sum(1))
    bound = (DIM + 2) * EPS24 * (np.sqrt((x64 * x64).sum(1))[:, None] * cn[None, :] + 0.5 * cn[None, :] ** 2).max(1)
    return s[:, -1] - s[:, -2] <= 2 * bound


def two_best(x, c):
    """int [n, 2]: the two centroids of largest exact score (what a banded row may choose between)."""
    return np.argsort(-scores64(x, c), axis=1, kind="stable")[:, :2]


def _ordered_sum(rows):
    """fp32 sum of the rows [m, 128] in order; zeros for m = 0."""
    if len(rows) == 0:
        return np.zeros(DIM, dtype=F32)
    return np.cumsum(rows.astype(F32), axis=0, dtype=F32)[-1]


def residual_sums(x, offsets, c, a):
    """float32 [n_images, K, 128]: per image and centroid the in-order fp32 sum of (row - centroid)."""
    x, c = np.asarray(x, dtype=F32), np.asarray(c, dtype=F32)
    out = np.zeros((len(offsets) - 1, len(c), DIM), dtype=F32)
    for i in range(len(offsets) - 1):
        seg, sa = x[offsets[i]:offsets[i + 1]], a[offsets[i]:offsets[i + 1]]
        for j in np.unique(sa):
            out[i, j] = _ordered_sum((seg[sa == j] - c[j][None, :]).astype(F32))
    return out


def normalise64(v, norm):
    """float64 [K * 128] from one image's float32 [K, 128] sums; the kernel rounds this to fp32 once."""
    w = np.asarray(v, dtype=F32).astype(F64)
    if norm == "intra":
        bn = np.sqrt((w * w).sum(1, keepdims=True))
        w = np.divide(w, bn, out=np.zeros_like(w), where=bn > 0)
    elif norm == "ssr":
        w = np.sign(w) * np.sqrt(np.abs(w))
    else:
        assert norm == "none"
    g = np.sqrt((w * w).sum())
    return (w / g if g > 0 else np.zeros_like(w)).reshape(-1)


def vlad64(x, offsets, c, norm="intra", a=None):
    """float64 [n_images, K * 128] of the restatement (assignment by assign32 unless given)."""
    if a is None:
        a = assign32(x, c)[0] if len(x) else np.zeros(0, np.int32)
    v = residual_sums(x, offsets, c, a)
    return np.stack([normalise64(v[i], norm) for i in range(len(v))], 0)


def ulp32(want):
    """One fp32 ulp at |want| (0 where want is 0: a zero stays exactly zero)."""
    w = np.abs(np.asarray(want, dtype=F64)).astype(F32)
    return np.where(w == 0, 0.0, np.spacing(w).astype(F64))


def within_one_ulp(got, want):
    return bool((np.abs(np.asarray(got, dtype=F64) - np.asarray(want, dtype=F64)) <= ulp32(want)).all())


def kmeans_ref(x, start, max_iters):
    """[(centroids float32 [K, 128], counts int64 [K], moved, assign)] after every iteration that runs."""
    x = np.asarray(x, dtype=F32)
    c = np.array(start, dtype=F32)
    k, n = len(c), len(x)
    prev = np.full(n, -1, dtype=np.int32)
    out = []
    for _ in range(max_iters):
        a, _s = assign32(x, c)
        moved = int((a != prev).sum())
        sum64, counts = np.zeros((k, DIM)), np.zeros(k, dtype=np.int64)
        for r0 in range(0, n, CHUNK):
            seg, sa = x[r0:r0 + CHUNK], a[r0:r0 + CHUNK]
            for j in range(k):
                sum64[j] += _ordered_sum(seg[sa == j]).astype(F64)
                counts[j] += int((sa == j).sum())
        c = c.copy()
        live = counts > 0
        c[live] = (sum64[live] / counts[live, None].astype(F64)).astype(F32)
        out.append((c, counts, moved, a))
        prev = a
        if moved == 0:
            break
    return out


# ---------------------------------------------------------------------------------------------------------------- families
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _grid(v):
    return (np.round(v * 128.0) / 128.0).astype(F32)


def exact_family(seed, n, k):
    """(x float32 [n, 128], centroids float32 [k, 128]) on the 2^-7 grid.  Rows sit near centroids.  Designed ties where k allows:
    centroid 1 is centroid 0 with elements 0 and 1 swapped and the rows 0, 5, 10, .. are centroid 0 with equal elements 0 and 1 (the
    same score against both); the last centroid duplicates centroid 2 (k >= 4), or centroid 0 (k == 2)."""
    rs = np.random.RandomState(seed)
    c = _grid(_unit(rs.standard_normal((k, DIM))))
    if k >= 3:
        c[1] = c[0]
        c[1, [0, 1]] = c[0, [1, 0]]
    if k >= 4:
        c[k - 1] = c[2]
    if k == 2:
        c[1] = c[0]
    which = rs.randint(0, k, n)
    x = _grid(_unit(c[which] + 0.03 * rs.standard_normal((n, DIM))))
    if k >= 3:
        x[::5] = c[0]
        x[::5, 1] = x[::5, 0]
    assert np.sqrt((x.astype(F64) ** 2).sum(1)).max() <= 1.1 and np.sqrt((c.astype(F64) ** 2).sum(1)).max() <= 1.1
    return x, c


def float_family(seed, n, k, noise=0.05):
    """(x, centroids): unit-norm rows around k unit cluster centres (noise per component), centroids = the fp32 means of each
    cluster's rows (the centre itself for a cluster without rows)."""
    rs = np.random.RandomState(seed)
    centres = _unit(rs.standard_normal((k, DIM)))
    which = rs.randint(0, k, n)
    x = _unit(centres[which] + noise * rs.standard_normal((n, DIM))).astype(F32)
    c = centres.astype(F32)
    for j in range(k):
        if (which == j).any():
            c[j] = x[which == j].astype(F64).mean(0).astype(F32)
    return x, c


def kmeans_case(seed, n, k, noise, n_clusters=None, spread=False):
    """(x, start): rows around n_clusters (default k) unit centres in random order.  The start is k rows drawn by the seed as
    vlad.kmeans draws them, or with spread the first row of each of the clusters 0 .. k - 1: no cluster is cut in two."""
    rs = np.random.RandomState(seed)
    m = n_clusters or k
    centres = _unit(rs.standard_normal((m, DIM)))
    which = rs.randint(0, m, n)
    x = _unit(centres[which] + noise * rs.standard_normal((n, DIM))).astype(F32)
    rows = [int(np.nonzero(which == j)[0][0]) for j in range(k)] if spread else np.random.RandomState(seed).permutation(n)[:k]
    return x, x[rows].copy()


def separated(seed, n, k):
    """Tight clusters, one start row in each of k of the k + 1 clusters: the rows of the last cluster are shared out among the
    centroids and pull them along for a few iterations, and no cluster is cut in two (a cut runs through a cluster's middle, where
    rows score alike against both sides: banded rows)."""
    return kmeans_case(seed, n, k, 0.02, n_clusters=k + 1, spread=True)


def overlapping(seed, n, k):
    return kmeans_case(seed, n, k, 0.12)


def aggregate_case(seed, k, family="float", lengths=AGG_LENGTHS):
    """(x, offsets, centroids): images of the given lengths; with k >= 3 centroid k - 2 is moved far from every row, so no row chooses it, and
    the image of 31 rows (where there is one) holds copies of rows of ONE centroid's cluster."""
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(offsets[-1])
    x, c = (exact_family if family == "exact" else float_family)(seed, n, k)
    if k >= 3:
        c[k - 2] = F32(3) * c[k - 2]                     # s = 3 x . c - 4.5 |c|^2 < 0 even for its own cluster's rows
    if 31 in lengths:
        i = list(lengths).index(31)
        x[offsets[i]:offsets[i + 1]] = x[offsets[i]]
    return x, offsets, c


# ---------------------------------------------------------------------------------------------------------------- edge families
def covering_family(family, seed, n, k, noise=None):
    """(x, centroids) in which row i < k sits near centroid i, so that with n >= k every centroid wins a row; the further rows go
    to random centroids.  No centroid is duplicated.  exact: on the 2^-7 grid; float: unit rows, centroids = the means of their rows."""
    rs = np.random.RandomState(seed)
    centres = _unit(rs.standard_normal((k, DIM)))
    which = np.concatenate([np.arange(k), rs.randint(0, k, max(n - k, 0))])[:n]
    if family == "exact":
        c = _grid(centres)
        x = _grid(_unit(c[which] + (noise or 0.03) * rs.standard_normal((n, DIM))))
        assert np.sqrt((x.astype(F64) ** 2).sum(1)).max() <= 1.1 and np.sqrt((c.astype(F64) ** 2).sum(1)).max() <= 1.1
        return x, c
    x = _unit(centres[which] + (noise or 0.05) * rs.standard_normal((n, DIM))).astype(F32)
    c = centres.astype(F32)
    for j in np.unique(which):
        c[j] = x[which == j].astype(F64).mean(0).astype(F32)
    return x, c


def lane_tie_lanes(k):
    """The two lanes (column index mod 16) whose columns lane_tie_family makes equal: 15, whose last column is padding when k is no
    multiple of 16, and the lane of the last centroid -- or 2 where that is 15 again, or 0 or 1 (the exact family's centroid 1 is
    centroid 0 with two elements swapped: a row near one of them may sit nearer the other)."""
    return (15, (k - 1) % 16 if (k - 1) % 16 not in (15, 0, 1) else 2)


def lane_tie_family(seed, n, k):
    """(x, centroids, rows, want): the exact family with, for each lane lc of lane_tie_lanes(k), every centroid 16 nt + lc < k
    (nt >= 1) a copy of centroid lc -- all the columns one lane of the assignment kernel holds are equal -- and the rows
    1 + i, 9 + i, 17 + i, .. (i = 0, 1: the lane) near centroid lc.  `rows` are those rows, `want` the lc of each: the smallest
    index of its group."""
    x, c = exact_family(seed, n, k)
    rs = np.random.RandomState(seed + 1000)
    rows, want = [], []
    for i, lc in enumerate(lane_tie_lanes(k)):
        if lc >= k:
            continue
        for j in range(16 + lc, k, 16):
            c[j] = c[lc]
        r = np.arange(1 + i, n, 8)
        x[r] = _grid(_unit(c[lc] + 0.03 * rs.standard_normal((len(r), DIM))))
        rows.append(r)
        want.append(np.full(len(r), lc))
    assert np.sqrt((x.astype(F64) ** 2).sum(1)).max() <= 1.1
    if not rows:
        return x, c, np.zeros(0, np.int64), np.zeros(0, np.int64)
    return x, c, np.concatenate(rows), np.concatenate(want)


def all_equal_family(n, k, group=None):
    """(x, centroids, want): every centroid is one grid vector, so every row ties k ways and goes to centroid 0.  With `group` the
    centroids are equal in groups of that many consecutive indices and row i sits near the vector of group i mod (number of groups):
    it ties `group` ways and goes to the group's first index."""
    rs = np.random.RandomState(77)
    g = group or k
    n_groups = (k + g - 1) // g
    vec = _grid(_unit(rs.standard_normal((n_groups, DIM))))
    c = vec[np.arange(k) // g]
    which = np.arange(n) % n_groups
    x = _grid(_unit(vec[which] + 0.03 * rs.standard_normal((n, DIM))))
    assert np.sqrt((x.astype(F64) ** 2).sum(1)).max() <= 1.1
    return x, np.ascontiguousarray(c), (which * g).astype(np.int32)


def negative_family(seed, n, k):
    """(x, centroids): lane_tie_family with the centroids times 4 (a power of two: the chains stay exact).  Every score is
    4 x . c - 8 |c|^2, about -4 for the nearest centroid and -8 for the others: the 0 of a padding column would beat them all."""
    x, c, _, _ = lane_tie_family(seed, n, k)
    return x, (F32(4) * c).astype(F32)


def kmeans_wide_case(i):
    """(x, start, empty) of KMEANS_WIDE[i]: a separated case; `empty` is the centroid whose start row is multiplied by 3 as in
    aggregate_case (its score is negative even for its own cluster's rows, which the other centroids share out), or None."""
    seed, n, k, empty = KMEANS_WIDE[i]
    x, start = separated(seed, n, k)
    if empty is not None:
        start[empty] = F32(3) * start[empty]
    return x, start, empty


def aggregate_seam_case(seed, k, family):
    """(x, offsets, centroids, a, b): images of AGG_SEAM_LENGTHS; the image of 64 rows starts at row 31 and its first 32 rows sit
    near centroid a = k - 1, its last 32 near centroid b = 1 or 2, the one of the other parity (the other owner thread of the
    aggregation kernel): the assignment changes on the seam between the image's two 32-row tiles."""
    offsets = np.concatenate([[0], np.cumsum(AGG_SEAM_LENGTHS)]).astype(np.int64)
    n = int(offsets[-1])
    x, c = covering_family(family, seed, n, k)
    rs = np.random.RandomState(seed + 1000)
    a = k - 1
    b = 2 if a & 1 else 1
    r0 = int(offsets[1])
    for j, lo in ((a, r0), (b, r0 + 32)):
        v = _unit(c[j].astype(F64) / np.linalg.norm(c[j].astype(F64)) + (0.03 if family == "exact" else 0.05) * rs.standard_normal((32, DIM)))
        x[lo:lo + 32] = _grid(v) if family == "exact" else v.astype(F32)
    return x, offsets, c, a, b


# ---------------------------------------------------------------------------------------------------------------- retrieval scene
def make_scene(seed=SCENE_SEED, n_landmarks=600, n_db=40, n_query=12, n_seen=60, n_clutter=30, window=90, noise=0.05):
    """{'names': [...], 'desc': {name: float32 [90, 128]}, 'seen': {name: set of landmarks}}: images `db/%03d.jpg` whose windows of
    `window` consecutive landmarks are spread evenly over the landmarks, and `query/%03d.jpg` with windows at random places; an image
    holds n_seen landmarks of its window (noisy, unit norm) and n_clutter random unit descriptors, in random order."""
    rs = np.random.RandomState(seed)
    land = _unit(rs.standard_normal((n_landmarks, DIM)))
    names, desc, seen = [], {}, {}
    starts = [int(round(i * (n_landmarks - window) / (n_db - 1))) for i in range(n_db)] + list(rs.randint(0, n_landmarks - window + 1, n_query))
    for i, s in enumerate(starts):
        name = f"db/{i:03d}.jpg" if i < n_db else f"query/{i - n_db:03d}.jpg"
        ids = s + rs.choice(window, n_seen, replace=False)
        d = np.concatenate([_unit(land[ids] + noise * rs.standard_normal((n_seen, DIM))), _unit(rs.standard_normal((n_clutter, DIM)))], 0)
        names.append(name)
        desc[name] = np.ascontiguousarray(d[rs.permutation(len(d))], dtype=F32)
        seen[name] = set(int(v) for v in ids)
    return {"names": names, "desc": desc, "seen": seen}


def scene_names(scene):
    return sorted(n for n in scene["names"] if n.startswith("db")), sorted(n for n in scene["names"] if n.startswith("query"))


def most_overlapping(scene):
    """Per query (sorted names) the index, among the sorted db names, of the db image sharing the most landmarks (the first of equals)."""
    db, qs = scene_names(scene)
    return [int(np.argmax([len(scene["seen"][q] & scene["seen"][d]) for d in db])) for q in qs]


def scene_vocabulary(scene, k=SCENE_K, max_iters=SCENE_ITERS, seed=0):
    """The restatement of train_vocabulary on the scene's db images: (centroids, iterations run)."""
    db, _ = scene_names(scene)
    x = np.concatenate([scene["desc"][n] for n in db], 0)
    start = x[np.random.RandomState(seed).permutation(len(x))[:k]]
    its = kmeans_ref(x, start, max_iters)
    return its[-1][0], len(its)


def scene_descriptors(scene, centroids, norm="intra", dtype=F32):
    """(db [40, K * 128], query [12, K * 128]) of the restatement, rounded to fp32 once (or left in fp64)."""
    db, qs = scene_names(scene)
    one = lambda n: vlad64(scene["desc"][n], np.array([0, len(scene["desc"][n])]), centroids, norm)[0].astype(dtype)  # noqa: E731
    return np.stack([one(n) for n in db], 0), np.stack([one(n) for n in qs], 0)


def write_scene_store(scene, path):
    """The scene as a feature store: `descriptors` float64 [128, N] per image, as the extractor writes them."""
    from sfd2_amd import feature_io
    with feature_io.open_store(str(path), "w") as st:
        for n in scene["names"]:
            d = scene["desc"][n]
            feature_io.write_features(st, n, {"keypoints": np.zeros((len(d), 2)), "descriptors": np.ascontiguousarray(d.T.astype(F64)),
                                              "scores": np.ones(len(d)), "image_size": np.array([640, 480])})
