"""Numpy restatement of the three pair selections (sfd2_amd/pairs.py; hloc/pairs_from_retrieval.py, pairs_from_covisibility.py,
pairs_from_poses.py), the synthetic inputs the tests run them on, and the positions where two correct implementations may differ
("banded").  One tie rule throughout: the better score first, then the smaller candidate index.

Bands
  retrieval     rank position whose exact (fp64) similarity is within 2 d 2^-24 of a neighbour's in the ranking, the (k + 1)-th
                candidate included.  For unit-norm rows an fp32 dot product computed as any chain of fused or unfused
                multiply-adds lies within gamma_d sum |a_i b_i| <= d 2^-24 |a| |b| = d 2^-24 of the exact one, so two candidates
                further apart than twice that are ordered alike by every fp32 implementation.
  poses, dR     a pair with |dR - thr| <= 1e-6 thr: acos near cos(30 deg) amplifies the ~1e-16 rounding differences of the trace
                by ~2, far inside this; the band only has to be generous.  A position is banded when such a pair lies at or
                before it by distance.
  poses, dist   rank position whose distance is within 1e-9 relative of a ranking neighbour's.
  covisibility  rank position whose count equals a ranking neighbour's (the (k + 1)-th candidate included): the reference orders
                equal counts as an unstable sort over dict order leaves them.
"""
from collections import defaultdict

import numpy as np

EPS24 = 2.0 ** -24
# the cases of tests/golden/pairs.npz, tests/test_pairs_host.py and tests/test_gpu_pairs.py
RETRIEVAL_SHAPES = ((1, 200, 3001, 256, 20), (1, 65, 700, 100, 50), (1, 33, 1500, 512, 10))      # (seed, nq, nd, d, k)
COVIS_SEED, COVIS_KS = 7, (5, 64)
POSES_SEED, POSES_N, POSES_K, POSES_THR = 3, 300, 10, 30.0


# ---------------------------------------------------------------------------------------------------------------- generators
def make_descriptors(seed, nq, nd, d, n_clusters=None, noise=0.7):
    """(query [nq, d], db [nd, d]) fp32, unit norm: cluster centres plus noise."""
    rs = np.random.RandomState(seed)
    nc = n_clusters or max(2, nd // 40)
    centres = rs.standard_normal((nc, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)

    def draw(n):
        x = centres[rs.randint(0, nc, n)] + noise * rs.standard_normal((n, d)) / np.sqrt(d)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        return x.astype(np.float32)

    return draw(nq), draw(nd)


def descriptor_names(nq, nd):
    return [f"query/{i:05d}.jpg" for i in range(nq)], [f"db/{i:05d}.jpg" for i in range(nd)]


def make_incidence(seed, n_images=40, n_points=600, window=10, n_dup=12):
    """A map as CSRs only (no geometry): images on a line, tracks of 2-8 images drawn inside a sliding window, n_dup duplicated
    entries on either side, image n_images - 3 without points, image n_images - 2 with points nobody else sees.  Returns a dict:
    obs_offsets, obs_point, track_offsets, track_image, image_ids (unsorted, with gaps), point_ids (sorted, with gaps), names,
    empty (index of the image without points), lonely (index of the self-only image)."""
    rs = np.random.RandomState(seed)
    empty, lonely = n_images - 3, n_images - 2
    usable = np.array([i for i in range(n_images) if i not in (empty, lonely)])
    tracks = []
    for _ in range(n_points):
        s = rs.randint(0, len(usable) - 1)
        win = usable[s:s + window]
        length = min(rs.randint(2, 9), len(win))
        tracks.append(list(rs.choice(win, length, replace=False)))
    for _ in range(25):                                      # the lonely image's own points: tracks of one
        tracks.append([lonely])
    for p in rs.choice(n_points, n_dup, replace=False):     # a point that lists one of its images twice
        tracks[p].append(tracks[p][0])
    obs = [[] for _ in range(n_images)]
    for p, t in enumerate(tracks):
        for im in sorted(set(t)):
            obs[im].append(p)
    for im in rs.choice(usable, n_dup, replace=True):       # an image with two key points on one point
        obs[im].append(obs[im][rs.randint(0, len(obs[im]))])
    for im in range(n_images):
        rs.shuffle(obs[im])
    oo = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    image_ids = (rs.permutation(n_images) * 3 + 5).astype(np.int64)
    return {"obs_offsets": oo, "obs_point": np.concatenate([np.asarray(o, dtype=np.int32) for o in obs]).astype(np.int32),
            "track_offsets": to, "track_image": np.concatenate([np.asarray(t, dtype=np.int32) for t in tracks]).astype(np.int32),
            "image_ids": image_ids, "point_ids": np.arange(len(tracks), dtype=np.int64) * 2 + 11,
            "names": np.array([f"db/im{int(i):04d}.jpg" for i in image_ids]), "empty": empty, "lonely": lonely}


def incidence_to_model(inc, Image, Point3D):
    """The incidence as the dicts of a COLMAP model (Image / Point3D: the record types of the reader in use).  Key points carry
    every observation in CSR order with a -1 between any two; dict order is the CSR's image order."""
    images, points3D = {}, {}
    for i, iid in enumerate(inc["image_ids"]):
        rows = inc["obs_point"][inc["obs_offsets"][i]:inc["obs_offsets"][i + 1]]
        pid = np.full(2 * len(rows) + 1, -1, dtype=np.int64)
        pid[1::2] = inc["point_ids"][rows]
        images[int(iid)] = Image(id=int(iid), qvec=np.array([1.0, 0, 0, 0]), tvec=np.array([float(i), 0, 0]), camera_id=1,
                                 name=str(inc["names"][i]), xys=np.zeros((len(pid), 2)), point3D_ids=pid)
    for r, pid in enumerate(inc["point_ids"]):
        t = inc["track_image"][inc["track_offsets"][r]:inc["track_offsets"][r + 1]]
        points3D[int(pid)] = Point3D(id=int(pid), xyz=np.zeros(3), rgb=np.zeros(3, np.uint8), error=0.0,
                                     image_ids=inc["image_ids"][t].astype(np.int32), point2D_idxs=np.zeros(len(t), np.int32))
    return images, points3D


def permute_incidence(inc, perm):
    """The same map with image perm[i] at position i."""
    perm = np.asarray(perm)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    obs = [inc["obs_point"][inc["obs_offsets"][p]:inc["obs_offsets"][p + 1]] for p in perm]
    out = dict(inc)
    out["obs_offsets"] = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int64)
    out["obs_point"] = np.concatenate(obs).astype(np.int32)
    out["track_image"] = inv[inc["track_image"]].astype(np.int32)
    out["image_ids"], out["names"] = inc["image_ids"][perm], inc["names"][perm]
    out["empty"], out["lonely"] = int(inv[inc["empty"]]), int(inv[inc["lonely"]])
    return out


def rotmat2qvec(R):
    """A unit quaternion (w, x, y, z) of a rotation matrix (largest-component branch)."""
    tr = np.trace(R)
    cand = np.array([tr, R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]])
    b = int(np.argmax(cand))
    if b == 0:
        q = np.array([1 + tr, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif b == 1:
        q = np.array([R[2, 1] - R[1, 2], 1 + cand[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif b == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1 + cand[2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1 + cand[3]])
    q = q / np.linalg.norm(q)
    return q if q[0] >= 0 else -q


def make_poses(seed, n=300):
    """(qvec [n, 4], tvec [n, 3]) world to camera: centres along a serpentine path inside a 21 x 9 field (so that |position| < 25
    and neighbours are ~0.7 apart), yaw uniform in +-40 degrees, a few degrees of pitch and roll."""
    rs = np.random.RandomState(seed)
    q, t = np.zeros((n, 4)), np.zeros((n, 3))
    for i in range(n):
        row, col = divmod(i, 30)
        x = 0.7 * (col if row % 2 == 0 else 29 - col)
        c = np.array([x + rs.uniform(-0.1, 0.1), 0.9 * row + rs.uniform(-0.1, 0.1), rs.uniform(-0.05, 0.05)])
        yaw, pitch, roll = np.deg2rad(rs.uniform(-40, 40)), np.deg2rad(rs.uniform(-3, 3)), np.deg2rad(rs.uniform(-3, 3))
        Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        Ry = np.array([[np.cos(pitch), 0, np.sin(pitch)], [0, 1, 0], [-np.sin(pitch), 0, np.cos(pitch)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(roll), -np.sin(roll)], [0, np.sin(roll), np.cos(roll)]])
        R = Rx @ Ry @ Rz
        q[i] = rotmat2qvec(R)
        t[i] = -qvec2rotmat(q[i]) @ c
    return q, t


# ------------------------------------------------------------------------------------- inputs whose answer is decided (top-k seams)
# the cases of tests/test_gpu_pairs_topk.py, guarded without a GPU by tests/test_pairs_host.py
TOPK_EXACT = (70, 600, 16)                                                    # (nq, nd, d) of exact_descriptors(TOPK_EXACT_SEED, ...)
TOPK_EXACT_SEED = 21
TOPK_EXACT_KS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
# (nq, nd, d, k, splits): d = 1 and k = nd; a db row alone in the second tile, d one past a 16-group, everybody selected; d one past
# a 32-chunk, a row alone in the second query strip; the vector loader below 16 columns with the largest LDS request; the vector
# loader with a partial second group; 65 tiles over 64 splits
TOPK_EXACT_SHAPES = ((3, 64, 1, 64, 0), (5, 129, 17, 129, 0), (65, 257, 33, 129, 0), (2, 256, 4, 256, 0), (1, 128, 20, 128, 0),
                     (130, 8300, 8, 200, 64))
TOPK_GENERAL = ((11, 70, 300, 64, 256), (12, 65, 257, 33, 129), (15, 130, 1000, 20, 193))       # (seed, nq, nd, d, k) of make_descriptors
TOPK_ORDER = (17, 600, 64)                                                    # (seed, nd, d): one query, the db rows reordered
TOPK_ORDER_KS = (64, 65, 256)
TOPK_DENSE_SEED, TOPK_DENSE_KS = 3, (63, 64, 65, 128, 129, 192, 193, 255, 256)
TOPK_STAR_SIZES, TOPK_STAR_KS = (63, 64, 65, 127, 128, 129, 255, 256, 257), (64, 128, 256)
TOPK_ORDERED_N = 300
TOPK_FIELD_SEED, TOPK_FIELD_N, TOPK_FIELD_KS = 5, 1100, (1024, 1023, 961, 960, 513, 320)
TOPK_DUP_GROUPS = ([5, 280, 555, 830, 1099], [10, 11], list(range(300, 370)))  # the first: one member in each wave's quarter
TOPK_LINE_KS = (64, 1024)


def exact_descriptors(seed, nq, nd, d):
    """(query [nq, d], db [nd, d]) fp32 with entries from {-1, 0, 1}: every product and partial sum is a small integer, so every
    fp32 summation order, fused or not, gives the exact similarity, and nearly every neighbouring pair of a ranking is a tie."""
    rs = np.random.RandomState(seed)
    return rs.randint(-1, 2, (nq, d)).astype(np.float32), rs.randint(-1, 2, (nd, d)).astype(np.float32)


def reorder_by_similarity(query_row, db, direction):
    """db with its rows permuted so that the exact similarity to query_row ascends with the row ('ascending'), descends
    ('descending'), or takes the two halves of the ascending order in turns ('interleaved')."""
    sim = db.astype(np.float64) @ np.asarray(query_row, dtype=np.float64)
    order = np.argsort(sim, kind="stable")
    if direction == "descending":
        order = order[::-1]
    elif direction == "interleaved":
        half = (len(order) + 1) // 2
        mixed = np.empty_like(order)
        mixed[0::2], mixed[1::2] = order[:half], order[half:]
        order = mixed
    elif direction != "ascending":
        raise ValueError(direction)
    return np.ascontiguousarray(db[order])


def _csr(obs, tracks):
    oo = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    cat = lambda parts: np.concatenate([np.asarray(p, dtype=np.int32) for p in parts]).astype(np.int32)  # noqa: E731
    return {"obs_offsets": oo, "obs_point": cat(obs), "track_offsets": to, "track_image": cat(tracks)}


def _csr_of_tracks(n_images, tracks):
    obs = [[] for _ in range(n_images)]
    for p, t in enumerate(tracks):
        for im in t:
            obs[im].append(p)
    return _csr(obs, tracks)


def dense_incidence(seed, n_images=400, n_points=30000, track=(2, 5)):
    """A map in which every image shares points with most others: each track is a uniform draw of track[0] .. track[1] distinct
    images.  The CSR arrays of make_incidence."""
    rs = np.random.RandomState(seed)
    tracks = [rs.choice(n_images, rs.randint(track[0], track[1] + 1), replace=False) for _ in range(n_points)]
    return _csr_of_tracks(n_images, tracks)


def star_incidence(sizes):
    """One hub image per entry m of sizes, sharing exactly one point with each of m partners of its own (no partner serves two
    hubs, partners share nothing with each other): every count of a hub is 1, its order is index order and its n_found is m.  A hub
    sits in the middle of its partners' index range.  The CSR arrays plus 'hubs' (the hub's index per entry)."""
    tracks, hubs, base = [], [], 0
    for m in sizes:
        hub = base + m // 2
        hubs.append(hub)
        tracks.extend([hub, j] for j in range(base, base + m + 1) if j != hub)
        base += m + 1
    out = _csr_of_tracks(base, tracks)
    out["hubs"] = np.asarray(hubs)
    return out


def ordered_incidence(n, direction):
    """Image 0 shares j + 1 points ('ascending') or n - j points ('descending') with image j = 1 .. n - 1, and nobody shares anything
    else: in index order every count of row 0 is a new best, or none is."""
    if direction not in ("ascending", "descending"):
        raise ValueError(direction)
    tracks = []
    for j in range(1, n):
        tracks.extend([0, j] for _ in range(j + 1 if direction == "ascending" else n - j))
    return _csr_of_tracks(n, tracks)


def pose_field(seed, n, dup_groups=()):
    """(qvec [n, 4], tvec [n, 3]): yaw uniform in +-10 degrees (any two images within 20 degrees of each other), centres uniform in
    a cube of side 40.  dup_groups: index lists whose rows become bit-identical copies, qvec and tvec, of the list's first row."""
    rs = np.random.RandomState(seed)
    yaw = np.deg2rad(rs.uniform(-10, 10, n))
    centres = rs.uniform(-20, 20, (n, 3))
    q, t = np.zeros((n, 4)), np.zeros((n, 3))
    for i in range(n):
        q[i] = [np.cos(yaw[i] / 2), 0.0, 0.0, np.sin(yaw[i] / 2)]
        t[i] = -qvec2rotmat(q[i]) @ centres[i]
    for group in dup_groups:
        q[group[1:]], t[group[1:]] = q[group[0]], t[group[0]]
    return q, t


def pose_line(n, direction):
    """(qvec, tvec): identity rotations, image 0 at the origin and image j at x = n - j ('decreasing': in index order every image
    is nearer to image 0 than all before it) or x = j ('increasing').  Neighbouring distances from image 0 differ by 1 in at most n."""
    if direction not in ("decreasing", "increasing"):
        raise ValueError(direction)
    q, t = np.zeros((n, 4)), np.zeros((n, 3))
    q[:, 0] = 1.0
    j = np.arange(1, n)
    t[1:, 0] = -(n - j if direction == "decreasing" else j)       # the position is -R t = -t
    return q, t


def _sequential_topk(scores, k, indices=None):
    """(profile of insertion_profile, the final list as [(score, index)], best first)."""
    import bisect
    scores = np.asarray(scores)
    indices = np.arange(len(scores)) if indices is None else np.asarray(indices)
    keys, profile = [], []                                       # keys: (-score, index) ascending = best first
    for s, i in zip(scores.tolist(), indices.tolist()):
        key = (-s, i)
        if len(keys) == k and not key < keys[-1]:
            continue
        pos = bisect.bisect_left(keys, key)
        profile.append((pos // 64, min(len(keys), k - 1) // 64))
        keys.insert(pos, key)
        del keys[k:]
    return profile, [(-a, b) for a, b in keys]


def insertion_profile(scores_in_offer_order, k, indices=None):
    """'Keep the k best, better score first then smaller index', restated as a sequential insertion (indices default to the offer
    position).  For every accepted candidate (pos // 64, min(len_before, k - 1) // 64): the register of the device's list (entry p in
    lane p & 63 of register p >> 6) the candidate lands in, and the last register its insertion shifts.  A guard for the tests'
    inputs, not a reference."""
    return _sequential_topk(scores_in_offer_order, k, indices)[0]


def retrieval_offers(sim_row, splits, k):
    """The sequences of (scores, indices) that the retrieval kernels offer to pairs_topk_scan for one query row: per split the
    similarities of its 128-row tiles in row order, then the merge's concatenation of the splits' lists."""
    nd = len(sim_row)
    tiles = (nd + 127) // 128
    splits = max(1, min(splits, tiles, 64))
    offers, merged_s, merged_i = [], [], []
    for s in range(splits):
        c0, c1 = min(nd, (s * tiles // splits) * 128), min(nd, ((s + 1) * tiles // splits) * 128)
        offers.append((sim_row[c0:c1], np.arange(c0, c1)))
        kept = _sequential_topk(sim_row[c0:c1], k, np.arange(c0, c1))[1]
        merged_s.extend(x for x, _ in kept)
        merged_i.extend(i for _, i in kept)
    offers.append((np.asarray(merged_s), np.asarray(merged_i, dtype=np.int64)))
    return offers


def poses_offers(dist_row, valid_row, k):
    """The same for the poses kernel and one image: four waves take a quarter of the images each, then wave 0 is offered the lists
    of waves 1 to 3 in turn.  Scores are -distance; the merge's three sequences come last."""
    n = len(dist_row)
    lists, offers = [], []
    for w in range(4):
        j = np.arange(w * n // 4, (w + 1) * n // 4)
        j = j[valid_row[j]]
        offers.append((-dist_row[j], j))
        lists.append(_sequential_topk(-dist_row[j], k, j)[1])
    for w in range(1, 4):
        offers.append((np.array([s for s, _ in lists[w]]), np.array([i for _, i in lists[w]], dtype=np.int64)))
    return offers, lists[0]


def profile_of_offers(offers, k, start=()):
    """The classes insertion_profile reports when the sequences of offers[...] go into one list in turn (start: the list's content
    before the first), and the number of accepted candidates."""
    scores = np.concatenate([np.asarray([s for s, _ in start], dtype=np.float64)] + [np.asarray(s, dtype=np.float64) for s, _ in offers])
    idx = np.concatenate([np.asarray([i for _, i in start], dtype=np.int64)] + [np.asarray(i, dtype=np.int64) for _, i in offers])
    profile = insertion_profile(scores, k, idx)[len(start):]
    return set(profile), len(profile)


# ---------------------------------------------------------------------------------------------------------------- restatement
def _rank(score, valid=None):
    """Candidate indices of one row by (score descending, index ascending); invalid ones dropped."""
    idx = np.arange(len(score))
    if valid is not None:
        idx = idx[valid]
    return idx[np.lexsort((idx, -score[idx]))]


def retrieval_ref(query, db, k):
    """{'idx' [nq, k], 'exact' [nq, k + 1] (fp64 similarity of the ranking's first k + 1, -inf where there is no (k + 1)-th),
    'band' bool [nq, k], 'sim64' [nq, nd]}."""
    q64, d64 = np.asarray(query, dtype=np.float64), np.asarray(db, dtype=np.float64)
    sim = q64 @ d64.T
    nq, nd = sim.shape
    d = q64.shape[1]
    idx = np.zeros((nq, k), dtype=np.int64)
    exact = np.full((nq, k + 1), -np.inf)
    for i in range(nq):
        r = _rank(sim[i])[:k + 1]
        idx[i] = r[:k]
        exact[i, :len(r)] = sim[i, r]
    near = np.abs(np.diff(exact, axis=1)) <= 2 * d * EPS24         # [nq, k]: position p against p + 1
    band = near.copy()
    band[:, 1:] |= near[:, :-1]
    return {"idx": idx, "exact": exact, "band": band, "sim64": sim}


def covisibility_counts(inc, i):
    """Counts of image i against every image, duplicates on both sides counted."""
    cnt = np.zeros(len(inc["obs_offsets"]) - 1, dtype=np.int64)
    for p in inc["obs_point"][inc["obs_offsets"][i]:inc["obs_offsets"][i + 1]]:
        t = inc["track_image"][inc["track_offsets"][p]:inc["track_offsets"][p + 1]]
        np.add.at(cnt, t[t != i], 1)
    return cnt


def covisibility_ref(inc, k):
    """{'idx' [n, k] (-1 beyond n_found), 'count' [n, k], 'n_found' [n], 'band' bool [n, k], 'counts' [n, n]}."""
    n = len(inc["obs_offsets"]) - 1
    idx = np.full((n, k), -1, dtype=np.int64)
    count = np.zeros((n, k), dtype=np.int64)
    nf = np.zeros(n, dtype=np.int64)
    band = np.zeros((n, k), dtype=bool)
    allc = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        c = covisibility_counts(inc, i)
        allc[i] = c
        r = _rank(c.astype(np.float64), c > 0)
        m = min(k, len(r))
        idx[i, :m], count[i, :m], nf[i] = r[:m], c[r[:m]], m
        ext = c[r[:k + 1]]
        for p in np.nonzero(np.diff(ext) == 0)[0]:           # position p ties with p + 1
            band[i, p] = True
            if p + 1 < k:
                band[i, p + 1] = True
    return {"idx": idx, "count": count, "n_found": nf, "band": band, "counts": allc}


def covisibility_loops(inc, k):
    """The same selection shaped as the reference's loops (a dict of counters per image, filled element by element): the host
    baseline of tools/pairs_bench.py.  Returns the list of (i, j) pairs."""
    oo, op, to, ti = (inc[x] for x in ("obs_offsets", "obs_point", "track_offsets", "track_image"))
    pairs = []
    for i in range(len(oo) - 1):
        covis = defaultdict(int)
        for p in op[oo[i]:oo[i + 1]]:
            for j in ti[to[p]:to[p + 1]]:
                if j != i:
                    covis[j] += 1
        if not covis:
            continue
        ids = np.array(list(covis.keys()))
        num = np.array([covis[j] for j in ids])
        order = np.lexsort((ids, -num))[:k]
        pairs.extend((i, int(j)) for j in ids[order])
    return pairs


def qvec2rotmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def pose_tables(qvec, tvec, true_centres=False):
    """(dist [n, n], dR degrees [n, n]) in fp64.  The position is -R t as the reference computes it (it multiplies by R before it
    transposes), or the camera centre -R^T t."""
    R = np.stack([qvec2rotmat(q) for q in np.asarray(qvec, dtype=np.float64)])
    t = np.asarray(tvec, dtype=np.float64)
    p = -np.einsum("nji,nj->ni", R, t) if true_centres else -np.einsum("nij,nj->ni", R, t)
    diff = p[:, None, :] - p[None, :, :]
    dist = np.sqrt(diff[..., 0] ** 2 + diff[..., 1] ** 2 + diff[..., 2] ** 2)
    trace = np.einsum("nab,mab->nm", R, R)
    dR = np.rad2deg(np.abs(np.arccos(np.clip((trace - 1) / 2, -1.0, 1.0))))
    return dist, dR


def poses_ref(qvec, tvec, k, thr=30.0, true_centres=False):
    """{'idx' [n, k] (-1 beyond n_found), 'dist' [n, k] (inf beyond), 'n_found' [n], 'band' bool [n, k], 'rot_band' bool [n, n],
    'dist_all', 'dR'}."""
    dist, dR = pose_tables(qvec, tvec, true_centres)
    n = len(dist)
    valid = dR < thr
    np.fill_diagonal(valid, False)
    rot_band = np.abs(dR - thr) <= 1e-6 * abs(thr)
    np.fill_diagonal(rot_band, False)
    idx = np.full((n, k), -1, dtype=np.int64)
    out = np.full((n, k), np.inf)
    nf = np.zeros(n, dtype=np.int64)
    band = np.zeros((n, k), dtype=bool)
    for i in range(n):
        r = _rank(-dist[i], valid[i])
        m = min(k, len(r))
        idx[i, :m], out[i, :m], nf[i] = r[:m], dist[i, r[:m]], m
        ext = dist[i, r[:k + 1]]
        near = np.abs(np.diff(ext)) <= 1e-9 * ext[1:]
        for p in np.nonzero(near)[0]:
            band[i, p] = True
            if p + 1 < k:
                band[i, p + 1] = True
        rb = dist[i, rot_band[i]]
        if len(rb):
            first = rb.min()
            band[i] |= ~(out[i] < first * (1 - 1e-9))        # every position at or behind the nearest gate-banded pair, unfilled ones too
    return {"idx": idx, "dist": out, "n_found": nf, "band": band, "rot_band": rot_band, "dist_all": dist, "dR": dR}


def poses_loops(qvec, tvec, k, thr=30.0):
    """The selection shaped as the reference's: full tables, then per row a partition and a sort of its part (the host baseline of
    tools/pairs_bench.py).  Returns the list of (i, j) pairs."""
    dist, dR = pose_tables(qvec, tvec)
    valid = dR < thr
    np.fill_diagonal(valid, False)
    dist = np.where(valid, dist, np.inf)
    pairs = []
    for i in range(len(dist)):
        part = np.argpartition(dist[i], k)[:k]
        part = part[np.argsort(dist[i][part])]
        pairs.extend((i, int(j)) for j in part[valid[i][part]])
    return pairs


# ---------------------------------------------------------------------------------------------------------------- comparison
def rows_agree(got_idx, want_idx, band):
    """Outside banded positions the two index tables are equal."""
    got_idx, want_idx = np.asarray(got_idx, dtype=np.int64), np.asarray(want_idx, dtype=np.int64)
    return bool((got_idx[~band] == want_idx[~band]).all())


def banded_rows_consistent(got_idx, want_idx, band, score_of, strictly_better_of):
    """Inside the band: per row the multisets of scores over the banded positions are equal, and every candidate strictly better
    than the row's k-th is present.  score_of(i, idx array) -> scores; strictly_better_of(i) -> set of candidate indices."""
    for i in np.nonzero(band.any(axis=1))[0]:
        g, w = np.asarray(got_idx[i]), np.asarray(want_idx[i])
        gb, wb = g[band[i] & (g >= 0)], w[band[i] & (w >= 0)]
        if len(gb) != len(wb) or not np.array_equal(np.sort(score_of(i, gb)), np.sort(score_of(i, wb))):
            return False
        if not set(strictly_better_of(i)) <= set(g[g >= 0].tolist()):
            return False
    return True


def parse_pairs_text(text):
    """[(name0, name1)] of a pairs file's content."""
    return [tuple(line.split(" ")) for line in text.split("\n")] if text else []
