"""pairs_topk_scan (sfd2_amd/csrc/pairs_kernels.hip) at its seams, on the MI355X: the sorted list of one wave, entry p in lane p & 63 of
register p >> 6, through its five call sites -- retrieval's tile epilogue and split merge (float, 4 registers), covisibility (int, 4)
and the per-wave pass and wave merge of poses (double, 16).  List lengths around every multiple of 64 up to the limits (256, 256,
1024), inputs that are mostly ties, candidates offered in ascending, descending and interleaved order of score, descriptor widths
around the loader's 16-groups and 32-chunks, both loaders on the same data.

The inputs are generated (tests/pairs_ref.py) so that the answer is decided: integer-valued similarities and counts are compared at
every position, everything else outside the bands of pairs_ref's docstring.  tests/test_pairs_host.py checks without a GPU that the
inputs are what they claim, the caps on the banded share, and that the cases insert into, and shift across, every register."""
import functools

import numpy as np
import pytest

import pairs_ref as pr
from test_gpu_pairs import _check_retrieval

pytestmark = pytest.mark.gpu


def _P():
    from sfd2_amd import pairs
    return pairs


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------------------------------------------------------- retrieval
@functools.lru_cache(maxsize=None)
def _exact(nq, nd, d):
    q, db = pr.exact_descriptors(pr.TOPK_EXACT_SEED, nq, nd, d)
    sim64 = q.astype(np.float64) @ db.astype(np.float64).T + 0.0          # + 0.0: a sum of products that is -0 on the host is +0 here
    ranking = np.stack([pr._rank(row) for row in sim64])
    return q, db, sim64, ranking


def _check_exact(idx, sim, sim64, ranking, k, what):
    """Integer similarities: the index table is the ranking's at every position and sim is float32(sim64) bit for bit."""
    assert idx.shape == (len(sim64), k) and idx.dtype == np.int32 and sim.dtype == np.float32
    want = ranking[:, :k]
    wrong = idx.astype(np.int64) != want
    ties = np.mean(np.diff(sim64[np.arange(len(sim64))[:, None], ranking[:, :k + 1]], axis=1) == 0) if ranking.shape[1] > 1 else 0.0
    print(f"retrieval, exact arithmetic, {what}: positions unlike the ranking {int(wrong.sum())} of {wrong.size}, equal neighbours {ties:.3f}")
    assert not wrong.any(), (what, np.argwhere(wrong)[:5].tolist())
    assert np.array_equal(_bits(sim), _bits(sim64[np.arange(len(sim64))[:, None], want].astype(np.float32))), what


@pytest.mark.parametrize("splits", (0, 1))
@pytest.mark.parametrize("k", pr.TOPK_EXACT_KS)
def test_retrieval_exact_arithmetic_every_list_length(k, splits):
    """600 db rows are 5 tiles.  splits = 0 lets the call choose (5: one tile each, the merge builds every list beyond 128);
    splits = 1 has the tile epilogue hold all k entries."""
    q, db, sim64, ranking = _exact(*pr.TOPK_EXACT)
    idx, sim = _P().retrieval_topk(q, db, k, splits=splits)
    _check_exact(idx, sim, sim64, ranking, k, f"70 x 600 x 16, k = {k}, splits = {splits}")


@pytest.mark.parametrize("shape", pr.TOPK_EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_retrieval_exact_arithmetic_shapes(shape):
    nq, nd, d, k, splits = shape
    q, db, sim64, ranking = _exact(nq, nd, d)
    idx, sim = _P().retrieval_topk(q, db, k, splits=splits)
    _check_exact(idx, sim, sim64, ranking, k, f"{nq} x {nd} x {d}, k = {k}, splits = {splits}")
    if k == nd:
        assert all(sorted(r.tolist()) == list(range(nd)) for r in idx)


def test_retrieval_lists_that_only_the_merge_fills():
    """300 db rows are 3 tiles: at 3 splits no split sees 256 candidates, at 2 one does not, at 1 the epilogue holds them all."""
    seed, nq, nd, d, k = pr.TOPK_GENERAL[0]
    q, db = pr.make_descriptors(seed, nq, nd, d)
    outs = [_P().retrieval_topk(q, db, k, splits=s) for s in (1, 2, 3)]
    for (idx, sim), s in zip(outs[1:], (2, 3)):
        assert np.array_equal(idx, outs[0][0]) and np.array_equal(_bits(sim), _bits(outs[0][1])), s
    _check_retrieval(*outs[2], q, db, pr.retrieval_ref(q, db, k), k)


@pytest.mark.parametrize("case", (1, 2))
def test_retrieval_general_descriptors_at_odd_widths(case):
    seed, nq, nd, d, k = pr.TOPK_GENERAL[case]
    q, db = pr.make_descriptors(seed, nq, nd, d)
    idx, sim = _P().retrieval_topk(q, db, k)
    _check_retrieval(idx, sim, q, db, pr.retrieval_ref(q, db, k), k)


def test_retrieval_vector_and_scalar_loader_give_the_same_bits():
    import torch
    seed, nq, nd, d, _ = pr.TOPK_GENERAL[0]
    q, db = pr.make_descriptors(seed, nq, nd, d)

    def on_device(a, shift):
        buf = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[shift:shift + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.is_contiguous() and view.data_ptr() % 16 == 4 * shift
        assert view.detach().to(torch.float32).contiguous().data_ptr() == view.data_ptr()      # what the wrapper does: no copy
        return view

    qa, dba, qu, dbu = on_device(q, 0), on_device(db, 0), on_device(q, 1), on_device(db, 1)
    assert qu.data_ptr() % 16 == 4 and dbu.data_ptr() % 16 == 4
    for k in (20, 256):
        ai, as_ = _P().retrieval_topk(qa, dba, k)
        for other in ((qu, dbu), (qu, dba), (qa, dbu)):                   # one misaligned pointer is enough for the scalar loader
            ui, us = _P().retrieval_topk(*other, k)
            assert np.array_equal(ai, ui) and np.array_equal(_bits(as_), _bits(us)), k
        hi, hs = _P().retrieval_topk(q, db, k)                            # and the host arrays, uploaded by the call
        assert np.array_equal(ai, hi) and np.array_equal(_bits(as_), _bits(hs)), k


@pytest.mark.parametrize("direction", ("ascending", "descending", "interleaved"))
def test_retrieval_offer_order(direction):
    """One query against 600 db rows sorted by their similarity to it.  Ascending: every row is a new best, goes in at position 0 and
    pushes the whole list through every register seam.  splits = 1 shows that order to the tile epilogue, 0 to the merge as well."""
    seed, nd, d = pr.TOPK_ORDER
    q, db = pr.make_descriptors(seed, 1, nd, d)
    db2 = pr.reorder_by_similarity(q[0], db, direction)
    for k in pr.TOPK_ORDER_KS:
        ref = pr.retrieval_ref(q, db2, k)
        for splits in (1, 0):
            idx, sim = _P().retrieval_topk(q, db2, k, splits=splits)
            _check_retrieval(idx, sim, q, db2, ref, k)              # the band rule, and sim non-increasing with equal values by ascending row


# ---------------------------------------------------------------------------------------------------------------- covisibility
def _device_covis(inc, k, global_counters):
    return _P().covisibility_topk_csr(inc["obs_offsets"], inc["obs_point"], inc["track_offsets"], inc["track_image"], k, global_counters=global_counters)


def _cut(ref, k):
    """The restatement at a smaller k: the first k columns of the same ranking."""
    return ref["idx"][:, :k], ref["count"][:, :k], np.minimum(ref["n_found"], k)


def _check_covis(inc, ref, k):
    want = _cut(ref, k)
    outs = []
    for global_counters in (False, True):
        got = _device_covis(inc, k, global_counters)
        for g, w, name in zip(got, want, ("idx", "count", "n_found")):
            assert np.array_equal(g, w), (name, k, global_counters, np.argwhere(np.asarray(g) != np.asarray(w))[:5].tolist())
        outs.append(got)
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    return outs[0]


@functools.lru_cache(maxsize=None)
def _dense():
    inc = pr.dense_incidence(pr.TOPK_DENSE_SEED)
    return inc, pr.covisibility_ref(inc, 256)


@pytest.mark.parametrize("k", pr.TOPK_DENSE_KS)
def test_covisibility_full_lists_of_tied_counts(k):
    inc, ref = _dense()
    idx, cnt, nf = _check_covis(inc, ref, k)
    print(f"covisibility, dense map, k = {k}: n_found {nf.min()} .. {nf.max()}, positions tied with a neighbour {np.mean(np.diff(cnt, axis=1) == 0):.3f}")
    assert (nf == k).all()


@functools.lru_cache(maxsize=None)
def _star():
    inc = pr.star_incidence(pr.TOPK_STAR_SIZES)
    return inc, pr.covisibility_ref(inc, 256)


@pytest.mark.parametrize("k", pr.TOPK_STAR_KS)
def test_covisibility_all_ties_cut_at_a_seam(k):
    inc, ref = _star()
    idx, cnt, nf = _check_covis(inc, ref, k)
    assert nf[inc["hubs"]].tolist() == [min(m, k) for m in pr.TOPK_STAR_SIZES]
    for hub, m in zip(inc["hubs"], pr.TOPK_STAR_SIZES):                   # the partners of smallest index, in index order
        partners = [j for j in range(hub - m // 2, hub - m // 2 + m + 1) if j != hub]
        assert idx[hub, :min(m, k)].tolist() == partners[:k] and (cnt[hub, :min(m, k)] == 1).all()
        assert (idx[hub, min(m, k):] == -1).all() and (cnt[hub, min(m, k):] == 0).all()


@functools.lru_cache(maxsize=None)
def _ordered(direction):
    inc = pr.ordered_incidence(pr.TOPK_ORDERED_N, direction)
    return inc, pr.covisibility_ref(inc, 256)


@pytest.mark.parametrize("direction", ("ascending", "descending"))
def test_covisibility_offer_order(direction):
    n = pr.TOPK_ORDERED_N
    inc, ref = _ordered(direction)
    for k in (64, 65, 256):
        idx, cnt, nf = _check_covis(inc, ref, k)
        best = list(range(n - 1, n - 1 - k, -1)) if direction == "ascending" else list(range(1, k + 1))
        assert nf[0] == k and idx[0].tolist() == best and cnt[0].tolist() == [n - j if direction == "descending" else j + 1 for j in best]
        assert (nf[1:] == 1).all() and (idx[1:, 0] == 0).all()


@pytest.mark.parametrize("n_images,global_counters,second", ((600, True, 88), (2100, False, 52)))
def test_covisibility_workgroups_that_take_a_second_image(n_images, global_counters, second):
    """512 workgroups on the global counters, 2048 on the LDS ones: the images beyond them find their counters zeroed again."""
    inc = pr.make_incidence(pr.COVIS_SEED, n_images=n_images, n_points=2 * n_images)
    assert n_images - (512 if global_counters else 2048) == second
    obs = np.diff(inc["obs_offsets"])
    ref = pr.covisibility_ref(inc, 5)
    idx, cnt, nf = _device_covis(inc, 5, global_counters)
    print(f"covisibility, {n_images} images, {obs.mean():.1f} observations per image: {second} workgroups take a second image")
    assert 8 <= obs.mean() <= 12
    assert np.array_equal(nf, ref["n_found"]) and np.array_equal(idx, ref["idx"]) and np.array_equal(cnt, ref["count"])


# ---------------------------------------------------------------------------------------------------------------- poses
def _check_fill_and_order(idx, dist, nf, k):
    filled = np.arange(k)[None, :] < nf[:, None]
    assert (idx[~filled] == -1).all() and np.isinf(dist[~filled]).all() and (dist[~filled] > 0).all()
    assert (idx[filled] >= 0).all() and np.isfinite(dist[filled]).all()
    ordered = np.where(filled, dist, np.inf)
    assert (ordered[:, 1:] >= ordered[:, :-1]).all()
    return filled


@functools.lru_cache(maxsize=None)
def _field(dups):
    return pr.pose_field(pr.TOPK_FIELD_SEED, pr.TOPK_FIELD_N, pr.TOPK_DUP_GROUPS if dups else ())


def _field_ref(dups, k):
    q, t = _field(dups)
    return q, t, pr.poses_ref(q, t, k, 30.0)


@pytest.mark.parametrize("k", pr.TOPK_FIELD_KS)
def test_poses_long_lists(k):
    q, t, ref = _field_ref(False, k)
    idx, dist, nf = _P().poses_topk_arrays(q, t, k, 30.0)
    assert np.array_equal(nf, ref["n_found"]) and (nf == k).all()
    assert not ref["band"].any() and pr.rows_agree(idx, ref["idx"], ref["band"])         # tests/test_pairs_host.py: nothing is banded
    filled = _check_fill_and_order(idx, dist, nf, k)
    rows = np.nonzero(filled)[0]
    exact = ref["dist_all"][rows, idx[filled]]
    rel = np.abs(dist[filled] - exact) / exact
    print(f"poses n = {len(q)}, k = {k}: max relative distance error {rel.max():.3e}")
    # tests/test_gpu_pairs.py's bound: positions are sums of three products of magnitude < 35 (error < 2e-14 absolute) and no two
    # images are nearer than 0.1
    assert exact.min() > 0.1 and rel.max() <= 1e-12


@pytest.mark.parametrize("k", (1024, 10))
def test_poses_duplicated_images(k):
    """Bit-identical copies have bit-equal distances from everybody: only the index orders them, across the waves' quarters too."""
    q, t, ref = _field_ref(True, k)
    n = len(q)
    idx, dist, nf = _P().poses_topk_arrays(q, t, k, 30.0)
    assert np.array_equal(nf, ref["n_found"]) and (nf == k).all()
    print(f"poses n = {n} with duplicate groups, k = {k}: banded positions {ref['band'].mean():.4f}, equal to the restatement {np.mean(idx == ref['idx']):.4f}")
    assert pr.rows_agree(idx, ref["idx"], ref["band"])
    _check_fill_and_order(idx, dist, nf, k)
    assert all(len(set(r.tolist())) == k and i not in r for i, r in enumerate(idx))
    straddles = 0
    for group in pr.TOPK_DUP_GROUPS:
        member = np.isin(idx, group)
        for i in range(n):
            pos = np.nonzero(member[i])[0]
            if not len(pos):
                continue
            assert pos[-1] - pos[0] == len(pos) - 1, (i, pos)            # consecutive positions
            got = idx[i, pos]
            assert (np.diff(got) > 0).all() and len(set(_bits(dist[i, pos]).tolist())) == 1
            others = [j for j in group if j != i]
            assert got.tolist() == others[:len(pos)]                     # the group's smallest indices
            if len(pos) < len(others):                                   # only because the cut goes through the group
                assert pos[-1] == k - 1
                straddles += 1
            if i in group:                                               # its own copies come first, at distance 0
                assert pos[0] == 0 and (dist[i, pos] == 0).all()
    print(f"  rows in which the cut goes through a group: {straddles}")
    assert straddles > 0 or k == 1024
    # the restatement breaks ties by index too, copies have the same distances on both sides, and tests/test_pairs_host.py shows that
    # nothing else is banded: the tables are equal
    assert np.array_equal(idx, ref["idx"])


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5))
def test_poses_fewer_images_than_waves(n):
    q, t = pr.pose_field(9, 8)
    q, t = q[:n], t[:n]
    for k in (1, 4, 64):
        ref = pr.poses_ref(q, t, k, 181.0)
        idx, dist, nf = _P().poses_topk_arrays(q, t, k, 181.0)
        assert (nf == min(k, n - 1)).all() and not ref["band"].any() and np.array_equal(idx, ref["idx"])
        _check_fill_and_order(idx, dist, nf, k)


@pytest.mark.parametrize("direction", ("decreasing", "increasing"))
def test_poses_offer_order(direction):
    n = pr.TOPK_FIELD_N
    q, t = pr.pose_line(n, direction)
    for k in pr.TOPK_LINE_KS:
        ref = pr.poses_ref(q, t, k, 30.0)
        assert not ref["band"][0].any() and ref["n_found"][0] == k
        idx, dist, nf = _P().poses_topk_arrays(q, t, k, 30.0)
        assert nf[0] == k and np.array_equal(idx[0], ref["idx"][0])
        near = list(range(n - 1, n - 1 - k, -1)) if direction == "decreasing" else list(range(1, k + 1))
        assert idx[0].tolist() == near
        # integer coordinates: every distance is exact on both sides, so the other rows (where images j - d and j + d tie) are
        # equal to the restatement as well
        assert np.array_equal(nf, ref["n_found"]) and (nf == k).all() and np.array_equal(idx, ref["idx"])
        assert (np.abs(dist - ref["dist"]) <= 1e-12 * ref["dist"]).all()
        _check_fill_and_order(idx, dist, nf, k)
