"""sfd2_covis_clusters on the MI355X against the restatement of tests/cluster_ref.py, cluster for cluster in order: list lengths at
the word and wave boundaries of the bit matrix, the shapes of map that break a wrong closure or a wrong order, the global-slot path
against the LDS table, batch independence byte for byte, and the input checks."""
import numpy as np
import pytest

import cluster_ref as clr

pytestmark = pytest.mark.gpu


def _mods():
    from sfd2_amd import _lib, covis, pairs
    return _lib, covis, pairs


def _raw(csr, off, frames, flags=0, fill=-7):
    """The C call on arrays.  Returns (rc, message, cluster, n_clusters); the outputs are pre-filled."""
    _lib, _, _ = _mods()
    oo, op, to, ti = [np.ascontiguousarray(a) for a in csr]
    off = np.ascontiguousarray(off, dtype=np.int64)
    frames = np.ascontiguousarray(frames, dtype=np.int32)
    cluster = np.full(max(len(frames), 1), fill, dtype=np.int32)
    n_clusters = np.full(max(len(off) - 1, 1), fill, dtype=np.int32)
    ctx = _lib.default_context(0)
    rc = ctx.lib.sfd2_covis_clusters(ctx.h, oo.ctypes.data, op.ctypes.data, len(oo) - 1, to.ctypes.data, ti.ctypes.data, len(to) - 1, off.ctypes.data,
                                     frames.ctypes.data, len(off) - 1, cluster.ctypes.data, n_clusters.ctypes.data, flags)
    return rc, ctx.lib.sfd2_last_error().decode(), cluster[:len(frames)], n_clusters[:len(off) - 1]


def _check(images, points3D, lists, mi=None):
    """Both table placements against the restatement, for every list."""
    _lib, covis, _ = _mods()
    mi = mi or covis.MapIndex(images, points3D)
    want = [clr.clusters(li, images, points3D) for li in lists]
    got = mi.clusters(lists)
    assert got == want
    assert mi.clusters(lists, global_slots=True) == want
    return want


@pytest.fixture(scope="module")
def big():
    """300 images: components of many sizes, noise images, a last image that observes nothing."""
    sizes = [40, 31, 25, 20, 17, 17, 12, 9, 9, 8, 7, 6, 5, 5, 4, 4, 3, 3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1] + [1] * 27
    images, points3D, comps = clr.planted_map(sizes, seed=4, noise_images=30, noise_points=80)
    _, covis, _ = _mods()
    assert len(images) == 300
    return images, points3D, comps, covis.MapIndex(images, points3D)


@pytest.mark.parametrize("k", [0, 1, 2, 63, 64, 65, 255, 256])
def test_list_lengths(big, k):
    images, points3D, comps, mi = big
    order = np.random.RandomState(k).permutation(np.arange(1, 301))
    li = [int(v) for v in order[:k]]
    want = _check(images, points3D, [li], mi)[0]
    assert sum(len(c) for c in want) == k and (k < 63 or len(want) > 10)
    if k == 0:
        assert want == []


def test_257_frames_is_an_error(big):
    images, points3D, comps, mi = big
    with pytest.raises(RuntimeError, match="more than 256"):
        mi.clusters([list(range(1, 258))])


def test_chain_through_256_frames_in_shuffled_order():
    images, points3D = clr.chain_map(256, extra_images=2)
    li = [int(v) + 1 for v in np.random.RandomState(1).permutation(256)]
    want = _check(images, points3D, [li, li[:200], list(range(1, 257))])
    assert want[0] == [li] and len(want[1]) > 20


def test_ties_keep_creation_order():
    images, points3D, comps = clr.planted_map([3, 3, 2, 2, 1], seed=3)
    for s in range(4):
        li = [i + 1 for i in clr.interleave(comps, seed=s)]
        want = _check(images, points3D, [li])[0]
        assert [len(c) for c in want] == [3, 3, 2, 2, 1]
        first = [li.index(c[0]) for c in want]
        assert first[0] < first[1] and first[2] < first[3]


def test_isolated_frames_and_one_cluster():
    images, points3D, comps = clr.planted_map([1] * 70, seed=5)
    li = [i + 1 for i in clr.interleave(comps, seed=1)]
    assert _check(images, points3D, [li])[0] == [[f] for f in li]
    images, points3D, comps = clr.planted_map([90], seed=6)
    li = [i + 1 for i in clr.interleave(comps, seed=2)]
    assert _check(images, points3D, [li])[0] == [li]


def test_a_map_without_points():
    """Three images, no point (obs_point and track_image are empty arrays), one query listing two of them: two clusters of one."""
    images, points3D = clr.build_map(3, [])
    assert _check(images, points3D, [[1, 3]])[0] == [[1], [3]]


def test_first_and_last_image_empty_frame_outside_partners_and_short_tracks(big):
    images, points3D, comps, mi = big
    n = len(images)
    assert (images[n].point3D_ids != -1).sum() == 0                 # the last image observes nothing
    noise = [i for i in range(1, n) if all(i - 1 not in c for c in comps)]
    partners = {int(b) for p in images[noise[0]].point3D_ids if p != -1 for b in points3D[int(p)].image_ids} - {noise[0]}
    assert partners and any(len(p.image_ids) == 1 for p in points3D.values())
    li = [n, 1, noise[0], 2, 3, comps[-1][0] + 1]                   # noise[0]'s points are seen by images outside the list only
    assert not partners & set(li)
    want = _check(images, points3D, [li], mi)[0]
    assert [n] in want and [noise[0]] in want and len(want[0]) >= 2


def test_directed_rule():
    images, points3D = clr.one_way_map()
    lists = [[1, 2], [2, 1], [1, 2, 3, 4, 5, 6], [4, 1, 2, 3], [2, 4, 1, 3], [6]]
    want = _check(images, points3D, lists)
    assert want[0] == [[1, 2]] and want[1] == [[2], [1]] and want[3] == [[4, 1, 2], [3]]


@pytest.mark.parametrize("n_images", ["bound", "bound + 1"])
def test_table_switches_to_global_above_the_lds_bound(n_images):
    """The same small map, padded with images that observe nothing, and one link to the very last image."""
    _lib, covis, pairs = _mods()
    n = _lib.CLUSTER_LDS_IMAGES + (1 if n_images == "bound + 1" else 0)
    images, points3D, comps = clr.planted_map([6, 4, 4, 1], seed=7, noise_images=4, noise_points=6)
    ids, oo, op, to, ti = pairs.covisibility_csr(images, points3D)
    small = len(ids)
    # one more point: observed by image 0 and by image n - 1, track (0, n - 1)
    op2 = np.concatenate([[len(to) - 1], op, [len(to) - 1]]).astype(np.int32)
    oo2 = np.concatenate([[0], oo[1:] + 1, np.full(n - small - 1, oo[-1] + 1), [oo[-1] + 2]]).astype(np.int64)
    to2 = np.concatenate([to, [to[-1] + 2]]).astype(np.int64)
    ti2 = np.concatenate([ti, [0, n - 1]]).astype(np.int32)
    li = [i for i in clr.interleave(comps, seed=3)] + [n - 1, n - 2]
    want = clr.clusters([i + 1 for i in li[:-2]], images, points3D)
    base = [[i - 1 for i in c] for c in want]
    with0 = next(c for c in base if 0 in c)
    expect = sorted([c for c in base if c is not with0] + [with0 + [n - 1], [n - 2]], key=lambda c: -len(c))   # sorted() is stable
    rc, msg, cluster, ncl = _raw((oo2, op2, to2, ti2), [0, len(li)], li)
    assert rc == 0, msg
    got = covis.MapIndex.clusters_from_ranks([li], np.array([0, len(li)]), cluster, ncl)[0]
    assert got == expect                                            # cluster for cluster, ties and members in order


def test_batch_composition_and_order_do_not_change_a_byte(big):
    _lib, covis, _ = _mods()
    images, points3D, comps, mi = big
    rs = np.random.RandomState(11)
    lens = [0, 1, 2, 5, 17, 0, 50, 63, 64, 65, 100, 256, 3, 0, 200, 31] * 4
    lists = [[int(v) for v in rs.permutation(np.arange(1, 301))[:k]] for k in lens]
    _, off, frames = mi.cluster_lists(lists)
    csr = mi.csr()[1:]
    results = {}
    for flags in (0, _lib.CLUSTER_FLAG_GLOBAL_SLOTS):
        rc, msg, cl, ncl = _raw(csr, off, frames, flags)
        assert rc == 0, msg
        results[flags] = (cl, ncl)
        perm = rs.permutation(len(lists))
        _, off_p, frames_p = mi.cluster_lists([lists[i] for i in perm])
        rc, msg, cl_p, ncl_p = _raw(csr, off_p, frames_p, flags)
        assert rc == 0, msg
        for j, i in enumerate(perm):
            assert cl_p[off_p[j]:off_p[j + 1]].tobytes() == cl[off[i]:off[i + 1]].tobytes() and ncl_p[j] == ncl[i]
        for i in range(len(lists)):                                   # each query alone
            rc, msg, c1, n1 = _raw(csr, [0, len(lists[i])], frames[off[i]:off[i + 1]], flags)
            assert rc == 0 and c1.tobytes() == cl[off[i]:off[i + 1]].tobytes() and n1[0] == ncl[i]
    assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1].tobytes() == results[1][1].tobytes()
    want = [clr.clusters(li, images, points3D) for li in lists]
    assert covis.MapIndex.clusters_from_ranks(lists, off, *results[0]) == want
    assert all(results[0][1][i] == 0 for i, k in enumerate(lens) if k == 0)


def test_more_queries_than_workgroups(big):
    images, points3D, comps, mi = big
    rs = np.random.RandomState(12)
    lists = [[int(v) for v in rs.choice(np.arange(1, 301), rs.randint(0, 5), replace=False)] for _ in range(600)]
    _check(images, points3D, lists, mi)


def test_bad_inputs_return_an_error_and_write_nothing(big):
    _lib, covis, _ = _mods()
    images, points3D, comps, mi = big
    oo, op, to, ti = mi.csr()[1:]
    off, frames = np.array([0, 3, 5]), np.array([0, 1, 2, 3, 4])

    def bad(csr=(oo, op, to, ti), off=off, frames=frames, flags=0, text=""):
        rc, msg, cl, ncl = _raw(csr, off, frames, flags)
        assert rc == -1 and text in msg and msg.startswith("sfd2_covis_clusters: ")
        assert (cl == -7).all() and (ncl == -7).all()

    def edit(a, i, v):
        a = a.copy()
        a[i] = v
        return a
    bad(csr=(edit(oo, 5, oo[6] + 1), op, to, ti), text="obs_offsets")
    bad(csr=(oo, op, edit(to, 9, to[8] - 1), ti), text="track_offsets")
    bad(off=np.array([0, 4, 3, 5]), text="frame_offsets")
    bad(off=np.array([1, 3, 5]), text="frame_offsets")
    bad(csr=(oo, edit(op, 7, len(to) - 1), to, ti), text="point row out of range")
    bad(csr=(oo, edit(op, 7, -1), to, ti), text="point row out of range")
    bad(csr=(oo, op, to, edit(ti, 3, len(oo) - 1)), text="image index out of range")
    bad(csr=(oo, op, to, edit(ti, 3, -2)), text="image index out of range")
    bad(frames=np.array([0, 1, len(oo) - 1, 3, 4]), text="query 0: image index out of range")
    bad(frames=np.array([0, 1, 2, 3, -1]), text="query 1: image index out of range")
    bad(frames=np.array([0, 1, 0, 3, 4]), text="lists image 0 twice")
    bad(off=np.array([0, 257]), frames=np.arange(257) % 300, text="more than 256")
    bad(flags=2, text="unknown flags")
    # the same image in two different queries is no repeat
    rc, msg, cl, ncl = _raw((oo, op, to, ti), off, np.array([0, 1, 2, 0, 1]))
    assert rc == 0, msg
