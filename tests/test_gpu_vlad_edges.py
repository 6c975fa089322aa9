"""The VLAD kernels on the MI355X at the shapes tests/test_gpu_vlad.py does not reach: every accumulator count of vlad_assign_kernel
with both sides of each seam between two of them, blocks that take a second and a third tile, ties inside one lane and among
up to 256 columns, rows whose best score is negative (a zero padding column would win), k-means (sums mode) at K = 1, odd and
large K and over 17 chunks, and the entry points' and drivers' rarer paths.  The generators and what they claim: tests/vlad_ref.py,
checked without a GPU by tests/test_vlad_host.py.

Tolerances are those of tests/test_gpu_vlad.py: exact families bit for bit (assignment and score), float families equal outside
the band and one of the two best inside it, vectors within one fp32 ulp of vlad64 from the device's assignment, k-means bit for bit."""
import functools

import numpy as np
import pytest

import vlad_ref as vr

pytestmark = pytest.mark.gpu

NORMS = ("intra", "ssr", "none")


def _V():
    from sfd2_amd import vlad
    return vlad


def _exact_want(x, c):
    """(assign int32, score float32) of a case whose chains are exact: the fp64 scores are the kernel's bits."""
    s64 = vr.scores64(x, c)
    want_s = s64.max(1).astype(np.float32)
    assert (want_s.astype(np.float64) == s64.max(1)).all()
    return np.argmax(s64, axis=1).astype(np.int32), want_s


def _assert_exact(x, c, want_a, want_s, ns, what):
    k = len(c)
    for n in ns:
        a, s = _V().assign(x[:n], c)
        assert a.dtype == np.int32 and s.dtype == np.float32 and a.shape == s.shape == (n,)
        assert a.min() >= 0 and a.max() < k, (what, n)
        np.testing.assert_array_equal(a, want_a[:n], err_msg=f"{what} n = {n}")
        assert s.tobytes() == want_s[:n].tobytes(), (what, n)


def _assert_float(x, c, ns, what):
    k = len(c)
    s64, band, best = vr.scores64(x, c), vr.banded(x, c), vr.two_best(x, c)
    want_a = np.argmax(s64, axis=1)
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    cn = np.sqrt((c64 * c64).sum(1))
    for n in ns:
        a, s = _V().assign(x[:n], c)
        assert a.min() >= 0 and a.max() < k, (what, n)
        np.testing.assert_array_equal(a[~band[:n]], want_a[:n][~band[:n]], err_msg=f"{what} n = {n}")
        for i in np.nonzero(band[:n])[0]:
            assert a[i] in best[i]
        bound = (vr.DIM + 2) * vr.EPS24 * (np.sqrt((x64[:n] ** 2).sum(1)) * cn[a] + 0.5 * cn[a] ** 2)
        err = np.abs(s.astype(np.float64) - s64[np.arange(n), a])
        assert (err <= bound).all(), (what, n, err.max())
    return want_a, band


# ------------------------------------------------------------------------------------------------------------------ every NT
@pytest.mark.parametrize("k", vr.EDGE_KS)
def test_assign_exact_families_at_every_accumulator_count(k):
    n = max(vr.EDGE_NS)
    x, c = vr.covering_family("exact", 20 + k, n, k)
    want_a, want_s = _exact_want(x, c)
    assert sorted(set(want_a.tolist())) == list(range(k))             # every column of every accumulator tile wins a row
    _assert_exact(x, c, want_a, want_s, vr.EDGE_NS, "covering")
    x, c = vr.exact_family(20 + k, n, k)                              # and with the designed ties 0 / 1 and 2 / k - 1
    want_a, want_s = _exact_want(x, c)
    assert (want_a[::5] == 0).all()
    _assert_exact(x, c, want_a, want_s, vr.EDGE_NS, "exact")


@pytest.mark.parametrize("k", vr.EDGE_KS)
def test_assign_float_families_at_every_accumulator_count(k):
    x, c = vr.covering_family("float", 20 + k, max(vr.EDGE_NS), k)
    want_a, band = _assert_float(x, c, vr.EDGE_NS, "covering")
    assert sorted(set(want_a[~band].tolist())) == list(range(k))
    x, c = vr.float_family(20 + k, 1000, k)
    _, band1000 = _assert_float(x, c, vr.EDGE_NS + (1000,), "float")
    print(f"assign float K = {k}: banded rows {int(band.sum())} of {len(band)} (covering), {int(band1000.sum())} of 1000")


# ------------------------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("k", vr.LANE_TIE_KS)
def test_assign_ties_inside_one_lane_go_to_the_smallest_index(k):
    x, c, rows, lane = vr.lane_tie_family(30 + k, 257, k)
    want_a, want_s = _exact_want(x, c)
    np.testing.assert_array_equal(want_a[rows], lane)
    assert len(rows) >= 2 * (257 // 8)
    _assert_exact(x, c, want_a, want_s, (65, 257), "lane ties")


@pytest.mark.parametrize("k,group", [(16, None), (17, None), (256, None), (96, 16)])
def test_assign_many_way_ties_go_to_the_first_of_the_group(k, group):
    x, c, want = vr.all_equal_family(257, k, group)
    want_a, want_s = _exact_want(x, c)
    np.testing.assert_array_equal(want_a, want)
    _assert_exact(x, c, want_a, want_s, (63, 257), "equal centroids")


# ------------------------------------------------------------------------------------------------------------------ negative scores
@pytest.mark.parametrize("k", vr.NEGATIVE_KS)
def test_negative_scores_keep_the_padding_columns_out(k):
    n = 257
    x, c = vr.negative_family(40 + k, n, k)
    want_a, want_s = _exact_want(x, c)
    assert (want_s < 0).all()
    _assert_exact(x, c, want_a, want_s, (65, n), "negative")
    _, s = _V().assign(x, c)
    assert (s < 0).all()
    offsets = np.array([0, 31, 64, 64, n])
    for norm in NORMS:
        out, a = _V().aggregate(x, offsets, c, norm=norm, return_assign=True)
        np.testing.assert_array_equal(a, want_a)
        want = vr.vlad64(x, offsets, c, norm, a)
        for i in range(len(want)):
            assert vr.within_one_ulp(out[i], want[i]), (norm, i, np.abs(out[i] - want[i]).max())
        assert (out[2] == 0).all() and np.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------------------ large n
@functools.lru_cache(maxsize=None)
def _large():
    x, c = vr.exact_family(50, max(vr.LARGE_NS), 17)
    return (x, c) + _exact_want(x, c)


def _assert_large(x, c, want_a, want_s):
    import torch
    n = len(x)
    a, s = _V().assign(x, c)
    for r, name in ((65535, "row 65 535, the last of the grid's first pass"), (65536, "row 65 536, the first of a block's second tile"), (n - 1, "the last row")):
        assert a[r] == want_a[r] and s[r:r + 1].tobytes() == want_s[r:r + 1].tobytes(), f"{name}: got {a[r]} ({s[r]}), want {want_a[r]} ({want_s[r]})"
    np.testing.assert_array_equal(a, want_a)
    assert s.tobytes() == want_s.tobytes()
    a1, s1 = _V().assign(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda())
    assert a1.tobytes() == a.tobytes() and s1.tobytes() == s.tobytes()


@pytest.mark.parametrize("n", vr.LARGE_NS)
def test_assign_blocks_that_take_further_tiles(n):
    x, c, want_a, want_s = _large()
    assert (n + 63) // 64 > 1024 and n % 64 == 1
    _assert_large(x[:n], c, want_a[:n], want_s[:n])


def test_assign_lane_ties_in_a_second_tile():
    x, c, rows, lane = vr.lane_tie_family(51, vr.LARGE_NS[0], 35)
    want_a, want_s = _exact_want(x, c)
    np.testing.assert_array_equal(want_a[rows], lane)
    assert (rows >= 65536).any()
    _assert_large(x, c, want_a, want_s)


# ------------------------------------------------------------------------------------------------------------------ k-means
def _assert_kmeans(got, its, upto):
    cen, counts, moved = got
    assert moved.tolist() == [v[2] for v in its[:upto]]
    assert cen.tobytes() == its[upto - 1][0].tobytes()
    np.testing.assert_array_equal(counts, its[upto - 1][1])


def test_kmeans_large_equals_restatement():
    import torch
    seed, n, k = vr.KMEANS_LARGE
    x, start = vr.separated(seed, n, k)
    its = vr.kmeans_ref(x, start, 20)
    moved = [v[2] for v in its]
    print(f"large k-means: moved per iteration {moved}")
    assert 3 <= len(its) < 20 and moved[0] == n and 0 < moved[1] < n and moved[-1] == 0
    xd = torch.from_numpy(x).cuda()
    _assert_kmeans(_V().kmeans_from(xd, start, max_iters=1), its, 1)
    _assert_kmeans(_V().kmeans_from(xd, start, max_iters=2), its, 2)
    _assert_kmeans(_V().kmeans_from(x, start, max_iters=20), its, len(its))


@pytest.mark.parametrize("i", range(len(vr.KMEANS_WIDE)))
def test_kmeans_wide_equals_restatement(i):
    seed, n, k, empty = vr.KMEANS_WIDE[i]
    x, start, _ = vr.kmeans_wide_case(i)
    its = vr.kmeans_ref(x, start, 20)
    assert its[-1][2] == 0 and len(its) < 20
    got = _V().kmeans_from(x, start, max_iters=20)
    _assert_kmeans(got, its, len(its))
    cen, counts, moved = got
    assert counts.sum() == n and moved[0] == n
    if k == 1:
        assert moved.tolist() == [n, 0]
    if empty is not None:
        assert counts[empty] == 0 and cen[empty].tobytes() == start[empty].tobytes() and (n + vr.CHUNK - 1) // vr.CHUNK >= 3
        assert (np.delete(counts, empty) > 0).all()


# ------------------------------------------------------------------------------------------------------------------ aggregation
@pytest.mark.parametrize("family", ("exact", "float"))
@pytest.mark.parametrize("k", vr.AGG_SEAM_KS)
def test_aggregate_with_an_assignment_change_on_the_tile_seam(k, family):
    x, offsets, c, ca, cb = vr.aggregate_seam_case(60 + k, k, family)
    s64 = vr.scores64(x, c)
    band = vr.banded(x, c) if family == "float" else np.zeros(len(x), dtype=bool)
    lengths = np.diff(offsets)
    assert int(offsets[1]) % 32 != 0 and (ca & 1) != (cb & 1)
    for norm in NORMS:
        out, a = _V().aggregate(x, offsets, c, norm=norm, return_assign=True)
        assert out.shape == (len(lengths), k * vr.DIM) and np.isfinite(out).all()
        np.testing.assert_array_equal(a[~band], np.argmax(s64, axis=1)[~band])
        assert (a[31:63] == ca).all() and (a[63:95] == cb).all()
        want = vr.vlad64(x, offsets, c, norm, a)
        for i in range(len(want)):
            assert vr.within_one_ulp(out[i], want[i]), (norm, i, np.abs(out[i] - want[i]).max())
        assert (out[lengths == 0] == 0).all()
        blocks = out.reshape(len(out), k, vr.DIM)
        assert sorted(np.nonzero((blocks[1] != 0).any(1))[0].tolist()) == sorted((ca, cb))


def test_aggregate_a_batch_of_empty_images():
    x, offsets, c = vr.aggregate_case(13, 17)
    first = _V().aggregate(x, offsets, c)                              # the work space holds vectors that are not zero
    for k in (17, 255):
        ck = vr.covering_family("float", 3, 300, k)[1]
        out = _V().aggregate(np.zeros((0, vr.DIM), np.float32), [0, 0, 0, 0], ck)
        assert out.shape == (3, k * vr.DIM) and out.dtype == np.float32 and (out == 0).all()
    again = _V().aggregate(x, offsets, c)
    assert again.tobytes() == first.tobytes() and (again != 0).any()


# ------------------------------------------------------------------------------------------------------------------ errors
def test_misaligned_and_non_finite_inputs_raise_and_leave_the_context_usable():
    import torch
    n, k = 257, 17
    x, c = vr.float_family(1, n, k)
    band, want = vr.banded(x, c), np.argmax(vr.scores64(x, c), axis=1)

    def good():
        a, _ = _V().assign(x, c)
        np.testing.assert_array_equal(a[~band], want[~band])

    def shifted(v):
        """The same values on the device, 4 bytes past a 16-byte boundary."""
        t = torch.empty(v.size + 1, dtype=torch.float32).cuda()[1:].view(*v.shape)
        t.copy_(torch.from_numpy(v))
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t

    good()
    xs, cs = shifted(x), shifted(c)
    calls = (("assign", lambda: _V().assign(xs, c)), ("assign", lambda: _V().assign(x, cs)), ("aggregate", lambda: _V().aggregate(xs, [0, 100, n], c)),
             ("aggregate", lambda: _V().aggregate(x, [0, 100, n], cs)), ("kmeans", lambda: _V().kmeans_from(xs, c)))
    for name, call in calls:
        with pytest.raises(RuntimeError, match=f"sfd2_vlad_{name}: device inputs must be 16-byte aligned"):
            call()
        good()

    inf_x, nan_c, nan_last, nan_c_last = x.copy(), c.copy(), x.copy(), c.copy()
    inf_x[100, 7] = np.inf
    nan_c[5, 64] = np.nan
    nan_last[-1, -1] = np.nan                                          # the very last element the finite check reads of x
    nan_c_last[-1, -1] = np.nan                                        # and of the centroids
    assert (n * vr.DIM) % 256 != 0
    for bx, bc in ((inf_x, c), (x, nan_c), (nan_last, c), (x, nan_c_last), (-inf_x, c)):
        with pytest.raises(RuntimeError, match="sfd2_vlad_assign: non-finite"):
            _V().assign(bx, bc)
        good()
        with pytest.raises(RuntimeError, match="sfd2_vlad_aggregate: non-finite"):
            _V().aggregate(bx, [0, 100, n], bc)
        good()
        with pytest.raises(RuntimeError, match="sfd2_vlad_kmeans: non-finite"):
            _V().kmeans_from(bx, bc)
        good()
    with pytest.raises(RuntimeError, match="sfd2_vlad_assign: non-finite"):
        _V().assign(torch.from_numpy(nan_last).cuda(), torch.from_numpy(c).cuda())
    good()


# ------------------------------------------------------------------------------------------------------------------ drivers
def _store_arrays(path):
    from sfd2_amd import feature_io
    with feature_io.open_store(str(path), "r") as st:
        return {n: np.array(st[n]["global_descriptor"].__array__()) for n in sorted(st.keys())}


def test_global_features_in_several_batches_and_a_batch_of_empty_images(tmp_path, monkeypatch):
    from sfd2_amd import global_features
    scene = vr.make_scene()
    feats, voc = tmp_path / "feats.h5", tmp_path / "voc.npz"
    vr.write_scene_store(scene, feats)
    global_features.main(feats, tmp_path / "one.h5", voc, train=True, train_prefix="db", k=vr.SCENE_K, max_iters=vr.SCENE_ITERS)
    one = _store_arrays(tmp_path / "one.h5")
    assert sorted(one) == sorted(scene["names"]) and all((v != 0).any() for v in one.values())

    calls = []
    aggregate = global_features.vlad.aggregate
    monkeypatch.setattr(global_features.vlad, "aggregate", lambda x, offsets, *a, **kw: calls.append(np.diff(offsets).tolist()) or aggregate(x, offsets, *a, **kw))
    need = 4 * vr.DIM * (90 + vr.SCENE_K)                              # what main counts for an image of 90 descriptors
    monkeypatch.setattr(global_features, "BATCH_BYTES", 3 * need)
    global_features.main(feats, tmp_path / "many.h5", voc)
    many = _store_arrays(tmp_path / "many.h5")
    assert [len(b) for b in calls] == [3] * 17 + [1]                   # 52 images, three to a batch
    assert sorted(many) == sorted(one) and all(many[n].tobytes() == one[n].tobytes() for n in one)

    extra = dict(scene, names=scene["names"] + ["db/017a.jpg", "db/017b.jpg"], desc=dict(scene["desc"]))
    for name in extra["names"][-2:]:
        extra["desc"][name] = np.zeros((0, vr.DIM), np.float32)
    feats2 = tmp_path / "feats2.h5"
    vr.write_scene_store(extra, feats2)
    del calls[:]
    monkeypatch.setattr(global_features, "BATCH_BYTES", 2 * 4 * vr.DIM * vr.SCENE_K)     # room for the two empty images, for no other two
    global_features.main(feats2, tmp_path / "holes.h5", voc)
    holes = _store_arrays(tmp_path / "holes.h5")
    assert calls.count([0, 0]) == 1 and all(b == [90] for b in calls if b != [0, 0]) and len(calls) == 53
    assert sorted(holes) == sorted(extra["names"])
    for name in extra["names"][-2:]:
        assert holes[name].shape == (vr.SCENE_K * vr.DIM,) and holes[name].dtype == np.float32 and (holes[name] == 0).all()
    assert all(holes[n].tobytes() == one[n].tobytes() for n in one)


def test_train_vocabulary_thins_beyond_max_train(tmp_path):
    from sfd2_amd import feature_io
    scene = vr.make_scene()
    db, _ = vr.scene_names(scene)
    feats = tmp_path / "feats.h5"
    vr.write_scene_store(scene, feats)
    max_train, seed = 1000, 3
    with feature_io.open_store(str(feats), "r") as st:
        voc = _V().train_vocabulary(st, db, k=vr.SCENE_K, max_train=max_train, max_iters=vr.SCENE_ITERS, seed=seed)
    x = np.concatenate([scene["desc"][n] for n in db], 0)
    n = len(x)
    assert n == 3600 > max_train
    thinned = x[[(j * n) // max_train for j in range(max_train)]]
    cen, counts, moved = _V().kmeans(thinned, vr.SCENE_K, vr.SCENE_ITERS, seed)
    assert voc["centroids"].tobytes() == cen.tobytes() and voc["counts"].tobytes() == counts.tobytes() and voc["moved"].tobytes() == moved.tobytes()
    assert voc["moved"][0] == max_train and voc["counts"].sum() == max_train and voc["iters_run"] == len(moved) and voc["k"] == vr.SCENE_K
    full = _V().kmeans(x, vr.SCENE_K, vr.SCENE_ITERS, seed)
    assert full[2][0] == n and full[0].tobytes() != cen.tobytes()     # without the thinning the result is another
