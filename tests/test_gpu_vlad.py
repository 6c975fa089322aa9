"""The VLAD global descriptors on the MI355X (sfd2_amd.vlad, sfd2_amd.global_features) against the numpy restatement and the input
families of tests/vlad_ref.py.

Exact family: every chain is exact in fp32, so assignments (designed ties included) and scores are compared bit for bit.  Float
family: assignments are compared on every row the restatement does not call banded (caps: tests/test_vlad_host.py); a banded row
must choose one of its two best.  Sums are restated as in-order fp32 loops FROM THE DEVICE'S ASSIGNMENT and normalised in fp64: a
component may round to the other side of an fp32 boundary, so |got - want| <= one fp32 ulp of |want|, and exactly 0 where want is 0.
k-means on separated clusters (no banded row in any iteration) is compared bit for bit after every iteration."""
import functools
import os

import numpy as np
import pytest

import pairs_ref as pr
import vlad_ref as vr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMS = ("intra", "ssr", "none")


def _V():
    from sfd2_amd import vlad
    return vlad


@functools.lru_cache(maxsize=None)
def _assign_case(family, k):
    x, c = (vr.exact_family if family == "exact" else vr.float_family)(20 + k, max(vr.ASSIGN_NS), k)
    return x, c, vr.scores64(x, c), vr.banded(x, c) if family == "float" else np.zeros(len(x), dtype=bool), vr.two_best(x, c) if k > 1 else None


@pytest.mark.parametrize("k", vr.ASSIGN_KS)
def test_assign_exact_family_bit_for_bit(k):
    x, c, s64, _, _ = _assign_case("exact", k)
    want_a, want_s = np.argmax(s64, axis=1).astype(np.int32), s64.max(1).astype(np.float32)
    assert (want_s.astype(np.float64) == s64.max(1)).all()
    for n in vr.ASSIGN_NS:
        a, s = _V().assign(x[:n], c)
        assert a.dtype == np.int32 and s.dtype == np.float32 and a.shape == s.shape == (n,)
        np.testing.assert_array_equal(a, want_a[:n])                 # ties included: the smaller index
        assert s.tobytes() == want_s[:n].tobytes()
    if k >= 3:
        assert (want_a[::5] == 0).all() and (s64[::5, 0] == s64[::5, 1]).all()        # the designed tie was in play


@pytest.mark.parametrize("k", vr.ASSIGN_KS)
def test_assign_float_family_outside_the_band(k):
    x, c, s64, band, best = _assign_case("float", k)
    want_a = np.argmax(s64, axis=1)
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    cn = np.sqrt((c64 * c64).sum(1))
    for n in vr.ASSIGN_NS:
        a, s = _V().assign(x[:n], c)
        assert a.min() >= 0 and a.max() < k
        np.testing.assert_array_equal(a[~band[:n]], want_a[:n][~band[:n]])
        for i in np.nonzero(band[:n])[0]:
            assert a[i] in best[i]
        bound = (vr.DIM + 2) * vr.EPS24 * (np.sqrt((x64[:n] ** 2).sum(1)) * cn[a] + 0.5 * cn[a] ** 2)
        err = np.abs(s.astype(np.float64) - s64[np.arange(n), a])
        assert (err <= bound).all(), (n, err.max())
    print(f"assign float K = {k}: banded rows {int(band.sum())} of {len(x)}")


@pytest.mark.parametrize("family,k,n", [("exact", 17, 257), ("float", 64, 1000), ("float", 256, 65), ("float", 1, 17)])
def test_assign_host_and_device_inputs_give_the_same_bytes(family, k, n):
    import torch
    x, c, _, _, _ = _assign_case(family, k)
    a0, s0 = _V().assign(x[:n], c)
    for xd, cd in ((torch.from_numpy(x[:n]).cuda(), torch.from_numpy(c).cuda()), (torch.from_numpy(x[:n]).cuda(), c), (torch.from_numpy(x[:n]), c)):
        a1, s1 = _V().assign(xd, cd)
        assert a1.tobytes() == a0.tobytes() and s1.tobytes() == s0.tobytes()


# ------------------------------------------------------------------------------------------------------------------ aggregate
@functools.lru_cache(maxsize=None)
def _agg_case(family, k):
    x, offsets, c = vr.aggregate_case(13, k, family)
    return x, offsets, c, vr.scores64(x, c), vr.banded(x, c) if family == "float" else np.zeros(len(x), dtype=bool)


def _check_aggregate(family, k, norm):
    x, offsets, c, s64, band = _agg_case(family, k)
    out, a = _V().aggregate(x, offsets, c, norm=norm, return_assign=True)
    assert out.shape == (len(offsets) - 1, k * vr.DIM) and out.dtype == np.float32 and np.isfinite(out).all()
    np.testing.assert_array_equal(a[~band], np.argmax(s64, axis=1)[~band])
    want = vr.vlad64(x, offsets, c, norm, a)
    worst = 0.0
    for i in range(len(want)):
        assert vr.within_one_ulp(out[i], want[i]), (i, np.abs(out[i] - want[i]).max())
        nz = want[i] != 0
        if nz.any():
            worst = max(worst, float((np.abs(out[i][nz] - want[i][nz]) / vr.ulp32(want[i][nz])).max()))
    lengths = np.diff(offsets)
    assert (out[lengths == 0] == 0).all()                             # an image without descriptors: zeros, never NaN
    norms = np.sqrt((out.astype(np.float64) ** 2).sum(1))
    assert np.allclose(norms, np.sqrt((want ** 2).sum(1)), atol=1e-6) and (np.abs(norms[lengths > 1] - 1.0) <= 1e-6).all()
    blocks = out.reshape(len(out), k, vr.DIM)
    if k >= 3:
        assert not (a == k - 2).any() and (blocks[:, k - 2] == 0).all()   # the centroid no row chooses
    i31 = list(lengths).index(31)
    assert len(set(a[offsets[i31]:offsets[i31 + 1]].tolist())) == 1 and ((blocks[i31] != 0).any(1).sum() == 1)   # every row to one centroid
    print(f"aggregate {family} K = {k} {norm}: largest error {worst:.3f} ulp, banded rows {int(band.sum())}")
    return out


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("k", vr.AGG_KS)
def test_aggregate_float_family_within_one_ulp(k, norm):
    _check_aggregate("float", k, norm)


@pytest.mark.parametrize("norm", NORMS)
def test_aggregate_exact_family_within_one_ulp(norm):
    _check_aggregate("exact", 17, norm)


@pytest.mark.parametrize("k", vr.AGG_KS)
def test_aggregate_does_not_depend_on_the_batch(k):
    import torch
    x, offsets, c, _, _ = _agg_case("float", k)
    out = _V().aggregate(x, offsets, c)
    n_img = len(offsets) - 1
    rev = [x[offsets[i]:offsets[i + 1]] for i in range(n_img)][::-1]
    out_rev = _V().aggregate(np.concatenate(rev, 0), np.concatenate([[0], np.cumsum([len(r) for r in rev])]), c)
    assert out_rev[::-1].tobytes() == out.tobytes()
    for i in range(n_img):
        one = _V().aggregate(x[offsets[i]:offsets[i + 1]], [0, offsets[i + 1] - offsets[i]], c)
        assert one.tobytes() == out[i:i + 1].tobytes(), i
    dev = _V().aggregate(torch.from_numpy(x).cuda(), offsets, torch.from_numpy(c).cuda())
    assert dev.tobytes() == out.tobytes()


# ------------------------------------------------------------------------------------------------------------------ k-means
@functools.lru_cache(maxsize=None)
def _separated(i):
    seed, n, k = vr.KMEANS_SEPARATED[i]
    x, start = vr.separated(seed, n, k)
    return x, start, vr.kmeans_ref(x, start, 20)


@pytest.mark.parametrize("i", range(len(vr.KMEANS_SEPARATED)))
def test_kmeans_separated_equals_restatement_in_every_iteration(i):
    x, start, its = _separated(i)
    assert its[-1][2] == 0 and len(its) < 20
    for it in range(1, len(its) + 1):
        cen, counts, moved = _V().kmeans_from(x, start, max_iters=it)
        assert cen.tobytes() == its[it - 1][0].tobytes(), it
        np.testing.assert_array_equal(counts, its[it - 1][1])
        assert moved.tolist() == [v[2] for v in its[:it]]
    cen, counts, moved = _V().kmeans_from(x, start, max_iters=20)      # stops on moved == 0 before max_iters
    assert len(moved) == len(its) < 20 and moved[-1] == 0 and moved[0] == len(x)
    assert cen.tobytes() == its[-1][0].tobytes() and counts.sum() == len(x)
    a, _ = _V().assign(x, start)
    np.testing.assert_array_equal(a, its[0][3])


def test_kmeans_duplicated_start_row():
    seed, n, k = vr.KMEANS_SEPARATED[0]
    x, start = vr.separated(seed, n, k)
    start[5] = start[2]
    cen, counts, moved = _V().kmeans_from(x, start, max_iters=1)
    assert counts[5] == 0 and cen[5].tobytes() == start[5].tobytes() and counts[2] > 0 and moved.tolist() == [n]
    its = vr.kmeans_ref(x, start, 20)
    cen, counts, moved = _V().kmeans_from(x, start, max_iters=20)
    assert moved.tolist() == [v[2] for v in its] and cen.tobytes() == its[-1][0].tobytes()
    np.testing.assert_array_equal(counts, its[-1][1])


def test_kmeans_overlapping_is_deterministic():
    import torch
    seed, n, k = vr.KMEANS_OVERLAP
    x, _ = vr.overlapping(seed, n, k)
    c0, n0, m0 = _V().kmeans(x, k, max_iters=20, seed=seed)
    c1, n1, m1 = _V().kmeans(x, k, max_iters=20, seed=seed)
    assert c0.tobytes() == c1.tobytes() and n0.tobytes() == n1.tobytes() and m0.tobytes() == m1.tobytes()
    assert n0.sum() == n and np.isfinite(c0).all() and m0[0] == n and 1 <= len(m0) <= 20 and (m0 >= 0).all()
    c2, n2, m2 = _V().kmeans_from(torch.from_numpy(x).cuda(), x[np.random.RandomState(seed).permutation(n)[:k]], max_iters=20)
    assert c2.tobytes() == c0.tobytes() and m2.tobytes() == m0.tobytes()


# ------------------------------------------------------------------------------------------------------------------ errors
def test_bad_arguments_raise_with_the_library_message():
    x, c = vr.float_family(1, 40, 4)
    big = np.zeros((257, vr.DIM), dtype=np.float32)
    with pytest.raises(RuntimeError, match=r"sfd2_vlad_assign: k must lie in \[1, 256\]"):
        _V().assign(x, c[:0])
    with pytest.raises(RuntimeError, match=r"sfd2_vlad_assign: k must lie in \[1, 256\]"):
        _V().assign(x, big)
    with pytest.raises(RuntimeError, match=r"sfd2_vlad_aggregate: k must lie in \[1, 256\]"):
        _V().aggregate(x, [0, 40], big)
    with pytest.raises(RuntimeError, match=r"sfd2_vlad_kmeans: k must lie in \[1, 256\]"):
        _V().kmeans_from(x, big)
    with pytest.raises(RuntimeError, match="sfd2_vlad_assign: n must be positive"):
        _V().assign(x[:0], c)
    with pytest.raises(RuntimeError, match="sfd2_vlad_aggregate: offsets must start at 0 and not decrease"):
        _V().aggregate(x, [0, 25, 10, 40], c)
    bad = x.copy()
    bad[17, 3] = np.nan
    with pytest.raises(RuntimeError, match="sfd2_vlad_assign: non-finite"):
        _V().assign(bad, c)
    with pytest.raises(RuntimeError, match="sfd2_vlad_aggregate: non-finite"):
        _V().aggregate(bad, [0, 40], c)
    with pytest.raises(RuntimeError, match="sfd2_vlad_kmeans: non-finite"):
        _V().kmeans_from(bad, c)
    a, _ = _V().assign(x, c)                                           # the context is as good as before
    np.testing.assert_array_equal(a[~vr.banded(x, c)], np.argmax(vr.scores64(x, c), axis=1)[~vr.banded(x, c)])


# ------------------------------------------------------------------------------------------------------------------ end to end
def _store_arrays(path):
    from sfd2_amd import feature_io
    with feature_io.open_store(str(path), "r") as st:
        return {n: np.array(st[n]["global_descriptor"].__array__()) for n in sorted(st.keys())}


def test_feature_store_in_pairs_file_out(tmp_path):
    from sfd2_amd import global_features, pairs_from_retrieval
    scene = vr.make_scene()
    db_names, q_names = vr.scene_names(scene)
    feats, glob, voc, pairs = tmp_path / "feats.h5", tmp_path / "global.h5", tmp_path / "voc.npz", tmp_path / "pairs.txt"
    vr.write_scene_store(scene, feats)
    global_features.main(feats, glob, voc, train=True, train_prefix="db", k=vr.SCENE_K, max_iters=vr.SCENE_ITERS)
    pairs_from_retrieval.main(glob, pairs, num_matched=vr.SCENE_TOP, query_prefix="query", db_prefix="db")

    centroids, iters = vr.scene_vocabulary(scene)
    v = _V().load_vocabulary(voc)
    assert v["centroids"].tobytes() == centroids.tobytes() and v["iters_run"] == iters and (v["k"], v["norm"], v["seed"]) == (vr.SCENE_K, "intra", 0)
    want_db, want_q = vr.scene_descriptors(scene, centroids, dtype=np.float64)
    got = _store_arrays(glob)
    assert sorted(got) == sorted(scene["names"])
    for names, want in ((db_names, want_db), (q_names, want_q)):
        for n, w in zip(names, want):
            assert got[n].dtype == np.float32 and got[n].shape == (vr.SCENE_K * vr.DIM,)
            assert vr.within_one_ulp(got[n], w), n

    ref = pr.retrieval_ref(want_q.astype(np.float32), want_db.astype(np.float32), vr.SCENE_TOP)
    listed = pr.parse_pairs_text(pairs.read_text())
    assert [a for a, _ in listed] == [q for q in q_names for _ in range(vr.SCENE_TOP)]
    idx = np.array([db_names.index(b) for _, b in listed]).reshape(len(q_names), vr.SCENE_TOP)
    print(f"scene: banded rank positions {int(ref['band'].sum())} of {ref['band'].size}, equal to the restatement {np.mean(idx == ref['idx']):.3f}")
    assert pr.rows_agree(idx, ref["idx"], ref["band"])
    best = vr.most_overlapping(scene)
    assert all(best[i] in idx[i] for i in range(len(q_names)))

    glob2 = tmp_path / "global2.h5"
    global_features.main(feats, glob2, voc)                            # the saved vocabulary: the same descriptors
    again = _store_arrays(glob2)
    assert sorted(again) == sorted(got) and all(again[n].tobytes() == got[n].tobytes() for n in got)
