"""The pair selection on the MI355X (sfd2_amd.pairs, sfd2_amd.pairs_from_*) against the numpy restatement and the synthetic inputs of
tests/pairs_ref.py.

Comparisons leave out what the restatement calls banded (pairs_ref's module docstring), under the caps tests/test_pairs_host.py
checks without a GPU.  Covisibility is integers with a fully defined tie rule: compared exactly, no band."""
import functools
import os

import numpy as np
import pytest

import pairs_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (seed, nq, nd, d, k): the three recorded shapes (ragged nq 33 / 65 / 200, nd 3001 across tile and split edges, d = 100 no multiple
# of the MFMA depth), a single-row batch, every candidate selected
RETRIEVAL_CASES = pr.RETRIEVAL_SHAPES + ((2, 1, 64, 128, 1), (3, 5, 70, 32, 70))


def _P():
    from sfd2_amd import pairs
    return pairs


@functools.lru_cache(maxsize=None)
def _retrieval(case):
    seed, nq, nd, d, k = RETRIEVAL_CASES[case]
    q, db = pr.make_descriptors(seed, nq, nd, d)
    return q, db, pr.retrieval_ref(q, db, k)


def _check_retrieval(idx, sim, q, db, ref, k):
    d = q.shape[1]
    sim64 = ref["sim64"]
    rows = np.arange(len(idx))[:, None]
    assert idx.min() >= 0 and idx.max() < len(db)
    assert all(len(set(r.tolist())) == k for r in idx), "a db row twice in one list"
    err = np.abs(sim.astype(np.float64) - sim64[rows, idx]).max()
    print(f"retrieval {q.shape[0]} x {db.shape[0]} x {d}, k = {k}: max |sim - exact| {err:.3e} (bound {d * pr.EPS24:.3e}), "
          f"banded share {ref['band'].mean():.4f}, equal to the restatement {np.mean(idx == ref['idx']):.4f}")
    assert err <= d * pr.EPS24
    assert pr.rows_agree(idx, ref["idx"], ref["band"])
    # the device's own order: similarity descending, equal similarities by ascending row
    ds, di = np.diff(sim, axis=1), np.diff(idx, axis=1)
    assert (ds <= 0).all() and (di[ds == 0] > 0).all()
    # nothing clearly better than the k-th is missing
    margin = 2 * d * pr.EPS24
    for i in range(len(idx)):
        sure = np.nonzero(sim64[i] > ref["exact"][i, k - 1] + margin)[0]
        assert set(sure.tolist()) <= set(idx[i].tolist())


@pytest.mark.parametrize("case", range(len(RETRIEVAL_CASES)))
def test_retrieval_equals_restatement(case):
    q, db, ref = _retrieval(case)
    k = RETRIEVAL_CASES[case][4]
    idx, sim = _P().retrieval_topk(q, db, k)
    assert idx.shape == (len(q), k) and idx.dtype == np.int32 and sim.dtype == np.float32
    _check_retrieval(idx, sim, q, db, ref, k)


def test_retrieval_exact_ties_come_back_in_ascending_index():
    q, db = pr.make_descriptors(5, 4, 300, 96)
    db = db.copy()
    copies = [41, 97, 140, 233]                      # row 41 and three bit-for-bit duplicates of it
    for c in copies[1:]:
        db[c] = db[41]
    # query 0: the copies lead; query 3: they sit in the middle of the ranking
    q = q.copy()
    q[0] = (db[41].astype(np.float64) + 0.05 * q[0]).astype(np.float32)
    q[0] /= np.linalg.norm(q[0])
    sim64 = q.astype(np.float64) @ db.astype(np.float64).T
    rank1 = int((sim64[3] > sim64[3, 41]).sum())    # candidates in front of the group for query 3
    assert (sim64[0] > sim64[0, 41]).sum() == 0 and 4 < rank1 < 250
    for row, k in ((0, 1), (0, 2), (0, 3), (0, 4), (0, 6), (3, rank1 + 1), (3, rank1 + 2), (3, rank1 + 3)):
        idx, sim = _P().retrieval_topk(q[row:row + 1], db, k)
        front = rank1 if row else 0
        take = min(k - front, 4)
        assert idx[0, front:front + take].tolist() == copies[:take], (row, k, idx[0])
        assert len(set(sim[0, front:front + take].tolist())) == 1
        assert not set(copies[take:]) & set(idx[0, :front + take].tolist())


def test_retrieval_does_not_depend_on_batch_or_splits():
    P = _P()
    q, db, ref = _retrieval(0)
    k = RETRIEVAL_CASES[0][4]
    idx, sim = P.retrieval_topk(q, db, k)
    one_i, one_s = P.retrieval_topk(q[17:18], db, k)
    assert np.array_equal(one_i[0], idx[17]) and np.array_equal(one_s[0].view(np.uint32), sim[17].view(np.uint32))
    for splits in (1, 2, 8):
        si, ss = P.retrieval_topk(q, db, k, splits=splits)
        assert np.array_equal(si, idx) and np.array_equal(ss.view(np.uint32), sim.view(np.uint32)), splits
    # descriptors already on the device: the same bits
    import torch
    ti, ts = P.retrieval_topk(torch.from_numpy(q).cuda(), torch.from_numpy(db).cuda(), k)
    assert np.array_equal(ti, idx) and np.array_equal(ts.view(np.uint32), sim.view(np.uint32))
    # an unaligned, odd-width view of the same data takes the scalar loader: the same similarities for the shared width
    qi, qs = P.retrieval_topk(q[:, :255], db[:, :255], k)
    r255 = pr.retrieval_ref(q[:, :255], db[:, :255], k)
    _check_retrieval(qi, qs, q[:, :255], db[:, :255], r255, k)


def test_retrieval_bad_input_raises():
    from sfd2_amd import _lib
    P = _P()
    q, db = pr.make_descriptors(0, 3, 10, 16)
    with pytest.raises(ValueError):
        P.retrieval_topk(q, db, 11)
    with pytest.raises(ValueError):
        P.retrieval_topk(q, np.tile(db, (30, 1)), 257)
    bad = db.copy()
    bad[7, 3] = np.nan
    with pytest.raises(RuntimeError, match="non-finite"):
        P.retrieval_topk(q, bad, 2)
    bad = q.copy()
    bad[2, 15] = np.inf
    with pytest.raises(RuntimeError, match="non-finite"):
        P.retrieval_topk(bad, db, 2)
    # the C ABI itself refuses the same arguments
    ctx = _lib.default_context(0)
    idx, sim = np.zeros((3, 300), np.int32), np.zeros((3, 300), np.float32)
    big = np.ascontiguousarray(np.tile(db, (30, 1)))
    for dbm, k, msg in ((db, 11, b"larger than"), (big, 257, b"k must lie")):
        rc = ctx.lib.sfd2_pairs_retrieval(ctx.h, q.ctypes.data, 3, dbm.ctypes.data, len(dbm), 16, k, 0, idx.ctypes.data, sim.ctypes.data, 0)
        assert rc == -1 and msg in ctx.lib.sfd2_last_error()
    # and still works afterwards
    i2, _ = P.retrieval_topk(q, db, 2)
    r2 = pr.retrieval_ref(q, db, 2)
    assert pr.rows_agree(i2, r2["idx"], r2["band"])


@functools.lru_cache(maxsize=None)
def _incidence():
    return pr.make_incidence(pr.COVIS_SEED)


def _device_covis(inc, k, global_counters):
    return _P().covisibility_topk_csr(inc["obs_offsets"], inc["obs_point"], inc["track_offsets"], inc["track_image"], k, global_counters=global_counters)


@pytest.mark.parametrize("k", pr.COVIS_KS)
def test_covisibility_equals_restatement_on_both_counter_paths(k):
    inc = _incidence()
    ref = pr.covisibility_ref(inc, k)
    outs = []
    for global_counters in (False, True):
        idx, cnt, nf = _device_covis(inc, k, global_counters)
        assert np.array_equal(nf, ref["n_found"]) and np.array_equal(idx, ref["idx"]) and np.array_equal(cnt, ref["count"]), global_counters
        assert nf[inc["empty"]] == 0 and nf[inc["lonely"]] == 0
        outs.append((idx, cnt, nf))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("global_counters", (False, True))
def test_covisibility_of_a_map_without_points(global_counters):
    """Three images, no point: obs_point and track_image are empty arrays (null pointers), every n_found is 0."""
    inc = dict(obs_offsets=np.zeros(4, np.int64), obs_point=np.zeros(0, np.int32), track_offsets=np.zeros(1, np.int64), track_image=np.zeros(0, np.int32))
    ref = pr.covisibility_ref(inc, 2)
    idx, cnt, nf = _device_covis(inc, 2, global_counters)
    assert ref["n_found"].tolist() == [0, 0, 0] and np.array_equal(nf, ref["n_found"])
    assert np.array_equal(idx, ref["idx"]) and np.array_equal(cnt, ref["count"])


def test_covisibility_in_a_permuted_image_order_gives_the_same_pairs_by_name():
    inc = _incidence()
    perm = np.random.RandomState(11).permutation(len(inc["names"]))
    inc2 = pr.permute_incidence(inc, perm)

    def by_name(m, idx, cnt, nf, band=None):
        out = {}
        for i, name in enumerate(m["names"]):
            keep = np.arange(nf[i]) if band is None else np.nonzero(~band[i, :nf[i]])[0]
            out[str(name)] = {str(m["names"][idx[i, p]]): int(cnt[i, p]) for p in keep}
        return out

    # k beyond every covisible set: the same partners with the same counts
    assert by_name(inc, *_device_covis(inc, 64, False)) == by_name(inc2, *_device_covis(inc2, 64, True))
    # k = 5: equal wherever no tie decides (a tie is broken by position in the image order, which changed)
    b1, b2 = pr.covisibility_ref(inc, 5)["band"], pr.covisibility_ref(inc2, 5)["band"]
    assert np.array_equal(b1[perm], b2)
    assert by_name(inc, *_device_covis(inc, 5, False), band=b1) == by_name(inc2, *_device_covis(inc2, 5, False), band=b2)


def test_covisibility_from_model_dicts_and_bad_input():
    from sfd2_amd import colmap_io
    P = _P()
    inc = _incidence()
    images, points3D = pr.incidence_to_model(inc, colmap_io.Image, colmap_io.Point3D)
    ids, idx, cnt, nf = P.covisibility_topk(images, points3D, 5)
    ref = pr.covisibility_ref(inc, 5)
    assert ids == [int(i) for i in inc["image_ids"]] and np.array_equal(idx, ref["idx"]) and np.array_equal(nf, ref["n_found"])
    bad = inc["track_image"].copy()
    bad[3] = len(inc["names"])
    with pytest.raises(RuntimeError, match="out of range"):
        P.covisibility_topk_csr(inc["obs_offsets"], inc["obs_point"], inc["track_offsets"], bad, 5)
    bad = inc["obs_point"].copy()
    bad[0] = -1
    with pytest.raises(RuntimeError, match="out of range"):
        P.covisibility_topk_csr(inc["obs_offsets"], bad, inc["track_offsets"], inc["track_image"], 5)
    with pytest.raises(ValueError):
        P.covisibility_topk_csr(inc["obs_offsets"], inc["obs_point"], inc["track_offsets"], inc["track_image"], 257)


@functools.lru_cache(maxsize=None)
def _poses():
    return pr.make_poses(pr.POSES_SEED, pr.POSES_N)


@pytest.mark.parametrize("true_centres", (False, True))
def test_poses_equal_restatement(true_centres):
    q, t = _poses()
    k = pr.POSES_K
    ref = pr.poses_ref(q, t, k, pr.POSES_THR, true_centres)
    idx, dist, nf = _P().poses_topk_arrays(q, t, k, pr.POSES_THR, true_centres=true_centres)
    clear = ~ref["band"].any(axis=1)
    assert np.array_equal(nf[clear], ref["n_found"][clear])
    assert pr.rows_agree(idx, ref["idx"], ref["band"])
    filled = np.arange(k)[None, :] < nf[:, None]
    assert (idx[~filled] == -1).all() and np.isinf(dist[~filled]).all()
    rows = np.nonzero(filled)[0]
    exact = ref["dist_all"][rows, idx[filled]]
    rel = np.abs(dist[filled] - exact) / exact
    print(f"poses n = {len(q)}, centres {true_centres}: max relative distance error {rel.max():.3e}, banded positions {ref['band'].mean():.4f}")
    # positions are sums of three products of magnitude < 25 (error < 1e-14 absolute), neighbours ~0.7 apart
    assert rel.max() <= 1e-12
    assert (np.diff(np.where(filled, dist, np.inf), axis=1) >= 0).all()


def test_poses_gates():
    P = _P()
    q, t = _poses()
    n = len(q)
    idx, dist, nf = P.poses_topk_arrays(q, t, 10, 1e-3)
    assert nf.max() == 0 and (idx == -1).all()
    # every rotation admitted and k = n - 1: every other image, nearest first (the reference raises for this k)
    idx, dist, nf = P.poses_topk_arrays(q, t, n - 1, 181.0)
    ref = pr.poses_ref(q, t, n - 1, 181.0)
    assert (nf == n - 1).all() and pr.rows_agree(idx, ref["idx"], ref["band"]) and (np.diff(dist, axis=1) >= 0).all()
    assert all(sorted(r.tolist()) == [j for j in range(n) if j != i] for i, r in enumerate(idx))
    # k >= n: a row has at most n - 1 entries
    idx, dist, nf = P.poses_topk_arrays(q[:7], t[:7], 12, 181.0)
    assert (nf == 6).all() and (idx[:, 6:] == -1).all()
    with pytest.raises(RuntimeError, match="non-finite"):
        P.poses_topk_arrays(np.where(np.arange(4 * n).reshape(n, 4) == 5, np.nan, q), t, 3)


def test_pairs_from_covisibility_end_to_end(tmp_path):
    from sfd2_amd import colmap_io, match_features, pairs_from_covisibility
    model = os.path.join(ROOT, "tests", "golden", "tri_model")
    out = tmp_path / "pairs-covis3.txt"
    pairs_from_covisibility.main(model, out, 3)
    text = out.read_text()
    assert text and not text.endswith("\n")
    _, images, points3D = colmap_io.read_model(model)
    names = {im.name for im in images.values()}
    # the two parsers of the stages downstream: match_features (cli) and triangulation.read_inputs
    pair_list = text.rstrip("\n").split("\n")
    uniq = match_features.unique_pairs(pair_list)
    tri_pairs = [p.split() for p in text.splitlines(keepends=True)]
    assert len(tri_pairs) == len(pair_list) and all(len(p) == 2 and p[0] in names and p[1] in names and p[0] != p[1] for p in tri_pairs)
    assert 0 < len(uniq) <= len(pair_list) <= 3 * len(images)
    # and the pairs are the restatement's on this model
    ids, oo, op, to, ti = _P().covisibility_csr(images, points3D)
    ref = pr.covisibility_ref({"obs_offsets": oo, "obs_point": op, "track_offsets": to, "track_image": ti}, 3)
    want = [(images[ids[i]].name, images[ids[j]].name) for i in range(len(ids)) for j in ref["idx"][i, :ref["n_found"][i]]]
    assert [tuple(p) for p in tri_pairs] == want


def test_pairs_from_poses_and_retrieval_end_to_end(tmp_path):
    from sfd2_amd import colmap_io, feature_io, pairs_from_poses, pairs_from_retrieval
    model = os.path.join(ROOT, "tests", "golden", "tri_model")
    images = colmap_io.read_images_binary(os.path.join(model, "images.bin"))
    ids = list(images)
    out = tmp_path / "pairs-poses.txt"
    pairs_from_poses.main(model, out, 2, rotation_threshold=181)
    got = pr.parse_pairs_text(out.read_text())
    q, t = np.array([images[i].qvec for i in ids]), np.array([images[i].tvec for i in ids])
    ref = pr.poses_ref(q, t, 2, 181.0)
    assert not ref["band"].any()
    assert got == [(images[ids[i]].name, images[ids[j]].name) for i in range(len(ids)) for j in ref["idx"][i, :ref["n_found"][i]]]
    # retrieval: a descriptor store written with the project's own writer, names by prefix and by model
    qd, dd = pr.make_descriptors(9, 3, len(ids), 64)
    store = feature_io.open_store(str(tmp_path / "global-feats.h5"), "a")
    db_names = [images[i].name for i in ids]
    for n, x in list(zip(["query/q0.jpg", "query/q1.jpg", "query/q2.jpg"], qd)) + list(zip(db_names, dd)):
        store.write_group(n, {"global_descriptor": x})
    store.close()
    out = tmp_path / "pairs-retrieval.txt"
    pairs_from_retrieval.main(tmp_path / "global-feats.h5", out, 2, query_prefix="query", db_model=model)
    got = pr.parse_pairs_text(out.read_text())
    ref = pr.retrieval_ref(qd, dd, 2)
    assert not ref["band"].any()
    assert got == [(f"query/q{i}.jpg", db_names[j]) for i in range(3) for j in ref["idx"][i]]
