"""The pair selection, the parts that need no GPU: the numpy restatement (tests/pairs_ref.py) against the pair files the reference's
three scripts wrote (tests/golden/pairs.npz, tests/golden/gen_pairs_goldens.py), the caps on the banded share the GPU tests rely on,
the CSR builder, the written file's format and the command lines."""
import os

import numpy as np
import pytest

import pairs_ref as pr
from sfd2_amd import colmap_io, pairs, pairs_from_covisibility, pairs_from_poses, pairs_from_retrieval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "pairs.npz"))


def _rows_by_name(text, names0, names1, k):
    """The golden pair text as an index table [len(names0), k] (-1 where a row is shorter), rows in names0 order."""
    pos0, pos1 = {n: i for i, n in enumerate(names0)}, {n: i for i, n in enumerate(names1)}
    idx = np.full((len(names0), k), -1, dtype=np.int64)
    fill = np.zeros(len(names0), dtype=np.int64)
    for a, b in pr.parse_pairs_text(text):
        i = pos0[a]
        idx[i, fill[i]] = pos1[b]
        fill[i] += 1
    return idx, fill


@pytest.mark.parametrize("case", range(len(pr.RETRIEVAL_SHAPES)))
def test_retrieval_restatement_equals_reference(case):
    seed, nq, nd, d, k = pr.RETRIEVAL_SHAPES[case]
    assert GOLD[f"retrieval/{case}/shape"].tolist() == [seed, nq, nd, d, k]
    q, db = pr.make_descriptors(seed, nq, nd, d)
    assert np.array_equal(GOLD[f"retrieval/{case}/checksum"], [q.astype(np.float64).sum(), db.astype(np.float64).sum()]), \
        "the generator no longer draws what the golden was recorded on"
    qn, dn = pr.descriptor_names(nq, nd)
    gold, fill = _rows_by_name(str(GOLD[f"retrieval/{case}/pairs"]), qn, dn, k)
    assert (fill == k).all()
    ref = pr.retrieval_ref(q, db, k)
    share = ref["band"].mean()
    print(f"retrieval {nq} x {nd} x {d}, k = {k}: banded share {share:.4f}, agreement with the reference {np.mean(gold == ref['idx']):.4f}")
    assert share <= 0.10
    assert pr.rows_agree(gold, ref["idx"], ref["band"])
    margin = 2 * d * pr.EPS24
    assert pr.banded_rows_consistent(gold, ref["idx"], ref["band"], lambda i, j: ref["sim64"][i, j],
                                     lambda i: np.nonzero(ref["sim64"][i] > ref["exact"][i, k - 1] + margin)[0].tolist())


def _gold_incidence():
    return {key: GOLD["covis/" + key] for key in ("obs_offsets", "obs_point", "track_offsets", "track_image", "image_ids", "point_ids", "names")}


def test_incidence_generator_is_the_recorded_one():
    inc, gold = pr.make_incidence(pr.COVIS_SEED), _gold_incidence()
    for key, v in gold.items():
        assert np.array_equal(inc[key], v), key


@pytest.mark.parametrize("k", pr.COVIS_KS)
def test_covisibility_restatement_equals_reference(k):
    inc = _gold_incidence()
    names = [str(n) for n in inc["names"]]
    gold, fill = _rows_by_name(str(GOLD[f"covis/pairs_k{k}"]), names, names, k)
    ref = pr.covisibility_ref(inc, k)
    assert np.array_equal(fill, ref["n_found"])
    assert pr.rows_agree(gold, ref["idx"], ref["band"])
    assert pr.banded_rows_consistent(gold, ref["idx"], ref["band"], lambda i, j: ref["counts"][i, j],
                                     lambda i: np.nonzero(ref["counts"][i] > max(ref["count"][i, -1], 0))[0].tolist()
                                     if ref["n_found"][i] == k else np.nonzero(ref["counts"][i] > 0)[0].tolist())
    # the loops shaped as the reference's give the restatement's pairs
    loops = pr.covisibility_loops(inc, k)
    want = [(i, int(j)) for i in range(len(names)) for j in ref["idx"][i, :ref["n_found"][i]]]
    assert loops == want


def test_covisibility_special_images():
    inc = pr.make_incidence(pr.COVIS_SEED)
    ref = pr.covisibility_ref(inc, 5)
    assert ref["n_found"][inc["empty"]] == 0 and ref["n_found"][inc["lonely"]] == 0
    assert inc["obs_offsets"][inc["empty"] + 1] == inc["obs_offsets"][inc["empty"]]
    assert inc["obs_offsets"][inc["lonely"] + 1] > inc["obs_offsets"][inc["lonely"]]
    assert (np.delete(ref["n_found"], [inc["empty"], inc["lonely"]]) == 5).all()
    # k = 64 is more than any image's covisible set
    assert pr.covisibility_ref(inc, 64)["n_found"].max() < 64


def test_poses_restatement_equals_reference():
    q, t = pr.make_poses(pr.POSES_SEED, pr.POSES_N)
    assert np.array_equal(q, GOLD["poses/qvec"]) and np.array_equal(t, GOLD["poses/tvec"])
    names = [str(n) for n in GOLD["poses/names"]]
    k = pr.POSES_K
    gold, fill = _rows_by_name(str(GOLD["poses/pairs"]), names, names, k)
    ref = pr.poses_ref(q, t, k, pr.POSES_THR)
    n = len(q)
    rot_share = ref["rot_band"].sum() / (n * (n - 1))
    near = (np.abs(ref["dR"] - pr.POSES_THR) < 0.03).sum() / (n * n)
    print(f"poses n = {n}: gate-banded pairs {rot_share:.5f}, pairs within 0.03 deg of the gate {near:.5f}, banded positions {ref['band'].mean():.4f}")
    assert rot_share <= 0.01 and ref["band"].mean() <= 0.01
    clear = ~ref["band"].any(axis=1)
    assert np.array_equal(fill[clear], ref["n_found"][clear])
    assert pr.rows_agree(gold, ref["idx"], ref["band"])
    assert pr.banded_rows_consistent(gold, ref["idx"], ref["band"], lambda i, j: ref["dist_all"][i, j], lambda i: [])
    loops = pr.poses_loops(q, t, k, pr.POSES_THR)
    assert loops == [(i, int(j)) for i in range(n) for j in ref["idx"][i, :ref["n_found"][i]]]


def test_poses_gates():
    q, t = pr.make_poses(pr.POSES_SEED, pr.POSES_N)
    assert pr.poses_ref(q, t, 10, 1e-3)["n_found"].max() == 0
    every = pr.poses_ref(q, t, pr.POSES_N - 1, 181.0)
    assert (every["n_found"] == pr.POSES_N - 1).all() and (np.diff(every["dist"], axis=1) >= 0).all()


def test_csr_builder_follows_dict_order_and_sorted_point_table():
    inc = pr.make_incidence(pr.COVIS_SEED)
    images, points3D = pr.incidence_to_model(inc, colmap_io.Image, colmap_io.Point3D)
    points3D = dict(reversed(list(points3D.items())))                     # dict order of the points must not matter
    ids, oo, op, to, ti = pairs.covisibility_csr(images, points3D)
    assert ids == [int(i) for i in inc["image_ids"]]
    for got, key in ((oo, "obs_offsets"), (op, "obs_point"), (to, "track_offsets"), (ti, "track_image")):
        assert got.dtype == inc[key].dtype and np.array_equal(got, inc[key]), key
    broken = dict(points3D)
    broken.pop(int(inc["point_ids"][0]))
    with pytest.raises(ValueError):
        pairs.covisibility_csr(images, broken)


def test_argument_errors_need_no_gpu():
    q, db = pr.make_descriptors(0, 3, 10, 8)
    with pytest.raises(ValueError):
        pairs.retrieval_topk(q, db, 11)
    with pytest.raises(ValueError):
        pairs.retrieval_topk(q, db, pairs.MAX_K + 1)
    with pytest.raises(ValueError):
        pairs.retrieval_topk(q, db[:, :7], 2)
    with pytest.raises(ValueError):
        pairs.poses_topk_arrays(np.zeros((3, 4)), np.zeros((2, 3)), 2)
    assert pairs.MAX_K == 256


def test_pairs_file_format(tmp_path):
    idx = np.array([[2, 0], [1, -1]])
    got = pairs.name_pairs(["q/a", "q/b"], ["db/x", "db/y", "db/z"], idx, [2, 1])
    assert got == [("q/a", "db/z"), ("q/a", "db/x"), ("q/b", "db/y")]
    assert pairs.name_pairs(["q/a"], ["db/x", "db/y"], idx[:1, :1] * 0 + 1) == [("q/a", "db/y")]
    path = tmp_path / "pairs.txt"
    pairs.write_pairs(path, got)
    text = path.read_text()
    assert text == "q/a db/z\nq/a db/x\nq/b db/y"
    assert pr.parse_pairs_text(text) == got
    pairs.write_pairs(path, [])
    assert path.read_text() == ""


def test_command_lines_are_the_references():
    a = pairs_from_covisibility.make_parser().parse_args(["--model", "m", "--output", "o", "--num_matched", "20"])
    assert vars(a) == {"model": a.model, "output": a.output, "num_matched": 20} and str(a.model) == "m"
    a = pairs_from_poses.make_parser().parse_args(["--model", "m", "--output", "o", "--num_matched", "5"])
    assert a.rotation_threshold == 30 and pairs_from_poses.DEFAULT_ROT_THRESH == 30
    a = pairs_from_poses.make_parser().parse_args(["--model", "m", "--output", "o", "--num_matched", "5", "--rotation_threshold", "12.5"])
    assert a.rotation_threshold == 12.5
    a = pairs_from_retrieval.make_parser().parse_args(["--descriptors", "d.h5", "--output", "o", "--num_matched", "50", "--query_prefix", "query",
                                                       "--db_prefix", "db", "mapping"])
    assert a.query_prefix == ["query"] and a.db_prefix == ["db", "mapping"] and a.query_list is None and a.db_list is None and a.db_model is None
    assert set(vars(a)) == {"descriptors", "output", "num_matched", "query_prefix", "query_list", "db_prefix", "db_list", "db_model"}
    for mod in (pairs_from_covisibility, pairs_from_poses, pairs_from_retrieval):
        with pytest.raises(SystemExit):
            mod.make_parser().parse_args(["--output", "o"])


def test_retrieval_name_selection(tmp_path):
    names = ["query/b.jpg", "db/2.jpg", "query/a.jpg", "db/1.jpg", "mapping/3.jpg"]
    assert pairs_from_retrieval.select_names(names, "query", None, None, "query") == ["query/a.jpg", "query/b.jpg"]
    assert pairs_from_retrieval.select_names(names, ["db", "mapping"], None, None, "DB") == ["db/1.jpg", "db/2.jpg", "mapping/3.jpg"]
    lst = tmp_path / "queries_with_intrinsics.txt"
    lst.write_text("query/b.jpg SIMPLE_RADIAL 640 480 500 320 240 0.1\nquery/a.jpg PINHOLE 640 480 500 500 320 240\n")
    assert pairs_from_retrieval.select_names(names, None, lst, None, "query") == ["query/b.jpg", "query/a.jpg"]
    with pytest.raises(ValueError):
        pairs_from_retrieval.select_names(names, None, None, None, "DB")
