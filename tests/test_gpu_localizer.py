"""Stage 1 of the localiser assembled on the device, and python -m sfd2_amd.localizer end to end, on the MI355X: localize_queries
with cluster_ids + Stage1 against the parent's path (StoreMatcher.match to the host, match_cluster_2D) bit for bit, and run() on
files written from the scene of tests/test_gpu_covis.py."""
import os

import numpy as np
import pytest

import covis_ref as cr
import loc_files as lf
import pose_ref as pr
from test_gpu_covis import _scene_with_descriptors

pytestmark = pytest.mark.gpu


def _mods():
    from sfd2_amd import covis, feature_io, localize, localizer
    return covis, feature_io, localize, localizer


@pytest.fixture(scope="module")
def scene():
    """The scene plus two database images that stage 1 must treat specially: 15 has three key points with a 3D point (<= 3: it
    never reaches the matcher and takes part without matches), 16 has no key points at all (no cluster_info entry)."""
    covis, feature_io, localize, localizer = _mods()
    from sfd2_amd import synth
    from sfd2_amd.matcher import Matcher, confs as mconfs
    sc = _scene_with_descriptors()
    assert len(sc["images"]) == 14 and len(sc["queries"]) == 20
    images, points3D, store = dict(sc["images"]), dict(sc["points3D"]), dict(sc["store"])
    some = [int(p) for p in sc["images"][5].point3D_ids if p != -1][:3]
    ids = np.full(40, -1, dtype=np.int64)
    ids[[3, 17, 30]] = some
    images[15] = cr.Img("db/015.jpg", sc["images"][5].qvec, sc["images"][5].tvec, ids)
    store["db/015.jpg"] = {"keypoints": np.zeros((40, 2), np.float32), "scores": np.zeros(40, np.float32),
                           "descriptors": np.ascontiguousarray(synth.make_descriptors(40, seed=77).astype(np.float64).T)}
    for p in some:
        points3D[p] = cr.Pt(points3D[p].xyz, list(points3D[p].image_ids) + [15])
    images[16] = cr.Img("db/016.jpg", sc["images"][6].qvec, sc["images"][6].tvec, np.zeros(0, dtype=np.int64))
    store["db/016.jpg"] = {"keypoints": np.zeros((0, 2), np.float32), "scores": np.zeros(0, np.float32), "descriptors": np.zeros((128, 0))}
    sc = dict(sc, images=images, points3D=points3D, store=store)
    sm = localize.StoreMatcher(Matcher(mconfs["NNM"]).eval().cuda(), store)
    mi = covis.MapIndex(images, points3D).to_device(0)
    yield sc, sm, mi
    sm.close()


def _lists(sc, kind, mi):
    """Per query the cluster ids: 'sng' one image per cluster (each query its own retrieval order over the 14 images), 'clu' the
    device clustering of those lists, 'special' lists that hold images 15 and 16 among ordinary ones."""
    rs = np.random.RandomState(3)
    lists = [[int(v) for v in rs.permutation(np.arange(1, 15))[:10]] for _ in sc["queries"]]
    if kind == "sng":
        return [[[i] for i in li] for li in lists]
    if kind == "clu":
        out = mi.clusters(lists)
        assert all(sorted(i for c in cl for i in c) == sorted(li) for cl, li in zip(out, lists))
        return out
    return [[[15], [16], [1, 16, 2, 15], [li[0]], [15, li[1], 16], [li[2], li[3]]] for li in lists]


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.asarray(a[0]).tobytes() == np.asarray(b[0]).tobytes()
    assert np.asarray(a[1]).tobytes() == np.asarray(b[1]).tobytes() and a[2] == b[2]
    ba, bb = a[3], b[3]
    assert set(ba) == set(bb)
    for k in ba:
        if isinstance(ba[k], (np.ndarray, list)) or isinstance(bb[k], (np.ndarray, list)):
            assert np.array_equal(np.asarray(ba[k]), np.asarray(bb[k])), k
        else:
            assert ba[k] == bb[k] or (ba[k] is None and bb[k] is None), k


@pytest.mark.parametrize("with_covis", [False, True])
@pytest.mark.parametrize("kind", ["sng", "clu", "special"])
def test_device_stage1_equals_the_host_path(scene, kind, with_covis):
    covis, feature_io, localize, localizer = _mods()
    sc, sm, mi = scene
    cluster_ids = _lists(sc, kind, mi)
    cov = localize.Covis(mi, sm, sc["store"], opt_type="clurefobs", covisibility_frame=12, iters=1, radius=30, obs_th=3, opt_th=12) if with_covis else None
    stage1 = localize.Stage1(mi, sm, sc["store"])
    assert stage1.on_device
    base = [dict(kpq=sc["store"][qn["qname"]]["keypoints"], camera=sc["cam"], qname=qn["qname"]) for qn in sc["queries"]]
    dev = localize.localize_queries([dict(b, cluster_ids=cl) for b, cl in zip(base, cluster_ids)], 12.0, inlier_th=20, points3D=sc["points3D"], covis=cov,
                                    stage1=stage1)
    host = localize.localize_queries([dict(b, clusters=localizer.host_clusters(sm, mi, b["qname"], cl)) for b, cl in zip(base, cluster_ids)], 12.0,
                                     inlier_th=20, points3D=sc["points3D"], covis=cov)
    for d, h in zip(dev, host):
        _same(d, h)
    assert sum(d[2] > 0 for d in dev) >= (15 if kind != "special" else 1)
    one = localize.pose_from_clusters(base[3]["kpq"], None, sc["cam"], 12.0, inlier_th=20, points3D=sc["points3D"], qname=base[3]["qname"], covis=cov,
                                      cluster_ids=cluster_ids[3], stage1=stage1)
    _same(one, dev[3])


def test_special_images_in_cluster_info(scene):
    """Image 15 has an empty entry (and can win a vote with 0), image 16 none."""
    covis, feature_io, localize, localizer = _mods()
    sc, sm, mi = scene
    qn = sc["queries"][0]["qname"]
    kpq = sc["store"][qn]["keypoints"]
    prepared = localize.Stage1(mi, sm, sc["store"]).assemble([(qn, kpq, [[15], [16], [1, 16, 2, 15]], 3)])[0]
    assert list(prepared[0][0]) == ["db/015.jpg"] and len(prepared[0][0]["db/015.jpg"]["qids"]) == 0 and prepared[0][1].shape == (0, 3)
    assert prepared[1][0] == {} and prepared[1][2].shape == (0, 2)
    assert list(prepared[2][0]) == ["db/001.jpg", "db/002.jpg", "db/015.jpg"] and len(prepared[2][4]) > 20
    ims = [sc["images"][i] for i in (1, 16, 2, 15)]
    ml = sm.match(qn, [im.name for im in ims], [im.point3D_ids for im in ims])
    info, mp3d, mkpq, ids3d, q_ids = localize.match_cluster_2D(kpq, ml, [im.point3D_ids for im in ims], sc["points3D"], obs_th=3, db_names=[im.name for im in ims])
    assert list(info) == list(prepared[2][0]) and [int(v) for v in ids3d] == [int(v) for v in prepared[2][3]]
    assert mkpq.tobytes() == prepared[2][2].tobytes() and mp3d.tobytes() == prepared[2][1].tobytes() and [int(v) for v in q_ids] == prepared[2][4].tolist()
    for name in info:
        assert [int(v) for v in info[name]["qids"]] == prepared[2][0][name]["qids"].tolist()
        assert [int(v) for v in info[name]["mp_3d_ids"]] == prepared[2][0][name]["mp_3d_ids"].tolist()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The plain scene as files: model, query list, retrieval (all 14 images per query, rotated), ground truth, a feature store."""
    covis, feature_io, localize, localizer = _mods()
    sc = _scene_with_descriptors()
    root = tmp_path_factory.mktemp("loc")
    names = [sc["images"][i].name for i in range(1, 15)]
    qnames = [q["qname"] for q in sc["queries"]]
    retrieval = {q: names[j % 14:] + names[:j % 14] for j, q in enumerate(qnames)}
    gt = {q["qname"].split("/")[-1]: (q["q"], q["t"]) for q in sc["queries"]}
    paths = lf.write_inputs(root, sc["images"], sc["points3D"], sc["cam"], qnames, retrieval, gt)
    paths["features"] = os.path.join(str(root), "feats-synth.pack")
    store = feature_io.open_store(paths["features"], "a")
    for name, f in sc["store"].items():
        feature_io.write_features(store, name, f)
    store.close()
    return sc, paths


@pytest.mark.parametrize("init_type", ["sng", "clu"])
def test_run_device_and_host_write_the_same_files(files, init_type):
    covis, feature_io, localize, localizer = _mods()
    sc, paths = files
    out = {}
    for stage1 in ("device", "host"):
        p = dict(paths, save_root=os.path.join(paths["save_root"], f"{init_type}_{stage1}"))
        args = localizer.make_parser().parse_args(lf.argv(p, dataset="aachen", db_imglist_fn="x", init_type=init_type, stage1=stage1, inlier_thresh=20,
                                                          with_match=True, do_covisible_opt=True, opt_type="clurefobs", covisibility_frame=12, iters=1,
                                                          radius=30, obs_thresh=3, opt_thresh=12))
        stem = localizer.main(lf.argv(p, dataset="aachen", db_imglist_fn="x", init_type=init_type, stage1=stage1, inlier_thresh=20, with_match=True,
                                      do_covisible_opt=True, opt_type="clurefobs", covisibility_frame=12, iters=1, radius=30, obs_thresh=3, opt_thresh=12))
        assert stem == localizer.output_stem(args) and os.path.basename(stem) == f"feats-synth_NNM_{init_type}_12_20all_o3op12clurefobsth12r30i1"
        out[stage1] = {ext: open(stem + ext).read() for ext in (".txt", ".log", ".txt.failed", "_full.log")}
    assert out["device"][".txt"] == out["host"][".txt"] and out["device"][".log"] == out["host"][".log"]
    assert out["device"][".txt.failed"] == out["host"][".txt.failed"] == ""
    lines = out["device"][".txt"].splitlines()
    assert len(lines) == 20 and len(out["device"][".log"].splitlines()) == 20 and len(out["device"]["_full.log"].splitlines()) == 20
    for line, q in zip(lines, sc["queries"]):
        p = line.split(" ")
        assert p[0] == q["qname"].split("/")[-1]
        qvec, tvec = np.array(p[1:5], float), np.array(p[5:], float)
        assert np.degrees(pr.rot_angle(qvec, q["q"])) <= 0.1
        assert np.linalg.norm(pr.centre(qvec, tvec) - pr.centre(q["q"], q["t"])) <= 0.005 * sc["depth"]
    assert all(int(l.split(" ")[2]) > 0 for l in out["device"][".log"].splitlines())      # every query localised


SCRIPT_SETS = {  # the localiser arguments of the reference's test_aachenv_1_1, test_robotcar and test_ecmu
    "aachen_v1.1": dict(ransac_thresh=15, opt_thresh=15, covisibility_frame=50, init_type="sng", opt_type="clurefobs", inlier_thresh=10, iters=5, radius=30,
                        obs_thresh=3),
    "robotcar": dict(ransac_thresh=12, opt_thresh=12, covisibility_frame=20, init_type="sng", opt_type="clurefpos", inlier_thresh=100, iters=5, radius=20,
                     obs_thresh=3),
    "ecmu": dict(ransac_thresh=15, opt_thresh=15, covisibility_frame=10, init_type="sng", opt_type="clurefobs", inlier_thresh=20, iters=5, radius=30,
                 obs_thresh=3, slice=18),
}


@pytest.mark.parametrize("dataset", list(SCRIPT_SETS))
def test_command_runs_the_reference_scripts_argument_sets(files, dataset):
    covis, feature_io, localize, localizer = _mods()
    sc, paths = files
    kw = SCRIPT_SETS[dataset]
    p = dict(paths, save_root=os.path.join(paths["save_root"], dataset))
    stem = localizer.main(lf.argv(p, dataset=dataset, db_imglist_fn="x", matcher_method="NNM", with_match=True, do_covisible_opt=True, image_dir="unused", **kw))
    tag = f"o3op{kw['covisibility_frame']}{kw['opt_type']}th{kw['opt_thresh']}r{kw['radius']}i5"
    want = f"feats-synth_NNM_sng_{kw['ransac_thresh']}_{kw['inlier_thresh']}" + ("vis_" if dataset == "ecmu" else "all_") + tag
    assert os.path.basename(stem) == ("slice18_" if dataset == "ecmu" else "") + want
    assert all(os.path.isfile(stem + ext) for ext in (".txt", ".txt.failed", ".log", "_full.log"))
    lines = open(stem + ".txt").read().splitlines()
    names = [q["qname"] if dataset == "robotcar" else q["qname"].split("/")[-1] for q in sc["queries"]]      # query/NNN.jpg: two parts for robotcar
    assert [l.split(" ")[0] for l in lines] == names and all(len(l.split(" ")) == 8 for l in lines)
    assert len(open(stem + ".log").read().splitlines()) == 20 and "q_error:" in open(stem + "_full.log").read()
