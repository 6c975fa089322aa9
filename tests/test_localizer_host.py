"""python -m sfd2_amd.localizer, the parts that need no GPU: the parsers, the output names of the three reference scripts' argument
sets, the naming and .failed rules, the missing-retrieval deviation, and run() end to end on a small synthetic model with the
scripted matcher / estimator / refiner of tests/covis_ref.py."""
import os

import numpy as np
import pytest

import cluster_ref as clr
import covis_ref as cr
import loc_files as lf
from sfd2_amd import covis, localize, localizer, pairs_from_retrieval, parsers

FEAT = "feats-ressegnetv2-20220810-wapv2-sd2mfsf-uspg-0001-n4096-r1600"
COMMON = ["--db_imglist_fn", "x", "--reference_sfm", "m", "--queries", "q.txt", "--matcher_method", "NNM", "--with_match", "--do_covisible_opt",
          "--obs_thresh", "3", "--init_type", "sng", "--iters", "5", "--save_root", "out"]
SCRIPTS = {  # the localiser argument sets of test_aachenv_1_1, test_robotcar and test_ecmu -> the reference's file stem
    "aachen": (["--dataset", "aachen_v1.1", "--features", f"o/{FEAT}.h5", "--ransac_thresh", "15", "--opt_thresh", "15", "--covisibility_frame", "50",
                "--opt_type", "clurefobs", "--inlier_thresh", "10", "--radius", "30"], f"out/{FEAT}_NNM_sng_15_10all_o3op50clurefobsth15r30i5"),
    "robotcar": (["--dataset", "robotcar", "--features", f"o/{FEAT}.h5", "--ransac_thresh", "12", "--opt_thresh", "12", "--covisibility_frame", "20",
                  "--opt_type", "clurefpos", "--inlier_thresh", "100", "--radius", "20"], f"out/{FEAT}_NNM_sng_12_100all_o3op20clurefposth12r20i5"),
    "ecmu": (["--dataset", "ecmu", "--features", "o/feats-ressegnetv2-20220810-sfd2-0001-n4096-r1024.h5", "--ransac_thresh", "15", "--opt_thresh", "15",
              "--covisibility_frame", "10", "--opt_type", "clurefobs", "--inlier_thresh", "20", "--radius", "30", "--slice", "18"],
             "out/slice18_feats-ressegnetv2-20220810-sfd2-0001-n4096-r1024_NNM_sng_15_20vis_o3op10clurefobsth15r30i5"),
}


def test_parsers(tmp_path):
    (tmp_path / "r.txt").write_text("q/a.jpg db/1.jpg\nq/a.jpg db/2.jpg\nq/b.jpg no_match\nq/c.jpg db/3.jpg\nq/a.jpg db/0.jpg\n")
    assert parsers.read_retrieval_results(tmp_path / "r.txt") == {"q/a.jpg": ["db/1.jpg", "db/2.jpg", "db/0.jpg"], "q/c.jpg": ["db/3.jpg"]}
    (tmp_path / "list_day.txt").write_text("q/a.jpg SIMPLE_RADIAL 1600 1200 1469.2 800 600 -0.05\nq/b.jpg PINHOLE 640 480 500 501 320 240\n")
    got = parsers.query_cameras(tmp_path / "list_*.txt")
    assert [n for n, _ in got] == ["q/a.jpg", "q/b.jpg"]
    assert got[0][1]["model"] == "SIMPLE_RADIAL" and got[0][1]["width"] == 1600 and got[0][1]["height"] == 1200
    assert got[0][1]["params"].tolist() == [1469.2, 800.0, 600.0, -0.05] and got[1][1]["params"].dtype == np.float64
    assert pairs_from_retrieval.parse_image_lists_with_intrinsics is parsers.parse_image_lists_with_intrinsics   # one parser
    name, (model, w, h, params) = parsers.parse_image_lists_with_intrinsics(tmp_path / "list_day.txt")[1]
    assert (name, model, w, h) == ("q/b.jpg", "PINHOLE", 640, 480)


def test_argument_defaults_are_the_reference_s():
    a = localizer.make_parser().parse_args(["--dataset", "aachen", "--db_imglist_fn", "x", "--reference_sfm", "m", "--queries", "q", "--features", "f.h5"])
    assert (a.ransac_thresh, a.covisibility_frame, a.with_match, a.do_covisible_opt, a.init_type, a.opt_type, a.matcher_method) == \
        (12, 50, False, False, "clu", "cluster", "NNM")
    assert (a.inlier_thresh, a.obs_thresh, a.opt_thresh, a.radius, a.iters, a.retrieval, a.gt_pose_fn, a.only_gt, a.slice) == (50, 3, 12, 20, 1, None, None, 0, 2)
    assert a.device == 0 and a.stage1 in ("device", "host")


@pytest.mark.parametrize("script", list(SCRIPTS))
def test_output_names_of_the_reference_scripts(script):
    extra, want = SCRIPTS[script]
    args = localizer.make_parser().parse_args(COMMON + extra)
    assert localizer.output_stem(args, ecmu=args.dataset == "ecmu") == want
    args.do_covisible_opt = False
    assert localizer.output_stem(args, ecmu=args.dataset == "ecmu") == want[:want.index("_o3op")]
    args.do_covisible_opt, args.iters = True, 0
    assert localizer.output_stem(args, ecmu=args.dataset == "ecmu") == want[:-2]       # no i<iters> for iters = 0


def test_naming_rules():
    q = "query/night/nexus5x/IMG_1.jpg"
    assert localizer.result_name("aachen", q) == localizer.result_name("aachen_v1.1", q) == "IMG_1.jpg"
    assert localizer.result_name("robotcar", "overcast/rear/123.jpg") == "rear/123.jpg"
    assert localizer.result_name("ecmu", q, ecmu=True) == "IMG_1.jpg"
    with pytest.raises(ValueError):
        localizer.result_name("ecmu", q)                            # run() has no ecmu rule, only run_ecmu()
    with pytest.raises(ValueError):
        localizer.result_name("inloc", q)


# ---------------------------------------------------------------------------------------------------------------- run() end to end
QUERIES = ["query/q0.jpg", "query/day/q1.jpg", "query/night/rear/q2.jpg", "query/q3.jpg", "query/q4.jpg"]


@pytest.fixture()
def world(tmp_path):
    """The refinement scene of covis_ref: 8 database images (image 3 without key points, image 4 under the <= 3 rule), and five
    queries that all carry the scene's one set of key points."""
    sc = cr.refinement_scene(seed=0)
    store = cr.feature_file(sc)
    for q in QUERIES[1:]:
        store[q] = store[cr.QNAME]
    names = {i: im.name for i, im in sc["images"].items()}
    retrieval = {QUERIES[0]: [names[1], names[2], "db/not_in_model.jpg", names[3], names[4], names[5]],
                 QUERIES[1]: [names[4], names[3], names[6], names[7], names[1]],
                 QUERIES[2]: None,                                  # a no_match line: absent from the parsed file
                 QUERIES[3]: ["db/not_in_model.jpg"],
                 QUERIES[4]: [names[8], names[2]]}
    gt = {"q0.jpg": (sc["q"], sc["t"]), "q4.jpg": (sc["q"], sc["t"] + [0.3, 0, 0])}
    paths = lf.write_inputs(tmp_path, sc["images"], sc["points3D"], cr.CAMERA, QUERIES, retrieval, gt)
    return sc, store, paths


def _run(world, dataset="aachen", est_kw=None, **kw):
    sc, store, paths = world
    args = localizer.make_parser().parse_args(lf.argv(paths, dataset=dataset, db_imglist_fn="x", features="feats-x.h5", **kw))
    est, refi = cr.make_estimator(sc, 0, **(est_kw or {})), cr.make_refiner(sc, 0)
    mi = covis.MapIndex(sc["images"], sc["points3D"])
    run = localizer.run_ecmu if dataset == "ecmu" else localizer.run
    stem = run(args, estimator=est, refiner=refi, matcher=cr.scripted_matcher(sc), features=store,
               clusterer=lambda lists: [clr.clusters(li, sc["images"], sc["points3D"]) for li in lists])
    read = lambda ext: open(stem + ext).read().splitlines()  # noqa: E731
    return args, stem, read(".txt"), read(".txt.failed"), read(".log"), read("_full.log"), (est, refi, mi)


def _expected(world, args, cluster_lists, est, covis_obj=None):
    """localize_queries fed directly, the way the parent's callers do: clusters of (image, matches0) from the scripted matcher."""
    sc, store, _ = world
    m = cr.scripted_matcher(sc)
    qs = []
    for qname, cl in cluster_lists:
        clusters = [[(sc["images"][i], m(qname, [sc["images"][i].name], None)[0]) for i in c] for c in cl]
        qs.append(dict(kpq=store[qname]["keypoints"], clusters=clusters, camera=cr.CAMERA, qname=qname))
    return localize.localize_queries(qs, args.ransac_thresh, inlier_th=args.inlier_thresh, points3D=sc["points3D"], obs_th=args.obs_thresh,
                                     estimator=est, covis=covis_obj)


@pytest.mark.parametrize("stage1", ["device", "host"])
def test_run_sng_writes_the_four_files(world, stage1, caplog):
    with caplog.at_level("WARNING"):
        args, stem, txt, failed, log, full, (est, refi, mi) = _run(world, init_type="sng", stage1=stage1, with_match=True)
    assert os.path.basename(stem) == "feats-x_NNM_sng_12_50all"
    lists = [(QUERIES[0], [[1], [2], [3], [4], [5]]), (QUERIES[1], [[4], [3], [6], [7], [1]]), (QUERIES[4], [[8], [2]])]
    want = _expected(world, args, lists, est)
    assert len(txt) == 3
    for line, (qname, _), (qvec, tvec, n, best) in zip(txt, lists, want):
        assert line == f"{qname.split('/')[-1]} {' '.join(map(str, qvec))} {' '.join(map(str, tvec))}"
        assert n > 0
    assert log == [f"{q} {b['dbname']} {int(b['num_inliers'])} {int(b['order'])}" for (q, _), (_, _, _, b) in zip(lists, want)]
    assert log[0].split()[0] == QUERIES[0] and log[0].split()[1] == "db/001.jpg" and log[0].split()[3] == "1"
    assert log[1].split()[1] != "db/004.jpg" and int(log[1].split()[3]) >= 3          # images 4 (<= 3 points) and 3 (no key points) give nothing
    # the deviation: a query missing from the retrieval file, or with nothing in the model, is skipped, warned about and listed as failed
    assert failed == [QUERIES[2], QUERIES[3]]
    text = caplog.text
    assert "db/not_in_model.jpg was retrieved but not in database" in text and f"{QUERIES[2]} is not in the retrieval file" in text
    assert f"{QUERIES[3]} has no retrieved image in the model" in text
    # summary lines: counters, and the ground-truth part for the two queries that have one
    assert len(full) == 3 and all(l.startswith("All 0/") and "time[cs/fn]:" in l for l in full)
    assert full[0].startswith("All 0/1 failed cases top@1:1.00") and "q_error:" in full[0] and full[0].endswith("/1") and "q_error" not in full[1]
    qe, te, _ = covis.compute_pose_error(want[2][0], want[2][1], world[0]["q"], world[0]["t"] + [0.3, 0, 0])
    assert f"q_error:{qe:.2f} t_error:{te:.2f}" in full[2] and full[2].endswith("/2")


def test_run_clu_and_the_covisibility_option(world):
    args, stem, txt, failed, log, full, (est, refi, mi) = _run(world, init_type="clu", do_covisible_opt=True, opt_type="clurefobs", iters=1, radius=20,
                                                               obs_thresh=3, opt_thresh=12, covisibility_frame=50, stage1="device")
    assert os.path.basename(stem) == "feats-x_NNM_clu_12_50all_o3op50clurefobsth12r20i1"
    sc = world[0]
    cl = lambda ids: clr.clusters(ids, sc["images"], sc["points3D"])  # noqa: E731
    lists = [(QUERIES[0], cl([1, 2, 3, 4, 5])), (QUERIES[1], cl([4, 3, 6, 7, 1])), (QUERIES[4], cl([8, 2]))]
    assert len(lists[0][1]) < 5                                     # clustering merged something
    est2, refi2 = cr.make_estimator(sc, 0), cr.make_refiner(sc, 0)
    cov = localize.Covis(mi, cr.scripted_matcher(sc), world[1], opt_type="clurefobs", covisibility_frame=50, iters=1, radius=20, obs_th=3.0, opt_th=12.0,
                         estimator=est2, refiner=refi2)
    want = _expected(world, args, lists, est2, cov)
    assert len(refi.calls) == len(refi2.calls) > 0                  # the refinement ran, as often as in the direct call
    assert [l.split(" ", 1)[0] for l in txt] == ["q0.jpg", "q1.jpg", "q4.jpg"] and failed == [QUERIES[2], QUERIES[3]]
    assert log == [f"{q} {b['dbname']} {int(b['num_inliers'])} {int(b['order'])}" for (q, _), (_, _, _, b) in zip(lists, want)]


def test_failed_lists_exactly_the_queries_that_return_zero(world):
    # no cluster reaches --inlier_thresh, the kept pose has >= 10 inliers: returned with 0 -> listed
    args, stem, txt, failed, log, full, _ = _run(world, init_type="sng", inlier_thresh=100000)
    assert failed == [QUERIES[2], QUERIES[3], QUERIES[0], QUERIES[1], QUERIES[4]] and len(txt) == 3
    assert full[-1].startswith("All 3/3 failed cases")
    # every estimate fails: the first image's pose with -1 -> a pose line, and NOT listed (the reference tests == 0)
    args, stem, txt, failed, log, full, _ = _run(world, init_type="sng", est_kw=dict(success=False))
    assert failed == [QUERIES[2], QUERIES[3]] and len(txt) == 3 and [l.split()[2:] for l in log] == [["0", "-1"]] * 3
    im = world[0]["images"][1]
    assert txt[0] == f"q0.jpg {' '.join(map(str, im.qvec))} {' '.join(map(str, im.tvec))}"


def test_robotcar_and_ecmu_dispatch(world):
    args, stem, txt, *_ = _run(world, dataset="robotcar", init_type="sng")
    assert [l.split(" ", 1)[0] for l in txt] == ["query/q0.jpg", "day/q1.jpg", "query/q4.jpg"]
    args, stem, txt, *_ = _run(world, dataset="ecmu", init_type="sng", slice=18)
    assert os.path.basename(stem) == "slice18_feats-x_NNM_sng_12_50vis" and [l.split(" ", 1)[0] for l in txt] == ["q0.jpg", "q1.jpg", "q4.jpg"]
    with pytest.raises(ValueError):
        _run(world, dataset="inloc", init_type="sng")
