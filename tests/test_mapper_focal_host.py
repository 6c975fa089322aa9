"""The mapper's registration of views whose camera nobody has seen (reconstruction option abs_pose_estimate_focal_length, DESIGN.md
section 22), no GPU: reconstruct() runs through the numpy stand-ins of tests/mapper_ref.py with a focal-sweeping DLT stand-in for
DeviceStages.absolute_pose_focal.  Which candidates take the new stage, the update of the camera record and of the views, the
shared-camera rule, the try counter, and that the option off gives the bytes of a run without the option."""
import numpy as np

import mapper_ref as mr
import pose_focal_ref as fr
import pose_ref as pr
import tri_ref as tr
from sfd2_amd import reconstruction as RC

FACTORS = np.linspace(0.5, 2.0, 13)          # 1.25, the true factor of every wrong camera below, is one of them
OFF = 1.25


class FocalStages(mr.RefStages):
    """RefStages with absolute_pose_focal: the DLT stand-in at every scaled camera, the sample with the most inliers wins (ties to the
    smaller mean error of the inliers: at 12 px neighbouring factors hold the same points).  fail_focal: views whose focal call always fails."""

    def __init__(self, scene, fail_views=(), fail_focal=()):
        super().__init__(scene, fail_views)
        self.fail_focal = set(fail_focal)
        self.calls["absolute_pose_focal"] = []
        self.seen_cameras = []

    def absolute_pose_focal(self, problems, cand, max_error_px, min_inlier_ratio, seed):
        self.calls["absolute_pose_focal"].append(list(cand))
        out = []
        for (p2, p3, cam), v in zip(problems, cand):
            self.seen_cameras.append((v, [float(x) for x in cam["params"]]))
            best = None
            for a in FACTORS:
                sc = fr.scaled_camera(cam, a)
                calls = self.calls["absolute_pose"]
                r = mr.RefStages.absolute_pose(self, [(p2, p3, sc)], [v], max_error_px, min_inlier_ratio, seed)[0]
                del calls[-1]                                                # the sweep's calls are no calls of the fixed stage
                if v in self.fail_focal:
                    r = dict(r, success=False, num_inliers=0)
                err = float(pr.reproj_error(sc, r["qvec"], r["tvec"], p2, p3)[r["inliers"]].mean()) if r["num_inliers"] else np.inf
                if best is None or (r["num_inliers"], -err) > (best["num_inliers"], -best["err"]):
                    best = dict(r, camera=sc, focal_factor=float(a), err=err)
            out.append(best)
        return out


def _scene():
    return mr.br.cached(("mapper_host_scene",), tr.make_scene)


def _unknown_cameras(sc, pair, shared=()):
    """Every image outside the initial pair gets a camera of its own (id 100 + image id) at the true focal / OFF; the images of
    `shared` use the first one's."""
    cameras = {cid: tr.Cam(dict(c, params=np.array(c["params"], dtype=np.float64))) for cid, c in sc["cameras"].items()}
    images = {}
    for iid, im in sc["images"].items():
        cid = im.camera_id
        if iid not in pair:
            cid = 100 + (shared[0] if iid in shared else iid)
            if cid not in cameras:
                true = sc["cameras"][sc["images"][cid - 100].camera_id]
                cameras[cid] = tr.Cam(dict(fr.scaled_camera(true, 1.0 / OFF), id=cid, params=np.array(fr.scaled_camera(true, 1.0 / OFF)["params"])))
        images[iid] = tr.Img(iid, im.qvec, im.tvec, cid, im.name)
    return cameras, images


def _reconstruct(sc, cameras, images, S, **kw):
    rep = {}
    out = RC.reconstruct(cameras, images, sc["keypoints"], sc["pair_matches"], stages=S, report=rep, **kw)
    return out, rep


def _base():
    def make():
        sc = _scene()
        rep = {}
        RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], stages=mr.RefStages(sc), report=rep)
        return rep
    return mr.br.cached(("mapper_focal_base",), make)


def _focal_run():
    def make():
        sc = _scene()
        pair = _base()["initial_pair"]
        cameras, images = _unknown_cameras(sc, pair)
        S = FocalStages(sc)
        out, rep = _reconstruct(sc, cameras, images, S, abs_pose_estimate_focal_length=True)
        return cameras, images, S, out, rep
    return mr.br.cached(("mapper_focal_run",), make)


def test_unseen_cameras_take_the_new_stage_and_are_updated():
    sc = _scene()
    cameras, images, S, (cams, ims, pts), rep = _focal_run()
    pair = rep["initial_pair"]
    assert pair == _base()["initial_pair"] and len(ims) == 12 and rep["final"]["n_registered"] == 12
    index = {iid: k for k, iid in enumerate(sorted(images, key=lambda i: (images[i].name, i)))}
    asked_focal = [v for c in S.calls["absolute_pose_focal"] for v in c]
    assert sorted(set(asked_focal)) == sorted(index[i] for i in images if i not in pair)     # every view outside the pair has an unseen camera
    assert S.calls["absolute_pose"] == []                                                    # and none went through the fixed stage
    for r in rep["rounds"]:
        assert r.get("focal_candidates", []) == r["candidates"]
    # the records: the true focal length again (the stand-in's grid holds the true factor), the given dict untouched
    for iid, im in images.items():
        cid = im.camera_id
        true = sc["cameras"][sc["images"][iid].camera_id]
        if iid in pair:
            assert np.array_equal(cams[cid]["params"], cameras[cid]["params"])
            continue
        nf = fr.N_FOCAL[true["model"]]
        assert np.allclose(cams[cid]["params"][:nf], np.asarray(true["params"])[:nf], rtol=1e-12), (iid, cams[cid]["params"])
        assert np.allclose(cameras[cid]["params"][:nf], np.asarray(true["params"])[:nf] / OFF, rtol=1e-12)      # the caller's dict is not written
        assert cams[cid]["model"] == true["model"] and np.array_equal(cams[cid]["params"][nf:], cameras[cid]["params"][nf:])
    # every focal call saw the prior: a camera is estimated once, before its first view registers
    for v, params in S.seen_cameras:
        iid = sorted(images, key=lambda i: (images[i].name, i))[v]
        assert params == [float(x) for x in cameras[images[iid].camera_id]["params"]]
    e = mr.model_errors(ims, pts, sc["images"])
    assert e["rotation"] < 0.02 and e["centre"] < 0.1, e


def test_option_off_changes_nothing():
    sc = _scene()
    a = RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], stages=mr.RefStages(sc))
    S = FocalStages(sc)
    b = RC.reconstruct(sc["cameras"], sc["images"], sc["keypoints"], sc["pair_matches"], stages=S, abs_pose_estimate_focal_length=False)
    assert len(a) == len(b) == 2 and S.calls["absolute_pose_focal"] == []
    assert sorted(a[0]) == sorted(b[0]) and sorted(a[1]) == sorted(b[1])
    for i in a[0]:
        assert a[0][i].qvec.tobytes() == b[0][i].qvec.tobytes() and a[0][i].tvec.tobytes() == b[0][i].tvec.tobytes()
        assert a[0][i].point3D_ids.tobytes() == b[0][i].point3D_ids.tobytes()
    for p in a[1]:
        assert a[1][p].xyz.tobytes() == b[1][p].xyz.tobytes() and a[1][p].image_ids.tobytes() == b[1][p].image_ids.tobytes()
    assert RC.DEFAULTS["abs_pose_estimate_focal_length"] is False
    assert RC.parser().parse_args(["--sfm_dir", "s", "--image_dir", "d", "--pairs", "p", "--features", "f", "--matches", "m"]).abs_pose_estimate_focal_length == 0
    assert RC.parser().parse_args(["--sfm_dir", "s", "--image_dir", "d", "--pairs", "p", "--features", "f", "--matches", "m",
                                   "--abs_pose_estimate_focal_length", "1"]).abs_pose_estimate_focal_length == 1


def test_known_cameras_keep_the_fixed_stage_with_the_option_on():
    """The scene as it is: four cameras over twelve images, all true.  Views of a camera the initial pair (or an earlier round) has
    registered go through the fixed stage; only a camera's first view takes the new one."""
    sc = _scene()
    S = FocalStages(sc)
    (cams, ims, pts), rep = _reconstruct(sc, sc["cameras"], sc["images"], S, abs_pose_estimate_focal_length=True)
    order = sorted(sc["images"], key=lambda i: (sc["images"][i].name, i))
    seen = {sc["images"][i].camera_id for i in rep["initial_pair"]}
    for r, fixed in zip([r for r in rep["rounds"] if r["candidates"]], S.calls["absolute_pose"] + [[]] * 12):
        want_focal = [i for i in r["candidates"] if sc["images"][i].camera_id not in seen]
        assert r.get("focal_candidates", []) == want_focal
        if want_focal:
            assert sorted(order[v] for v in fixed) == sorted(set(r["candidates"]) - set(want_focal))
        seen |= {sc["images"][i].camera_id for i in r["registered"]}
    assert len(ims) == 12 and len(seen) == 4


def test_shared_camera_first_to_register_sets_it_and_the_others_wait_without_losing_a_try():
    sc = _scene()
    base = _base()
    pair = base["initial_pair"]
    first_round = [i for i in base["rounds"][0]["candidates"]]
    model_of = {i: sc["cameras"][sc["images"][i].camera_id]["model"] for i in sc["images"]}
    shared = next([a, b] for a in first_round for b in first_round if a < b and model_of[a] == model_of[b])      # two candidates of round one, one model
    cameras, images = _unknown_cameras(sc, pair, shared=shared)
    S = FocalStages(sc)
    (cams, ims, pts), rep = _reconstruct(sc, cameras, images, S, abs_pose_estimate_focal_length=True)
    order = sorted(images, key=lambda i: (images[i].name, i))
    r0 = rep["rounds"][0]
    assert set(shared) <= set(r0["candidates"]) and set(shared) <= set(r0["focal_candidates"])
    cand_order = [i for i in r0["candidates"] if i in shared]
    assert cand_order[0] in r0["registered"] and cand_order[1] not in r0["registered"]       # the first sets the camera, the other waits
    r1 = rep["rounds"][1]
    assert cand_order[1] in r1["candidates"] and cand_order[1] not in r1.get("focal_candidates", []) and cand_order[1] in r1["registered"]
    v = order.index(cand_order[1])
    assert sum(v in c for c in S.calls["absolute_pose_focal"]) == 1 and sum(v in c for c in S.calls["absolute_pose"]) == 1
    assert len(ims) == 12
    # the waiting view lost no try: with one try allowed it still registers in round two
    S1 = FocalStages(sc)
    (_, ims1, _), rep1 = _reconstruct(sc, cameras, images, S1, abs_pose_estimate_focal_length=True, max_reg_trials=1)
    assert cand_order[1] in rep1["rounds"][1]["registered"] and len(ims1) == 12


def test_a_focal_call_that_fails_costs_a_try():
    sc = _scene()
    pair = _base()["initial_pair"]
    cameras, images = _unknown_cameras(sc, pair)
    order = sorted(images, key=lambda i: (images[i].name, i))
    target = order.index(_base()["rounds"][0]["candidates"][0])
    S = FocalStages(sc, fail_focal=[target])
    (cams, ims, pts), rep = _reconstruct(sc, cameras, images, S, abs_pose_estimate_focal_length=True)
    assert sum(target in c for c in S.calls["absolute_pose_focal"]) == 3 and target + 1 not in ims and len(ims) == 11
    cid = images[order[target]].camera_id
    assert np.array_equal(cams[cid]["params"], cameras[cid]["params"])                       # never registered: the record keeps the prior
