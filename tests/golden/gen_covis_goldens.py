"""Golden generator for the covisibility stage: runs the REFERENCE's it_loc/localize_cv2.py (get_covisibility_frames,
get_covisibility_frames_by_pose, pose_refinement_covisibility) on the seeded synthetic maps of tests/covis_ref.py and writes
tests/golden/covis.npz -- numbers and names only.

Run only where the reference is mounted (SFD2_REFERENCE, default /root/reference); CPU only:
    python tests/golden/gen_covis_goldens.py

Stand-ins for what the authoring machine lacks: empty cv2 / h5py / tqdm modules, a pycolmap module whose two functions are the
scripted ones of covis_ref, and it_loc.common.sciR replaced by a wrapper that maps as_dcm to scipy's as_matrix."""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFD2_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

for name in ("cv2", "h5py", "pycolmap"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["cv2"].INTER_NEAREST = 0
try:
    import tqdm  # noqa: F401
except Exception:
    sys.modules["tqdm"] = types.ModuleType("tqdm")
    sys.modules["tqdm"].tqdm = lambda x, *a, **k: x
for name in ("float", "int", "bool"):
    if not hasattr(np, name):
        setattr(np, name, {"float": float, "int": int, "bool": bool}[name])

from scipy.spatial.transform import Rotation  # noqa: E402

import it_loc.common as ref_common  # noqa: E402


class _SciR:
    def __init__(self, r):
        self.r = r

    @classmethod
    def from_quat(cls, quat):
        return cls(Rotation.from_quat(quat))

    def as_dcm(self):
        return self.r.as_matrix()

    def as_quat(self):
        return self.r.as_quat()


ref_common.sciR = _SciR
import it_loc.localize_cv2 as ref  # noqa: E402
import pycolmap  # noqa: E402

import covis_ref as cr  # noqa: E402


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def main():
    out = {}
    # ---- frame selections
    images, points3D = cr.selection_map()
    saw_fallback = saw_tie = False
    for c, (kind, frame, cf, obs_th, pose) in enumerate(cr.SELECTION_CASES):
        q, t = cr.selection_pose(images, frame, pose, c)
        if kind == "obs":
            got = quiet(ref.get_covisibility_frames, frame_id=frame, all_images=images, points3D=points3D, covisibility_frame=cf,
                        ref_3Dpoints=None, obs_th=obs_th, pred_qvec=q, pred_tvec=t)
            if pose == "far":
                saw_fallback = True
                assert len(got) > 0                         # only the <= 3 fallback can have filled it
        else:
            got = quiet(ref.get_covisibility_frames_by_pose, frame_id=frame, all_images=images, points3D=points3D, covisibility_frame=cf,
                        ref_3Dpoints=None, pred_qvec=q, pred_tvec=t, q_th=10, t_th=10, obs_th=obs_th)
        if 7 in got and 8 in got:
            saw_tie = True
        out[f"sel{c}"] = np.array(got, dtype=np.int64)
    assert saw_fallback and saw_tie
    # ---- the refinement, end to end
    for ci, (name, (opt_type, iters, success, limit)) in enumerate(cr.REFINE_CASES.items()):
        sc = cr.refinement_scene(seed=ci)
        q0, t0 = cr.start_pose(sc, ci)
        est, refi = cr.make_estimator(sc, ci, success, limit), cr.make_refiner(sc, ci)
        pycolmap.absolute_pose_estimation = lambda x, X, cfg, th: est.one(x, X, cfg, th)
        pycolmap.pose_refinement = lambda tv, qv, x, X, m, cfg: refi.one(tv, qv, x, X, m, cfg)
        recorded = []

        def matcher(data):
            i = int(data["descriptors1"][0, 0])
            plan, ids = sc["plan"][i], sc["images"][i].point3D_ids
            to_masked = np.cumsum(ids != -1) - 1
            m = np.full(len(plan), -1, dtype=np.int64)
            m[plan >= 0] = to_masked[plan[plan >= 0]]
            return {"matches0": m}

        fm = ref.feature_matching

        def recording(**kw):
            r = fm(**kw)
            recorded.append(np.array(r, dtype=np.int64).copy())
            return r
        ref.feature_matching = recording
        try:
            ret = quiet(ref.pose_refinement_covisibility, qname=cr.QNAME, cfg=cr.CAMERA, feature_file=cr.feature_file(sc), db_frame_id=1,
                        db_images=sc["images"], points3D=sc["points3D"], thresh=12.0, matcher=matcher, covisibility_frame=cr.FRAMES,
                        iters=iters, obs_th=cr.OBS_TH, opt_th=cr.OPT_TH, qvec=q0, tvec=t0, radius=cr.RADIUS, log_info="", opt_type=opt_type)
        finally:
            ref.feature_matching = fm
        db_ids = list(ret["db_ids"])
        live = [d for d in db_ids if sc["images"][d].point3D_ids.size]
        assert len(recorded) == len(live)
        for d, m in zip(live, recorded):                   # the mapped-back matches are the plan (or all -1 under the <= 3 rule)
            want = sc["plan"][d] if (sc["images"][d].point3D_ids != -1).sum() > 3 else np.full(len(m), -1)
            assert np.array_equal(m, want), d
            out[f"{name}_matches_{d}"] = m
        # margins: no gate error near the radius, no refinement error near opt_th
        gated_first = False
        for d in live:
            ids = sc["images"][d].point3D_ids
            for idx in np.flatnonzero(sc["plan"][d] >= 0):
                pid = int(ids[sc["plan"][d][idx]])
                e = np.sqrt(np.sum((sc["kpq"][idx] - ref.reproject(sc["points3D"][pid].xyz.reshape(-1, 3), q0, t0, cr.CAMERA)) ** 2))
                assert abs(e - cr.RADIUS) > 1e-6
                if idx == 0 and pid == 117 and d == db_ids[min(db_ids.index(1), db_ids.index(2))]:
                    gated_first = e > cr.RADIUS
        assert gated_first, "key point 0's first match to point 117 must be gated out"
        mkpq = np.asarray(ret["mkpq"], float)
        assert not any(i3 == 117 and np.array_equal(p, sc["kpq"][0].astype(float) + 0.5) for i3, p in zip(ret["3D_ids"], mkpq))
        mp3d = np.array([sc["points3D"][int(i)].xyz for i in ret["3D_ids"]]).reshape(-1, 3)
        for qv, tv in [(q0, t0)] + refi.poses[:len(refi.calls)]:
            e = (mkpq - ref.reproject(mp3d, qv, tv, cr.CAMERA)) ** 2
            assert (np.abs(np.sqrt(e[:, 0] + e[:, 1]) - cr.OPT_TH) > 1e-6).all()
        assert len(refi.calls) == {"iters1": 1, "iters2": 2, "ransac_failure": 0, "few_inliers": 0, "no_ref": 0, "by_pose": 1}[name]
        assert opt_type.find("pos") < 0 or (3 in db_ids and 4 in db_ids)   # the image without 3D points (and the one under the <= 3 rule) among the frames
        out[f"{name}_success"] = np.array(bool(ret["success"]))
        out[f"{name}_qvec"] = np.asarray(ret["qvec"], float)
        out[f"{name}_tvec"] = np.asarray(ret["tvec"], float)
        out[f"{name}_inliers"] = np.asarray(ret["inliers"], bool)
        out[f"{name}_num_inliers"] = np.array(int(ret["num_inliers"]))
        out[f"{name}_mkpq"] = mkpq
        out[f"{name}_3D_ids"] = np.asarray(ret["3D_ids"], dtype=np.int64)
        out[f"{name}_db_ids"] = np.asarray(db_ids, dtype=np.int64)
        out[f"{name}_score_q"] = np.asarray(ret["score_q"], dtype=np.float32)
        print(name, "success", ret["success"], "m", len(mkpq), "inliers", int(ret["num_inliers"]), "frames", db_ids)
    path = os.path.join(HERE, "covis.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
