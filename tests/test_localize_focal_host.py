"""The localiser glue with an estimator that returns a camera, no GPU: the options reach the estimator through
**ransac, the kept result carries the camera, and without one nothing changes."""
import numpy as np

from sfd2_amd import localize, pose


class _Pt:
    def __init__(self, xyz, image_ids):
        self.xyz, self.image_ids = np.asarray(xyz, float), image_ids


class _Img:
    def __init__(self, name, point3D_ids):
        self.name, self.point3D_ids, self.qvec, self.tvec = name, np.asarray(point3D_ids), np.array([1.0, 0, 0, 0]), np.zeros(3)


def _query(rs, sizes, nq=300):
    clusters, points3D = [], {}
    for c, n in enumerate(sizes):
        ids = np.arange(1000 * (c + 1), 1000 * (c + 1) + n)
        matches = np.full(nq, -1)
        matches[rs.choice(nq, n, replace=False)] = np.arange(n)
        clusters.append([(_Img(f"db{c}", ids), matches)])
        for pid in ids:
            points3D[int(pid)] = _Pt(rs.rand(3), [0, 1, 2, 3])
    return rs.rand(nq, 2) * 300, clusters, points3D


CAM = {"model": "SIMPLE_RADIAL", "width": 640, "height": 480, "params": [768.0, 320.0, 240.0, 0.0]}


def _estimator(script, with_camera):
    def est(problems):
        out = []
        for (x, X, cam, thr), (ok, ni, f) in zip(problems, script):
            inl = np.zeros(len(x), bool)
            inl[:ni] = True
            r = {"success": ok, "qvec": np.array([1.0, 0, 0, 0]), "tvec": np.array([float(ni), 0, 0]), "num_inliers": ni, "inliers": inl}
            if with_camera:
                r["camera"] = dict(cam, params=[f, 320.0, 240.0, 0.0])
            out.append(r)
        return out
    return est


def test_the_kept_result_carries_the_camera():
    kpq, clusters, points3D = _query(np.random.RandomState(3), [100, 120, 90])
    script = [(True, 30, 500.0), (True, 70, 640.0), (True, 20, 900.0)]
    q, t, n, best = localize.pose_from_clusters(kpq, clusters, CAM, 12.0, points3D=points3D, estimator=_estimator(script, True))
    assert n == 70 and best["camera"]["params"][0] == 640.0 and best["camera"]["model"] == "SIMPLE_RADIAL"
    q2, t2, n2, best2 = localize.pose_from_clusters(kpq, clusters, CAM, 12.0, points3D=points3D, estimator=_estimator(script, False))
    assert n2 == n and np.array_equal(t2, t) and "camera" not in best2
    assert {k: v for k, v in best.items() if k not in ("camera", "inlier", "qvec", "tvec")} == \
        {k: v for k, v in best2.items() if k not in ("inlier", "qvec", "tvec")}


def test_options_reach_the_default_estimator(monkeypatch):
    seen = {}

    def fake(problems, **kw):
        seen.update(kw)
        return _estimator([(True, 60, 700.0)] * len(problems), True)(problems)
    monkeypatch.setattr(pose, "absolute_pose_estimation_batch", fake)
    kpq, clusters, points3D = _query(np.random.RandomState(4), [100])
    out = localize.localize_queries([{"kpq": kpq, "clusters": clusters, "camera": CAM}], 12.0, points3D=points3D, estimate_focal_length=True,
                                    refine_focal_length=True, seed=2)
    assert seen == {"estimate_focal_length": True, "refine_focal_length": True, "seed": 2}
    assert out[0][2] == 60 and out[0][3]["camera"]["params"][0] == 700.0
