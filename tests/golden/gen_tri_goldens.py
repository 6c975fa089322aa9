"""Golden generator for sfd2_amd/colmap_io.py: a tiny COLMAP model (the synthetic scene of tests/tri_ref.py and the map its numpy
restatement triangulates, plus one RADIAL camera no image uses) written by the REFERENCE's hloc/utils/read_write_model.py into
tests/golden/tri_model/{cameras,images,points3D}.bin, and the values it holds into tests/golden/tri_model/expected.npz.

Run only where the reference is mounted (SFD2_REFERENCE, default /root/reference); CPU only:
    python tests/golden/gen_tri_goldens.py"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFD2_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

spec = importlib.util.spec_from_file_location("ref_read_write_model", os.path.join(REF, "hloc", "utils", "read_write_model.py"))
rw = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rw)

import tri_ref as tr  # noqa: E402


def main():
    out = os.path.join(HERE, "tri_model")
    os.makedirs(out, exist_ok=True)
    sc = tr.make_scene(seed=3, n_images=6, n_points=260, n_clutter=40, n_joiners=4, n_weak_pairs=1, depth=(8.0, 20.0))
    L = tr.Layout(sc["cameras"], sc["images"], sc["keypoints"])
    m, off, _, _, _ = tr.verify_ref(L, sc["pair_matches"])
    _, t_off, t_nodes = tr.tracks_ref(int(L.off[-1]), tr.edges_of(L, sc["pair_matches"], m, off))
    tri = tr.triangulate_ref(L, t_off, t_nodes)
    rs = np.random.RandomState(0)
    cameras = {cid: rw.Camera(id=cid, model=c["model"], width=c["width"], height=c["height"], params=np.array(c["params"], float))
               for cid, c in sc["cameras"].items()}
    cameras[9] = rw.Camera(id=9, model="RADIAL", width=1024, height=768, params=np.array([900.0, 512.0, 384.0, -0.05, 0.01]))
    node_pid = np.full(int(L.off[-1]), -1, dtype=np.int64)
    points3D, pid = {}, 0
    for t in range(len(t_off) - 1):
        for p in range(tr.MAX_POINTS):
            if tri["n_obs"][t, p] == 0:
                continue
            pid += 1
            nodes = t_nodes[t_off[t]:t_off[t + 1]][tri["obs_point"][t_off[t]:t_off[t + 1]] == p].astype(np.int64)
            node_pid[nodes] = pid
            view = L.node_view[nodes]
            points3D[pid] = rw.Point3D(id=pid, xyz=tri["xyz"][t, p], rgb=rs.randint(0, 256, 3), error=float(tri["error"][t, p]),
                                       image_ids=np.array([L.ids[v] for v in view]), point2D_idxs=nodes - L.off[view])
    images = {}
    for k, iid in enumerate(L.ids):
        im = sc["images"][iid]
        images[iid] = rw.Image(id=iid, qvec=im.qvec, tvec=im.tvec, camera_id=im.camera_id, name=im.name,
                               xys=L.px[L.off[k]:L.off[k + 1]], point3D_ids=node_pid[L.off[k]:L.off[k + 1]])
    rw.write_model(cameras, images, points3D, out, ext=".bin")
    cam_ids = sorted(cameras)
    exp = {"cam/ids": np.array(cam_ids), "cam/models": np.array([cameras[c].model for c in cam_ids]),
           "cam/wh": np.array([[cameras[c].width, cameras[c].height] for c in cam_ids]),
           "cam/nparams": np.array([len(cameras[c].params) for c in cam_ids]),
           "cam/params": np.concatenate([cameras[c].params for c in cam_ids]),
           "img/ids": np.array(L.ids), "img/qvec": np.array([images[i].qvec for i in L.ids]), "img/tvec": np.array([images[i].tvec for i in L.ids]),
           "img/camera_id": np.array([images[i].camera_id for i in L.ids]), "img/names": np.array([images[i].name for i in L.ids]),
           "img/offsets": L.off, "img/xys": L.px, "img/point3D_ids": node_pid,
           "pt/ids": np.array(sorted(points3D)), "pt/xyz": np.array([points3D[i].xyz for i in sorted(points3D)]),
           "pt/rgb": np.array([points3D[i].rgb for i in sorted(points3D)]), "pt/error": np.array([points3D[i].error for i in sorted(points3D)]),
           "pt/offsets": np.concatenate([[0], np.cumsum([len(points3D[i].image_ids) for i in sorted(points3D)])]),
           "pt/image_ids": np.concatenate([points3D[i].image_ids for i in sorted(points3D)]),
           "pt/point2D_idxs": np.concatenate([points3D[i].point2D_idxs for i in sorted(points3D)])}
    np.savez_compressed(os.path.join(out, "expected.npz"), **exp)
    for f in sorted(os.listdir(out)):
        print(f, os.path.getsize(os.path.join(out, f)))


if __name__ == "__main__":
    main()
