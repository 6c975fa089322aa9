"""Writes the files `python -m sfd2_amd.localizer` reads from a synthetic scene (shared by the localiser tests, never imported by
the product): a COLMAP model, a query list with intrinsics, a retrieval file and a ground-truth pose file."""
import os

import numpy as np

from sfd2_amd import colmap_io


def write_model(images, points3D, cam, path):
    """images / points3D as covis_ref builds them (Img, Pt) -> cameras.bin, images.bin, points3D.bin."""
    cameras = {1: colmap_io.Camera(1, cam["model"], cam["width"], cam["height"], cam["params"])}
    ims = {i: colmap_io.Image(id=i, qvec=im.qvec, tvec=im.tvec, camera_id=1, name=im.name, xys=np.zeros((len(im.point3D_ids), 2)),
                              point3D_ids=np.asarray(im.point3D_ids, dtype=np.int64)) for i, im in images.items()}
    pts = {p: colmap_io.Point3D(id=p, xyz=pt.xyz, rgb=np.zeros(3, np.uint8), error=0.0, image_ids=np.asarray(pt.image_ids, dtype=np.int32),
                                point2D_idxs=np.zeros(len(pt.image_ids), np.int32)) for p, pt in points3D.items()}
    colmap_io.write_model(cameras, ims, pts, path)


def write_inputs(root, images, points3D, cam, queries, retrieval, gt=None):
    """queries: names; retrieval: {query name: [db names]} (a name mapped to None is written as a no_match line); gt: {name: (qvec,
    tvec)}.  Returns the paths as a dict of the command's arguments."""
    root = str(root)
    write_model(images, points3D, cam, os.path.join(root, "model"))
    with open(os.path.join(root, "queries.txt"), "w") as f:
        for q in queries:
            f.write(" ".join([q, cam["model"], str(cam["width"]), str(cam["height"])] + [repr(float(v)) for v in cam["params"]]) + "\n")
    with open(os.path.join(root, "retrieval.txt"), "w") as f:
        for q, names in retrieval.items():
            for n in (names if names is not None else ["no_match"]):
                f.write(f"{q} {n}\n")
    out = dict(reference_sfm=os.path.join(root, "model"), queries=os.path.join(root, "queries.txt"), retrieval=os.path.join(root, "retrieval.txt"),
               save_root=os.path.join(root, "out"))
    if gt is not None:
        with open(os.path.join(root, "gt.txt"), "w") as f:
            for n, (qv, tv) in gt.items():
                f.write(" ".join([n] + [repr(float(v)) for v in list(qv) + list(tv)]) + "\n")
        out["gt_pose_fn"] = os.path.join(root, "gt.txt")
    return out


def argv(paths, **kw):
    """The command line for the paths of write_inputs plus options (True = a flag)."""
    a = []
    for k, v in {**paths, **kw}.items():
        a += [f"--{k}"] if v is True else [f"--{k}", str(v)]
    return a
