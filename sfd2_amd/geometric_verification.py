"""Geometric verification of a match store without poses: what `colmap matches_importer` does to the matches before COLMAP maps or
triangulates them (hloc/triangulation.py:114, hloc/reconstruction.py:145), on the device through sfd2_amd.two_view.  For every pair of
the pair list the relative pose is estimated from the pair's matches (five-point LO-RANSAC); the output store holds the
input's groups and datasets with the rejected entries of matches0 set to -1, so that match_features' readers,
`triangulation --skip_geometric_verification` and the localiser read it as they read any other match store.

  python -m sfd2_amd.geometric_verification --pairs P --features F --matches M --output V
         (--reference_sfm_model R | --intrinsics LIST...) [--max_error 4 --min_num_inliers 15 --relative_poses T]
  python -m sfd2_amd.geometric_verification --model fundamental --pairs P --features F --matches M --output V
         [--max_error 4 --min_num_inliers 15 --fundamental_matrices T]
  python -m sfd2_amd.geometric_verification --model geometry --pairs P --features F --matches M --output V
         [--reference_sfm_model R | --intrinsics LIST...] [--max_error 4 --min_num_inliers 15 --two_view_geometries T]

Intrinsics come from a COLMAP binary model (its poses go unused) or from lists `name model width height params...`
(parsers.parse_image_lists_with_intrinsics).  A pair with an image without intrinsics is skipped, as triangulation.read_inputs skips
it; a pair the match store lacks is an error.  --relative_poses writes one line per verified pair:
name0 name1 success num_inliers qw qx qy qz tx ty tz tri_angle_deg.

--model fundamental needs no intrinsics: every listed pair is verified by its fundamental matrix (seven-point LO-RANSAC),
as COLMAP verifies a pair without a trusted focal length.  --fundamental_matrices writes one line per verified pair:
name0 name1 success num_inliers and the nine entries of F (row-major, x1^T F x0 = 0 in pixels).

--model geometry estimates F and H for every pair, and E too where intrinsics are given, and keeps the matches of
two_view.decide_two_view_geometry's choice, as COLMAP labels a pair calibrated, uncalibrated, planar, panoramic or degenerate: a planar or
rotation-only pair keeps its matches through H where a fundamental matrix alone loses or pollutes them.  --two_view_geometries writes one
line per verified pair: name0 name1 config num_inliers_E num_inliers_F num_inliers_H num_kept (num_inliers_E is -1 without intrinsics).

--guided_matching (with any --model) takes the opposite step after the estimation: every verified pair's descriptors, read
from the feature store, are matched again with only those candidates allowed that agree with the pair's model within --max_error
(two_view.guided_match_pairs: E through F from focal lengths and principal points, F, or H, whichever mask the pair kept), under the
rule --guided_conf names (a key of match_features.confs, default NNM).  matches0 and matching_scores0 of the output then hold the
guided result, in the input datasets' types and shapes; a pair without a model keeps all -1.  `reconstruction
--skip_geometric_verification` reads that store as it is."""
import argparse
import logging
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from . import colmap_io, feature_io, parsers, two_view
from .match_features import confs as match_confs, names_to_pair


def read_cameras(reference_sfm_model=None, intrinsics=()):
    """image name -> camera dict, from a COLMAP model and / or lists with intrinsics (a list entry wins)."""
    out = {}
    if reference_sfm_model is not None:
        cameras = colmap_io.read_cameras_binary(Path(reference_sfm_model) / "cameras.bin")
        for im in colmap_io.read_images_binary(Path(reference_sfm_model) / "images.bin").values():
            out[im.name] = cameras[im.camera_id]
    for lst in intrinsics or ():
        out.update(dict(parsers.query_cameras(lst)))
    if not out:
        raise ValueError("no intrinsics: give --reference_sfm_model or --intrinsics")
    return out


def _write_group(store, name, arrays):
    if hasattr(store, "write_group"):
        store.write_group(name, arrays)
        return
    grp = store.create_group(name)
    for k, v in arrays.items():
        grp.create_dataset(k, data=v)


def main(pairs, features, matches, output, reference_sfm_model=None, intrinsics=(), max_error=4.0,
         min_num_inliers=two_view.DEFAULTS["min_num_inliers"], relative_poses=None, device=0, model="essential", fundamental_matrices=None,
         two_view_geometries=None, guided_matching=False, guided_conf="NNM", **ransac):
    """Returns the per-pair result dicts of two_view.verify_pairs_two_view (model "essential"), two_view.verify_pairs_fundamental
    (model "fundamental", no intrinsics) or two_view.verify_pairs_geometry (model "geometry", with or without intrinsics), keyed by
    (name0, name1)."""
    if model not in ("essential", "fundamental", "geometry"):
        raise ValueError(f"unknown model {model!r}")
    if model != "essential" and relative_poses is not None:
        raise ValueError("--relative_poses needs --model essential: a fundamental matrix has no pose")
    if model != "fundamental" and fundamental_matrices is not None:
        raise ValueError("--fundamental_matrices needs --model fundamental")
    if model != "geometry" and two_view_geometries is not None:
        raise ValueError("--two_view_geometries needs --model geometry")
    if guided_conf not in match_confs:
        raise ValueError(f"unknown --guided_conf {guided_conf!r} (one of {', '.join(match_confs)})")
    name_cam = None
    if model == "essential" or (model == "geometry" and (reference_sfm_model is not None or intrinsics)):
        name_cam = read_cameras(reference_sfm_model, intrinsics)
    with open(str(pairs), "r") as f:
        listed = [p.split() for p in f.readlines() if p.strip()]
    ids = {}
    todo, seen = [], set()
    feats = feature_io.open_store(features, "r")
    src = feature_io.open_store(matches, "r")
    try:
        for name0, name1 in listed:
            if (name_cam is not None and (name0 not in name_cam or name1 not in name_cam)) or (name0, name1) in seen:
                continue
            pair = names_to_pair(name0, name1)
            if pair not in src:
                raise ValueError(f"Could not find pair {(name0, name1)} in {matches}")
            seen |= {(name0, name1), (name1, name0)}
            for n in (name0, name1):
                ids.setdefault(n, len(ids))
            todo.append((name0, name1, pair))
        keypoints = {i: np.asarray(feats[n]["keypoints"].__array__(), dtype=np.float32).reshape(-1, 2)[:, :2] for n, i in ids.items()}
        groups = {pair: {k: np.asarray(src[pair][k].__array__()) for k in src[pair].keys()} for _, _, pair in todo}
        descriptors = None
        if guided_matching:     # stored [128, n] (match_features reads them so)
            descriptors = {i: np.ascontiguousarray(np.asarray(feats[n]["descriptors"].__array__(), dtype=np.float32).T) for n, i in ids.items()}
    finally:
        feats.close()
        src.close()
    pair_matches = []
    for name0, name1, pair in todo:
        m0 = groups[pair]["matches0"].reshape(-1).astype(np.int64)
        pair_matches.append((ids[name0], ids[name1], np.stack([np.arange(len(m0)), m0], 1)))
    logging.info("Verifying %d pairs over %d images...", len(todo), len(ids))
    images = cameras = None
    if name_cam is not None:
        images = {i: SimpleNamespace(camera_id=i, name=n) for n, i in ids.items()}
        cameras = {i: name_cam[n] for n, i in ids.items()}
    if model == "fundamental":
        m, off, _, results = two_view.verify_pairs_fundamental(keypoints, pair_matches, max_error, min_num_inliers, device, **ransac)
    elif model == "geometry":
        m, off, _, results = two_view.verify_pairs_geometry(keypoints, pair_matches, cameras, images, max_error, min_num_inliers, device=device,
                                                            **ransac)
    else:
        m, off, _, results = two_view.verify_pairs_two_view(cameras, images, keypoints, pair_matches, max_error, min_num_inliers, device, **ransac)
    if guided_matching:
        logging.info("Matching %d pairs again under their models (%s)...", len(todo), guided_conf)
        gm, goff, _, gs = two_view.guided_match_pairs(keypoints, descriptors, pair_matches, results, max_error, match_confs[guided_conf], cameras,
                                                      images, device)
    dst = feature_io.open_store(output, "w")
    try:
        for p, (_, _, pair) in enumerate(todo):
            g = dict(groups[pair])
            if guided_matching:
                g["matches0"] = gm[goff[p]:goff[p + 1], 1].astype(g["matches0"].dtype).reshape(g["matches0"].shape)
                if "matching_scores0" in g:
                    g["matching_scores0"] = gs[goff[p]:goff[p + 1]].astype(g["matching_scores0"].dtype).reshape(g["matching_scores0"].shape)
            else:
                kept = m[off[p]:off[p + 1], 1]
                g["matches0"] = np.where(kept >= 0, g["matches0"].reshape(-1), -1).astype(g["matches0"].dtype).reshape(g["matches0"].shape)
            _write_group(dst, pair, g)
    finally:
        dst.close()
    if relative_poses is not None:
        with open(str(relative_poses), "w") as f:
            for (name0, name1, _), r in zip(todo, results):
                vals = [*r["qvec"], *r["tvec"], r["tri_angle_deg"]]
                f.write(f"{name0} {name1} {int(r['success'])} {r['num_inliers']} " + " ".join(f"{v:.17g}" for v in vals) + "\n")
    if fundamental_matrices is not None:
        with open(str(fundamental_matrices), "w") as f:
            for (name0, name1, _), r in zip(todo, results):
                f.write(f"{name0} {name1} {int(r['success'])} {r['num_inliers']} " + " ".join(f"{v:.17g}" for v in r["F"].reshape(-1)) + "\n")
    if two_view_geometries is not None:
        with open(str(two_view_geometries), "w") as f:
            for (name0, name1, _), r in zip(todo, results):
                nE = r["E"]["num_inliers"] if r["E"] is not None else -1
                f.write(f"{name0} {name1} {r['config']} {nE} {r['F']['num_inliers']} {r['H']['num_inliers']} {r['num_inliers']}\n")
    return {(n0, n1): r for (n0, n1, _), r in zip(todo, results)}


def parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--pairs", type=Path, required=True)
    p.add_argument("--features", type=Path, required=True)
    p.add_argument("--matches", type=Path, required=True)
    p.add_argument("--output", type=Path, required=True)
    p.add_argument("--reference_sfm_model", type=Path)
    p.add_argument("--intrinsics", type=Path, nargs="+", default=[])
    p.add_argument("--max_error", type=float, default=4.0)
    p.add_argument("--min_num_inliers", type=int, default=two_view.DEFAULTS["min_num_inliers"])
    p.add_argument("--relative_poses", type=Path)
    p.add_argument("--model", choices=("essential", "fundamental", "geometry"), default="essential")
    p.add_argument("--fundamental_matrices", type=Path)
    p.add_argument("--two_view_geometries", type=Path)
    p.add_argument("--guided_matching", action="store_true")
    p.add_argument("--guided_conf", type=str, default="NNM", choices=list(match_confs))
    return p


if __name__ == "__main__":
    args = parser().parse_args()
    if args.model == "essential" and args.reference_sfm_model is None and not args.intrinsics:
        parser().error("one of --reference_sfm_model and --intrinsics is required")
    if args.model != "essential" and args.relative_poses is not None:
        parser().error("--relative_poses needs --model essential")
    if args.model != "fundamental" and args.fundamental_matrices is not None:
        parser().error("--fundamental_matrices needs --model fundamental")
    if args.model != "geometry" and args.two_view_geometries is not None:
        parser().error("--two_view_geometries needs --model geometry")
    logging.basicConfig(level=logging.INFO)
    main(**args.__dict__)
