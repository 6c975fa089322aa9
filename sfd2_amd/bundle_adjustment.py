"""Bundle adjustment on the device (include/sfd2_hip.h sfd2_bundle_adjust): Levenberg-Marquardt over camera
poses and 3D points, the points eliminated, the reduced camera system solved by matrix-free preconditioned conjugate gradients.
The joint refinement `colmap bundle_adjuster` does for a model, reduced to what is built: intrinsics stay fixed, the loss is trivial
or Cauchy.

  adjust          the C call on numpy arrays.
  bundle_adjust   on colmap_io records: returns new images, new points3D (error = mean reprojection error of the point) and the report.
  main / command  python -m sfd2_amd.bundle_adjustment --input_path M --output_path O [--max_num_iterations N]
                  [--loss trivial|cauchy] [--loss_scale S] [--constant_images FILE]

Without --constant_images the two registered images with the smallest ids keep their poses.  COLMAP fixes the first image's pose and
one coordinate of the second's translation; fixing both poses completely is this project's deviation (it removes the same seven
degrees of freedom and a little more).  Nothing here computes on the CPU: without a GPU the calls raise."""
import argparse
import ctypes
import logging
from pathlib import Path

import numpy as np

try:        # torch's HIP runtime first (see sfd2_amd/jpeg.py)
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    pass

from . import _lib, colmap_io
from .pose import camera_model
from .triangulation import make_views

DEFAULTS = dict(max_iterations=100, gradient_tolerance=1e-10, function_tolerance=0.0, pcg_tolerance=0.1, pcg_max_iterations=100,
                pcg_batch=0, loss="trivial", loss_scale=1.0, initial_lambda=1e-4)
LOSSES = {"trivial": _lib.BA_LOSS_TRIVIAL, "cauchy": _lib.BA_LOSS_CAUCHY}
STATUS = {_lib.BA_ST_GRADIENT: "gradient_tolerance", _lib.BA_ST_FUNCTION: "function_tolerance", _lib.BA_ST_MAX_ITERATIONS: "max_iterations",
          _lib.BA_ST_LAMBDA: "lambda_overflow", _lib.BA_ST_NONFINITE: "non_finite_cost"}


def _conf(options):
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown options {sorted(unknown)}")
    o = dict(DEFAULTS, **options)
    if o["loss"] not in LOSSES:
        raise ValueError(f"loss {o['loss']!r} is not supported (one of {', '.join(LOSSES)})")
    conf = _lib.BaConf()
    conf.max_iterations, conf.pcg_max_iterations = int(o["max_iterations"]), int(o["pcg_max_iterations"])
    conf.loss, conf.pcg_batch = LOSSES[o["loss"]], int(o["pcg_batch"])
    conf.gradient_tolerance, conf.function_tolerance = float(o["gradient_tolerance"]), float(o["function_tolerance"])
    conf.pcg_tolerance, conf.loss_scale, conf.initial_lambda = float(o["pcg_tolerance"]), float(o["loss_scale"]), float(o["initial_lambda"])
    return conf


def adjust(views, n_views, view_constant, xyz, point_constant, point_offsets, obs_view, obs_xy, flags=0, device=0, **options):
    """views: triangulation.make_views()'s array (poses IN/OUT); view_constant [n_views], point_constant [n_points]: non-zero = fixed;
    xyz [n_points, 3]; point p holds the observations point_offsets[p] .. point_offsets[p + 1] of (obs_view, obs_xy in pixels as
    given).  options: DEFAULTS.  Returns (xyz [n_points, 3], obs_error [n_obs], report dict); the views array holds the new poses."""
    conf = _conf(options)
    n_views = int(n_views)
    vc = np.ascontiguousarray(np.asarray(view_constant).reshape(-1) != 0, dtype=np.uint8)
    pts = np.array(xyz, dtype=np.float64).reshape(-1, 3)
    pc = np.ascontiguousarray(np.asarray(point_constant).reshape(-1) != 0, dtype=np.uint8)
    off = np.ascontiguousarray(point_offsets, dtype=np.int64).reshape(-1)
    ov = np.ascontiguousarray(obs_view, dtype=np.int32).reshape(-1)
    xy = np.ascontiguousarray(np.asarray(obs_xy, dtype=np.float64).reshape(-1, 2))
    P = len(pts)
    if n_views < 1 or len(vc) != n_views or len(pc) != P or len(off) != P + 1 or len(ov) != len(xy):
        raise ValueError("the view, point, offset and observation arrays do not fit together")
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != len(ov):
        raise ValueError("point_offsets must start at 0, not decrease and end at the number of observations")
    bad = np.nonzero((ov < 0) | (ov >= n_views))[0]
    if len(bad):
        raise ValueError(f"observation {int(bad[0])}: view index out of range")
    bad = np.nonzero(~np.isfinite(pts).all(1))[0]
    if len(bad):
        raise ValueError(f"point {int(bad[0])}: non-finite coordinates")
    bad = np.nonzero(~np.isfinite(xy).all(1))[0]
    if len(bad):
        raise ValueError(f"observation {int(bad[0])}: non-finite coordinates")
    err = np.zeros(len(ov), dtype=np.float64)
    res = _lib.BaResult()
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_bundle_adjust(ctx.h, views, n_views, vc.ctypes.data, pts.ctypes.data, P, pc.ctypes.data, off.ctypes.data, ov.ctypes.data,
                                          xy.ctypes.data, ctypes.byref(conf), ctypes.byref(res), err.ctypes.data, int(flags)))
    report = {"status": STATUS[res.status], "iterations": int(res.iterations), "accepted_steps": int(res.accepted_steps),
              "pcg_iterations": int(res.pcg_iterations), "initial_cost": float(res.initial_cost), "final_cost": float(res.final_cost),
              "gradient_max": float(res.gradient_max), "lambda": float(res.lambda_)}
    return pts, err, report


def pack_model(cameras, images, points3D):
    """The arrays of adjust() from a model: (image ids, views, point ids, xyz, offsets, obs_view, obs_xy).  Only images with at least one
    point3D_ids != -1 entry become views; a point's observations are its track entries in track order, those whose image entry does
    not name the point (or is absent) dropped."""
    ids = sorted(i for i, im in images.items() if (np.asarray(im.point3D_ids) != -1).any())
    for i in ids:
        camera_model(cameras[images[i].camera_id])
    ids, views = make_views(cameras, images, ids)
    index = {iid: k for k, iid in enumerate(ids)}
    pids, xyz, off, ov, xy = [], [], [0], [], []
    for pid in sorted(points3D):
        p = points3D[pid]
        n = 0
        for iid, idx in zip(np.asarray(p.image_ids).tolist(), np.asarray(p.point2D_idxs).tolist()):
            im = images.get(iid)
            if im is None or iid not in index or idx >= len(im.point3D_ids) or int(im.point3D_ids[idx]) != pid:
                continue
            ov.append(index[iid])
            xy.append(np.asarray(im.xys[idx], dtype=np.float64))
            n += 1
        pids.append(pid)
        xyz.append(np.asarray(p.xyz, dtype=np.float64))
        off.append(off[-1] + n)
    return (ids, views, pids, np.array(xyz, dtype=np.float64).reshape(-1, 3), np.array(off, dtype=np.int64), np.array(ov, dtype=np.int32),
            np.array(xy, dtype=np.float64).reshape(-1, 2))


def bundle_adjust(cameras, images, points3D, constant_images=(), constant_points=(), flags=0, device=0, **options):
    """cameras, images, points3D: colmap_io records.  constant_images / constant_points: ids whose pose / position stays.  Returns (new
    images, new points3D with error = the point's mean reprojection error, report).  An image without observations is returned
    unchanged."""
    _conf(options)
    ids, views, pids, xyz, off, ov, xy = pack_model(cameras, images, points3D)
    if not ids:
        raise ValueError("the model has no observations")
    cset, pset = set(int(i) for i in constant_images), set(int(p) for p in constant_points)
    vc = np.array([iid in cset for iid in ids], dtype=np.uint8)
    pc = np.array([pid in pset for pid in pids], dtype=np.uint8)
    new_xyz, err, report = adjust(views, len(ids), vc, xyz, pc, off, ov, xy, flags=flags, device=device, **options)
    out_images = dict(images)
    for k, iid in enumerate(ids):
        im = images[iid]
        out_images[iid] = colmap_io.Image(iid, np.array(views[k].qvec[:], dtype=np.float64), np.array(views[k].tvec[:], dtype=np.float64), im.camera_id,
                                          im.name, im.xys, im.point3D_ids)
    out_points = {}
    for r, pid in enumerate(pids):
        p = points3D[pid]
        e = err[off[r]:off[r + 1]]
        out_points[pid] = colmap_io.Point3D(pid, new_xyz[r].copy(), p.rgb, float(e.mean()) if len(e) else float(p.error), p.image_ids, p.point2D_idxs)
    report["obs_error"] = err
    report["point_offsets"] = off
    report["point_ids"] = pids
    return out_images, out_points, report


def default_constant_images(images):
    """The two registered images with the smallest ids."""
    return sorted(images)[:2]


def read_constant_images(path, images):
    """One image name per line (blank lines and # comments skipped) -> ids; a name the model lacks is an error."""
    by_name = {im.name: i for i, im in images.items()}
    out = []
    with open(str(path), "r") as f:
        for line in f:
            name = line.strip()
            if not name or name.startswith("#"):
                continue
            if name not in by_name:
                raise ValueError(f"constant image {name!r} is not in the model")
            out.append(by_name[name])
    return out


def main(input_path, output_path, max_num_iterations=DEFAULTS["max_iterations"], loss="trivial", loss_scale=1.0, constant_images=None, **options):
    """Reads the model at input_path, adjusts it, writes it to output_path; returns the report."""
    input_path, output_path = Path(input_path), Path(output_path)
    cameras, images, points3D = colmap_io.read_model(input_path)
    const = default_constant_images(images) if constant_images is None else read_constant_images(constant_images, images)
    out_images, out_points, report = bundle_adjust(cameras, images, points3D, constant_images=const, max_iterations=max_num_iterations, loss=loss,
                                                   loss_scale=loss_scale, **options)
    output_path.mkdir(parents=True, exist_ok=True)
    colmap_io.write_model(cameras, out_images, out_points, output_path)
    logging.info("Bundle adjustment: %s", {k: v for k, v in report.items() if not isinstance(v, (np.ndarray, list))})
    return report


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--input_path", type=Path, required=True)
    ap.add_argument("--output_path", type=Path, required=True)
    ap.add_argument("--max_num_iterations", type=int, default=DEFAULTS["max_iterations"])
    ap.add_argument("--loss", choices=sorted(LOSSES), default="trivial")
    ap.add_argument("--loss_scale", type=float, default=1.0)
    ap.add_argument("--constant_images", type=Path, default=None)
    return ap


if __name__ == "__main__":
    main(**parser().parse_args().__dict__)
