"""Bundle adjustment on the device (include/sfd2_hip.h sfd2_bundle_adjust): Levenberg-Marquardt over camera
poses and 3D points, the points eliminated, the reduced camera system solved by matrix-free preconditioned conjugate gradients
(solver="pcg", the default) or formed as a dense matrix and solved by a Cholesky factorisation on the device (solver="dense", DESIGN.md
section 21: up to 2048 views, constant intrinsics only).
The joint refinement `colmap bundle_adjuster` does for a model, reduced to what is built: the loss is trivial or Cauchy; intrinsics
stay fixed unless one of the refine options is set (sfd2_bundle_adjust_cameras).

  adjust          the C call on numpy arrays.
  adjust_cameras  the C call with camera intrinsics among the unknowns, on numpy arrays.
  spd_solve       A x = b for a symmetric positive definite A by the dense solver's factor and solve kernels.
  bundle_adjust   on colmap_io records: returns new images, new points3D (error = mean reprojection error of the point) and the report;
                  with a refine option also the new cameras, first.
  main / command  python -m sfd2_amd.bundle_adjustment --input_path M --output_path O [--max_num_iterations N]
                  [--loss trivial|cauchy] [--loss_scale S] [--constant_images FILE] [--solver pcg|dense]
                  [--refine_focal_length 0|1] [--refine_principal_point 0|1] [--refine_extra_params 0|1]

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
                pcg_batch=0, loss="trivial", loss_scale=1.0, initial_lambda=1e-4, solver="pcg")
SOLVERS = {"pcg": _lib.BA_SOLVER_PCG, "dense": _lib.BA_SOLVER_DENSE}
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
    if o["solver"] not in SOLVERS:
        raise ValueError(f"solver {o['solver']!r} is not supported (one of {', '.join(SOLVERS)})")
    conf = _lib.BaConf()
    conf.solver = SOLVERS[o["solver"]]
    conf.max_iterations, conf.pcg_max_iterations = int(o["max_iterations"]), int(o["pcg_max_iterations"])
    conf.loss, conf.pcg_batch = LOSSES[o["loss"]], int(o["pcg_batch"])
    conf.gradient_tolerance, conf.function_tolerance = float(o["gradient_tolerance"]), float(o["function_tolerance"])
    conf.pcg_tolerance, conf.loss_scale, conf.initial_lambda = float(o["pcg_tolerance"]), float(o["loss_scale"]), float(o["initial_lambda"])
    return conf


def refine_mask(refine_focal_length=False, refine_principal_point=False, refine_extra_params=False):
    """The SFD2_BA_REFINE_* bits of the three options."""
    return ((_lib.BA_REFINE_FOCAL if refine_focal_length else 0) | (_lib.BA_REFINE_PRINCIPAL if refine_principal_point else 0) |
            (_lib.BA_REFINE_EXTRA if refine_extra_params else 0))


def adjust(views, n_views, view_constant, xyz, point_constant, point_offsets, obs_view, obs_xy, flags=0, device=0, **options):
    """views: triangulation.make_views()'s array (poses IN/OUT); view_constant [n_views], point_constant [n_points]: non-zero = fixed;
    xyz [n_points, 3]; point p holds the observations point_offsets[p] .. point_offsets[p + 1] of (obs_view, obs_xy in pixels as
    given).  options: DEFAULTS.  Returns (xyz [n_points, 3], obs_error [n_obs], report dict); the views array holds the new poses."""
    return _adjust(None, views, n_views, view_constant, xyz, point_constant, point_offsets, obs_view, obs_xy, flags, device, options)


def adjust_cameras(cam_models, cam_params, cam_refine, view_camera, views, n_views, view_constant, xyz, point_constant, point_offsets, obs_view, obs_xy,
                   flags=0, device=0, **options):
    """adjust() with camera intrinsics among the unknowns.  cam_models [n_cameras] (model ids), cam_params [n_cameras, 8] (COLMAP order,
    zero padded), cam_refine [n_cameras] (SFD2_BA_REFINE_* bits, 0 = constant), view_camera [n_views] (index into the cameras).  The
    views' own model / params words are not read; they leave with their camera's new values.  Returns (cam_params [n_cameras, 8], xyz,
    obs_error, report)."""
    if options.get("solver", DEFAULTS["solver"]) == "dense":
        raise ValueError('solver "dense" does not take camera intrinsics among the unknowns (DESIGN.md section 21): use solver "pcg" with a refine option')
    models = np.ascontiguousarray(cam_models, dtype=np.int32).reshape(-1)
    params = np.array(cam_params, dtype=np.float64).reshape(-1, 8)
    refine = np.ascontiguousarray(cam_refine, dtype=np.int32).reshape(-1)
    vcam = np.ascontiguousarray(view_camera, dtype=np.int32).reshape(-1)
    n = len(models)
    if n < 1 or len(params) != n or len(refine) != n or len(vcam) != int(n_views):
        raise ValueError("the camera arrays and view_camera do not fit together")
    bad = np.nonzero((vcam < 0) | (vcam >= n))[0]
    if len(bad):
        raise ValueError(f"view {int(bad[0])}: camera index out of range")
    bad = np.nonzero(refine & ~(_lib.BA_REFINE_FOCAL | _lib.BA_REFINE_PRINCIPAL | _lib.BA_REFINE_EXTRA))[0]
    if len(bad):
        raise ValueError(f"camera {int(bad[0])}: unknown refine bits")
    bad = np.nonzero(~np.isfinite(params).all(1))[0]
    if len(bad):
        raise ValueError(f"camera {int(bad[0])}: non-finite parameters")
    cams = (_lib.BaCamera * n)()
    for i in range(n):
        cams[i].model, cams[i].refine = int(models[i]), int(refine[i])
        cams[i].params[:] = params[i].tolist()
    pts, err, report = _adjust((cams, n, vcam), views, n_views, view_constant, xyz, point_constant, point_offsets, obs_view, obs_xy, flags, device, options)
    return np.array([list(c.params) for c in cams], dtype=np.float64), pts, err, report


def _adjust(cameras, views, n_views, view_constant, xyz, point_constant, point_offsets, obs_view, obs_xy, flags, device, options):
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
    rest = (views, n_views, vc.ctypes.data, pts.ctypes.data, P, pc.ctypes.data, off.ctypes.data, ov.ctypes.data, xy.ctypes.data, ctypes.byref(conf),
            ctypes.byref(res), err.ctypes.data, int(flags))
    if cameras is None:
        _lib.check(ctx.lib.sfd2_bundle_adjust(ctx.h, *rest))
    else:
        _lib.check(ctx.lib.sfd2_bundle_adjust_cameras(ctx.h, cameras[0], cameras[1], cameras[2].ctypes.data, *rest))
    report = {"status": STATUS[res.status], "iterations": int(res.iterations), "accepted_steps": int(res.accepted_steps),
              "pcg_iterations": int(res.pcg_iterations), "initial_cost": float(res.initial_cost), "final_cost": float(res.final_cost),
              "gradient_max": float(res.gradient_max), "lambda": float(res.lambda_),
              "solver": dict((v, k) for k, v in SOLVERS.items())[conf.solver]}
    return pts, err, report


def spd_solve(A, b, device=0):
    """A x = b for a symmetric positive definite A [n, n] (only its lower triangle is read) and b [n], fp64, by a blocked Cholesky
    factorisation on the device (sfd2_spd_solve).  Returns (x, info): info = 0 and the solution, or info = k + 1 for the first pivot
    k that is not positive, with x = None.  Non-finite input raises."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or len(b) != A.shape[0] or len(b) < 1:
        raise ValueError("A must be [n, n] and b [n], n >= 1")
    x = np.zeros(len(b), dtype=np.float64)
    info = ctypes.c_int32(0)
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_spd_solve(ctx.h, A.ctypes.data, len(b), b.ctypes.data, x.ctypes.data, ctypes.byref(info)))
    return (x if info.value == 0 else None), int(info.value)


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


def bundle_adjust(cameras, images, points3D, constant_images=(), constant_points=(), flags=0, device=0, refine_focal_length=False,
                  refine_principal_point=False, refine_extra_params=False, constant_cameras=(), **options):
    """cameras, images, points3D: colmap_io records.  constant_images / constant_points: ids whose pose / position stays.  Returns (new
    images, new points3D with error = the point's mean reprojection error, report).  An image without observations is returned
    unchanged.  With a refine option set the intrinsics of every camera id not in constant_cameras are refined too (one camera id is
    one camera: images that share it share its parameters), and the return is (new cameras, new images, new points3D, report)."""
    _conf(options)
    mask = refine_mask(refine_focal_length, refine_principal_point, refine_extra_params)
    if mask and options.get("solver", DEFAULTS["solver"]) == "dense":
        raise ValueError('solver "dense" does not take camera intrinsics among the unknowns (DESIGN.md section 21): use solver "pcg" with a refine option')
    ids, views, pids, xyz, off, ov, xy = pack_model(cameras, images, points3D)
    if not ids:
        raise ValueError("the model has no observations")
    cset, pset = set(int(i) for i in constant_images), set(int(p) for p in constant_points)
    vc = np.array([iid in cset for iid in ids], dtype=np.uint8)
    pc = np.array([pid in pset for pid in pids], dtype=np.uint8)
    if mask:
        held = set(int(c) for c in constant_cameras)
        cam_ids = sorted(set(images[iid].camera_id for iid in ids))
        cam_index = {cid: k for k, cid in enumerate(cam_ids)}
        packed = [camera_model(cameras[cid]) for cid in cam_ids]
        cam_params, new_xyz, err, report = adjust_cameras([m for m, _ in packed], [p for _, p in packed], [0 if cid in held else mask for cid in cam_ids],
                                                          [cam_index[images[iid].camera_id] for iid in ids], views, len(ids), vc, xyz, pc, off, ov, xy,
                                                          flags=flags, device=device, **options)
        out_cameras = dict(cameras)
        for k, cid in enumerate(cam_ids):
            cam = cameras[cid]
            out_cameras[cid] = colmap_io.Camera(cam["id"], cam["model"], cam["width"], cam["height"], cam_params[k][:len(cam["params"])])
    else:
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
    if mask:
        return out_cameras, out_images, out_points, report
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


def main(input_path, output_path, max_num_iterations=DEFAULTS["max_iterations"], loss="trivial", loss_scale=1.0, constant_images=None,
         refine_focal_length=0, refine_principal_point=0, refine_extra_params=0, solver=DEFAULTS["solver"], **options):
    """Reads the model at input_path, adjusts it, writes it to output_path (with a refine option: the refined cameras too); returns the
    report."""
    input_path, output_path = Path(input_path), Path(output_path)
    cameras, images, points3D = colmap_io.read_model(input_path)
    const = default_constant_images(images) if constant_images is None else read_constant_images(constant_images, images)
    out = bundle_adjust(cameras, images, points3D, constant_images=const, max_iterations=max_num_iterations, loss=loss, loss_scale=loss_scale,
                        refine_focal_length=bool(refine_focal_length), refine_principal_point=bool(refine_principal_point),
                        refine_extra_params=bool(refine_extra_params), **({} if solver == DEFAULTS["solver"] else {"solver": solver}), **options)
    if len(out) == 4:
        cameras = out[0]
    out_images, out_points, report = out[-3:]
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
    ap.add_argument("--refine_focal_length", type=int, choices=(0, 1), default=0)
    ap.add_argument("--refine_principal_point", type=int, choices=(0, 1), default=0)
    ap.add_argument("--refine_extra_params", type=int, choices=(0, 1), default=0)
    ap.add_argument("--solver", choices=sorted(SOLVERS), default=DEFAULTS["solver"])
    return ap


if __name__ == "__main__":
    main(**parser().parse_args().__dict__)
