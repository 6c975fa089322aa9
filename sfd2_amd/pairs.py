"""Image-pair selection on the device: the stages of hloc/pairs_from_retrieval.py, pairs_from_covisibility.py and
pairs_from_poses.py as functions on arrays (include/sfd2_hip.h, "pair selection").  All three keep the k best candidates of a row
under one total order -- the better score first, then the smaller candidate index -- so a result depends on the inputs alone.
Nothing here computes on the CPU: without a GPU the stages raise."""
import numpy as np

try:        # torch's HIP runtime first (see sfd2_amd/jpeg.py)
    import torch
except Exception:  # pragma: no cover
    torch = None

from . import _lib

MAX_K = _lib.PAIRS_MAX_K                 # retrieval and covisibility
POSES_MAX_K = _lib.PAIRS_POSES_MAX_K     # poses: its lists are per image, not per 64-row strip


def _check_k(k, most=MAX_K):
    k = int(k)
    if not 1 <= k <= most:
        raise ValueError(f"k must lie in [1, {most}], got {k}")
    return k


def _f32_matrix(a, what):
    """(array or tensor, on_device): contiguous fp32 [n, d]; a torch tensor on the GPU stays there."""
    if torch is not None and isinstance(a, torch.Tensor):
        if a.is_cuda:
            a = a.detach().to(torch.float32).contiguous()
            if a.dim() != 2:
                raise ValueError(f"{what} must be [n, d]")
            return a, 1
        a = a.detach().numpy()
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError(f"{what} must be [n, d]")
    return a, 0


def retrieval_topk(query_desc, db_desc, k, splits=0, device=0):
    """query_desc [nq, d], db_desc [nd, d] (numpy, or torch on the host or on the GPU).  Returns (idx int32 [nq, k], sim float32
    [nq, k]): per query the k db rows of largest fp32 dot product, best first, ties by the smaller db row.  splits: the number of
    workgroups the db range of a query strip is divided over (0: chosen by the library); the result does not depend on it."""
    k = _check_k(k)
    q, q_dev = _f32_matrix(query_desc, "query_desc")
    db, db_dev = _f32_matrix(db_desc, "db_desc")
    if q_dev != db_dev:                                   # one flag for both: bring the host one over
        if q_dev:
            db = torch.from_numpy(db).to(q.device)
        else:
            q = torch.from_numpy(q).to(db.device)
        q_dev = db_dev = 1
    if q_dev:
        device = q.device.index or 0
        torch.cuda.synchronize(q.device)                  # the library runs on its own stream
    if q.shape[1] != db.shape[1] or q.shape[0] < 1 or db.shape[0] < 1 or q.shape[1] < 1:
        raise ValueError(f"query_desc {tuple(q.shape)} and db_desc {tuple(db.shape)} do not fit together")
    if k > db.shape[0]:
        raise ValueError(f"k = {k} is larger than the {db.shape[0]} db rows")
    if not 0 <= int(splits) <= 255:
        raise ValueError("splits must lie in [0, 255]")
    nq, nd, d = int(q.shape[0]), int(db.shape[0]), int(q.shape[1])
    idx = np.empty((nq, k), dtype=np.int32)
    sim = np.empty((nq, k), dtype=np.float32)
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_pairs_retrieval(ctx.h, _lib.ptr(q), nq, _lib.ptr(db), nd, d, k, q_dev, idx.ctypes.data, sim.ctypes.data,
                                            _lib.pairs_splits(splits)))
    return idx, sim


def covisibility_csr(images, points3D):
    """The two CSRs of sfd2_pairs_covisibility from the dicts colmap_io.read_model returns.  Image order is dict order, as the reference
    iterates; point ids go through a sorted table, as covis.MapIndex does.  Returns (image ids, obs_offsets int64, obs_point int32,
    track_offsets int64, track_image int32); duplicates on either side are kept."""
    ids = list(images.keys())
    index = {iid: i for i, iid in enumerate(ids)}
    pids = np.array(sorted(points3D.keys()), dtype=np.int64)
    obs, obs_off = [], np.zeros(len(ids) + 1, dtype=np.int64)
    for i, iid in enumerate(ids):
        p = np.asarray(images[iid].point3D_ids, dtype=np.int64).reshape(-1)
        p = p[p != -1]
        rows = np.searchsorted(pids, p)
        if len(p) and (len(pids) == 0 or (rows >= len(pids)).any() or (pids[np.minimum(rows, len(pids) - 1)] != p).any()):
            raise ValueError(f"image {iid} observes a point the model does not have")
        obs.append(rows.astype(np.int32))
        obs_off[i + 1] = obs_off[i] + len(rows)
    trk, trk_off = [], np.zeros(len(pids) + 1, dtype=np.int64)
    for r, pid in enumerate(pids):
        t = points3D[int(pid)].image_ids
        try:
            trk.append(np.fromiter((index[int(x)] for x in t), dtype=np.int32, count=len(t)))
        except KeyError as e:
            raise ValueError(f"point {pid} is seen by image {e.args[0]}, which the model does not have") from None
        trk_off[r + 1] = trk_off[r] + len(t)
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, np.int32)  # noqa: E731
    return ids, obs_off, cat(obs).astype(np.int32), trk_off, cat(trk).astype(np.int32)


def covisibility_topk_csr(obs_offsets, obs_point, track_offsets, track_image, k, global_counters=False, device=0):
    """The array level of covisibility_topk.  Returns (idx int32 [n, k], count int32 [n, k], n_found int32 [n]); slots beyond
    n_found hold (-1, 0).  global_counters forces the counters into global memory (the path of maps too large for LDS)."""
    k = _check_k(k)
    oo = np.ascontiguousarray(obs_offsets, dtype=np.int64)
    op = np.ascontiguousarray(obs_point, dtype=np.int32)
    to = np.ascontiguousarray(track_offsets, dtype=np.int64)
    ti = np.ascontiguousarray(track_image, dtype=np.int32)
    n, npts = len(oo) - 1, len(to) - 1
    if n < 1 or npts < 0 or oo[-1] != len(op) or to[-1] != len(ti):
        raise ValueError("offsets and arrays do not fit together")
    idx = np.empty((n, k), dtype=np.int32)
    cnt = np.empty((n, k), dtype=np.int32)
    nf = np.empty(n, dtype=np.int32)
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_pairs_covisibility(ctx.h, oo.ctypes.data, op.ctypes.data if len(op) else None, n, to.ctypes.data,
                                               ti.ctypes.data if len(ti) else None, npts, k, idx.ctypes.data, cnt.ctypes.data, nf.ctypes.data,
                                               _lib.PAIRS_FLAG_GLOBAL_COUNTERS if global_counters else 0))
    return idx, cnt, nf


def covisibility_topk(images, points3D, k, global_counters=False, device=0):
    """Per image the k images that share the most 3D points with it (pairs_from_covisibility.py:16-45).  Returns (image ids in dict
    order, idx [n, k] = positions in that list, count [n, k], n_found [n])."""
    ids, oo, op, to, ti = covisibility_csr(images, points3D)
    if not ids:
        return ids, np.zeros((0, int(k)), np.int32), np.zeros((0, int(k)), np.int32), np.zeros(0, np.int32)
    return (ids,) + covisibility_topk_csr(oo, op, to, ti, k, global_counters, device)


def poses_topk_arrays(qvec, tvec, k, rotation_threshold=30, true_centres=False, device=0):
    """qvec [n, 4] (w x y z), tvec [n, 3], world to camera.  Returns (idx int32 [n, k], dist float64 [n, k], n_found int32 [n]): per
    image the k nearest others whose relative rotation is below rotation_threshold degrees, nearest first; slots beyond n_found hold
    (-1, inf).  The position is the reference's -R t (pairs_from_poses.py:25-26) unless true_centres asks for -R^T t."""
    k = _check_k(k, POSES_MAX_K)
    q = np.ascontiguousarray(qvec, dtype=np.float64).reshape(-1, 4)
    t = np.ascontiguousarray(tvec, dtype=np.float64).reshape(-1, 3)
    if len(q) != len(t) or len(q) < 1:
        raise ValueError("qvec and tvec do not fit together")
    n = len(q)
    idx = np.empty((n, k), dtype=np.int32)
    dist = np.empty((n, k), dtype=np.float64)
    nf = np.empty(n, dtype=np.int32)
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_pairs_poses(ctx.h, q.ctypes.data, t.ctypes.data, n, k, float(rotation_threshold), idx.ctypes.data, dist.ctypes.data,
                                        nf.ctypes.data, _lib.PAIRS_FLAG_CENTRES if true_centres else 0))
    return idx, dist, nf


def poses_topk(images, k, rotation_threshold=30, true_centres=False, device=0):
    """images: the dict colmap_io.read_images_binary returns.  Returns (image ids in dict order, idx, dist, n_found) of
    poses_topk_arrays.  Where the reference raises for k >= n a row simply has at most n - 1 entries."""
    ids = list(images.keys())
    if not ids:
        return ids, np.zeros((0, int(k)), np.int32), np.zeros((0, int(k))), np.zeros(0, np.int32)
    q = np.array([np.asarray(images[i].qvec, dtype=np.float64) for i in ids])
    t = np.array([np.asarray(images[i].tvec, dtype=np.float64) for i in ids])
    return (ids,) + poses_topk_arrays(q, t, k, rotation_threshold, true_centres, device)


def name_pairs(names0, names1, idx, n_found=None):
    """[(names0[i], names1[idx[i, j]])] row by row, the first n_found[i] entries of a row (all of it without n_found)."""
    out = []
    for i, row in enumerate(np.asarray(idx)):
        m = len(row) if n_found is None else int(n_found[i])
        out.extend((names0[i], names1[int(j)]) for j in row[:m])
    return out


def write_pairs(path, pairs):
    """The reference's pairs file: 'name0 name1' per line, joined by newlines, no trailing newline."""
    with open(str(path), "w") as f:
        f.write("\n".join(" ".join([i, j]) for i, j in pairs))
