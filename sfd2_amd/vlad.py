"""Global descriptors on the device: VLAD over the 128-d local descriptors (include/sfd2_hip.h, "global descriptors") as functions on
arrays -- nearest-centroid assignment, residual aggregation with its normalisation, and the k-means (Lloyd) vocabulary.  The
project's own choice, not a port: the reference retrieves with NetVLAD descriptors from another project.
The arithmetic is fixed by the header, so a row's or an image's result depends on that row or image and the centroids alone.
Nothing here computes on the CPU: without a GPU the stages raise."""
import ctypes

import numpy as np

try:        # torch's HIP runtime first (see sfd2_amd/jpeg.py)
    import torch
except Exception:  # pragma: no cover
    torch = None

from . import _lib

DIM = _lib.VLAD_DIM
MAX_K = _lib.VLAD_MAX_K
CHUNK = _lib.VLAD_CHUNK
NORMS = {"intra": _lib.VLAD_NORM_INTRA, "ssr": _lib.VLAD_NORM_SSR, "none": _lib.VLAD_NORM_NONE}


def _rows(a, what):
    """(array or tensor, on_device): contiguous fp32 [n, 128]; a torch tensor on the GPU stays there."""
    dev = 0
    if torch is not None and isinstance(a, torch.Tensor):
        if a.is_cuda:
            a, dev = a.detach().to(torch.float32).contiguous(), 1
        else:
            a = a.detach().numpy()
    if not dev:
        a = np.ascontiguousarray(a, dtype=np.float32)
    if len(a.shape) != 2 or a.shape[1] != DIM:
        raise ValueError(f"{what} must be [n, {DIM}], got {tuple(a.shape)}")
    return a, dev


def _pair(x, centroids):
    """x and centroids under one inputs_on_device flag: the host one is brought over when the other is on the GPU."""
    x, x_dev = _rows(x, "x")
    c, c_dev = _rows(centroids, "centroids")
    device = 0
    if x_dev != c_dev:
        if x_dev:
            c = torch.from_numpy(c).to(x.device)
        else:
            x = torch.from_numpy(x).to(c.device)
        x_dev = 1
    if x_dev:
        device = x.device.index or 0
        torch.cuda.synchronize(x.device)                  # the library runs on its own stream
    return x, c, x_dev, device


def assign(x, centroids, device=0):
    """x [n, 128], centroids [K, 128] (numpy, or torch on the host or on the GPU).  Returns (assign int32 [n], score float32 [n]): per
    row the centroid of largest s = x . c - 0.5 |c|^2 (the nearest one), a tie to the smaller index, and that s."""
    x, c, on_dev, dev = _pair(x, centroids)
    n, k = int(x.shape[0]), int(c.shape[0])
    a = np.empty(n, dtype=np.int32)
    s = np.empty(n, dtype=np.float32)
    ctx = _lib.default_context(dev if on_dev else device)
    _lib.check(ctx.lib.sfd2_vlad_assign(ctx.h, _lib.ptr(x), n, _lib.ptr(c), k, on_dev, a.ctypes.data, s.ctypes.data, 0))
    return a, s


def aggregate(x, offsets, centroids, norm="intra", return_assign=False, device=0):
    """Image i owns the rows offsets[i] .. offsets[i + 1] - 1 of x [n, 128].  Returns float32 [n_images, K * 128]: per image the sums
    of (row - its centroid) per centroid, normalised ("intra": each centroid's block, then the vector; "ssr": signed square root, then
    the vector; "none": the vector only).  An image without rows gives zeros."""
    if norm not in NORMS:
        raise ValueError(f"norm must be one of {sorted(NORMS)}, got {norm!r}")
    x, c, on_dev, dev = _pair(x, centroids)
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if len(off) < 1 or off[-1] != x.shape[0]:
        raise ValueError("offsets and x do not fit together")
    n_images, k = len(off) - 1, int(c.shape[0])
    out = np.empty((n_images, max(k, 0) * DIM), dtype=np.float32)
    a = np.empty(int(x.shape[0]), dtype=np.int32) if return_assign else None
    ctx = _lib.default_context(dev if on_dev else device)
    _lib.check(ctx.lib.sfd2_vlad_aggregate(ctx.h, _lib.ptr(x) if x.shape[0] else None, off.ctypes.data, n_images, _lib.ptr(c), k, on_dev,
                                           NORMS[norm], out.ctypes.data, _lib.ptr(a), 0))
    return (out, a) if return_assign else out


def kmeans_from(x, start, max_iters=20, device=0):
    """Lloyd iterations on the device from the start centroids [K, 128].  Returns (centroids float32 [K, 128], counts int64 [K],
    moved int64 [iterations run]): moved[it] is the number of rows that changed centroid in iteration it (all of them in the first);
    the call ends after the first iteration with moved == 0 or after max_iters.  A centroid without rows keeps its value."""
    x, x_dev = _rows(x, "x")
    c = np.array(start.detach().cpu().numpy() if torch is not None and isinstance(start, torch.Tensor) else start, dtype=np.float32, order="C")
    if c.ndim != 2 or c.shape[1] != DIM:
        raise ValueError(f"start must be [K, {DIM}], got {tuple(c.shape)}")
    if x_dev:
        device = x.device.index or 0
        torch.cuda.synchronize(x.device)
    k = int(c.shape[0])
    counts = np.zeros(max(k, 0), dtype=np.int64)
    moved = np.zeros(max(int(max_iters), 0), dtype=np.int64)
    run = ctypes.c_int(0)
    ctx = _lib.default_context(device)
    _lib.check(ctx.lib.sfd2_vlad_kmeans(ctx.h, _lib.ptr(x), int(x.shape[0]), k, int(max_iters), x_dev, c.ctypes.data, counts.ctypes.data,
                                        moved.ctypes.data, ctypes.byref(run), 0))
    return c, counts, moved[:run.value]


def kmeans(x, k, max_iters=20, seed=0, device=0):
    """kmeans_from with the rows np.random.RandomState(seed).permutation(n)[:k] as the start."""
    x, _ = _rows(x, "x")
    n, k = int(x.shape[0]), int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must lie in [1, {MAX_K}], got {k}")
    if n < k:
        raise ValueError(f"{n} rows cannot start {k} centroids")
    rows = np.random.RandomState(seed).permutation(n)[:k]
    start = x[rows] if isinstance(x, np.ndarray) else x[torch.from_numpy(rows).to(x.device)].cpu().numpy()
    return kmeans_from(x, start, max_iters, device)


def _descriptors(group):
    """An image's descriptors as float32 [N, 128] from the store's float64 [128, N]."""
    d = np.asarray(group["descriptors"].__array__())
    if d.ndim != 2 or d.shape[0] != DIM:
        raise ValueError(f"descriptors must be [{DIM}, N], got {d.shape}")
    return np.ascontiguousarray(d.T, dtype=np.float32)


def train_vocabulary(store, names, k=64, max_train=1 << 20, max_iters=20, seed=0, device=0):
    """The k-means vocabulary of the descriptors of the images `names` (in that order) of a feature store.  More than max_train rows
    are thinned to the rows floor(j * n / max_train), j = 0 .. max_train - 1.  Returns {"centroids", "k", "seed", "iters_run",
    "counts", "moved"}."""
    x = np.concatenate([_descriptors(store[n]) for n in names], 0) if len(names) else np.zeros((0, DIM), np.float32)
    n = len(x)
    if n > max_train:
        x = x[(np.arange(max_train, dtype=np.int64) * n) // max_train]
    centroids, counts, moved = kmeans(x, k, max_iters, seed, device)
    return {"centroids": centroids, "k": int(k), "seed": int(seed), "iters_run": len(moved), "counts": counts, "moved": moved}


def save_vocabulary(path, centroids, norm="intra", seed=0, iters_run=0):
    """An .npz with centroids, k, norm, seed and iters_run."""
    c = np.ascontiguousarray(centroids, dtype=np.float32)
    if c.ndim != 2 or c.shape[1] != DIM or not 1 <= len(c) <= MAX_K or norm not in NORMS:
        raise ValueError("not a vocabulary")
    with open(str(path), "wb") as f:
        np.savez(f, centroids=c, k=np.int64(len(c)), norm=np.str_(norm), seed=np.int64(seed), iters_run=np.int64(iters_run))


def load_vocabulary(path):
    """{"centroids" float32 [k, 128], "k", "norm", "seed", "iters_run"} of save_vocabulary's file."""
    with np.load(str(path), allow_pickle=False) as z:
        v = {"centroids": np.ascontiguousarray(z["centroids"], dtype=np.float32), "k": int(z["k"]), "norm": str(z["norm"]),
             "seed": int(z["seed"]), "iters_run": int(z["iters_run"])}
    if v["centroids"].shape != (v["k"], DIM) or v["norm"] not in NORMS:
        raise ValueError(f"{path} is not a vocabulary")
    return v
