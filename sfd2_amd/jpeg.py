"""Baseline JPEG on the device (include/sfd2_hip.h sfd2_jpeg_*): the host parses the headers and removes the byte stuffing in
place; the MI355X decodes to the uint8 [H, W, 4] RGBX image sfd2_extract / sfd2_preprocess take with SFD2_FLAG_IMG_U8_X.  The pixels
equal np.asarray(PIL.Image.open(p).convert("RGB")) for every file parse() calls supported; anything else (progressive, arithmetic,
12-bit, CMYK, PNG, ...) is the caller's to decode on the CPU."""
import ctypes

import numpy as np

try:        # torch's HIP runtime first: a process that loads libsfd2hip before torch initialises its own copy of the runtime sees no device
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    pass

from . import _lib

REASONS = {0: "ok", 1: "not a JPEG", 2: "truncated", 3: "progressive", 4: "arithmetic", 5: "precision", 6: "colour space",
           7: "sampling", 8: "multi-scan", 9: "process", 10: "malformed"}


def _as_u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def parse(data):
    """bytes / uint8 array -> sfd2_jpeg_info (fields: width, height, n_components, h_samp, v_samp, restart_interval, supported, reason,
    ...).  Host only."""
    a = _as_u8(data)
    info = _lib.JpegInfo()
    _lib.load().sfd2_jpeg_parse(a.ctypes.data if a.size else None, int(a.size), ctypes.byref(info))
    return info


def supported(data):
    return bool(parse(data).supported)


def reason(info):
    return REASONS.get(int(info.reason), str(int(info.reason)))


def reserve_bytes(nbytes):
    """Bytes to reserve for a file of nbytes so that prepare() fits in the common case (prepared_cap says exactly, after the parse)."""
    return int(nbytes) + int(nbytes) // 4 + 65536


def prepare(buf, info):
    """In place: buf (writable uint8, holding the file in its first info.file_bytes bytes, at least info.prepared_cap long) becomes the
    prepared form sfd2_jpeg_decode uploads."""
    if buf.size < info.prepared_cap:
        raise ValueError("buffer smaller than prepared_cap")
    _lib.check(_lib.load().sfd2_jpeg_prepare(buf.ctypes.data, int(buf.size), ctypes.byref(info)))


def _context(model_or_ctx):
    return getattr(model_or_ctx, "context", model_or_ctx)


def decode(model_or_ctx, data, out=None):
    """Synchronous decode of one JPEG file's bytes -> torch.uint8 cuda [H, W, 4] (RGBX; the fourth byte is 255).  Raises ValueError for a
    file the device decoder does not take (see parse) or whose entropy-coded data it finds invalid."""
    import torch
    ctx = _context(model_or_ctx)
    a = _as_u8(data)
    info = parse(a)
    if not info.supported:
        raise ValueError(f"not decodable on the device: {reason(info)} ({_lib.load().sfd2_last_error().decode()})")
    buf = np.zeros(int(info.prepared_cap), dtype=np.uint8)
    buf[:a.size] = a
    prepare(buf, info)
    if out is None:
        out = torch.empty((info.height, info.width, 4), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    st = np.zeros(1, dtype=np.uint32)
    rc = ctx.lib.sfd2_jpeg_decode(ctx.h, buf.ctypes.data, int(info.prepared_bytes), ctypes.byref(info), 0, out.data_ptr(),
                                  int(out.numel()), st.ctypes.data, 0)
    if rc != 0:
        raise ValueError(ctx.lib.sfd2_last_error().decode("utf-8", "replace"))
    return out


def decode_async(ctx, buf, info, out, status):
    """Queues the decode of a prepared pinned buffer on ctx's stream (status: pinned uint32 [1] or a device tensor).  buf and status
    must stay untouched until the stream has passed."""
    on_dev = 0 if isinstance(status, np.ndarray) else 1
    _lib.check(ctx.lib.sfd2_jpeg_decode(ctx.h, buf.ctypes.data, int(info.prepared_bytes), ctypes.byref(info), _lib.FLAG_ASYNC,
                                        out.data_ptr(), int(out.numel()), _lib.ptr(status), on_dev))


def read_prepared(path, reserve):
    """File -> (pinned prepared buffer view, info) or (None, info) when the device decoder does not take the file.  reserve(nbytes) ->
    writable uint8 buffer (the pipelined driver's pinned buffers); its contents are lost when it has to grow."""
    import os
    n = os.path.getsize(path)
    buf = reserve(reserve_bytes(n))
    with open(path, "rb") as f:
        got = f.readinto(memoryview(buf)[:n])
    if got != n:
        raise ValueError(f"Cannot read image {str(path)}.")
    info = _lib.JpegInfo()
    _lib.load().sfd2_jpeg_parse(buf.ctypes.data if n else None, int(n), ctypes.byref(info))
    if not info.supported:
        return None, info
    if info.prepared_cap > buf.size:                      # pathological restart layouts: grow and read again
        buf = reserve(int(info.prepared_cap))
        with open(path, "rb") as f:
            f.readinto(memoryview(buf)[:n])
    prepare(buf[:int(info.prepared_cap)], info)
    return buf, info
