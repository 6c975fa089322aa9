"""COLMAP's binary sparse model (cameras.bin, images.bin, points3D.bin), read and written from the format itself: little-endian
records, counts as uint64.

  cameras.bin   n; per camera: int32 id, int32 model id, uint64 width, uint64 height, float64 params[model]
  images.bin    n; per image: int32 id, float64 qvec[4] (w x y z), float64 tvec[3], int32 camera id, name + NUL, uint64 m,
                m x (float64 x, float64 y, int64 point3D id or -1)
  points3D.bin  n; per point: uint64 id, float64 xyz[3], uint8 rgb[3], float64 error, uint64 k, k x (int32 image id, int32 point2D idx)

The readers return dicts id -> record with the field names sfd2_amd.covis.MapIndex and sfd2_amd.localize read (.id .model .width
.height .params; .id .qvec .tvec .camera_id .name .xys .point3D_ids; .id .xyz .rgb .error .image_ids .point2D_idxs).  A Camera is
also a mapping ('model', 'width', 'height', 'params'), the form sfd2_amd.pose takes, so it goes into absolute_pose_estimation as
read.  Text-format models are not handled."""
import os
import struct

import numpy as np

# model id -> (name, number of parameters): COLMAP's camera model table
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
CAMERA_MODEL_IDS = {name: (mid, n) for mid, (name, n) in CAMERA_MODELS.items()}

_POINT2D = np.dtype([("xy", "<f8", 2), ("id", "<i8")])
_TRACK = np.dtype([("image_id", "<i4"), ("point2D_idx", "<i4")])


class _Record:
    __slots__ = ()

    def __init__(self, *args, **kw):
        names = self.__slots__
        if len(args) > len(names):
            raise TypeError(f"{type(self).__name__} takes {len(names)} fields")
        vals = dict(zip(names, args))
        vals.update(kw)
        for n in names:
            setattr(self, n, vals[n])

    def _asdict(self):
        return {n: getattr(self, n) for n in self.__slots__}

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{n}={getattr(self, n)!r}' for n in self.__slots__)})"


class Camera(dict):
    """id, model (name), width, height, params (float64); attribute and mapping access."""

    def __init__(self, id, model, width, height, params):
        super().__init__(id=int(id), model=model, width=int(width), height=int(height), params=np.asarray(params, dtype=np.float64))

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class Image(_Record):
    __slots__ = ("id", "qvec", "tvec", "camera_id", "name", "xys", "point3D_ids")


class Point3D(_Record):
    __slots__ = ("id", "xyz", "rgb", "error", "image_ids", "point2D_idxs")


class _Reader:
    def __init__(self, path):
        self.path = str(path)
        with open(self.path, "rb") as f:
            self.buf = f.read()
        self.at = 0

    def take(self, fmt):
        n = struct.calcsize(fmt)
        if self.at + n > len(self.buf):
            raise ValueError(f"{self.path}: truncated at byte {self.at} (needs {n} more, {len(self.buf) - self.at} left)")
        out = struct.unpack_from(fmt, self.buf, self.at)
        self.at += n
        return out

    def array(self, dtype, count):
        n = np.dtype(dtype).itemsize * count
        if self.at + n > len(self.buf):
            raise ValueError(f"{self.path}: truncated at byte {self.at} (needs {n} more, {len(self.buf) - self.at} left)")
        out = np.frombuffer(self.buf, dtype=dtype, count=count, offset=self.at)
        self.at += n
        return out

    def cstring(self):
        end = self.buf.find(b"\x00", self.at)
        if end < 0:
            raise ValueError(f"{self.path}: truncated inside a name at byte {self.at}")
        s = self.buf[self.at:end].decode("utf-8")
        self.at = end + 1
        return s

    def done(self):
        if self.at != len(self.buf):
            raise ValueError(f"{self.path}: {len(self.buf) - self.at} bytes after the last record")


def read_cameras_binary(path):
    r = _Reader(path)
    cameras = {}
    for _ in range(r.take("<Q")[0]):
        cid, mid, w, h = r.take("<iiQQ")
        if mid not in CAMERA_MODELS:
            raise ValueError(f"{r.path}: camera {cid} has the unknown model id {mid}")
        name, n = CAMERA_MODELS[mid]
        cameras[cid] = Camera(cid, name, w, h, r.array("<f8", n).copy())
    r.done()
    return cameras


def read_images_binary(path):
    r = _Reader(path)
    images = {}
    for _ in range(r.take("<Q")[0]):
        v = r.take("<i7di")
        name = r.cstring()
        p = r.array(_POINT2D, r.take("<Q")[0])
        images[v[0]] = Image(v[0], np.array(v[1:5]), np.array(v[5:8]), v[8], name, p["xy"].copy().reshape(-1, 2), p["id"].copy())
    r.done()
    return images


def read_points3D_binary(path):
    r = _Reader(path)
    points = {}
    for _ in range(r.take("<Q")[0]):
        v = r.take("<Q3d3Bd")
        t = r.array(_TRACK, r.take("<Q")[0])
        points[v[0]] = Point3D(v[0], np.array(v[1:4]), np.array(v[4:7], dtype=np.uint8), v[7], t["image_id"].copy(), t["point2D_idx"].copy())
    r.done()
    return points


def write_cameras_binary(cameras, path):
    out = [struct.pack("<Q", len(cameras))]
    for cid, c in cameras.items():
        model = c["model"] if not hasattr(c, "model") else c.model
        model = model if isinstance(model, str) else getattr(model, "name", str(model))
        if model not in CAMERA_MODEL_IDS:
            raise ValueError(f"camera {cid} has the unknown model {model!r}")
        mid, n = CAMERA_MODEL_IDS[model]
        params = np.asarray(c["params"] if isinstance(c, dict) else c.params, dtype="<f8").reshape(-1)
        if params.size != n:
            raise ValueError(f"camera {cid}: model {model} takes {n} parameters, got {params.size}")
        width, height = (c["width"], c["height"]) if isinstance(c, dict) else (c.width, c.height)
        out += [struct.pack("<iiQQ", int(cid), mid, int(width), int(height)), params.tobytes()]
    with open(str(path), "wb") as f:
        f.write(b"".join(out))


def write_images_binary(images, path):
    out = [struct.pack("<Q", len(images))]
    for iid, im in images.items():
        xys = np.asarray(im.xys, dtype=np.float64).reshape(-1, 2)
        ids = np.asarray(im.point3D_ids).reshape(-1)
        if len(xys) != len(ids):
            raise ValueError(f"image {iid}: {len(xys)} key points for {len(ids)} point3D ids")
        p = np.empty(len(ids), dtype=_POINT2D)
        p["xy"], p["id"] = xys, ids
        out += [struct.pack("<i7di", int(iid), *(float(x) for x in im.qvec), *(float(x) for x in im.tvec), int(im.camera_id)),
                im.name.encode("utf-8") + b"\x00", struct.pack("<Q", len(ids)), p.tobytes()]
    with open(str(path), "wb") as f:
        f.write(b"".join(out))


def write_points3D_binary(points3D, path):
    out = [struct.pack("<Q", len(points3D))]
    for pid, pt in points3D.items():
        t = np.empty(len(pt.image_ids), dtype=_TRACK)
        t["image_id"], t["point2D_idx"] = pt.image_ids, pt.point2D_idxs
        out += [struct.pack("<Q3d3Bd", int(pid), *(float(x) for x in pt.xyz), *(int(x) for x in pt.rgb), float(pt.error)),
                struct.pack("<Q", len(t)), t.tobytes()]
    with open(str(path), "wb") as f:
        f.write(b"".join(out))


def read_model(path):
    """(cameras, images, points3D) of the directory `path`."""
    path = str(path)
    return (read_cameras_binary(os.path.join(path, "cameras.bin")), read_images_binary(os.path.join(path, "images.bin")),
            read_points3D_binary(os.path.join(path, "points3D.bin")))


def write_model(cameras, images, points3D, path):
    path = str(path)
    os.makedirs(path, exist_ok=True)
    write_cameras_binary(cameras, os.path.join(path, "cameras.bin"))
    write_images_binary(images, os.path.join(path, "images.bin"))
    write_points3D_binary(points3D, os.path.join(path, "points3D.bin"))
