"""Golden generator for the covisibility clustering: runs the REFERENCE's it_loc/localize_cv2.py do_covisibility_clustering on the
seeded maps of tests/cluster_ref.py and writes tests/golden/clusters.npz -- per case and list the clusters in the reference's order
(members concatenated, and the sizes).  The member order inside a cluster is set.pop()'s and is compared as a set.

Run only where the reference is mounted (SFD2_REFERENCE, default /root/reference); CPU only:
    python tests/golden/gen_cluster_goldens.py

Stand-ins for what the authoring machine lacks, as in gen_covis_goldens.py: empty cv2 / h5py / pycolmap / tqdm modules."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFD2_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

for name in ("cv2", "h5py", "pycolmap"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["cv2"].INTER_NEAREST = 0
try:
    import tqdm  # noqa: F401
except Exception:
    sys.modules["tqdm"] = types.ModuleType("tqdm")
    sys.modules["tqdm"].tqdm = lambda x, *a, **k: x
for name in ("float", "int", "bool"):
    if not hasattr(np, name):
        setattr(np, name, {"float": float, "int": int, "bool": bool}[name])

import it_loc.localize_cv2 as ref  # noqa: E402

import cluster_ref as clr  # noqa: E402


def main():
    out = {}
    saw_tie = saw_repeat = False
    for name in clr.GOLDEN_CASES:
        images, points3D, lists = clr.golden_inputs(name)
        out[f"{name}_n"] = np.array(len(lists))
        for i, frame_ids in enumerate(lists):
            got = ref.do_covisibility_clustering(frame_ids=frame_ids, all_images=images, points3D=points3D)
            sizes = [len(c) for c in got]
            saw_tie |= len(set(sizes)) < len(sizes)
            saw_repeat |= len(set(frame_ids)) < len(frame_ids)
            out[f"{name}_{i}_sizes"] = np.array(sizes, dtype=np.int64)
            out[f"{name}_{i}_members"] = np.array([f for c in got for f in c], dtype=np.int64)
            print(name, i, sizes)
    assert saw_tie and saw_repeat
    path = os.path.join(HERE, "clusters.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
