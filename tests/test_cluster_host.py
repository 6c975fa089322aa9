"""Covisibility clustering, the parts that need no GPU: the restatement of tests/cluster_ref.py against results recorded from the
reference (tests/golden/gen_cluster_goldens.py), the host part of MapIndex.clusters, and the kernel's resource metadata."""
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_ref as clr
from sfd2_amd import _lib, build, covis, pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "clusters.npz"))


@pytest.mark.parametrize("name", list(clr.GOLDEN_CASES))
def test_restatement_equals_reference(name):
    images, points3D, lists = clr.golden_inputs(name)
    assert int(GOLD[f"{name}_n"]) == len(lists)
    for i, frame_ids in enumerate(lists):
        got = clr.clusters(frame_ids, images, points3D)
        sizes, members = GOLD[f"{name}_{i}_sizes"].tolist(), GOLD[f"{name}_{i}_members"].tolist()
        assert [len(c) for c in got] == sizes                       # cluster order and sizes exactly
        o = 0
        for c, n in zip(got, sizes):
            assert set(c) == set(members[o:o + n]) and len(set(c)) == n   # members as sets
            o += n
        pos = {f: frame_ids.index(f) for f in frame_ids}
        assert all(c == sorted(c, key=pos.get) for c in got)        # the stated member order


def test_restatement_keeps_creation_order_among_equal_sizes():
    images, points3D, comps = clr.planted_map([3, 3, 2, 2, 1], seed=3)
    ids = [i + 1 for i in clr.interleave(comps, seed=5)]
    got = clr.clusters(ids, images, points3D)
    assert [len(c) for c in got] == [3, 3, 2, 2, 1]
    first = [min(ids.index(f) for f in c) for c in got]
    assert first[0] < first[1] and first[2] < first[3]
    assert sorted(map(sorted, got)) == sorted(sorted(i + 1 for i in c) for c in comps)


def test_directed_rule():
    images, points3D = clr.one_way_map()
    assert clr.clusters([1, 2], images, points3D) == [[1, 2]]       # 0 -> 1: the seed reaches it
    assert clr.clusters([2, 1], images, points3D) == [[2], [1]]     # 1 observes nothing: it reaches nobody, and 0 finds it visited
    assert clr.clusters([4, 1, 2, 3], images, points3D) == [[4, 1, 2], [3]]


def test_cluster_lists_drop_repeats_and_index_the_csr():
    images, points3D, comps = clr.planted_map([4, 2, 1], seed=0)
    mi = covis.MapIndex(images, points3D)
    lists, off, frames = mi.cluster_lists([[3, 1, 3, 2, 1], [], [7, 7], np.array([5, 6])])
    assert lists == [[3, 1, 2], [], [7], [5, 6]] and off.tolist() == [0, 3, 3, 4, 6] and off.dtype == np.int64
    index = mi.csr()[0]
    assert frames.dtype == np.int32 and frames.tolist() == [index[i] for i in (3, 1, 2, 7, 5, 6)]
    with pytest.raises(KeyError):
        mi.cluster_lists([[1, 10 ** 6]])
    # the CSRs are pairs.covisibility_csr's, built once
    ids, oo, op, to, ti = pairs.covisibility_csr(images, points3D)
    assert mi.csr() is mi.csr() and index == {iid: i for i, iid in enumerate(ids)}
    for a, b in zip(mi.csr()[1:], (oo, op, to, ti)):
        assert np.array_equal(a, b) and a.dtype == b.dtype
    assert oo[-1] == sum(int((im.point3D_ids != -1).sum()) for im in images.values())
    assert to[-1] == sum(len(p.image_ids) for p in points3D.values())       # repeated track elements kept


def test_clusters_from_ranks():
    lists = [[9, 4, 7, 2], [], [5]]
    off = np.array([0, 4, 4, 5])
    got = covis.MapIndex.clusters_from_ranks(lists, off, np.array([1, 0, 1, 0, 0], np.int32), np.array([2, 0, 1], np.int32))
    assert got == [[[4, 2], [9, 7]], [], [[5]]]


def test_header_and_binding_agree_on_the_cluster_constants():
    hdr = open(os.path.join(ROOT, "include", "sfd2_hip.h")).read()
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1))  # noqa: E731
    assert val("SFD2_CLUSTER_MAX_FRAMES") == _lib.CLUSTER_MAX_FRAMES == 256
    assert val("SFD2_CLUSTER_LDS_IMAGES") == _lib.CLUSTER_LDS_IMAGES
    assert val("SFD2_CLUSTER_FLAG_GLOBAL_SLOTS") == _lib.CLUSTER_FLAG_GLOBAL_SLOTS
    assert "sfd2_covis_clusters" in _lib.EXPORTS
    assert 2 * _lib.CLUSTER_LDS_IMAGES + 16 * 1024 <= 160 * 1024     # the table beside the kernel's static LDS


def test_cluster_kernel_compiles_without_private_segment_or_spills(tmp_path):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path / "cluster.s"
    src = os.path.join(ROOT, "sfd2_amd", "csrc", "cluster_kernels.hip")
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(out)])
    meta = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*covis_cluster_kernel\S*)", meta)
    assert len(kernels) == 2                                        # the LDS table and the global one
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta) == ["0"] * 2
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", meta) == ["0"] * 2
    assert re.findall(r"\.sgpr_spill_count:\s+(\d+)", meta) == ["0"] * 2
    assert re.findall(r"\.wavefront_size:\s+(\d+)", meta) == ["64"] * 2
    assert all(int(v) <= 16 * 1024 for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", meta))
