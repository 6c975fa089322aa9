"""sparse_da0_kernel (convDa.0 on the key points' blocks), the parts that need no GPU: the compiled kernel's resources and the properties its
chunk loop shares with conv3x3_rf -- counted waits only, the filter ring and one patch piece per unit, one barrier per chunk."""
import os
import re
import subprocess

import pytest

from sfd2_amd import build

SRC = "sparse_da0_kernel.hip"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not build.have_hipcc():
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("da0") / "sparse_da0.s"
    flags = [f for f in build.FLAGS if f != "-fPIC"] + build.SRC_FLAGS.get(SRC, [])
    subprocess.check_call([build._hipcc()] + flags + ["-S", "--cuda-device-only", os.path.join(build.CSRC, SRC), "-o", str(out)])
    return out.read_text()


def test_sparse_da0_is_built_with_its_neighbours_flags():
    assert SRC in build.SOURCES
    assert build.SRC_FLAGS.get(SRC) == build.SRC_FLAGS["conv3rf_kernels.hip"]      # the branch-free ReLU of the shared epilogue


def test_sparse_da0_kernel_resources(asm):
    kernels = re.findall(r"\.name:\s+(\S*sparse_da0_kernel\S*)", asm)
    assert len(kernels) == 2                                                       # the two tap orders (conv3x3_rf's, conv3x3_pp's)
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", asm)]
    assert len(vgprs) == 2 and max(vgprs) <= 256                                   # two waves per SIMD
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm) == ["0"] * 2
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm) == ["0"] * 2
    assert re.findall(r"\.sgpr_spill_count:\s+(\d+)", asm) == ["0"] * 2
    assert re.findall(r"\.wavefront_size:\s+(\d+)", asm) == ["64"] * 2
    assert re.findall(r"\.group_segment_fixed_size:\s+(\d+)", asm) == ["0"] * 2    # all LDS is dynamic (three patch buffers + the corners of two tiles)


def test_sparse_da0_chunk_loop_keeps_counted_waits(asm):
    bodies = [m.group(2).split("\n") for m in re.finditer(r"^(_Z\w*sparse_da0_kernel\w*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M)]
    assert len(bodies) == 2
    for body in bodies:
        _check_loop(body)


def _check_loop(body):
    idx = [i for i, l in enumerate(body) if "v_mfma" in l]
    span = body[idx[0]:idx[-1] + 1]
    count = lambda lines, pat: sum(1 for l in lines if re.search(pat, l))
    assert count(span, r"v_mfma_f32_32x32x16_f16") == 72                   # 9 units x 2 K halves x 4 pixel fragments: one chunk body
    assert count(span, r"\bscratch_") == 0
    assert count(span, r"s_waitcnt.*vmcnt\(0\)") == 0                      # no full drain: filter loads and patch copies are waited for by count
    assert count(span, r"s_waitcnt vmcnt\(33\) lgkmcnt\(0\)") == 1 and count(span, r"s_barrier") == 1
    assert count(span, r"global_load_dwordx4") == 16                       # the filter ring: 2 loads per unit (the last unit's follow its MFMAs)
    assert count(span, r"buffer_load_dwordx4 .* lds") == 2                 # one patch piece per unit for three units (the first precedes the span)
    assert count(body, r"global_load_lds") == 0                            # (hipcc drains behind the FLAT form)
    assert count(span, r"ds_read_b128") == 72 - 4                          # 4 fragment reads per K half (the first half's precede the span)
    # the key points reach the kernel through scalar loads: no vector load joins the counted ones
    assert count(body, r"global_load_dword\b") == 0
