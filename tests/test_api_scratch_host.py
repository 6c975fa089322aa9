"""The geometry entry points' host helpers (sfd2_amd/csrc/api_scratch.h: align256, Carve, at, monotone, in_range / first_outside,
all_finite) as a stand-alone C++ program under AddressSanitizer and UBSan.  No GPU, no HIP, nothing loaded into Python: the program
(tests/host/api_scratch_main.cpp) is built with the host compiler and run as a child process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host", "api_scratch_main.cpp")
HEADER = os.path.join(ROOT, "sfd2_amd", "csrc", "api_scratch.h")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_header_is_host_only():
    text = open(HEADER).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == ["<algorithm>", "<cmath>", "<cstddef>", "<cstdint>"]


def test_helpers_under_asan_ubsan(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "api_scratch_main")
    # the sanitizer runtimes linked into the program where the compiler has them as archives (clang does so by itself): a runtime that
    # is a shared library refuses to start in a process that has any other library preloaded
    for static in ([] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]), []:
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + SAN + static + [MAIN, "-o", exe],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0, run.stdout
    assert "api_scratch: ok" in run.stdout
