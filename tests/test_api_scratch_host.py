"""The geometry entry points' host helpers (sfd2_amd/csrc/api_scratch.h: align256, Carve, at, monotone, in_range / first_outside,
all_finite, and the RANSAC entry points' trial limits and option check) as a stand-alone C++ program under AddressSanitizer and UBSan.
No GPU, no HIP, nothing loaded into Python: the program (tests/host/api_scratch_main.cpp) is built with the host compiler and run as
a child process; the trial limits it answers are compared with the restatement (tests/ransac_ref.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ransac_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host", "api_scratch_main.cpp")
HEADER = os.path.join(ROOT, "sfd2_amd", "csrc", "api_scratch.h")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask(lines) -> the program's output lines: its answers, one per request, then 'api_scratch: ok'"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("api_scratch") / "api_scratch_main")
    # the sanitizer runtimes linked into the program where the compiler has them as archives (clang does so by itself): a runtime that
    # is a shared library refuses to start in a process that has any other library preloaded
    for static in ([] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]), []:
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + SAN + static + [MAIN, "-o", exe],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stdout

    def run(lines):
        r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert r.returncode == 0, r.stdout
        out = r.stdout.splitlines()
        assert out[-1] == "api_scratch: ok" and len(out) == len(lines) + 1, r.stdout
        return out
    return run


def test_header_is_host_only():
    text = open(HEADER).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == ["<algorithm>", "<cmath>", "<cstddef>", "<cstdint>"]


def test_helpers_under_asan_ubsan(ask):
    assert "api_scratch: ok" in ask([])


def test_trial_limits_against_the_restatement(ask):
    """trial_limits on the all-inlier probability the entry points hand it, against ransac_ref.trial_limits at every sample size: the
    closed ends of confidence and min_inlier_ratio, min_num_trials above max_num_trials, a cap above, between and below both limits
    (the focal sweep's; the restatement applies it as pose_focal_ref.capped does, to both options beforehand)."""
    cases = []
    for k in (3, 4, 5, 7):
        for ratio in (0.0, 1e-6, 0.01, 0.25, 0.3, 0.5, 0.5000099, 0.6, 0.7, 0.999, 1.0):
            for conf in (0.0, 0.5, 0.99, 0.999, 0.9999, 1.0):
                for mn, mx in ((0, 10000), (1000, 100000), (50000, 10000), (513, 5000), (0, 1), (5, 10 ** 9)):
                    for cap in (2 ** 63 - 1, 1024, 300, 1):
                        cases.append((k, ratio, conf, mn, mx, cap))
    assert any(cap < min(mn, mx) for _, _, _, mn, mx, cap in cases) and any(mn > mx for _, _, _, mn, mx, _ in cases)
    reqs = []
    for k, ratio, conf, mn, mx, cap in cases:
        p_all = float((np.floor(ratio * 100000) / 100000.0) ** k)           # as ransac_ref.num_trials_needed forms it
        reqs.append("limits %s %s %d %d %d" % (p_all.hex(), float(conf).hex(), mn, mx, cap))
    got = ask(reqs)
    seen = set()
    for (k, ratio, conf, mn, mx, cap), ans in zip(cases, got):
        want = rr.trial_limits(ratio, min(mn, cap), min(mx, cap), conf, k)
        assert tuple(int(v) for v in ans.split()) == want, (k, ratio, conf, mn, mx, cap, ans, want)
        seen.add(want[1])
    assert {1, 104, 257, 300, 1024, 5000, 5295, 10000, 100000, 10 ** 9} <= seen      # the formula, both options and the cap each set the limit somewhere


def test_option_check_texts(ask):
    both = ": confidence and min_inlier_ratio must lie in [0, 1]"
    limits = ": trial limits out of range (1 <= max_num_trials <= 1e9, min_num_trials >= 0)"
    cases = [((0.999, 0.25, 0, 10000), "ok"), ((0.0, 0.0, 0, 1), "ok"), ((1.0, 1.0, 10 ** 9, 10 ** 9), "ok"),
             ((-1e-9, 0.25, 0, 10000), both), ((1.0000001, 0.25, 0, 10000), both), ((0.999, -0.1, 0, 10000), both),
             ((0.999, 1.5, 0, 10000), both), ((float("nan"), 0.25, 0, 10000), both), ((0.999, float("nan"), 0, 10000), both),
             ((0.999, 0.25, 0, 0), limits), ((0.999, 0.25, 0, 10 ** 9 + 1), limits), ((0.999, 0.25, -1, 10000), limits),
             ((2.0, 0.25, -1, 0), both)]                                     # the first check that fails speaks
    got = ask(["check %s %s %d %d" % (float(c).hex() if c == c else "nan", float(r).hex() if r == r else "nan", mn, mx) for (c, r, mn, mx), _ in cases])
    for (case, want), ans in zip(cases, got):
        assert ans == want, (case, ans)
