"""What the four RANSAC kernels share without the device (sfd2_amd/csrc/ransac_math.h: chol_solve, sample_k, ransac_enough) as a
stand-alone C++ program under AddressSanitizer and UBSan.  No GPU, no HIP, nothing loaded into Python: the program
(tests/host/ransac_math_main.cpp) is built with the host compiler, fed one request per line and its answers are compared with numpy
and with the restatements (pose_ref.sample3, two_view_ref.sample5, fundamental_ref.num_trials_needed)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import fundamental_ref as fr
import pose_ref as pr
import two_view_ref as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "host", "ransac_math_main.cpp")
HEADER = os.path.join(ROOT, "sfd2_amd", "csrc", "ransac_math.h")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# relative error of chol_solve against numpy.linalg.solve at condition <= 1e6: 1e6 * 2^-52 * N^2 is 1.4e-8 at N = 8 at the very
# worst; measured 7.4e-12 at most over the cases below
SOLVE_TOL = 1e-9


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask(lines) -> the program's answers, one per request"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ransac_math") / "ransac_math_main")
    # the sanitizer runtimes linked into the program where the compiler has them as archives (clang does so by itself): a runtime that
    # is a shared library refuses to start in a process that has any other library preloaded
    for static in ([] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]), []:
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas"] + SAN + static +
                               [MAIN, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stdout

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert r.returncode == 0, r.stdout
        out = r.stdout.splitlines()
        assert out[-1] == "ransac_math: done" and len(out) == len(lines) + 1, r.stdout
        return out[:-1]
    return run


def test_header_is_hip_free():
    text = open(HEADER).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == ["<math.h>", "<stdint.h>"]
    assert "#define SFD2_PD inline" in text
    for word in ("threadIdx", "__shfl", "__syncthreads", "double2", "__global__"):
        assert word not in text, word


def _packed(H, g):
    n = len(g)
    return [H[a, b] for a in range(n) for b in range(a, n)] + list(g)


def _request(n, lam, H, g):
    return "chol %d %s " % (n, float(lam).hex()) + " ".join(float(v).hex() for v in _packed(H, g))


def _spd(rs, n, cond):
    q, _ = np.linalg.qr(rs.standard_normal((n, n)))
    return (q * np.logspace(0, -math.log10(cond), n)) @ q.T * 10.0 ** rs.uniform(-3, 3)


def test_chol_solve_against_numpy(ask):
    rs = np.random.RandomState(7)
    cases = []
    for n in (5, 6, 7, 8):
        for cond in (1.0, 1e3, 1e6):
            for lam in (0.0, 1e-4, 10.0):
                H = _spd(rs, n, cond)
                H = 0.5 * (H + H.T)
                cases.append((n, lam, H, rs.standard_normal(n) * np.sqrt(np.diag(H).max())))
    worst = 0.0
    for (n, lam, H, g), ans in zip(cases, ask([_request(*c) for c in cases])):
        assert ans.startswith("ok "), (n, lam, ans)
        d = np.array([float.fromhex(v) for v in ans.split()[1:]])
        A = H + lam * np.diag(np.diag(H)) + 1e-15 * np.diag(H).max() * np.eye(n)
        want = np.linalg.solve(A, -g)
        err = np.linalg.norm(d - want) / np.linalg.norm(want)
        worst = max(worst, err)
        assert err <= SOLVE_TOL, (n, lam, np.linalg.cond(H), err)
    print("chol_solve: worst relative error %.3g" % worst)


def test_chol_solve_refuses(ask):
    reqs, names = [], []
    for n in (5, 6, 7, 8):
        eye, g = np.eye(n), np.ones(n)
        nan_diag = eye.copy()
        nan_diag[n // 2, n // 2] = np.nan
        indefinite = eye.copy()
        indefinite[0, n - 1] = indefinite[n - 1, 0] = 2.0
        negative = eye.copy()
        negative[n - 1, n - 1] = -1.0
        g_inf = g.copy()
        g_inf[n - 1] = np.inf
        for name, H, gg in (("zero", np.zeros((n, n)), g), ("nan on the diagonal", nan_diag, g), ("indefinite", indefinite, g),
                            ("negative pivot", negative, g), ("inf in the gradient", eye, g_inf), ("inf on the diagonal", np.diag(np.full(n, np.inf)), g)):
            reqs.append(_request(n, 1e-4, H, gg))
            names.append((n, name))
        reqs.append(_request(n, 0.0, eye, g))
        names.append((n, "identity"))
    for (n, name), ans in zip(names, ask(reqs)):
        if name == "identity":
            d = np.array([float.fromhex(v) for v in ans.split()[1:]])
            assert ans.startswith("ok ") and np.allclose(d, -1.0, rtol=0, atol=1e-14), (n, ans)
        else:
            assert ans == "fail", (n, name, ans)


def test_sample_k_equals_the_restatements(ask):
    cases = [(k, seed, trial, n) for k in (3, 5) for n in (k, k + 1, 40, 2 ** 31 - 1) for trial in (0, 1, 255, 256, 2 ** 40)
             for seed in (0, 12345, 2 ** 64 - 1)]
    got = ask(["sample %d %d %d %d" % c for c in cases])
    for (k, seed, trial, n), ans in zip(cases, got):
        want = pr.sample3(seed, trial, n) if k == 3 else tv.sample5(seed, trial, n)
        assert tuple(int(v) for v in ans.split()) == tuple(int(v) for v in want), (k, seed, trial, n)


def _want_stop(k, trials, mn, mx, conf, n, best):
    if trials >= mx:
        return True
    if trials < mn or best <= 0:
        return False
    # num_trials_needed is fundamental_ref's for sample size 7; the same rule at another size through the same function
    return trials >= fr.num_trials_needed((best / n) ** (k / 7.0), conf)


def test_ransac_enough_against_the_restatement(ask):
    cases = []
    for k in (3, 4, 5, 7):
        cases += [(k, 10 ** 6, 0, 10 ** 9, 1.0, 100, 90),            # confidence 1: never enough
                  (k, 256, 0, 10 ** 9, 0.999, 100, 100),              # ratio 1: enough at once ...
                  (k, 256, 512, 10 ** 9, 0.999, 100, 100),            # ... but not before min_trials
                  (k, 512, 512, 10 ** 9, 0.999, 100, 100),
                  (k, 10 ** 8, 0, 10 ** 9, 0.999, 10 ** 6, 1),        # ratio 1e-6: den == 1, never enough
                  (k, 1000, 0, 1000, 1.0, 100, 90),                   # trials == max_trials ends it whatever the rest
                  (k, 1000, 2000, 1000, 0.999, 100, 0),
                  (k, 999, 0, 1000, 1.0, 100, 90),
                  (k, 10 ** 6, 0, 10 ** 9, 0.999, 100, 0)]            # no hypothesis yet
    # sample size 7 in general position: a tenth short of and beyond num_trials_needed (the power's last bit cannot matter there)
    for best, conf in ((50, 0.999), (30, 0.99), (80, 0.9999), (60, 0.5)):
        need = fr.num_trials_needed(best / 100.0, conf)
        assert 1 < need < 1e8
        cases += [(7, int(need * 0.9) - 1, 0, 10 ** 9, conf, 100, best), (7, int(need * 1.1) + 2, 0, 10 ** 9, conf, 100, best)]
    got = ask(["enough %d %d %d %d %s %d %d" % (k, t, mn, mx, float(c).hex(), n, b) for k, t, mn, mx, c, n, b in cases])
    for case, ans in zip(cases, got):
        assert ans == ("1" if _want_stop(*case) else "0"), case
    assert [a for a in got[-8:]] == ["0", "1"] * 4
