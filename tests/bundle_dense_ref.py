"""Helpers of the dense solver's tests (tests/test_gpu_bundle_dense.py, tests/test_bundle_dense_host.py), for the tests only: the
symmetric systems sfd2_spd_solve is tried on and the measure its answers are judged by.  Everything is seeded; nothing here is
imported by the product."""
import numpy as np

SPD_SIZES = (1, 5, 6, 63, 64, 65, 127, 128, 129, 258, 1000)      # either side of one, two and four 64-wide tiles, and a ragged sixteenth
FAIL_N, FAIL_AT = 258, (1, 64, 65, 200)                            # the first non-positive leading minor: first pivot, last of a tile, first of the next, inside the fourth
U = 2.0 ** -53


def spd_system(n, family, seed=2024):
    """(A, b): 'random' A = M M^T + n I with standard normal M; 'ill' eigenvalues log-spaced over ten decades (1 down to 1e-10) in the
    basis of a random orthogonal matrix, symmetrised.  b is standard normal."""
    rs = np.random.RandomState(seed + 7 * n + (0 if family == "random" else 1))
    if family == "random":
        M = rs.standard_normal((n, n))
        A = M @ M.T + n * np.eye(n)
    else:
        Q, _ = np.linalg.qr(rs.standard_normal((n, n)))
        A = (Q * np.logspace(0, -10, n)) @ Q.T
    return 0.5 * (A + A.T), rs.standard_normal(n)


def backward_error(A, x, b):
    """|A x - b| / (|A| |x| + |b|), 2-norms, the residual and the vector norms in numpy.longdouble."""
    ld = np.longdouble
    Al, xl, bl = A.astype(ld), np.asarray(x).astype(ld), b.astype(ld)
    r = Al @ xl - bl
    norm = lambda v: np.sqrt((v * v).sum())
    return float(norm(r) / (ld(np.linalg.norm(A, 2)) * norm(xl) + norm(bl)))


def higham_bound(n):
    """The normwise backward error bound of a Cholesky solve, n (3 n + 1) u."""
    return n * (3 * n + 1) * U


def indefinite(k, n=FAIL_N, seed=77):
    """A symmetric [n, n] matrix with exactly one negative eigenvalue whose leading k x k minor is the first that is not positive: an
    SPD matrix B with twice B[k-1, k-1] taken off that entry.  A rank-one change downwards leaves at most one negative eigenvalue, the
    leading minors before k are B's, and pivot k - 1 of B is at most B[k-1, k-1]."""
    rs = np.random.RandomState(seed + k)
    M = rs.standard_normal((n, n))
    A = M @ M.T + n * np.eye(n)
    A = 0.5 * (A + A.T)
    A[k - 1, k - 1] -= 2.0 * A[k - 1, k - 1]
    return A, rs.standard_normal(n)
