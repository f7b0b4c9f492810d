"""The yardstick of the dense SPD toolbox on the device (plssvm_amd/csrc/lssvm_dense.hip): the test matrices, the three derived error bounds, a
numpy reference of each step, and ctypes wrappers of the three testing aids.  Shared by tests/test_dense_host.py (CPU) and tests/test_gpu_dense.py (GPU).

The bounds (u = eps64 / 2; |.| and <= entry by entry; residuals evaluated in numpy float64):
  factorisation  |A + nu I - L L^T| <= 2 (m + 1) eps64 |L||L^T|        Higham, Accuracy and Stability, Thm 10.3 (gamma_{m+1}, any order of the inner sums), plus numpy's own
                                                                        product (gamma_m): about (m + 1) eps64 together; the factor 2 is the margin and covers a_jj + nu
  solve          |b - (A + nu I) x| <= (5 m + 3) eps64 |L||L^T||x|     Thm 10.4 (gamma_{3m+1}) plus about 2 gamma_{m+1} for numpy's evaluation
  inverse        min(max |V L - I| / (2 (m + 1) eps64 |V||L|), max |L V - I| / (2 (m + 1) eps64 |L||V|)) <= 1 on the lower triangle: a substitution method meets the left or
                 the right residual bound (gamma_m) depending on its orientation (sections 14.2 - 14.3), the evaluation adds gamma_m
"""

import ctypes as C

import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
MAX_RANK = 1024
CONDS = (1e2, 1e10)


def sizes(block: int):
    """The sizes of the toolbox tests: around 16 (the MFMA tile), around one and two blocks, one that is no multiple of anything, and the cap."""
    return sorted({1, 2, 15, 16, 17, block - 1, block, block + 1, 2 * block + 1, 300, MAX_RANK})


def spd_matrix(m: int, cond: float, seed: int = 0):
    """A = Q diag(logspace(0, -log10 cond, m)) Q^T, symmetrised, Q from the QR of a seeded normal matrix."""
    rng = np.random.default_rng(1000 + 7 * m + seed)
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    A = (Q * np.logspace(0.0, -np.log10(cond), m)) @ Q.T
    return 0.5 * (A + A.T)


def indefinite(m: int, j: int):
    """The cond-1e2 matrix with A[j][j] = -1: the leading j x j block is well conditioned and the pivot of column j is -1 - sum l^2 < 0 whatever the summation order."""
    A = spd_matrix(m, 1e2).copy()
    A[j, j] = -1.0
    return A


def right_hand_sides(m: int, k: int, seed: int = 3):
    return np.random.default_rng(seed + m).standard_normal((k, m))


def safe_ratio(err, scale):
    """max err / scale over the entries where either is nonzero; an error on an exactly zero scale counts as infinite."""
    err, scale = np.asarray(err), np.asarray(scale)
    if np.any((scale == 0.0) & (err != 0.0)):
        return float("inf")
    mask = scale > 0.0
    return float(np.max(err[mask] / scale[mask])) if np.any(mask) else 0.0


def factor_ratio(A, nu, L):
    m = A.shape[0]
    target = np.tril(A) + nu * np.eye(m)
    return safe_ratio(np.abs(np.tril(target - L @ L.T)), 2.0 * (m + 1) * EPS64 * np.tril(np.abs(L) @ np.abs(L.T)))


def solve_ratio(A, nu, L, B, X, extra=None):
    """The largest ratio over the k rows of B / X; ``extra``: a further allowance per entry (k x m), e.g. for the roundings of an assembly."""
    m = A.shape[0]
    full = np.tril(A) + np.tril(A, -1).T + nu * np.eye(m)
    scale = (5 * m + 3) * EPS64 * (np.abs(X) @ (np.abs(L) @ np.abs(L.T)).T)
    if extra is not None:
        scale = scale + extra
    return safe_ratio(np.abs(B - X @ full.T), scale)


def inverse_ratio(L, V):
    m = L.shape[0]
    eye = np.eye(m)
    left = safe_ratio(np.abs(np.tril(V @ L - eye)), 2.0 * (m + 1) * EPS64 * np.tril(np.abs(V) @ np.abs(L)))
    right = safe_ratio(np.abs(np.tril(L @ V - eye)), 2.0 * (m + 1) * EPS64 * np.tril(np.abs(L) @ np.abs(V)))
    return min(left, right), left, right


# ---- the numpy yardstick: numpy.linalg.cholesky, row-wise substitution, a row-wise forward-substitution inverse (the order of the host path's invert_lower_rows) ----
def reference_solve(L, B):
    m = L.shape[0]
    X = np.zeros_like(B)
    for c in range(B.shape[0]):
        z = np.zeros(m)
        for j in range(m):
            z[j] = (B[c, j] - L[j, :j] @ z[:j]) / L[j, j]
        x = np.zeros(m)
        for j in range(m - 1, -1, -1):
            x[j] = (z[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
        X[c] = x
    return X


def reference_inverse(L):
    m = L.shape[0]
    V = np.zeros((m, m))
    for n in range(m):
        row = -(L[n, :n] @ V[:n, :])
        row[n] += 1.0
        V[n] = row / L[n, n]
    return np.tril(V)


def unblocked_cholesky_failure(A):
    """0 where the unblocked lower Cholesky factorisation of A's lower triangle completes, else 1 + the column whose pivot is not positive and finite."""
    m = A.shape[0]
    L = np.zeros((m, m))
    for j in range(m):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not (d > 0.0 and np.isfinite(d)):
            return j + 1
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return 0


# ---- the three testing aids (include/plssvm_amd_testing.h) ----
def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def device_cholesky(A, nu=0.0):
    """(L, status, ms): lssvm_mi355_dense_cholesky on the m x m float64 A."""
    from plssvm_amd import _capi
    A = np.ascontiguousarray(A, dtype=np.float64)
    m = A.shape[0]
    L, status, ms = np.full((m, m), np.nan), C.c_uint64(99), C.c_double(0.0)
    _capi.check(_capi.dense_entry("lssvm_mi355_dense_cholesky")(_dp(A), m, float(nu), _dp(L), C.byref(status), C.byref(ms)))
    return L, int(status.value), float(ms.value)


def device_solve(L, B):
    from plssvm_amd import _capi
    L, B = np.ascontiguousarray(L, dtype=np.float64), np.ascontiguousarray(np.atleast_2d(B), dtype=np.float64)
    X, ms = np.full(B.shape, np.nan), C.c_double(0.0)
    _capi.check(_capi.dense_entry("lssvm_mi355_dense_solve")(_dp(L), L.shape[0], _dp(B), B.shape[0], _dp(X), C.byref(ms)))
    return X, float(ms.value)


def device_invert_lower(L):
    from plssvm_amd import _capi
    L = np.ascontiguousarray(L, dtype=np.float64)
    V, ms = np.full(L.shape, np.nan), C.c_double(0.0)
    _capi.check(_capi.dense_entry("lssvm_mi355_dense_invert_lower")(_dp(L), L.shape[0], _dp(V), C.byref(ms)))
    return V, float(ms.value)
