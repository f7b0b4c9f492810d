"""The numpy model of the Nystrom preconditioner and of PCG on it (plssvm_amd/csrc/lssvm_precond.hip is the device side).

Notation: n = N - 1, sigma = 1 / C, E = [I_n | -1], H = K + sigma I, Abar = E H E^T.  From m landmarks: L L^T = K_mm + nu I, B_f = K_Nm L^-T, Bhat = [E B_f | sqrt(sigma) 1],
P = E (B_f B_f^T + sigma I) E^T = Bhat Bhat^T + sigma I, G = Bhat^T Bhat + sigma I and P^-1 r = (r - Bhat G^-1 Bhat^T r) / sigma.

``dtype`` is the problem's real type: Bhat and every iteration vector are stored in it, sums and scalars are float64 -- as on the device.  Everything named ``*_f64`` is the
float64 yardstick the tests compare against.  Not collected by pytest (no test_ prefix); tests/test_pcg_host.py checks the model, tests/test_gpu_pcg.py the device against it.
"""

from __future__ import annotations

import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
MAX_RANK = 512


def make_data(N: int, d: int, seed: int, dtype=np.float64):
    """Uniform data in [-1, 1]^d and random +-1 labels (both classes present), as the issue's table."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, size=(N, d)).astype(dtype)
    y = np.where(rng.random(N) < 0.5, -1.0, 1.0)
    y[0], y[-1] = 1.0, -1.0
    return X, y.astype(dtype)


def draw_landmarks(N: int, m: int, seed: int):
    return np.sort(np.random.default_rng(seed).choice(N, size=m, replace=False)).astype(np.uint64)


def kernel_matrix(kernel: str, A, B, gamma: float, coef0: float = 0.0, degree: int = 3):
    """K(a_i, b_j) in float64 from the data as given (rounded to its dtype, then promoted)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if kernel == "linear":
        return A @ B.T
    if kernel == "polynomial":
        return (gamma * (A @ B.T) + coef0) ** degree
    if kernel == "rbf":
        d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)
        return np.exp(-gamma * np.maximum(d2, 0.0))
    raise ValueError(kernel)


def reduced_matrix(kernel: str, X, cost: float, **kw):
    """Abar = E H E^T, dense float64: Abar_ij = H_ij - H_iN - H_Nj + H_NN."""
    N = X.shape[0]
    H = kernel_matrix(kernel, X, X, **kw) + np.eye(N) / cost
    n = N - 1
    return H[:n, :n] - H[:n, n:] - H[n:, :n] + H[n, n]


def reduced_rhs(y):
    y = np.asarray(y, dtype=np.float64)
    return y[:-1] - y[-1]


class Preconditioner:
    """Steps 1-7 of the formulation.  ``Bhat``: n x (m + 1) in ``dtype``; ``Ginv``: float64, symmetric; ``nu``: the jitter that let K_mm factor."""

    def __init__(self, kernel: str, X, cost: float, landmarks, dtype=np.float64, **kw):
        X = np.asarray(X)
        N = X.shape[0]
        lm = np.asarray(landmarks, dtype=np.int64)
        if not (1 <= lm.size <= min(N - 1, MAX_RANK)) or len(set(lm.tolist())) != lm.size or lm.min() < 0 or lm.max() >= N:
            raise ValueError("bad landmarks")
        self.dtype, self.sigma, self.n, self.m = np.dtype(dtype), 1.0 / cost, N - 1, lm.size
        K_Nm = kernel_matrix(kernel, X, X[lm], **kw)
        K_mm = K_Nm[lm]
        nu = EPS64 * np.trace(K_mm)
        for attempt in range(7):
            try:
                L = np.linalg.cholesky(0.5 * (K_mm + K_mm.T) + nu * np.eye(lm.size))
                break
            except np.linalg.LinAlgError:
                if attempt == 6:
                    raise
                nu *= 10.0
        self.nu = nu
        self.B_f = np.linalg.solve(L, K_Nm.T).T                      # K_Nm L^-T, N x m, float64
        Btilde = self.B_f[:-1] - self.B_f[-1]                        # E B_f
        Bhat64 = np.hstack([Btilde, np.full((N - 1, 1), np.sqrt(self.sigma))])
        self.Bhat = Bhat64.astype(self.dtype)                        # stored once, in the problem's real type
        B = self.Bhat.astype(np.float64)
        G = B.T @ B + self.sigma * np.eye(lm.size + 1)
        Ginv = np.linalg.inv(G)
        self.Ginv = 0.5 * (Ginv + Ginv.T)

    def dense_f64(self):
        """P = E (Khat + sigma I) E^T from the float64 Nystrom factor (never rounded to ``dtype``)."""
        N = self.n + 1
        Hhat = self.B_f @ self.B_f.T + self.sigma * np.eye(N)
        n = self.n
        return Hhat[:n, :n] - Hhat[:n, n:] - Hhat[n:, :n] + Hhat[n, n]

    def dense_from_bhat(self):
        B = self.Bhat.astype(np.float64)
        return B @ B.T + self.sigma * np.eye(self.n)

    def apply(self, r):
        """z = r - Bhat G^-1 Bhat^T r = sigma P^-1 r: sums in float64, the result stored in ``dtype``."""
        r = np.asarray(r, dtype=self.dtype)
        B = self.Bhat.astype(np.float64)
        s = self.Ginv @ (B.T @ r.astype(np.float64))
        return (r.astype(np.float64) - B @ s).astype(self.dtype)

    def apply_residual(self, z, r):
        """|P (z / sigma) - r| / |r| against the float64 P."""
        r = np.asarray(r, dtype=np.float64)
        return float(np.linalg.norm(self.dense_f64() @ (np.asarray(z, dtype=np.float64) / self.sigma) - r) / np.linalg.norm(r))


def solve(Abar, b, eps: float, max_iter: int, dtype=np.float64, precond: Preconditioner | None = None):
    """The reference recipe (x0 = 1, stop at |r|^2 <= eps^2 |r0|^2 on the recurrence residual, the true residual every 50th iteration), plain (``precond`` None) or
    preconditioned.  Vectors and the matrix are held in ``dtype``, scalars in float64.  Returns ``(x, iterations, converged)``."""
    dt = np.dtype(dtype).type
    A = np.asarray(Abar).astype(dtype)
    b = np.asarray(b).astype(dtype)
    x = np.ones_like(b)
    r = (b - A @ x).astype(dtype)
    delta0 = delta = float(dt(np.dot(r.astype(np.float64), r.astype(np.float64))))
    target = dt(eps) * dt(eps) * dt(delta0)
    if dt(delta) <= target:
        return x, 0, True
    z = precond.apply(r) if precond is not None else r
    rz = float(np.dot(r.astype(np.float64), z.astype(np.float64)))
    d = z.copy()
    for it in range(max_iter):
        Ad = (A @ d).astype(dtype)
        alpha = dt(rz / float(np.dot(d.astype(np.float64), Ad.astype(np.float64))))
        x = (x + alpha * d).astype(dtype)
        r = (b - A @ x).astype(dtype) if it % 50 == 49 else (r - alpha * Ad).astype(dtype)
        delta = float(dt(np.dot(r.astype(np.float64), r.astype(np.float64))))
        if dt(delta) <= target:
            return x, it + 1, True
        z = precond.apply(r) if precond is not None else r
        rz_new = float(np.dot(r.astype(np.float64), z.astype(np.float64)))
        d = (z + dt(rz_new / rz) * d).astype(dtype)
        rz = rz_new
    return x, max_iter, False


def true_residual(Abar, b, x):
    """|b - Abar x| / |b - Abar 1| in float64."""
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(b - Abar @ np.asarray(x, dtype=np.float64)) / np.linalg.norm(b - Abar @ np.ones_like(b)))


def bias_rho(kernel: str, X, y, cost: float, x, **kw):
    """rho = -bias from the returned alpha through the float64 bias formula, bias = y_N + (k_NN + sigma) sum(x) - q.x with q_i = k(x_i, x_N), and the natural scale of
    its summands: ``(rho, scale)``."""
    X64 = np.asarray(X, dtype=np.float64)
    q = kernel_matrix(kernel, X64[:-1], X64[-1:], **kw)[:, 0]
    QA = float(kernel_matrix(kernel, X64[-1:], X64[-1:], **kw)[0, 0]) + 1.0 / cost
    x = np.asarray(x, dtype=np.float64)
    return -(float(y[-1]) + QA * x.sum() - float(q @ x)), abs(float(y[-1])) + abs(QA) * np.abs(x).sum() + np.abs(q * x).sum()


# ---- the problems of the issue's table: (name, N, d, kernel, kernel parameters, cost, landmarks) and the seeds this project fixed for them ----
TABLE = [
    ("rbf_777x5", 777, 5, "rbf", dict(gamma=0.2), 100.0, 64),
    ("poly_777x16", 777, 16, "polynomial", dict(gamma=1.0 / 16, coef0=1.0, degree=3), 10.0, 200),
    ("rbf_1025x5", 1025, 5, "rbf", dict(gamma=0.2), 1000.0, 64),
    ("linear_777x8", 777, 8, "linear", dict(gamma=1.0), 1e4, 32),
    ("rbf_2000x128", 2000, 128, "rbf", dict(gamma=1.0 / 128), 100.0, 256),
    ("rbf_777x300_flat", 777, 300, "rbf", dict(gamma=1.0 / 300), 100.0, 64),
]
DATA_SEED, LANDMARK_SEED = 20, 21


def table_problem(name: str, dtype=np.float64):
    for row in TABLE:
        if row[0] == name:
            _, N, d, kernel, kw, cost, m = row
            X, y = make_data(N, d, DATA_SEED, dtype)
            return dict(name=name, X=X, y=y, kernel=kernel, kw=kw, cost=cost, landmarks=draw_landmarks(N, m, LANDMARK_SEED))
    raise KeyError(name)


# ---- the inputs of tests/test_gpu_pcg.py: (name, dtype, N, d, kernel, kernel parameters, cost, rank, library options, last point among the landmarks) ----
# N in {300, 777, 1025}: no multiple of 128, 1025 one point past a tile edge; ranks 1, 37, 64, 200 (and the linear row's 32): no multiple of 16 but 64, rank + 1 on both sides of 64.
GPU_CASES = [
    ("f32_rbf5", np.float32, 777, 5, "rbf", dict(gamma=0.2), 100.0, 64, {}, False),                       # centred and scaled data
    ("f32_rbf130", np.float32, 300, 130, "rbf", dict(gamma=1.0 / 130), 10.0, 37, {}, False),              # ... beyond 128 features
    ("f32_rbf_direct", np.float32, 1025, 5, "rbf", dict(gamma=0.2), 100.0, 1, {"rbf_form": 1}, False),    # the direct form: unscaled data
    ("f64_rbf", np.float64, 1025, 5, "rbf", dict(gamma=0.2), 1000.0, 64, {}, False),
    ("f64_rbf_last", np.float64, 300, 5, "rbf", dict(gamma=0.2), 100.0, 37, {}, True),
    ("f64_poly16", np.float64, 777, 16, "polynomial", dict(gamma=1.0 / 16, coef0=1.0, degree=3), 10.0, 200, {}, False),  # sqrt(gamma)-scaled data
    ("f32_poly", np.float32, 300, 16, "polynomial", dict(gamma=1.0 / 16, coef0=1.0, degree=3), 10.0, 37, {}, False),
    ("f64_linear", np.float64, 777, 8, "linear", dict(gamma=1.0), 1e4, 32, {}, False),                    # exact rank
]
GPU_EPS = {np.dtype(np.float32): 1e-4, np.dtype(np.float64): 1e-8}


def gpu_case(name: str):
    for case in GPU_CASES:
        if case[0] == name:
            _, dtype, N, d, kernel, kw, cost, rank, options, with_last = case
            X, y = make_data(N, d, DATA_SEED, dtype)
            lm = draw_landmarks(N, rank, LANDMARK_SEED)
            if with_last and N - 1 not in lm:
                lm[-1] = N - 1
            if not with_last and N - 1 in lm:
                lm[lm == N - 1] = next(i for i in range(N) if i not in lm)
            return dict(name=name, dtype=np.dtype(dtype), X=X, y=y, kernel=kernel, kw=kw, cost=cost, landmarks=lm, options=options, eps=GPU_EPS[np.dtype(dtype)])
    raise KeyError(name)
