"""The numpy model of the fixed-size (reduced) LS-SVM (plssvm_amd/csrc/lssvm_reduced.hip is the device side).

Notation: N points, landmarks L (m distinct indices), sigma = 1 / C, Phi = K(X, X_L) (N x m), K_mm = Phi[L, :], k right-hand sides Y (k x N).  The model minimises
1/2 beta^T K_mm beta + C/2 sum_i (y_i - Phi_i beta - b)^2.  Device side: Pt = [Phi | 1 | y_0 ... y_{k-1}] (N x (m + 1 + k)) and St = Pt^T Pt.  Host side:
S = St[:m,:m], s = St[m,:m], t_c = St[m+1+c,:m], eta_c = St[m+1+c,m], M = S - s s^T / N + sigma K_mm, (M + nu I) beta_c = t_c - s eta_c / N, b_c = (eta_c - s^T beta_c) / N,
rho_c = -b_c; nu starts at eps64 trace(M) and is raised tenfold, six times at most, while the Cholesky factorisation fails.

Everything is float64 on the data as given (rounded to its dtype, then promoted).  Data, kernels and the landmark rule come from tests/pcg_model.py.  Not collected by
pytest (no test_ prefix); tests/test_reduced_host.py checks the model, tests/test_gpu_reduced.py the device against it.
"""

from __future__ import annotations

import numpy as np

import pcg_model as pm

EPS64 = pm.EPS64
EPS32 = float(np.finfo(np.float32).eps)
MAX_RANK = 1024


def library_landmarks(N: int, rank: int):
    """The library's own choice (include/plssvm_amd.h): the first ``rank`` entries of a Fisher-Yates shuffle of 0 ... N-1 driven by splitmix64 from a fixed state."""
    mask = (1 << 64) - 1
    perm = list(range(N))
    state = 0x243F6A8885A308D3
    for i in range(rank):
        state = (state + 0x9E3779B97F4A7C15) & mask
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        j = i + z % (N - i)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array(perm[:rank], dtype=np.uint64)


def check_landmarks(landmarks, N: int):
    lm = np.asarray(landmarks, dtype=np.int64)
    if lm.ndim != 1 or not (1 <= lm.size <= min(N, MAX_RANK)) or len(set(lm.tolist())) != lm.size or lm.min() < 0 or lm.max() >= N:
        raise ValueError("bad landmarks")
    return lm


LOG2E = 1.4426950408889634073599246810019


def held_data(kernel: str, X, direct: bool = False, **kw):
    """``(X_held, kernel parameters on it)``: the data as the library's problem holds it, where that is not the data as given up to roundings of float64 size.  A float32
    rbf problem off the direct form (``rbf_direct`` = 0 in its info) centres its data and scales it by the float32 value of sqrt(2 gamma log2 e), both in float32
    (k_center: (x - mean) * scale), and the landmark block evaluates exp(-gamma / scale^2 |x'_i - x'_j|^2) on that in double.  Every other float32 problem holds the data
    as given; float64 problems centre / scale in float64, which the tests' bounds cover with a term of their own."""
    X = np.asarray(X)
    if kernel == "rbf" and X.dtype == np.float32 and not direct:
        gamma = np.float32(kw["gamma"])
        scale = np.float32(np.sqrt(2.0 * float(gamma) * LOG2E))
        mean = X.astype(np.float64).mean(axis=0).astype(np.float32)
        held = ((X - mean).astype(np.float32) * scale).astype(np.float32)
        return held, dict(kw, gamma=float(gamma) / (float(scale) * float(scale)))
    return X, kw


def rounded_parameters(dtype, **kw):
    """gamma and coef0 as the library uses them: rounded to the problem's real type (static_cast<T>, as the reference does)."""
    return {name: (value if name == "degree" else float(np.dtype(dtype).type(value))) for name, value in kw.items()}


def augmented(kernel: str, X, Y, landmarks, **kw):
    """Pt = [Phi | 1 | y_0 ... y_{k-1}], N x (m + 1 + k), float64."""
    X = np.asarray(X)
    lm = check_landmarks(landmarks, X.shape[0])
    Y2 = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    Phi = pm.kernel_matrix(kernel, X, X[lm], **kw)
    return np.hstack([Phi, np.ones((X.shape[0], 1)), Y2.T])


def landmark_gram(kernel: str, X, Y, landmarks, **kw):
    """``(St, |Pt|^T |Pt|)``: the operator and the scale of its entries' summands."""
    P = augmented(kernel, X, Y, landmarks, **kw)
    return P.T @ P, np.abs(P).T @ np.abs(P)


class ReducedModel:
    """The formulation, step by step.  ``betas`` (k x m), ``rhos`` (k), ``nu`` (the jitter that let M factor), ``retries``, ``cond`` (of M + nu I).  ``held``:
    ``(X_held, its kernel parameters)`` of :func:`held_data` where Phi is to be evaluated on the data as the problem holds it; the decision values are always evaluated
    with the kernel on the data as given, as a user of the model evaluates them."""

    def __init__(self, kernel: str, X, Y, cost: float, landmarks, held=None, **kw):
        X = np.asarray(X)
        N = X.shape[0]
        self.kernel, self.kw, self.lm = kernel, kw, check_landmarks(landmarks, N)
        self.X_L = np.asarray(X[self.lm], dtype=np.float64)
        m = self.lm.size
        sigma = 1.0 / cost
        X_train, kw_train = (X, kw) if held is None else held
        P = augmented(kernel, X_train, Y, self.lm, **kw_train)
        St = P.T @ P
        k = St.shape[0] - m - 1
        S, s = St[:m, :m], St[m, :m]
        K_mm = P[self.lm, :m]
        M = S - np.outer(s, s) / N + sigma * K_mm
        M = 0.5 * (M + M.T)
        nu = EPS64 * np.trace(M)
        for attempt in range(7):
            try:
                L = np.linalg.cholesky(M + nu * np.eye(m))
                break
            except np.linalg.LinAlgError:
                if attempt == 6:
                    raise
                nu *= 10.0
        self.nu, self.retries = nu, attempt
        self.cond = float(np.linalg.cond(M + nu * np.eye(m)))
        # the condition number on the range of Phi: where Phi has rank r < m (the linear kernel with m > d landmarks) the other m - r directions of beta are carried by
        # nu alone and change no decision value, so the error of f follows the r largest eigenvalues
        w = np.sort(np.linalg.eigvalsh(M + nu * np.eye(m)))[::-1]
        self.cond_range = float(w[0] / w[np.linalg.matrix_rank(P[:, :m]) - 1])
        self.betas, self.rhos = np.zeros((k, m)), np.zeros(k)
        for c in range(k):
            t, eta = St[m + 1 + c, :m], St[m + 1 + c, m]
            beta = np.linalg.solve(L.T, np.linalg.solve(L, t - s * eta / N))
            self.betas[c] = beta
            self.rhos[c] = -(eta - s @ beta) / N

    def decision_values(self, points, betas=None, rhos=None):
        """f[c, i] = sum_j beta[c, j] k(x_i, x_L[j]) - rho[c] in float64, from this model's coefficients or the given ones (e.g. the device's)."""
        return decision_values(self.kernel, self.X_L, self.betas if betas is None else betas, self.rhos if rhos is None else rhos, points, **self.kw)


def decision_values(kernel: str, X_L, betas, rhos, points, **kw):
    K = pm.kernel_matrix(kernel, points, X_L, **kw)
    return np.atleast_2d(np.asarray(betas, dtype=np.float64)) @ K.T - np.atleast_1d(np.asarray(rhos, dtype=np.float64))[:, None]


def summand_scale(kernel: str, X_L, betas, rhos, points, **kw):
    """sum_j |beta_j k_j| + |b| per (classifier, point): the scale a float32 evaluation of the decision function is rounded on."""
    K = pm.kernel_matrix(kernel, points, X_L, **kw)
    B = np.abs(np.atleast_2d(np.asarray(betas, dtype=np.float64)))
    return B @ np.abs(K).T + np.abs(np.atleast_1d(rhos))[:, None]


def stacked_least_squares(kernel: str, X, Y, cost: float, landmarks, points, held=None, **kw):
    """The same objective solved WITHOUT the normal equations: min |[sqrt(C) (Phi beta + b 1 - y); R beta]|^2 with R^T R = K_mm (eigen-decomposition, negative rounding
    clipped), by numpy's SVD-based least squares.  Returns the decision values f[c, i] at ``points``: the yardstick of ``e_model``."""
    X = np.asarray(X)
    lm = check_landmarks(landmarks, X.shape[0])
    Y2 = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    X_train, kw_train = (X, kw) if held is None else held
    Phi = pm.kernel_matrix(kernel, X_train, np.asarray(X_train)[lm], **kw_train)
    K_mm = Phi[lm]
    w, V = np.linalg.eigh(0.5 * (K_mm + K_mm.T))
    R = np.sqrt(np.maximum(w, 0.0))[:, None] * V.T
    N, m = Phi.shape
    A = np.vstack([np.sqrt(cost) * np.hstack([Phi, np.ones((N, 1))]), np.hstack([R, np.zeros((m, 1))])])
    rhs = np.vstack([np.sqrt(cost) * Y2.T, np.zeros((m, Y2.shape[0]))])
    sol = np.linalg.lstsq(A, rhs, rcond=None)[0]
    return decision_values(kernel, X[lm], sol[:m].T, -sol[m], points, **kw)


def e_model(kernel: str, X, Y, cost: float, landmarks, points, held=None, **kw):
    """max |f_normal_equations - f_stacked| / max |f_stacked| over ``points``: what the normal equations of this input cost against a backward-stable solve."""
    f = ReducedModel(kernel, X, Y, cost, landmarks, held=held, **kw).decision_values(points)
    g = stacked_least_squares(kernel, X, Y, cost, landmarks, points, held=held, **kw)
    return float(np.max(np.abs(f - g)) / np.max(np.abs(g)))


def dense_full_solution(kernel: str, X, y, cost: float, points, held=None, **kw):
    """The full dual LS-SVM of the reference ([K + I / C, 1; 1^T, 0] [alpha; b] = [y; 0]), dense float64: decision values at ``points``.  ``held``: as for
    :class:`ReducedModel` -- K of the system from the data as the problem holds it, the decision values from the data as given."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    X_train, kw_train = (X, kw) if held is None else held
    A = np.zeros((N + 1, N + 1))
    A[:N, :N] = pm.kernel_matrix(kernel, X_train, X_train, **kw_train) + np.eye(N) / cost
    A[:N, N] = A[N, :N] = 1.0
    sol = np.linalg.solve(A, np.append(np.asarray(y, dtype=np.float64), 0.0))
    return pm.kernel_matrix(kernel, points, X, **kw) @ sol[:N] + sol[N]


def fit_tolerance(model: ReducedModel, e: float, f):
    """The bound of the GPU tests on decision values: 8 x max(e_model, cond(M) eps64) x max |f| (the factor 8 is the margin of tests/test_gpu_pcg.py)."""
    return 8.0 * max(e, model.cond * EPS64) * float(np.max(np.abs(f)))


def range_tolerance(model: ReducedModel, e: float, f):
    """:func:`fit_tolerance` with the condition number of M on the range of Phi: the bound where M is singular by construction (the linear kernel with more landmarks than
    features), where cond(M + nu I) ~ trace / nu makes :func:`fit_tolerance` vacuous."""
    return 8.0 * max(e, model.cond_range * EPS64) * float(np.max(np.abs(f)))


# ---- the inputs of the fit tests: (name, N, d, kernel, kernel parameters, cost, rank) on pcg_model.make_data; held-out points from another seed ----
FIT_CASES = [
    ("rbf_777x5", 777, 5, "rbf", dict(gamma=0.2), 100.0, 64),
    ("poly_777x16", 777, 16, "polynomial", dict(gamma=1.0 / 16, coef0=1.0, degree=3), 10.0, 64),
]
ALL_LANDMARKS_CASE = ("rbf_200x4", 200, 4, "rbf", dict(gamma=0.5), 10.0, 200)
LINEAR_CASE = ("linear_300x6", 300, 6, "linear", dict(gamma=1.0), 10.0, 8)
HELD_OUT_SEED, HELD_OUT = 22, 200


def case(row, dtype=np.float64, k: int = 1):
    name, N, d, kernel, kw, cost, rank = row
    X, y = pm.make_data(N, d, pm.DATA_SEED, dtype)
    rng = np.random.default_rng(23)
    Y = np.stack([y] + [np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(dtype) for _ in range(k - 1)])
    points = pm.make_data(HELD_OUT, d, HELD_OUT_SEED, dtype)[0]
    lm = np.arange(N, dtype=np.uint64) if rank == N else pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
    kw = rounded_parameters(dtype, **kw)
    return dict(name=name, dtype=np.dtype(dtype), X=X, Y=Y, kernel=kernel, kw=kw, cost=cost, landmarks=lm, points=points, held=held_data(kernel, X, **kw))


def fit_case(name: str, dtype=np.float64, k: int = 1):
    for row in FIT_CASES + [ALL_LANDMARKS_CASE, LINEAR_CASE]:
        if row[0] == name:
            return case(row, dtype, k)
    raise KeyError(name)


def blobs(N: int, d: int, classes: int, seed: int, spread: float = 0.35, dtype=np.float64):
    """Well-separated blobs: class c around a centre drawn from [-2, 2]^d, labels 0 ... classes-1 in turn."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, (classes, d)) * 2.0
    labels = np.arange(N) % classes
    return (centres[labels] + spread * rng.standard_normal((N, d))).astype(dtype), labels
