"""The numpy model of the WEIGHTED fixed-size LS-SVM and of its exact leave-one-out scores (k_reduced_gram<true> and k_reduced_leverage of
plssvm_amd/csrc/lssvm_reduced.hip are the device side).

Notation as tests/reduced_model.py and tests/reduced_loo_model.py, with weights w_i >= 0, W = sum_i w_i, q_i = sqrt(w_i).  The model minimises

    1/2 beta^T K_mm beta + C/2 sum_i w_i (y_i - Phi_i beta - b)^2

and has the normal equations of the unweighted model with St = Pt^T diag(w) Pt and W wherever N stands (K_mm is not weighted):

    M = S - s s^T / W + sigma K_mm,   (M + nu I) beta_c = t_c - s eta_c / W,   b_c = (eta_c - s^T beta_c) / W.

It is still a linear smoother: h_ii = w_i (1 / W + |L^-1 (phi_i - s / W)|^2) and f^(-i)(x_i) = y_i - (y_i - f(x_i)) / (1 - h_ii), where f^(-i) is THE SAME MODEL WITH
w_i SET TO 0.  A point of weight 0 has h = 0 and its leave-one-out value is f(x_i) itself.  Everything is float64; q is np.sqrt of the weights (correctly rounded, as the
library's std::sqrt).  Not collected by pytest (no test_ prefix); tests/test_reduced_weighted_host.py checks the model, tests/test_gpu_reduced_weighted.py the device
against it.  reduced_model, reduced_loo_model and pcg_model are imported, not edited.
"""

from __future__ import annotations

import numpy as np

import pcg_model as pm
import reduced_loo_model as lm_
import reduced_model as rm

EPS64 = rm.EPS64
WEIGHT_SEED = 29


def make_weights(N: int, seed: int = WEIGHT_SEED, zeros: float = 0.05, large=(1024.0, 1024.0, 1024.0)):
    """exp(N(0, 1)), about ``zeros`` of them exact zeros, and ``len(large)`` points at the given (large, power-of-two) values."""
    rng = np.random.default_rng(seed)
    w = np.exp(rng.standard_normal(N))
    w[rng.random(N) < zeros] = 0.0
    at = rng.choice(N, size=len(large), replace=False)
    w[at] = np.asarray(large, dtype=np.float64)
    return w


def checked_weights(w, N: int):
    w = np.asarray(w, dtype=np.float64)
    if w.shape != (N,) or not np.all(np.isfinite(w)) or np.any(w < 0.0) or not (np.isfinite(w.sum()) and w.sum() > 0.0):
        raise ValueError("bad weights")
    return w


def weighted_gram(kernel: str, X, Y, landmarks, w, **kw):
    """``(St, |Pw|^T |Pw|)`` for Pw = diag(q) Pt: the weighted operator and the scale of its entries' summands."""
    P = rm.augmented(kernel, X, Y, landmarks, **kw)
    Pw = np.sqrt(checked_weights(w, P.shape[0]))[:, None] * P
    return Pw.T @ Pw, np.abs(Pw).T @ np.abs(Pw)


def _factor(M):
    m = M.shape[0]
    M = 0.5 * (M + M.T)
    nu = EPS64 * np.trace(M)
    for attempt in range(7):
        try:
            return M, np.linalg.cholesky(M + nu * np.eye(m)), nu, attempt
        except np.linalg.LinAlgError:
            if attempt == 6:
                raise
            nu *= 10.0


class WeightedReducedModel:
    """reduced_model.ReducedModel with weights: ``betas`` (k x m), ``rhos`` (k), ``nu``, ``retries``, ``cond`` (of M + nu I), ``cond_range``."""

    def __init__(self, kernel: str, X, Y, cost: float, landmarks, w, held=None, **kw):
        X = np.asarray(X)
        N = X.shape[0]
        self.kernel, self.kw, self.lm = kernel, kw, rm.check_landmarks(landmarks, N)
        self.X_L = np.asarray(X[self.lm], dtype=np.float64)
        self.w = checked_weights(w, N)
        W = float(np.sum(self.w))  # (numpy's pairwise sum; the library sums in index order: they differ by roundings of W, which the bounds cover)
        m = self.lm.size
        X_train, kw_train = (X, kw) if held is None else held
        P = rm.augmented(kernel, X_train, Y, self.lm, **kw_train)
        Pw = np.sqrt(self.w)[:, None] * P
        St = Pw.T @ Pw
        k = St.shape[0] - m - 1
        S, s = St[:m, :m], St[m, :m]
        K_mm = P[self.lm, :m]
        M, L, self.nu, self.retries = _factor(S - np.outer(s, s) / W + K_mm / cost)
        self.M, self.L, self.W, self.s = M, L, W, s
        self.cond = float(np.linalg.cond(M + self.nu * np.eye(m)))
        ev = np.sort(np.linalg.eigvalsh(M + self.nu * np.eye(m)))[::-1]
        self.cond_range = float(ev[0] / ev[np.linalg.matrix_rank(Pw[:, :m]) - 1])
        self.betas, self.rhos = np.zeros((k, m)), np.zeros(k)
        for c in range(k):
            t, eta = St[m + 1 + c, :m], St[m + 1 + c, m]
            beta = np.linalg.solve(L.T, np.linalg.solve(L, t - s * eta / W))
            self.betas[c] = beta
            self.rhos[c] = -(eta - s @ beta) / W

    def decision_values(self, points, betas=None, rhos=None):
        return rm.decision_values(self.kernel, self.X_L, self.betas if betas is None else betas, self.rhos if rhos is None else rhos, points, **self.kw)


def _stacked(Phi, K_mm, Y2, cost, w):
    """The weighted objective as ONE least-squares problem: min |[sqrt(C) diag(q) (Phi beta + b 1 - y); R beta]|^2 with R^T R = K_mm; returns (beta[m, k], b[k])."""
    N, m = Phi.shape
    q = np.sqrt(w)[:, None]
    R = lm_._penalty_root(K_mm)
    A = np.vstack([np.sqrt(cost) * q * np.hstack([Phi, np.ones((N, 1))]), np.hstack([R, np.zeros((m, 1))])])
    rhs = np.vstack([np.sqrt(cost) * q * Y2.T, np.zeros((m, Y2.shape[0]))])
    sol = np.linalg.lstsq(A, rhs, rcond=None)[0]
    return sol[:m], sol[m]


def stacked_weighted_least_squares(kernel: str, X, Y, cost: float, landmarks, w, points, held=None, **kw):
    """The weighted objective solved WITHOUT the normal equations (numpy's SVD-based least squares on the stacked matrix, its data rows scaled by sqrt(C w_i)): the
    decision values f[c, i] at ``points``, the yardstick of :func:`e_model`."""
    X = np.asarray(X)
    Phi, K_mm, Y2 = lm_._blocks(kernel, X, Y, landmarks, held, **kw)
    beta, b = _stacked(Phi, K_mm, Y2, cost, checked_weights(w, X.shape[0]))
    return rm.decision_values(kernel, X[rm.check_landmarks(landmarks, X.shape[0])], beta.T, -b, points, **kw)


def e_model(kernel: str, X, Y, cost: float, landmarks, w, points, held=None, **kw):
    """max |f_normal_equations - f_stacked| / max |f_stacked| over ``points`` (reduced_model.e_model with weights)."""
    f = WeightedReducedModel(kernel, X, Y, cost, landmarks, w, held=held, **kw).decision_values(points)
    g = stacked_weighted_least_squares(kernel, X, Y, cost, landmarks, w, points, held=held, **kw)
    return float(np.max(np.abs(f - g)) / np.max(np.abs(g)))


def dense_full_solution(kernel: str, X, y, cost: float, w, points, held=None, **kw):
    """The weighted full dual LS-SVM ([K + diag(1 / (C w)), 1; 1^T, 0] [alpha; b] = [y; 0]) over the points of weight > 0, dense float64: decision values at ``points``."""
    X = np.asarray(X, dtype=np.float64)
    w = checked_weights(w, X.shape[0])
    keep = np.flatnonzero(w > 0.0)
    X_train, kw_train = (X, kw) if held is None else held
    Xk = np.asarray(X_train, dtype=np.float64)[keep]
    n = keep.size
    A = np.zeros((n + 1, n + 1))
    A[:n, :n] = pm.kernel_matrix(kernel, Xk, Xk, **kw_train) + np.diag(1.0 / (cost * w[keep]))
    A[:n, n] = A[n, :n] = 1.0
    sol = np.linalg.solve(A, np.append(np.asarray(y, dtype=np.float64)[keep], 0.0))
    return pm.kernel_matrix(kernel, points, X[keep], **kw) @ sol[:n] + sol[n]


def loo_values(Y, f, h, w):
    """y - (y - f) / (1 - h); f itself where w = 0 (h is 0 there, and the point took no part in the fit)."""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    return np.where(np.asarray(w)[None, :] == 0.0, f, Y - (Y - f) / (1.0 - np.asarray(h)[None, :]))


def press_of(Y, loo, w):
    """sum_i w_i (y_ic - loo_ic)^2 per right-hand side."""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    return (np.asarray(w)[None, :] * (Y - np.atleast_2d(loo)) ** 2).sum(axis=1)


def errors_of(Y, loo, w):
    """The sign mismatches over the points of weight > 0, per right-hand side."""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    return ((np.sign(np.atleast_2d(loo)) != np.sign(Y)) & (np.asarray(w)[None, :] > 0.0)).sum(axis=1)


class WeightedLooModel:
    """reduced_loo_model.LooModel with weights, by the normal equations as the library takes them: ``h`` (N), ``f`` and ``loo`` (k x N), ``betas``, ``rhos``, ``nu``,
    ``retries``, ``cond``, ``press``, ``loo_errors``, ``max_leverage``."""

    def __init__(self, kernel: str, X, Y, cost: float, landmarks, w, held=None, **kw):
        Phi, K_mm, Y2 = lm_._blocks(kernel, X, Y, landmarks, held, **kw)
        N, m = Phi.shape
        self.w = w = checked_weights(w, N)
        W = float(np.sum(w))
        s = w @ Phi
        S = Phi.T @ (w[:, None] * Phi)
        self.M, L, self.nu, self.retries = _factor(S - np.outer(s, s) / W + K_mm / cost)
        self.cond = float(np.linalg.cond(self.M + self.nu * np.eye(m)))
        Phic = Phi - s[None, :] / W
        T = np.linalg.solve(L, Phic.T)  # m x N
        self.h = w * (1.0 / W + (T * T).sum(axis=0))
        eta = Y2 @ w
        self.betas = np.stack([np.linalg.solve(L.T, np.linalg.solve(L, Phi.T @ (w * y) - s * e / W)) for y, e in zip(Y2, eta)])
        self.rhos = -(eta - self.betas @ s) / W
        self.f = self.betas @ Phic.T + (eta / W)[:, None]
        self.loo = loo_values(Y2, self.f, self.h, w)
        self.press, self.loo_errors = press_of(Y2, self.loo, w), errors_of(Y2, self.loo, w)
        self.max_leverage = float(self.h.max())


def stable(kernel: str, X, Y, cost: float, landmarks, w, held=None, **kw):
    """``(h, f, loo)`` without the normal equations and without nu: h_ii = w_i / W + the squared norm of row i of Q's top block for the thin QR of the stacked matrix on the
    block centred by its WEIGHTED mean, [sqrt(C) diag(q) Phic; R] (a row of weight 0 is a zero row: h = 0); f from the SVD-based least squares of :func:`_stacked`."""
    Phi, K_mm, Y2 = lm_._blocks(kernel, X, Y, landmarks, held, **kw)
    N = Phi.shape[0]
    w = checked_weights(w, N)
    W = float(np.sum(w))
    Phic = Phi - (w @ Phi)[None, :] / W
    A = np.vstack([np.sqrt(cost) * np.sqrt(w)[:, None] * Phic, lm_._penalty_root(K_mm)])
    Q = np.linalg.qr(A, mode="reduced")[0][:N]
    h = w / W + (Q * Q).sum(axis=1)
    beta, b = _stacked(Phi, K_mm, Y2, cost, w)
    f = (Phi @ beta + b[None, :]).T
    return h, f, loo_values(Y2, f, h, w)


def e_loo(model: WeightedLooModel, stable_loo):
    """max |loo_normal_equations - loo_stable| / max |loo_stable|."""
    return float(np.max(np.abs(model.loo - stable_loo)) / np.max(np.abs(stable_loo)))


def brute_force(kernel: str, X, Y, cost: float, landmarks, w, held=None, **kw):
    """loo[c, i] = the value at x_i of the same model with w_i set to 0 (landmarks and K_mm held fixed): N least-squares solves of the stacked weighted problem."""
    Phi, K_mm, Y2 = lm_._blocks(kernel, X, Y, landmarks, held, **kw)
    N = Phi.shape[0]
    w = checked_weights(w, N)
    out = np.zeros((Y2.shape[0], N))
    for i in range(N):
        wi = w.copy()
        wi[i] = 0.0
        beta, b = _stacked(Phi, K_mm, Y2, cost, wi)
        out[:, i] = Phi[i] @ beta + b
    return out


def expand(X, Y, w_int):
    """The unweighted problem that integer weights stand for: row i repeated w_i times (0: removed).  Returns ``(X_dup, Y_dup, first[i] = the index of the first copy of
    row i in the expanded set, or -1)``."""
    w_int = np.asarray(w_int, dtype=np.int64)
    idx = np.repeat(np.arange(w_int.size), w_int)
    first = np.full(w_int.size, -1, dtype=np.int64)
    first[w_int > 0] = np.flatnonzero(np.r_[True, idx[1:] != idx[:-1]])
    return np.ascontiguousarray(np.asarray(X)[idx]), np.ascontiguousarray(np.atleast_2d(Y)[:, idx]), first


# ---- the inputs: the cases of reduced_model with weights exp(N(0, 1)), about 5 % exact zeros, three points at 1 024 ----
# cond(M) eps64 and e_model as a float64 run of these formulas gave them with weights of this kind, for the record: the host test asserts the order of magnitude
RECORDED = {"rbf_777x5": (8e-8, 2e-8), "poly_777x16": (1.5e-11, 2e-11), "rbf_200x4": (7e-6, 1e-8), "linear_300x6": (0.98, 5e-13)}


def fit_case(name: str, dtype=np.float64, k: int = 1):
    """reduced_model.fit_case with ``w``.  rbf_200x4 (every point a landmark, compared with the dense full solution over the points of weight > 0): clipped to >= 0.01."""
    p = rm.fit_case(name, dtype, k)
    w = make_weights(p["X"].shape[0])
    if name == "rbf_200x4":
        w = np.maximum(w, 0.01)
    return dict(p, w=w)


LOO_CASE = ("rbf_255x5", 255, 5, "rbf", dict(gamma=0.2))
LOO_COSTS = (10.0, 1000.0)


def loo_case(dtype=np.float64, k: int = 1, rank: int = 16):
    """255 x 5 rbf; weights exp(N(0, 1)) with exact zeros and ONE large weight, 64 (1 024 would drive h to 0.999 and only amplify rounding)."""
    _, N, d, kernel, kw = LOO_CASE
    X, y = pm.make_data(N, d, pm.DATA_SEED, dtype)
    rng = np.random.default_rng(23)
    Y = np.stack([y] + [np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(dtype) for _ in range(k - 1)])
    kw = rm.rounded_parameters(dtype, **kw)
    return dict(dtype=np.dtype(dtype), X=X, Y=Y, kernel=kernel, kw=kw, landmarks=pm.draw_landmarks(N, rank, pm.LANDMARK_SEED), held=rm.held_data(kernel, X, **kw),
                w=make_weights(N, large=(64.0,)))
