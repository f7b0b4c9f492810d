"""The numpy model of the exact leave-one-out scores of the fixed-size LS-SVM (k_reduced_leverage of plssvm_amd/csrc/lssvm_reduced.hip is the
device side).  Leave-one-out with the landmark set held fixed.

Notation as tests/reduced_model.py.  The fit is a linear smoother with an unpenalised intercept: with s = Phi^T 1, Phic = Phi - 1 s^T / N and M + nu I = L L^T
(M = Phic^T Phic + sigma K_mm, the matrix the fit factors),

    h_ii = 1 / N + |L^-1 (phi_i - s / N)|^2,   f_c(x_i) = (phi_i - s / N) beta_c + eta_c / N,   f_c^(-i)(x_i) = y_ic - (y_ic - f_c(x_i)) / (1 - h_ii)

where f_c^(-i) is the model refitted without point i on the same landmarks and the same K_mm.  Three routes to the same numbers:

  * :func:`normal_equations` -- the formulas above, as the library evaluates them;
  * :func:`stable` -- a thin QR of the stacked matrix of ``reduced_model.stacked_least_squares`` on the CENTRED block [sqrt(C) Phic; R] (R^T R = K_mm): h_ii = the
    squared norm of row i of Q's top block plus the intercept's share 1 / N, fitted values = Q_top Q_top^T (y - mean) + mean.  No normal equations, no nu;
  * :func:`brute_force` -- N refits, each a least-squares solve of the stacked matrix without row i.

``e_loo`` = the largest difference of the first two routes' leave-one-out values relative to max |loo|: what the normal equations cost on this input.  Everything is float64.
Not collected by pytest (no test_ prefix); tests/test_reduced_loo_host.py checks the model, tests/test_gpu_reduced_loo.py the device against it.
"""

from __future__ import annotations

import numpy as np

import pcg_model as pm
import reduced_model as rm

EPS64 = rm.EPS64
MAX_COSTS = 64


def _blocks(kernel, X, Y, landmarks, held=None, **kw):
    X = np.asarray(X)
    lm = rm.check_landmarks(landmarks, X.shape[0])
    X_train, kw_train = (X, kw) if held is None else held
    Phi = pm.kernel_matrix(kernel, X_train, np.asarray(X_train)[lm], **kw_train)
    return Phi, Phi[lm], np.atleast_2d(np.asarray(Y, dtype=np.float64))


class LooModel:
    """``h`` (N), ``f`` and ``loo`` (k x N), ``betas`` (k x m), ``rhos`` (k), ``nu``, ``cond`` (of M + nu I), ``press`` and ``loo_errors`` (k), ``max_leverage`` -- by the
    normal equations, step by step as the library takes them."""

    def __init__(self, kernel: str, X, Y, cost: float, landmarks, held=None, **kw):
        Phi, K_mm, Y2 = _blocks(kernel, X, Y, landmarks, held, **kw)
        N, m = Phi.shape
        s = Phi.sum(axis=0)
        S = Phi.T @ Phi
        M = S - np.outer(s, s) / N + K_mm / cost
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
        self.M = M
        self.cond = float(np.linalg.cond(M + nu * np.eye(m)))
        Phic = Phi - s[None, :] / N
        self.Phic, self.V, self.shift = Phic, np.linalg.inv(L), s / N
        T = np.linalg.solve(L, Phic.T)  # m x N
        self.h = 1.0 / N + (T * T).sum(axis=0)
        eta = Y2.sum(axis=1)
        self.betas = np.stack([np.linalg.solve(L.T, np.linalg.solve(L, Phi.T @ y - s * e / N)) for y, e in zip(Y2, eta)])
        self.rhos = -(eta - self.betas @ s) / N
        self.f = self.betas @ Phic.T + (eta / N)[:, None]
        self.loo = loo_values(Y2, self.f, self.h)
        self.press, self.loo_errors = press_of(Y2, self.loo), errors_of(Y2, self.loo)
        self.max_leverage = float(self.h.max())


def loo_values(Y, f, h):
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    return Y - (Y - f) / (1.0 - np.asarray(h)[None, :])


def press_of(Y, loo):
    """sum_i (y_ic - loo_ic)^2 per right-hand side."""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    return ((Y - np.atleast_2d(loo)) ** 2).sum(axis=1)


def errors_of(Y, loo):
    """The number of points whose leave-one-out value has another sign than y (sign(0) = 0), per right-hand side."""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    return (np.sign(np.atleast_2d(loo)) != np.sign(Y)).sum(axis=1)


def _penalty_root(K_mm):
    w, V = np.linalg.eigh(0.5 * (K_mm + K_mm.T))
    return np.sqrt(np.maximum(w, 0.0))[:, None] * V.T


def stable(kernel: str, X, Y, cost: float, landmarks, held=None, **kw):
    """``(h, f, loo)`` by the backward-stable route of the module docstring."""
    Phi, K_mm, Y2 = _blocks(kernel, X, Y, landmarks, held, **kw)
    N, m = Phi.shape
    Phic = Phi - Phi.mean(axis=0)[None, :]
    A = np.vstack([np.sqrt(cost) * Phic, _penalty_root(K_mm)])
    Q = np.linalg.qr(A, mode="reduced")[0][:N]
    h = 1.0 / N + (Q * Q).sum(axis=1)
    ybar = Y2.mean(axis=1)[:, None]
    f = ((Y2 - ybar) @ Q) @ Q.T + ybar
    return h, f, loo_values(Y2, f, h)


def e_loo(model: LooModel, stable_loo):
    """max |loo_normal_equations - loo_stable| / max |loo_stable|."""
    return float(np.max(np.abs(model.loo - stable_loo)) / np.max(np.abs(stable_loo)))


def brute_force(kernel: str, X, Y, cost: float, landmarks, held=None, **kw):
    """loo[c, i] = the value at x_i of the model refitted WITHOUT point i -- the landmark set, and with it K_mm, held fixed (a landmark that is left out stays a basis
    function; its data term goes): N least-squares solves of min |sqrt(C) (Phi_-i beta + b 1 - y_-i)|^2 + |R beta|^2."""
    Phi, K_mm, Y2 = _blocks(kernel, X, Y, landmarks, held, **kw)
    N, m = Phi.shape
    R = _penalty_root(K_mm)
    top = np.sqrt(cost) * np.hstack([Phi, np.ones((N, 1))])
    bottom = np.hstack([R, np.zeros((m, 1))])
    out = np.zeros((Y2.shape[0], N))
    for i in range(N):
        keep = np.arange(N) != i
        A = np.vstack([top[keep], bottom])
        rhs = np.vstack([np.sqrt(cost) * Y2[:, keep].T, np.zeros((m, Y2.shape[0]))])
        sol = np.linalg.lstsq(A, rhs, rcond=None)[0]
        out[:, i] = Phi[i] @ sol[:m] + sol[m]
    return out


def tolerance(model: LooModel, e: float, scale: float):
    """8 x max(e_loo, cond(M) eps64) x scale: the rule of reduced_model.fit_tolerance with this model's yardstick."""
    return 8.0 * max(e, model.cond * EPS64) * float(scale)


# ---- the inputs of the identity tests: (name, N, d, kernel, kernel parameters, rank), each at IDENTITY_COSTS ----
IDENTITY_CASES = [
    ("rbf_255x5", 255, 5, "rbf", dict(gamma=0.2), 16),
    ("poly_255x16", 255, 16, "polynomial", dict(gamma=1.0 / 16, coef0=1.0, degree=3), 16),
]
IDENTITY_COSTS = (0.1, 1.0, 100.0, 1e4)
FIT_COSTS = (0.1, 10.0, 1000.0)


def identity_case(name: str, dtype=np.float64):
    for row in IDENTITY_CASES:
        if row[0] == name:
            _, N, d, kernel, kw, rank = row
            X, y = pm.make_data(N, d, pm.DATA_SEED, dtype)
            kw = rm.rounded_parameters(dtype, **kw)
            return dict(name=name, dtype=np.dtype(dtype), X=X, Y=y[None, :], kernel=kernel, kw=kw, landmarks=pm.draw_landmarks(N, rank, pm.LANDMARK_SEED),
                        held=rm.held_data(kernel, X, **kw))
    raise KeyError(name)


def overlapping_blobs(N: int, d: int, classes: int, seed: int, dtype=np.float64):
    """Blobs that overlap (reduced_model.blobs with a spread of the centres' distance): no cost separates them, so the leave-one-out score moves with the cost."""
    return rm.blobs(N, d, classes, seed, spread=1.5, dtype=dtype)
