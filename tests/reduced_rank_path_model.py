"""The numpy model of the rank path of the fixed-size LS-SVM: the leave-one-out scores of every prefix rank from one fit (DESIGN.md section 18;
k_reduced_leverage_prefix of plssvm_amd/csrc/lssvm_reduced.hip is the device side).

Notation as tests/reduced_weighted_model.py (weights w_i >= 0, W = sum_i w_i; without weights w = 1 and W = N).  The landmark list is ordered.  For a prefix length r
the model on the first r landmarks needs only leading blocks of the rank-m quantities: M_r = M[:r, :r], and with M + nu I = L L^T the factor of the leading block is the
leading block of the factor.  With U = L^-1 Phic^T (m x N) and z_c = L^-1 (t_c - s eta_c / W):

    h_ii^(r) = w_i (1 / W + sum_{j<r} U_ji^2),   f_c^(r)(x_i) = sum_{j<r} U_ji z_cj + eta_c / W,   beta_c^(r) = L_r^-T z_c[:r],   b_c^(r) = (eta_c - s[:r]^T beta_c^(r)) / W

:class:`RankPathModel` takes the prefixes of the FULL-rank factor with a given nu (None: the library's rule on the full rank, eps64 trace(M), tenfold per failed
factorisation).  :func:`from_scratch` is the fit on landmarks[:r] alone with a given nu, by the formulas of reduced_weighted_model.WeightedLooModel: with the same nu the two
are the same numbers up to rounding (the nesting identity), with the prefix's own nu they differ by what :func:`jitter_bound` states.
Everything is float64.  Not collected by pytest (no test_ prefix); tests/test_reduced_rank_path_host.py checks the model, tests/test_gpu_reduced_rank_path.py the device
against it.  reduced_model, reduced_loo_model, reduced_weighted_model and pcg_model are imported, not edited.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import reduced_loo_model as rlm
import reduced_model as rm
import reduced_weighted_model as rw

EPS64 = rm.EPS64
MAX_RANKS = 16
MAX_CELLS = 64


def check_ranks(ranks, rank: int):
    r = np.asarray(ranks, dtype=np.int64)
    if r.ndim != 1 or not 1 <= r.size <= MAX_RANKS or r[0] < 1 or r[-1] > rank or np.any(r[1:] <= r[:-1]):
        raise ValueError("bad rank list")
    return r


def _normal_equations(Phi, K_mm, Y2, cost, w):
    W = float(np.sum(w))
    s = w @ Phi
    S = Phi.T @ (w[:, None] * Phi)
    M = S - np.outer(s, s) / W + K_mm / cost
    eta = Y2 @ w
    rhs = np.stack([Phi.T @ (w * y) - s * e / W for y, e in zip(Y2, eta)])  # k x m
    return 0.5 * (M + M.T), s, W, eta, rhs


def _scores(Y2, U, Z, L, s, W, eta, w, r, M, nu):
    """One prefix model from the leading blocks: U (m x N), Z (k x m), L (m x m) of a rank >= r."""
    m = L.shape[0]
    h = w * (1.0 / W + (U[:r] * U[:r]).sum(axis=0))
    f = Z[:, :r] @ U[:r] + (eta / W)[:, None]
    loo = rw.loo_values(Y2, f, h, w)
    betas = np.zeros((Y2.shape[0], m))
    betas[:, :r] = np.linalg.solve(L[:r, :r].T, Z[:, :r].T).T
    rhos = -(eta - betas[:, :r] @ s[:r]) / W
    d2 = np.diag(L)[:r] ** 2
    return SimpleNamespace(rank=int(r), h=h, f=f, loo=loo, betas=betas, rhos=rhos, nu=nu, cond=float(np.linalg.cond(M[:r, :r] + nu * np.eye(r))),
                           cond_hint=float(d2.max() / d2.min()), press=rw.press_of(Y2, loo, w), loo_errors=rw.errors_of(Y2, loo, w), max_leverage=float(h.max()),
                           norm=float(np.linalg.norm(M[:r, :r], 2)), rho_scale=float(np.max((np.abs(eta) + np.abs(betas[:, :r]) @ np.abs(s[:r])) / W)))


class RankPathModel:
    """``at[q]`` for every checkpoint of ``ranks``: ``h`` (N), ``f`` and ``loo`` (k x N), ``betas`` (k x m, zeros from r_q on), ``rhos`` (k), ``cond`` (of
    M_r + nu I), ``cond_hint`` (max / min of the squared diagonal of the factor's leading block), ``press``, ``loo_errors``, ``max_leverage``, ``norm`` (the 2-norm of
    M_r), ``rho_scale`` (the largest (|eta_c| + |s[:r]|^T |beta_c|) / W: rho is a difference of terms of that size, and its rounding is relative to them, not to rho) -- the prefixes of the full-rank factor with ``nu`` (None: the library's rule on the full rank; ``retries`` then says how often it failed)."""

    def __init__(self, kernel: str, X, Y, cost: float, landmarks, ranks, w=None, nu=None, held=None, **kw):
        Phi, K_mm, Y2 = rlm._blocks(kernel, X, Y, landmarks, held, **kw)
        N, m = Phi.shape
        self.ranks = check_ranks(ranks, m)
        self.w = w = np.ones(N) if w is None else rw.checked_weights(w, N)
        M, s, W, eta, rhs = _normal_equations(Phi, K_mm, Y2, cost, w)
        if nu is None:
            _, L, nu, self.retries = rw._factor(M)
        else:
            L, self.retries = np.linalg.cholesky(M + nu * np.eye(m)), 0
        self.Phi, self.K_mm, self.M, self.L, self.nu, self.shift = Phi, K_mm, M, L, float(nu), s / W
        self.V = np.linalg.inv(L)
        self.Phic = Phi - s[None, :] / W
        self.U = np.linalg.solve(L, self.Phic.T)
        self.Z = np.linalg.solve(L, rhs.T).T
        self.at = [_scores(Y2, self.U, self.Z, L, s, W, eta, w, int(r), M, self.nu) for r in self.ranks]


def from_scratch(kernel: str, X, Y, cost: float, landmarks, r: int, nu, w=None, held=None, **kw):
    """The fit on landmarks[:r] ALONE with the jitter ``nu`` (None: its own, by the library's rule), by the formulas of reduced_weighted_model.WeightedLooModel: the same
    fields as an entry of :attr:`RankPathModel.at`, the betas r long."""
    lm = np.asarray(landmarks)[:r]
    Phi, K_mm, Y2 = rlm._blocks(kernel, X, Y, lm, held, **kw)
    N = Phi.shape[0]
    w = np.ones(N) if w is None else rw.checked_weights(w, N)
    M, s, W, eta, rhs = _normal_equations(Phi, K_mm, Y2, cost, w)
    if nu is None:
        _, L, nu, _ = rw._factor(M)
    else:
        L = np.linalg.cholesky(M + nu * np.eye(r))
    T = np.linalg.solve(L, (Phi - s[None, :] / W).T)
    h = w * (1.0 / W + (T * T).sum(axis=0))
    betas = np.linalg.solve(L.T, np.linalg.solve(L, rhs.T)).T
    f = betas @ (Phi - s[None, :] / W).T + (eta / W)[:, None]
    loo = rw.loo_values(Y2, f, h, w)
    return SimpleNamespace(rank=int(r), h=h, f=f, loo=loo, betas=betas, rhos=-(eta - betas @ s) / W, nu=float(nu), cond=float(np.linalg.cond(M + nu * np.eye(r))),
                           press=rw.press_of(Y2, loo, w), loo_errors=rw.errors_of(Y2, loo, w), max_leverage=float(h.max()), norm=float(np.linalg.norm(M, 2)))


def jitter_bound(prefix, nu_full: float, nu_own: float, scale: float):
    """What the documented difference to a separate fit on landmarks[:r] may move the results by: that fit solves with M_r + nu_r I, the rank path with M_r + nu_m I, a
    relative perturbation of the matrix of (nu_m - nu_r) / |M_r|, which first-order perturbation theory of a linear system amplifies by cond(M_r):
    8 cond(M_r) (nu_m - nu_r) / |M_r| x scale, the 8 the margin of :func:`reduced_loo_model.tolerance`."""
    return 8.0 * prefix.cond * (nu_full - nu_own) / prefix.norm * float(scale)


# ---- the inputs of the nesting tests: the 255-point identity cases of reduced_loo_model with 40 landmarks ----
NESTING_RANK = 40
NESTING_PREFIXES = (1, 7, 16, 17, 40)
NESTING_COSTS = (1.0, 100.0)


def nesting_case(name: str, k: int = 1):
    """An identity case of reduced_loo_model with NESTING_RANK landmarks, k right-hand sides and weights uniform in [0, 2] with some exact zeros."""
    import pcg_model as pm

    _, N, d, kernel, kw, _ = next(row for row in rlm.IDENTITY_CASES if row[0] == name)
    X, y = pm.make_data(N, d, pm.DATA_SEED, np.float64)
    rng = np.random.default_rng(31)
    Y = np.stack([y] + [np.where(rng.random(N) < 0.5, -1.0, 1.0) for _ in range(k - 1)])
    w = rng.uniform(0.0, 2.0, N)
    w[rng.random(N) < 0.05] = 0.0
    return dict(name=name, X=X, Y=Y, kernel=kernel, kw=kw, landmarks=pm.draw_landmarks(N, NESTING_RANK, pm.LANDMARK_SEED), held=rm.held_data(kernel, X, **kw), w=w)
