"""The cost path in numpy (plssvm_amd/csrc/lssvm_path.hip restates it on the device): every cost of a grid from ONE multi-shift CG sequence.

Reduced LS-SVM system of N points, n = N - 1 unknowns, sigma = 1 / C:

    Abar(sigma) = A0 + sigma M,   A0 v = K v + (k_ll S - q.v) 1 - S q  (S = sum v),   M = I + 1 1^T,   b = y[:n] - y[n]
    P = M^(-1/2) = I - theta 1 1^T,  theta = (1 - 1 / sqrt(N)) / n;   (P A0 P + sigma_s I) z_s = P b,   x_s = P z_s

``multi_shift_cg`` runs the recurrences in a given dtype (vectors and the Gram product in that dtype, every sum and scalar in float64, the scalars rounded to the dtype
where they meet a vector -- as the device does); ``dense_system`` / ``dense_solve`` give the float64 reduced system per cost.  Test infrastructure: never imported by
the package."""

from __future__ import annotations

import numpy as np


def kernel_matrix(kernel: str, X, degree: int = 3, gamma: float | None = None, coef0: float = 0.0) -> np.ndarray:
    """The full N x N kernel matrix in float64 (gamma defaults to 1 / num_features, as plssvm_amd.parameter.Parameter resolves it)."""
    X = np.asarray(X, dtype=np.float64)
    gamma = 1.0 / X.shape[1] if gamma is None else gamma
    G = X @ X.T
    if kernel == "linear":
        return G
    if kernel == "polynomial":
        return (gamma * G + coef0) ** degree
    if kernel == "rbf":
        sq = np.diag(G)
        return np.exp(-gamma * np.maximum(sq[:, None] + sq[None, :] - 2.0 * G, 0.0))
    raise ValueError(kernel)


def reduced_parts(Kfull: np.ndarray, y):
    """``(K[n, n], q[n], k_ll, b[n], y_last)`` of the reduced system, float64."""
    y = np.asarray(y, dtype=np.float64)
    n = Kfull.shape[0] - 1
    return Kfull[:n, :n], Kfull[:n, n].copy(), float(Kfull[n, n]), y[:n] - y[n], float(y[n])


def theta_of(n: int) -> float:
    return (1.0 - 1.0 / np.sqrt(n + 1.0)) / n


def apply_P(v: np.ndarray) -> np.ndarray:
    """P v = v - theta sum(v), float64."""
    v = np.asarray(v, dtype=np.float64)
    return v - theta_of(v.size) * v.sum()


def apply_P_inv(v: np.ndarray) -> np.ndarray:
    """P^-1 v = M^(1/2) v = v + (sqrt(N) - 1) / n sum(v), float64."""
    v = np.asarray(v, dtype=np.float64)
    n = v.size
    return v + (np.sqrt(n + 1.0) - 1.0) / n * v.sum()


def dense_system(K: np.ndarray, q: np.ndarray, k_ll: float, cost: float) -> np.ndarray:
    """Abar(1 / cost), float64 [n, n]."""
    n = K.shape[0]
    sigma = 1.0 / cost
    return K + sigma * np.eye(n) + (k_ll + sigma) - q[:, None] - q[None, :]


def dense_solve(K, q, k_ll, b, cost) -> np.ndarray:
    return np.linalg.solve(dense_system(K, q, k_ll, cost), b)


def condition_numbers(K, q, k_ll, costs) -> np.ndarray:
    """kappa_2(P Abar(1 / cost) P) for every cost from ONE eigenvalue decomposition: P Abar(sigma) P = P A0 P + sigma I (P M P = I)."""
    n = K.shape[0]
    P = np.eye(n) - theta_of(n)
    A0 = K + k_ll - q[:, None] - q[None, :]
    lam = np.linalg.eigvalsh(P @ A0 @ P)
    lo, hi = max(lam[0], 0.0), lam[-1]  # (A0 is positive semi-definite: a negative smallest eigenvalue is rounding)
    return np.array([(hi + 1.0 / c) / (lo + 1.0 / c) for c in costs])


def true_residual_norm(K, q, k_ll, b, cost, x) -> float:
    """|P (b - Abar(1 / cost) x)| in float64."""
    x = np.asarray(x, dtype=np.float64)
    sigma = 1.0 / cost
    S = x.sum()
    ax = K @ x + sigma * x + ((k_ll + sigma) * S - q @ x) - S * q
    return float(np.linalg.norm(apply_P(b - ax)))


def finish(x, q, k_ll, y_last, cost):
    """``(alpha_N, rho)`` from the reduced solution: alpha_N = -sum x, rho = -(y_last + (k_ll + sigma) sum x - q.x)."""
    x = np.asarray(x, dtype=np.float64)
    S = x.sum()
    return -S, -(y_last + (k_ll + 1.0 / cost) * S - q @ x)


def multi_shift_cg(K, q, k_ll, b, costs, eps: float, max_iter: int, dtype=np.float64):
    """Returns ``(xs[m, n] in dtype, iterations[m], converged[m], seed_iterations)``: row s the solution x_s = P z_s for costs[s]."""
    dt = np.dtype(dtype).type
    Kd, qd = np.asarray(K, dtype=dtype), np.asarray(q, dtype=dtype)
    n = Kd.shape[0]
    theta = theta_of(n)
    sigma = np.array([float(dt(1) / dt(c)) for c in costs])
    sigma0 = sigma.min()
    delta = sigma - sigma0
    m = sigma.size

    def f64(v):
        return v.astype(np.float64)

    bd = np.asarray(b, dtype=dtype)
    r = (f64(bd) - theta * f64(bd).sum()).astype(dtype)
    p = r.copy()
    rr = float(f64(r) @ f64(r))
    rr0 = rr
    z = np.zeros((m, n), dtype=dtype)
    ps = np.tile(r, (m, 1))
    zeta, zeta_old = np.ones(m), np.ones(m)
    a_old, beta_old = 1.0, 0.0
    active = np.full(m, not rr <= eps * eps * rr0)
    iterations = np.zeros(m, dtype=np.int64)
    it = 0
    while active.any() and it < max_iter:
        it += 1
        Sp = f64(p).sum()
        u = (f64(p) - theta * Sp).astype(dtype)
        Su, Qu = f64(u).sum(), float(f64(u) @ f64(qd))
        t = (f64(Kd @ u) + (k_ll * Su - Qu) - Su * f64(qd)).astype(dtype)
        St, pt, pp = f64(t).sum(), float(f64(p) @ f64(t)), float(f64(p) @ f64(p))
        a = rr / (pt - theta * St * Sp + sigma0 * pp)
        w = (f64(t) - theta * St + sigma0 * f64(p)).astype(dtype)
        r = r - dt(a) * w
        rr_new = float(f64(r) @ f64(r))
        beta = rr_new / rr
        for s in np.flatnonzero(active):
            zn = zeta[s] * zeta_old[s] * a_old / (a * beta_old * (zeta_old[s] - zeta[s]) + zeta_old[s] * a_old * (1.0 + a * delta[s]))
            ratio = zn / zeta[s]
            z[s] += dt(a * ratio) * ps[s]
            ps[s] = dt(zn) * r + dt(beta * ratio * ratio) * ps[s]
            zeta_old[s], zeta[s] = zeta[s], zn
            if zn * zn * rr_new <= eps * eps * rr0:
                active[s] = False
                iterations[s] = it
        p = r + dt(beta) * p
        rr, a_old, beta_old = rr_new, a, beta
    iterations[active] = it
    xs = np.stack([(f64(z[s]) - theta * f64(z[s]).sum()).astype(dtype) for s in range(m)])
    return xs, iterations, ~active, it
