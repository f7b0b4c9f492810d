"""The numpy model of the fixed-size kernel logistic regression by iteratively reweighted least squares (k_reduced_logistic_step and the loop of
plssvm_amd/csrc/lssvm_logistic.hip are the device side).

Notation as tests/reduced_weighted_model.py.  With labels y_i in {-1, +1}, prior weights a_i >= 0 and the cost C the model minimises

    J(beta, b) = 1/2 beta^T K_mm beta + C sum_i a_i log(1 + exp(-y_i eta_i)),    eta_i = Phi_i beta + b.

One Newton step from (beta, b) is the weighted fixed-size fit at the same C with v_i = a_i max(mu_i, delta), z_i = eta_i + g_i / max(mu_i, delta), delta = 2^-32, and
W = sum_i v_i as the Gram matrix holds it.  The elementwise quantities are evaluated in the library's cancellation-free forms (:func:`row_quantities`); the loop
(:func:`fit`) is the library's, rule for rule: pass t >= 1 compares J_t with the objective J' of the last accepted iterate -- J' - J_t < -tol J' rejects the iterate (it
becomes the midpoint of itself and the last accepted one: a halving), |J' - J_t| <= tol J' converges on the iterate of the smaller J (two objectives within the rounding
of their own sums, 2 (N + 16) eps64 J', count as equal and the newer iterate is returned: this close to the minimum the older one is the less accurate by a Newton step, and
which of the two sums came out smaller is decided by their last bits), anything else accepts it and solves for the next.  ``max_iter`` counts passes, rejected ones
included; 30 halvings in a row give up.  Everything is float64.  Not collected by pytest (no test_ prefix); tests/test_reduced_logistic_host.py checks the model,
tests/test_gpu_reduced_logistic.py the device against it.
"""

from __future__ import annotations

import numpy as np

import pcg_model as pm
import reduced_loo_model as lm_
import reduced_model as rm
import reduced_weighted_model as wm

EPS64 = rm.EPS64
DELTA = 2.0 ** -32
MAX_HALVINGS = 30


def row_quantities(y, a, eta):
    """``(q, z, loss, mu, g)`` per row from s = y eta and e = exp(-|s|): mu = e / ((1 + e)(1 + e)), loss = max(-s, 0) + log1p(e), g = y (s >= 0 ? e / (1 + e) :
    1 / (1 + e)), q = sqrt(a max(mu, delta)), z = eta + g / max(mu, delta).  No p (1 - p) is formed from p."""
    y, a, eta = np.asarray(y, dtype=np.float64), np.asarray(a, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    s = y * eta
    e = np.exp(-np.abs(s))
    ope = 1.0 + e
    mu = e / (ope * ope)
    loss = np.maximum(-s, 0.0) + np.log1p(e)
    g = y * np.where(s >= 0.0, e / ope, 1.0 / ope)
    mf = np.maximum(mu, DELTA)
    return np.sqrt(a * mf), eta + g / mf, loss, mu, g


def objective(Phi, K_mm, y, a, cost, beta, b):
    loss = row_quantities(y, a, Phi @ beta + b)[2]
    return 0.5 * float(beta @ (K_mm @ beta)) + cost * float(np.sum(a * loss))


def gradient(Phi, K_mm, y, a, cost, beta, b):
    """dJ / d(beta, b): K_mm beta - C Phi^T (a g) and -C sum a g."""
    g = row_quantities(y, a, Phi @ beta + b)[4]
    return np.append(K_mm @ beta - cost * (Phi.T @ (a * g)), -cost * float(np.sum(a * g)))


def newton_step(Phi, K_mm, q, z, cost):
    """The weighted fixed-size fit on [Phi | 1 | z] with sqrt(v) = q by the normal equations, as the library takes them: ``(beta, rho, nu, cond(M + nu I), M)``."""
    m = Phi.shape[1]
    Pw = q[:, None] * np.hstack([Phi, np.ones((Phi.shape[0], 1)), z[:, None]])
    St = Pw.T @ Pw
    S, s, W = St[:m, :m], St[m, :m], St[m, m]
    M, L, nu, _ = wm._factor(S - np.outer(s, s) / W + K_mm / cost)
    t, eta = St[m + 1, :m], St[m + 1, m]
    beta = np.linalg.solve(L.T, np.linalg.solve(L, t - s * eta / W))
    return beta, -(eta - s @ beta) / W, nu, float(np.linalg.cond(M + nu * np.eye(m))), M


def stacked_step(Phi, K_mm, q, z, cost):
    """The same step WITHOUT the normal equations: numpy's SVD-based least squares on the stacked matrix (reduced_weighted_model._stacked)."""
    beta, b = wm._stacked(Phi, K_mm, z[None, :], cost, q * q)
    return beta[:, 0], -float(b[0]), 0.0, 0.0, None


def fit(Phi, K_mm, y, a=None, cost=1.0, tol=1e-8, max_iter=50, start=None, halving=True, step=newton_step):
    """The loop.  Returns a dict: ``beta``, ``rho``, ``passes``, ``halvings``, ``converged``, ``objective``, ``last_decrease``, ``accepted`` (the J of every accepted
    iterate, in order), ``cond`` (of the last solve's M + nu I) and ``M`` (the last solve's).  ``halving=False``: the loop without its rejection rule (every iterate is accepted
    unless it converges), for the test of the safeguard."""
    Phi, K_mm, y = np.asarray(Phi, dtype=np.float64), np.asarray(K_mm, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N, m = Phi.shape
    a = np.ones(N) if a is None else np.asarray(a, dtype=np.float64)
    cur = np.zeros(m + 1) if start is None else np.append(np.asarray(start[0], dtype=np.float64), float(start[1]))
    acc, J_acc, have_acc, consecutive = cur.copy(), 0.0, False, 0
    out = dict(passes=0, halvings=0, converged=0, last_decrease=0.0, accepted=[], cond=0.0, M=None, nu=0.0)

    def done(result, J, converged):
        return dict(out, beta=result[:m].copy(), rho=float(result[m]), objective=float(J), converged=int(converged))

    while True:
        q, z, loss, _, _ = row_quantities(y, a, Phi @ cur[:m] - cur[m])
        J = 0.5 * float(cur[:m] @ (K_mm @ cur[:m])) + cost * float(np.sum(a * loss))
        out["passes"] += 1
        last = out["passes"] >= max_iter
        if have_acc:
            decrease = J_acc - J
            out["last_decrease"] = decrease
            if halving and not decrease >= -tol * J_acc:
                out["halvings"] += 1
                consecutive += 1
                if consecutive >= MAX_HALVINGS or last:
                    return done(acc, J_acc, False)
                cur = 0.5 * (cur + acc)
                continue
            if abs(decrease) <= tol * J_acc:
                return done(cur, J, True) if J - J_acc <= 2.0 * (N + 16) * EPS64 * J_acc else done(acc, J_acc, True)
        acc, J_acc, have_acc, consecutive = cur.copy(), J, True, 0
        out["accepted"].append(J)
        beta, rho, out["nu"], out["cond"], out["M"] = step(Phi, K_mm, q, z, cost)
        cur = np.append(beta, rho)
        if last:
            return done(cur, J_acc, False)


class LogisticModel:
    """The fit of one case on the data as the problem holds it (``held``: reduced_model.held_data), its decision values with the kernel on the data as given."""

    def __init__(self, kernel: str, X, y, cost: float, landmarks, a=None, held=None, tol=1e-8, max_iter=50, start=None, halving=True, step=newton_step, **kw):
        X = np.asarray(X)
        self.kernel, self.kw, self.lm = kernel, kw, rm.check_landmarks(landmarks, X.shape[0])
        self.X_L = np.asarray(X[self.lm], dtype=np.float64)
        self.Phi, self.K_mm, _ = lm_._blocks(kernel, X, y, landmarks, held, **kw)
        self.y, self.a, self.cost = np.asarray(y, dtype=np.float64), a, cost
        self.result = fit(self.Phi, self.K_mm, self.y, a, cost, tol, max_iter, start, halving, step)
        self.beta, self.rho = self.result["beta"], self.result["rho"]
        self.cond = self.result["cond"]

    def decision_values(self, points, beta=None, rho=None):
        return rm.decision_values(self.kernel, self.X_L, self.beta if beta is None else beta, self.rho if rho is None else rho, points, **self.kw)[0]

    def cond_range(self):
        """cond of the last solve's M on the range of Phi (reduced_model.range_tolerance: the linear kernel with more landmarks than features)."""
        M, m = self.result["M"], self.Phi.shape[1]
        ev = np.sort(np.linalg.eigvalsh(M + self.result["nu"] * np.eye(m)))[::-1]
        return float(ev[0] / ev[np.linalg.matrix_rank(self.Phi) - 1])


def e_model(case, cost, points, tol=1e-12):
    """max |eta_normal_equations - eta_stacked| / max |eta_stacked| over ``points``: what the normal equations cost against a Newton iteration that solves every step by
    SVD least squares on the stacked matrix."""
    args = (case["kernel"], case["X"], case["y"], cost, case["landmarks"])
    f = LogisticModel(*args, held=case["held"], tol=tol, **case["kw"]).decision_values(points)
    g = LogisticModel(*args, held=case["held"], tol=tol, step=stacked_step, **case["kw"]).decision_values(points)
    return float(np.max(np.abs(f - g)) / np.max(np.abs(g)))


# ---- the inputs: reduced_model.blobs(N, d, 2, seed 7, spread), labels -1 / +1, landmarks from pcg_model.draw_landmarks ----
CASES = [
    ("rbf_600x4", "rbf", 600, 4, 1.0, dict(gamma=0.5), 32),
    ("rbf_777x5", "rbf", 777, 5, 0.6, dict(gamma=0.2), 64),
    ("poly_600x8", "polynomial", 600, 8, 0.5, dict(gamma=1.0 / 8, coef0=1.0, degree=3), 48),
    ("linear_300x6", "linear", 300, 6, 0.5, dict(gamma=1.0), 8),
]
COSTS = (1.0, 100.0)
CASE_NAMES = [row[0] for row in CASES]
HELD_OUT_SEED, HELD_OUT = 22, 200
# e_model at tol 1e-12 as a float64 run of these formulas gave it, for the record (name, cost): the host test asserts the order of magnitude
RECORDED = {("rbf_600x4", 1.0): 3.4e-14, ("rbf_600x4", 100.0): 1.7e-13, ("rbf_777x5", 1.0): 4.2e-13, ("rbf_777x5", 100.0): 1.3e-12, ("poly_600x8", 1.0): 3.7e-13,
            ("poly_600x8", 100.0): 1.7e-12, ("linear_300x6", 1.0): 2.5e-14, ("linear_300x6", 100.0): 1.9e-10}


def fit_tolerance(model: LogisticModel, e: float, f, linear: bool = False):
    """The bound of the GPU tests on decision values: 8 x max(e_model, cond(M_last) eps64) x max |eta|; the linear case, where M is singular by construction, takes the
    condition number on the range of Phi (reduced_model.range_tolerance)."""
    cond = model.cond_range() if linear else model.cond
    return 8.0 * max(e, cond * EPS64) * float(np.max(np.abs(f)))


def case(name: str, dtype=np.float64):
    for row in CASES:
        if row[0] == name:
            _, kernel, N, d, spread, kw, rank = row
            X, labels = rm.blobs(N, d, 2, 7, spread, dtype)
            y = np.where(labels == 1, 1.0, -1.0).astype(dtype)
            kw = rm.rounded_parameters(dtype, **kw)
            points = rm.blobs(HELD_OUT, d, 2, 7, 2.0 * spread, dtype)[0]  # (the same centres, wider: points on both sides of the boundary)
            return dict(name=name, dtype=np.dtype(dtype), X=X, y=y, kernel=kernel, kw=kw, landmarks=pm.draw_landmarks(N, rank, pm.LANDMARK_SEED), points=points,
                        held=rm.held_data(kernel, X, **kw))
    raise KeyError(name)
