"""The numpy model of the landmark selection (plssvm_amd/csrc/lssvm_select.hip is the device side): the pivots of a partial Cholesky factorisation
of the kernel matrix over a candidate set, chosen greedily or at random in proportion to the residual diagonal (randomly pivoted Cholesky), statement for statement as
include/plssvm_amd.h gives the algorithm -- the sums of d over blocks of 256 candidates added in ascending block order, splitmix64 from 0x243F6A8885A308D3 ^ seed.

Everything is float64.  The kernel function is evaluated from the data as given, features summed ascending; the tests hand over the data as the problem holds it
(reduced_model.held_data) where that differs by more than float64 roundings.  Not collected by pytest (no test_ prefix); tests/test_landmark_select_host.py checks the
model, tests/test_gpu_select_landmarks.py the device against it.
"""

from __future__ import annotations

import numpy as np

import pcg_model as pm
import reduced_model as rm

EPS64 = pm.EPS64
MAX_RANK = 1024
BLOCK = 256
MASK = (1 << 64) - 1
METHODS = ("greedy", "rpcholesky")


def candidates(N: int, pool: int):
    """Point indices of the candidates: all points in order (``pool`` 0) or the first ``pool`` entries of the library's fixed shuffle."""
    return np.arange(N, dtype=np.int64) if pool == 0 else rm.library_landmarks(N, pool).astype(np.int64)


def kernel_column(kernel: str, X, xp, gamma: float, coef0: float = 0.0, degree: int = 3):
    """k(x_i, xp) for every row of X: the sum over the features in ascending order, then the epilogue of the landmark block."""
    X = np.asarray(X, dtype=np.float64)
    xp = np.asarray(xp, dtype=np.float64)
    acc = np.zeros(X.shape[0])
    for f in range(X.shape[1]):
        acc += (X[:, f] - xp[f]) ** 2 if kernel == "rbf" else X[:, f] * xp[f]
    if kernel == "rbf":
        return np.exp(-gamma * acc)
    if kernel == "polynomial":
        base, k = gamma * acc + coef0, np.ones(X.shape[0])
        for _ in range(abs(degree)):
            k = k * base
        return 1.0 / k if degree < 0 else k
    return gamma * acc


def kernel_diagonal(kernel: str, X, gamma: float, coef0: float = 0.0, degree: int = 3):
    X = np.asarray(X, dtype=np.float64)
    acc = np.zeros(X.shape[0])
    for f in range(X.shape[1]):
        acc += (X[:, f] - X[:, f]) ** 2 if kernel == "rbf" else X[:, f] * X[:, f]
    if kernel == "rbf":
        return np.exp(-gamma * acc)
    if kernel == "polynomial":
        base, k = gamma * acc + coef0, np.ones(X.shape[0])
        for _ in range(abs(degree)):
            k = k * base
        return 1.0 / k if degree < 0 else k
    return gamma * acc


class Selection:
    """The state of a selection, one step at a time: :meth:`propose` chooses the pivot of the next step (None at the stop), :meth:`apply` takes the step with a pivot --
    the proposed one, or another (the device's, where the model's own margin excuses a difference).  Positions are candidate positions; ``cand`` maps them to points."""

    def __init__(self, kernel: str, X, method: str, pool: int = 0, seed: int = 0, tol: float = 0.0, **kw):
        if method not in METHODS:
            raise ValueError(method)
        X = np.asarray(X)
        self.kernel, self.kw, self.method, self.tol = kernel, kw, method, float(tol)
        self.cand = candidates(X.shape[0], pool)
        self.Xc = np.asarray(X, dtype=np.float64)[self.cand]
        self.n = self.cand.size
        self.d = kernel_diagonal(kernel, self.Xc, **kw)
        self.d0 = float(self.d.max())
        self.state = 0x243F6A8885A308D3 ^ (int(seed) & MASK)
        self.F = []           # rows of the factor, each n doubles
        self.pivots = []      # candidate positions
        self.trace = []       # S after every step
        self.S0 = self.total()

    def next_u(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & MASK
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        z ^= z >> 31
        return float(z >> 11) * 2.0 ** -53

    def block_sums(self):
        return [float(np.sum(self.d[b:b + BLOCK])) for b in range(0, self.n, BLOCK)]

    def total(self):
        S = 0.0
        for s in self.block_sums():  # ascending block order
            S += s
        return S

    def greedy(self):
        """(position, margin): the largest d, among equal values the smallest position; the gap to the second best over d0."""
        p = int(np.argmax(self.d))  # (the first of equal maxima)
        others = np.delete(self.d, p)
        gap = (self.d[p] - others.max()) / self.d0 if others.size else 1.0
        return p, float(gap)

    def propose(self):
        """``(position, margin)`` of the next step's pivot, or ``(None, 0.0)`` where the stop test fires.  Draws u for rpcholesky."""
        p, margin = self.greedy()
        if self.method == "rpcholesky":
            S = self.total()
            t = self.next_u() * S
            prefix, hit = 0.0, None
            for b, s in enumerate(self.block_sums()):
                if prefix + s > t:
                    run = np.cumsum(self.d[b * BLOCK:(b + 1) * BLOCK])  # sequential, ascending
                    inside = np.flatnonzero(run > t - prefix)
                    if inside.size and self.d[b * BLOCK + inside[0]] > 0.0:
                        hit = b * BLOCK + int(inside[0])
                        lower = prefix + (run[inside[0] - 1] if inside[0] > 0 else 0.0)
                        upper = prefix + run[inside[0]]
                        margin = float(min(t - lower, upper - t) / S)
                    break
                prefix += s
            if hit is not None:
                p = hit
        if self.d[p] <= max(self.tol, 64.0 * EPS64) * self.d0:
            return None, 0.0
        return p, margin

    def apply(self, p: int):
        p = int(p)
        dp = self.d[p]
        c = kernel_column(self.kernel, self.Xc, self.Xc[p], **self.kw)
        s = np.zeros(self.n)
        for row in self.F:  # t ascending
            s += row * row[p]
        f = (c - s) / np.sqrt(dp)
        self.d = np.maximum(self.d - f * f, 0.0)
        self.d[p] = 0.0
        self.F.append(f)
        self.pivots.append(p)
        self.trace.append(self.total())

    def run(self, rank: int):
        for _ in range(rank):
            p, _ = self.propose()
            if p is None:
                break
            self.apply(p)
        return self

    @property
    def rank_found(self):
        return len(self.pivots)

    @property
    def landmarks(self):
        """The pivots as point indices, in the order they were chosen."""
        return self.cand[np.asarray(self.pivots, dtype=np.int64)].astype(np.uint64)

    def residual(self, N: int):
        """The final d per POINT: NaN for points that were not candidates."""
        out = np.full(N, np.nan)
        out[self.cand] = self.d
        return out


def select(kernel: str, X, rank: int, method: str, pool: int = 0, seed: int = 0, tol: float = 0.0, **kw):
    return Selection(kernel, X, method, pool=pool, seed=seed, tol=tol, **kw).run(rank)


def nystrom_residual(kernel: str, X, points, pivots, **kw):
    """``(diag(K - K[:, P] K[P, P]^-1 K[P, :]) over the rows `points`, cond(K_PP))`` from the closed form: float64, an eigendecomposition of K_PP with eigenvalues below
    eps64 times the largest dropped (the pseudo-inverse: K_PP of duplicated or rank-exhausting pivots is singular)."""
    X = np.asarray(X, dtype=np.float64)
    P = np.asarray(pivots, dtype=np.int64)
    K_nP = pm.kernel_matrix(kernel, X[np.asarray(points, dtype=np.int64)], X[P], **kw)
    K_PP = pm.kernel_matrix(kernel, X[P], X[P], **kw)
    w, V = np.linalg.eigh(0.5 * (K_PP + K_PP.T))
    keep = w > EPS64 * w.max() * P.size
    proj = (K_nP @ V[:, keep]) / np.sqrt(w[keep])
    diag = np.array([float(pm.kernel_matrix(kernel, X[i:i + 1], X[i:i + 1], **kw)[0, 0]) for i in np.asarray(points, dtype=np.int64)])
    return diag - (proj * proj).sum(axis=1), float(w.max() / w[keep].min())


def nystrom_trace(kernel: str, X, landmarks, **kw):
    """The trace of the Nystrom residual over ALL points for the given landmarks (what the issue's tables list)."""
    r, _ = nystrom_residual(kernel, X, np.arange(np.asarray(X).shape[0]), landmarks, **kw)
    return float(np.maximum(r, 0.0).sum())


# ---- the two data recipes on which a rule wins, and the kernels they are used with (N = 777, C = 100) ----
def clusters(seed: int, N: int = 777, dtype=np.float64):
    """One cluster of 700 points and eleven of 7: centres N(0, 3^2) in 5 dimensions, spread 0.3, rows permuted."""
    rng = np.random.default_rng(seed)
    sizes = [700] + [7] * 11
    centres = rng.normal(0.0, 3.0, size=(len(sizes), 5))
    X = np.vstack([c + 0.3 * rng.normal(size=(s, 5)) for c, s in zip(centres, sizes)])
    X = X[rng.permutation(X.shape[0])][:N]
    y = np.where(rng.random(X.shape[0]) < 0.5, -1.0, 1.0)
    y[0], y[-1] = 1.0, -1.0
    return X.astype(dtype), y.astype(dtype)


def heavy_rows(seed: int, N: int = 777, dtype=np.float64):
    """Uniform [-1, 1]^8 with each row scaled by exp(N(0, 1))."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, size=(N, 8)) * np.exp(rng.normal(size=(N, 1)))
    y = np.where(rng.random(N) < 0.5, -1.0, 1.0)
    y[0], y[-1] = 1.0, -1.0
    return X.astype(dtype), y.astype(dtype)


RECIPES = {
    # name: (data, kernel, kernel parameters, rank, the rule that wins, trace of the rule <= factor x trace of the fixed shuffle)
    "clusters": (clusters, "rbf", dict(gamma=0.5), 64, "rpcholesky", 0.7),
    "heavy_rows": (heavy_rows, "polynomial", dict(gamma=1.0 / 8, coef0=1.0, degree=2), 16, "greedy", 0.5),
}
RECIPE_COST = 100.0
