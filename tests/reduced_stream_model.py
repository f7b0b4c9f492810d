"""The numpy model of the fixed-size LS-SVM from a stream of chunks (ReducedStream of plssvm_amd/csrc/lssvm_reduced.hip is the device side).

What a stream keeps of its rows is S~ = Pt^T diag(w) Pt for Pt = [Phi | 1 | y_0 ... y_{k-1}], additive over rows: the state of a concatenation is the sum of the
chunks' states, a merge of shard states is a sum, and "total minus a fold" is the state of the other folds.  The fit reads S~ and K_mm only (:func:`solve_state`: the
formulas of reduced_weighted_model.WeightedReducedModel with W = S~[m][m]).

The landmarks of a stream are ROWS held on their own, not indices.  The sibling models (reduced_model, reduced_weighted_model, reduced_loo_model, reduced_grid_model;
imported, not edited) take indices into the data: :func:`with_landmark_rows` appends the landmark rows at weight 0 -- such a row takes no part in the fit -- so that they
have indices; where the landmarks ARE streamed rows their own indices serve.

Everything is evaluated on the data as the stream stages it: ``X.astype(float64) - centre`` (:func:`held`), the centre the landmarks' mean for rbf (summed in ascending
row order, in double) and 0 otherwise -- read back from the handle by the GPU tests, formed by :func:`centre_of` here.  rbf is translation invariant: the function is
the one on the data as given.  Not collected by pytest (no test_ prefix); tests/test_reduced_stream_host.py checks the model, tests/test_gpu_reduced_stream.py the device
against it.
"""

from __future__ import annotations

import numpy as np

import pcg_model as pm
import reduced_grid_model as gm
import reduced_loo_model as lm
import reduced_model as rm
import reduced_weighted_model as wm

EPS64 = rm.EPS64


def centre_of(kernel: str, landmark_rows):
    """c_f = (sum_l X_L[l][f], l ascending, in double) / m for rbf; zeros for any other kernel."""
    XL = np.asarray(landmark_rows).astype(np.float64)
    acc = np.zeros(XL.shape[1])
    if kernel != "rbf":
        return acc
    for row in XL:
        acc = acc + row
    return acc / XL.shape[0]


def held(X, centre):
    """The rows as the stream stages them: (double) x_f - c_f."""
    return np.asarray(X).astype(np.float64) - np.asarray(centre, dtype=np.float64)[None, :]


def padded_features(d: int) -> int:
    """ldx of a stream: d rounded up to 16, whatever the dtype."""
    return (d + 15) // 16 * 16


def phi(kernel: str, X_held, XL_held, **kw):
    """Phi = K(X, X_L) on the staged rows, N x m."""
    return pm.kernel_matrix(kernel, X_held, XL_held, **kw)


def augmented(kernel: str, X_held, Y, XL_held, **kw):
    Y2 = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    return np.hstack([phi(kernel, X_held, XL_held, **kw), np.ones((np.asarray(X_held).shape[0], 1)), Y2.T])


def state(kernel: str, X_held, Y, XL_held, w=None, **kw):
    """S~ of these rows, (m + 1 + k)^2."""
    P = augmented(kernel, X_held, Y, XL_held, **kw)
    if w is None:
        return P.T @ P
    return P.T @ (np.asarray(w, dtype=np.float64)[:, None] * P)


def solve_state(S, K_mm, k: int, cost: float):
    """``(betas[k, m], rhos[k], nu, cond)`` from S~ and K_mm alone: M = S - s s^T / W + K_mm / C with W = S~[m][m], the jitter rule, the solves."""
    m = S.shape[0] - 1 - k
    W = S[m, m]
    s = S[m, :m]
    M, L, nu, _ = wm._factor(S[:m, :m] - np.outer(s, s) / W + K_mm / cost)
    cond = float(np.linalg.cond(M + nu * np.eye(m)))
    betas, rhos = np.zeros((k, m)), np.zeros(k)
    for c in range(k):
        t, eta = S[m + 1 + c, :m], S[m + 1 + c, m]
        betas[c] = np.linalg.solve(L.T, np.linalg.solve(L, t - s * eta / W))
        rhos[c] = -(eta - s @ betas[c]) / W
    return betas, rhos, nu, cond


def decision_values(kernel: str, XL_held, betas, rhos, points_held, **kw):
    return rm.decision_values(kernel, XL_held, betas, rhos, points_held, **kw)


def with_landmark_rows(X_held, Y, w, XL_held):
    """``(X', Y', w', landmark indices)``: the landmark rows appended at weight 0 (right-hand side 0), for the index-based sibling models."""
    X_held, XL_held = np.asarray(X_held, dtype=np.float64), np.asarray(XL_held, dtype=np.float64)
    N, m = X_held.shape[0], XL_held.shape[0]
    Y2 = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    w = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    return (np.vstack([X_held, XL_held]), np.hstack([Y2, np.zeros((Y2.shape[0], m))]), np.concatenate([w, np.zeros(m)]), np.arange(N, N + m, dtype=np.uint64))


def expanded_sums(kernel: str, X_held, XL_held):
    """D[i, l] as k_cross_product forms it: the dot products, and for rbf n_i + n_l - 2 a . b clamped at 0.  No "the landmark itself" test: a streamed row carries no
    index."""
    A, B = np.asarray(X_held, dtype=np.float64), np.asarray(XL_held, dtype=np.float64)
    dot = A @ B.T
    if kernel != "rbf":
        return dot
    return np.maximum(((A * A).sum(axis=1)[:, None] + (B * B).sum(axis=1)[None, :]) - 2.0 * dot, 0.0)


def direct_and_bound(kernel: str, X_held, XL_held, ldx: int):
    """``(reduced_grid_model.direct_sums, reduced_grid_model.expansion_bound)`` for landmark ROWS: N x m each."""
    A, B = np.asarray(X_held, dtype=np.float64), np.asarray(XL_held, dtype=np.float64)
    both = np.vstack([A, B])
    at = np.arange(A.shape[0], A.shape[0] + B.shape[0])
    return gm.direct_sums(kernel, both, at)[:A.shape[0]], gm.expansion_bound(kernel, both, at, ldx)[:A.shape[0]]


__all__ = ["centre_of", "held", "padded_features", "phi", "augmented", "state", "solve_state", "decision_values", "with_landmark_rows", "expanded_sums", "direct_and_bound", "lm", "wm", "gm", "rm"]
