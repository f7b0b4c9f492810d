"""The numpy model of the (gamma, cost) grid of the fixed-size LS-SVM (k_landmark_acc / k_landmark_product / k_kernel_values of
plssvm_amd/csrc/lssvm_landmark.hip.hpp and lssvm_reduced.hip are the device side).

A cell (g, s) of the grid is the (weighted) leave-one-out model of tests/reduced_loo_model.py / tests/reduced_weighted_model.py at the cost C_s with the kernel's gamma
replaced by gamma_g -- evaluated ON THE DATA AS THE PROBLEM HOLDS IT.  The problem was created with its OWN gamma, and that gamma decides how the data is held
(reduced_model.held_data: a float32 rbf problem off the direct form holds x' = scale (x - mean) with scale = float32(sqrt(2 gamma_own log2 e))); the grid then evaluates
gamma_g with the kernel parameter gamma'_g = gamma_g / scale^2 on x'.  Everywhere else the data is held as given up to roundings of float64 size and gamma'_g = gamma_g.

What the gammas share: D[i, l] = sum_f (a_f - b_f)^2 (rbf) or sum_f a_f b_f (polynomial) over the held features.  :func:`direct_sums` is that sum as written;
:func:`expanded_sums` is the form the matrix-core path takes for rbf, n_i + n_l - 2 a . b clamped at 0 and exactly 0 at the landmark itself; :func:`expansion_bound` is
the bound of their difference (the module docstring of tests/test_gpu_reduced_grid.py derives it).  Everything is float64.  Not collected by pytest (no test_ prefix);
tests/test_reduced_grid_host.py checks the model, tests/test_gpu_reduced_grid.py the device against it.  The sibling models are imported, not edited.
"""

from __future__ import annotations

import numpy as np

import reduced_loo_model as lm
import reduced_model as rm
import reduced_weighted_model as wm

EPS64 = rm.EPS64
MAX_CELLS = 64


def padded_features(d: int, dtype) -> int:
    """ldx of the resident data (padded_features of plssvm_amd/csrc/lssvm_problem.hip.hpp): the k-chunk is 32 features in float32, 16 in float64."""
    f32 = np.dtype(dtype) == np.float32
    kc = 32 if f32 else 16
    up = lambda v, m: (v + m - 1) // m * m  # noqa: E731
    ldx = up(d, kc)
    if not f32 and ldx > 16 * kc:
        return up(d, 64)
    return up(d, 2 * kc) if (4 if f32 else 8) * kc < ldx <= 16 * kc else ldx


def held_for_grid(kernel: str, X, own_kw: dict, gammas, direct: bool = False):
    """``(X_held, [kernel parameters of gamma_g on X_held])``: reduced_model.held_data of the problem's OWN parameters, every gamma_g (rounded to the data's type, as the
    library rounds it) divided by the square of the factor the held data carries."""
    X = np.asarray(X)
    held, held_kw = rm.held_data(kernel, X, direct=direct, **own_kw)
    own = float(np.dtype(X.dtype).type(own_kw["gamma"])) if X.dtype == np.float32 else float(own_kw["gamma"])
    scale2 = own / held_kw["gamma"]  # 1.0 where the data is held as given
    rounded = [float(np.dtype(X.dtype).type(g)) for g in gammas]
    return held, [dict(held_kw, gamma=g / scale2) for g in rounded]


def given_kw(own_kw: dict, dtype, gamma: float):
    """The kernel parameters of gamma_g on the data as given: what a model of the cell carries."""
    return dict(own_kw, gamma=float(np.dtype(dtype).type(gamma)))


class GridModel:
    """``cells[g][s]``: reduced_loo_model.LooModel (``w`` None) or reduced_weighted_model.WeightedLooModel at (gamma_g, C_s); ``e[g][s]``: the cell's e_loo against the
    backward-stable route of its sibling module.  ``held``: the held data and, per gamma, its kernel parameters."""

    def __init__(self, kernel: str, X, Y, landmarks, gammas, costs, own_kw: dict, w=None, direct: bool = False, with_e: bool = True):
        if len(gammas) * len(costs) > MAX_CELLS or len(gammas) == 0:
            raise ValueError("bad grid")
        self.held = held_for_grid(kernel, X, own_kw, gammas, direct)
        X_held, kws = self.held
        self.cells, self.e = [], []
        for kw_g in kws:
            row, e_row = [], []
            for cost in costs:
                if w is None:
                    cell = lm.LooModel(kernel, X, Y, cost, landmarks, held=(X_held, kw_g), **kw_g)
                    e = lm.e_loo(cell, lm.stable(kernel, X, Y, cost, landmarks, held=(X_held, kw_g), **kw_g)[2]) if with_e else 0.0
                else:
                    cell = wm.WeightedLooModel(kernel, X, Y, cost, landmarks, w, held=(X_held, kw_g), **kw_g)
                    e = wm.e_loo(cell, wm.stable(kernel, X, Y, cost, landmarks, w, held=(X_held, kw_g), **kw_g)[2]) if with_e else 0.0
                row.append(cell)
                e_row.append(e)
            self.cells.append(row)
            self.e.append(e_row)


def direct_sums(kernel: str, X_held, landmarks):
    """D[i, l] as written: sum_f (a_f - b_f)^2 (rbf) or sum_f a_f b_f (any other kernel), float64."""
    A = np.asarray(X_held, dtype=np.float64)
    B = A[np.asarray(landmarks, dtype=np.int64)]
    if kernel == "rbf":
        diff = A[:, None, :] - B[None, :, :]
        return (diff * diff).sum(axis=2)
    return A @ B.T


def expanded_sums(kernel: str, X_held, landmarks):
    """D[i, l] as the matrix-core path forms it: the dot products, and for rbf n_i + n_l - 2 a . b clamped at 0 and exactly 0 where i is the landmark itself."""
    A = np.asarray(X_held, dtype=np.float64)
    at = np.asarray(landmarks, dtype=np.int64)
    dot = A @ A[at].T
    if kernel != "rbf":
        return dot
    n = (A * A).sum(axis=1)
    D = np.maximum((n[:, None] + n[at][None, :]) - 2.0 * dot, 0.0)
    D[at, np.arange(at.size)] = 0.0
    return D


def expansion_bound(kernel: str, X_held, landmarks, ldx: int):
    """|dD| of the matrix-core path: (ldx + 4) eps64 (n_i + n_l + 2 sum_f |a_f b_f|) for rbf, (ldx + 2) eps64 sum_f |a_f b_f| for the dot products."""
    A = np.asarray(X_held, dtype=np.float64)
    at = np.asarray(landmarks, dtype=np.int64)
    absdot = np.abs(A) @ np.abs(A[at]).T
    if kernel != "rbf":
        return (ldx + 2) * EPS64 * absdot
    n = (A * A).sum(axis=1)
    return (ldx + 4) * EPS64 * (n[:, None] + n[at][None, :] + 2.0 * absdot)


def kernel_values(kernel: str, D, kw: dict):
    """Phi from D: landmark_kernel_value of plssvm_amd/csrc/lssvm_landmark.hip.hpp."""
    if kernel == "rbf":
        return np.exp(-kw["gamma"] * D)
    base = kw["gamma"] * D + kw["coef0"]
    k = base ** abs(int(kw["degree"]))
    return 1.0 / k if kw["degree"] < 0 else k


def values_error(kernel: str, D, dD, kw: dict):
    """|dPhi| that |dD| becomes: gamma' k dD (rbf) or |degree| gamma' |base|^(|degree| - 1) dD (polynomial; a negative degree: times k^2, the derivative of 1 / p)."""
    if kernel == "rbf":
        return kw["gamma"] * np.exp(-kw["gamma"] * D) * dD
    base = np.abs(kw["gamma"] * D + kw["coef0"])
    deg = abs(int(kw["degree"]))
    slope = deg * kw["gamma"] * base ** (deg - 1) * dD
    return slope / base ** (2 * deg) if kw["degree"] < 0 else slope
