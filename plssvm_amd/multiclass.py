"""One-vs-all multi-class classification on top of the binary LS-SVM (no counterpart in the reference version this package mirrors, which is binary only).

A model of ``k`` classes is ``k`` binary classifiers over the SAME training points: classifier ``c`` is trained on ``y = +1`` for class ``c`` and ``-1`` for every
other class, with the same point weights in every classifier.  Its decision value is ``f_c(x) = sum_i alpha[c, i] k(x_i, x) - rho[c]``; the predicted class is
``classes[argmax_c f_c(x)]``, ties to the lowest index.  All ``k`` weight vectors share their support vectors, which is what the backend's
``solve_systems_of_linear_equations`` (one resident problem), ``predict_values_multi`` (one preparation, two weight vectors per pass over the Gram tiles) and the
resident predictor of a one-vs-all model (``MI355CSVM.decision_values_resident``: the model stays in HBM across calls) use.
"""

from __future__ import annotations

import numpy as np

from .exceptions import InvalidParameterError

__all__ = ["OneVsAllModel", "one_vs_all_targets", "fit_one_vs_all", "decision_values", "predict_classes"]


class OneVsAllModel:
    """``classes[k]``, ``support_vectors[n, d]``, ``alpha[k, n]``, ``rho[k]``, the resolved kernel parameters and, for the linear kernel, the cached ``w[k, d]``."""

    def __init__(self, params, classes, support_vectors, alpha, rho, infos):
        self.params, self.classes, self.support_vectors, self.alpha, self.rho, self.infos = params, classes, support_vectors, alpha, rho, infos
        self.w = None


def one_vs_all_targets(classes, y, dtype) -> np.ndarray:
    """``B[c, i] = +1`` where ``y[i] == classes[c]``, else ``-1``: the right-hand sides of the ``k`` classifiers."""
    classes, y = np.asarray(classes), np.asarray(y)
    return np.where(y[None, :] == classes[:, None], 1.0, -1.0).astype(dtype)


def fit_one_vs_all(svm, params, X, y, classes, epsilon: float, max_iter: int | None = None, weights=None) -> OneVsAllModel:
    """Train the ``len(classes)`` classifiers with the backend object ``svm`` (a :class:`plssvm_amd.csvm.CSVM`).  ``weights``: one value >= 0 per point, the same in every
    classifier; points of weight 0 take no part in the solve or the model (as ``CSVM.fit`` treats them)."""
    if epsilon <= 0.0:
        raise InvalidParameterError(f"epsilon must be less than 0.0, but is {epsilon}!")  # csvm.hpp:283 (message verbatim)
    if max_iter is not None and max_iter <= 0:
        raise InvalidParameterError(f"max_iter must be greater than 0, but is {max_iter}!")  # csvm.hpp:291
    X, y = np.asarray(X), np.asarray(y)
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != y.shape:
            raise InvalidParameterError(f"The number of data points ({y.size}) and the number of sample weights ({w.size}) must be the same!")
        if not (np.all(np.isfinite(w)) and np.all(w >= 0.0)):
            raise InvalidParameterError("Every sample weight must be finite and greater than or equal to 0.0!")
        keep = np.flatnonzero(w > 0.0)
        if keep.size < 2 or len(set(y[keep].tolist())) < 2:
            raise InvalidParameterError(f"The points of weight > 0 ({keep.size} of {w.size}) must include at least two points of two different classes!")
        if keep.size < w.size:
            X, y = X[keep], y[keep]
        weights = np.ascontiguousarray(w[keep])
    X = np.ascontiguousarray(X)
    resolved = params.resolved(X.shape[1])
    B = one_vs_all_targets(classes, y, X.dtype)
    alpha, rho, infos = svm.solve_systems_of_linear_equations(resolved, X, B, epsilon, X.shape[0] if max_iter is None else max_iter, sample_weight=weights)
    return OneVsAllModel(resolved, np.asarray(classes), X, np.asarray(alpha), np.asarray(rho), infos)


def decision_values(svm, model: OneVsAllModel, X) -> np.ndarray:
    """``f[i, c]`` of every row of ``X``: shape ``(n, k)``.  A backend object that offers ``decision_values_resident`` (the MI355X backend) keeps the model in HBM across
    calls; every other one runs its ``predict_values_multi``."""
    resident = getattr(svm, "decision_values_resident", None)
    if resident is not None:
        return resident(model, X)
    values, w = svm.predict_values_multi(model.params, model.support_vectors, model.alpha, model.rho, model.w, np.asarray(X, dtype=model.support_vectors.dtype))
    if w is not None:
        model.w = w
    return values


def predict_classes(classes, values) -> np.ndarray:
    """``classes[argmax_c values[i, c]]``; an exact tie goes to the lowest class index (numpy's argmax)."""
    return np.asarray(classes)[np.argmax(values, axis=1)]
