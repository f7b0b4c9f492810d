"""scikit-learn ``SVC`` on top of CSVM, the counterpart of the reference's bindings/Python/sklearn.cpp: the same keywords, parameters and fitted attributes,
with the LS-SVM solver behind ``fit``.  Beyond the reference: ``class_weight`` and ``sample_weight`` (the weighted LS-SVM system), ``get_params(deep)`` /
``set_params`` in scikit-learn's contract (``clone``, ``GridSearchCV``, ``Pipeline``), ``dual_coef_`` / ``intercept_`` / ``coef_``, ``decision_function``, and more
than two classes (one-vs-all, :mod:`plssvm_amd.multiclass`).

An estimator that duck-types scikit-learn's protocol: scikit-learn itself is not needed to use it."""

from __future__ import annotations

import numpy as np

from . import _capi
from . import csvm as _csvm
from . import multiclass as _multiclass
from .csvm import make_csvm
from .data_set import DataSet
from .exceptions import InvalidParameterError
from .model import Model
from .parameter import Parameter

__all__ = ["SVC", "fit_cost_path", "cost_path_scores"]

# the keywords of the reference's constructor that it rejects (sklearn.cpp:52, :73-108): the same words here
_NOT_IMPLEMENTED = ("shrinking", "probability", "cache_size", "decision_function_shape", "break_ties", "random_state")
# what get_params reports: the reference's keys (sklearn.cpp:208-228) + class_weight + real_type
_PARAM_NAMES = ("C", "kernel", "degree", "gamma", "coef0", "tol", "verbose", "max_iter", "class_weight", "real_type")


def _not_fitted(name):
    return AttributeError(f"'SVC' object has no attribute '{name}'")


def _fitted_attribute(name, doc):
    def get(self):
        if self._fit is None:
            raise _not_fitted(name)
        return self._fit[name]
    return property(get, doc=doc)


def _not_implemented(name, what="attribute"):
    def get(self):
        raise AttributeError(f"'SVC' object has no {what} '{name}' (not implemented)")
    return property(get)


def _set_verbosity(verbose) -> None:
    _csvm.verbosity = "full" if bool(verbose) else "quiet"  # sklearn.cpp:88-94


class SVC:
    """C-support vector classification with the LS-SVM solver.  ``gamma``: a number, or any string for the PLSSVM default 1 / n_features.
    More than two classes are classified ONE-VS-ALL -- unlike scikit-learn's ``SVC``, which trains one-vs-one: one classifier per class (that class against the rest) over
    the same training points, the predicted class is the one of the largest decision value (ties: the lowest class index).  The fitted attributes then have one row per
    class: ``dual_coef_ (k, n_SV)``, ``intercept_ (k,)``, ``coef_ (k, n_features)``, ``n_iter_ (k,)``, ``decision_function(X) (n, k)`` (scikit-learn's "ovr" shape).
    ``class_weight``: None, ``"balanced"`` (n_samples / (n_classes * count(class))) or a dict {label: weight}; with ``sample_weight`` in ``fit``, point i is
    regularised by 1 / (C * sample_weight[i] * class_weight[y[i]]) -- the weighted LS-SVM system -- and points of weight 0 take no part."""

    def __init__(self, C=1.0, kernel="rbf", degree=3, gamma="scale_features", coef0=0.0, tol=1e-3, verbose=False, max_iter=-1, class_weight=None, real_type=np.float64,
                 **kwargs):
        for name in kwargs:
            if name in _NOT_IMPLEMENTED:
                raise AttributeError(f"The '{name}' parameter for a call to the 'SVC' constructor is not implemented yet!")
            raise TypeError(f"SVC.__init__() got an unexpected keyword argument '{name}'")
        # stored verbatim: sklearn.base.clone checks that the constructor keeps what get_params hands it
        self.C, self.kernel, self.degree, self.gamma, self.coef0, self.tol = C, kernel, degree, gamma, coef0, tol
        self.verbose, self.max_iter, self.class_weight, self.real_type = verbose, max_iter, class_weight, real_type
        _set_verbosity(verbose)
        self._svm = None
        self._model = None
        self._fit = None

    # ------------------------------------------------------------------ parameters (scikit-learn's estimator contract)
    def get_params(self, deep=True):
        """Parameters for this estimator (no nested estimators: ``deep`` changes nothing)."""
        return {name: getattr(self, name) for name in _PARAM_NAMES}

    def set_params(self, **params):
        """Set the parameters of this estimator; returns self.  An unknown key raises ValueError, the keywords the reference rejects raise AttributeError."""
        for name in params:
            if name in _NOT_IMPLEMENTED:
                raise AttributeError(f"The '{name}' parameter for a call to the 'SVC' constructor is not implemented yet!")
            if name not in _PARAM_NAMES:
                raise ValueError(f"Invalid parameter {name!r} for estimator SVC. Valid parameters are: {sorted(_PARAM_NAMES)!r}.")
        for name, value in params.items():
            setattr(self, name, value)
        if "verbose" in params:
            _set_verbosity(params["verbose"])
        return self

    _estimator_type = "classifier"  # (scikit-learn before 1.6)

    def __sklearn_tags__(self):
        """What scikit-learn's tooling asks of an estimator (is_classifier: stratified folds in GridSearchCV, ...); only scikit-learn calls this."""
        from sklearn.utils import ClassifierTags, Tags, TargetTags

        return Tags(estimator_type="classifier", target_tags=TargetTags(required=True), classifier_tags=ClassifierTags(multi_class=True))

    def __repr__(self):
        return "SVC(" + ", ".join(f"{k}={v!r}" for k, v in self.get_params().items()) + ")"

    def _params(self):
        if self.kernel not in ("linear", "poly", "polynomial", "rbf"):
            raise InvalidParameterError(f'The kernel "{self.kernel}" is not supported; use linear, poly or rbf')
        gamma = None if isinstance(self.gamma, str) else float(self.gamma)  # any string = the PLSSVM default 1 / n_features
        return Parameter(kernel_type=self.kernel, degree=self.degree, gamma=gamma, coef0=self.coef0, cost=self.C)

    def _class_weight(self, classes, y):
        """The multiplier of each class (scikit-learn's compute_class_weight)."""
        cw = self.class_weight
        if cw is None:
            return np.ones(len(classes))
        if isinstance(cw, str):
            if cw != "balanced":
                raise InvalidParameterError(f'class_weight must be None, "balanced" or a dict, but is "{cw}"!')
            counts = np.array([np.count_nonzero(y == c) for c in classes], dtype=np.float64)
            return y.size / (len(classes) * counts)
        if isinstance(cw, dict):
            unknown = [k for k in cw if not np.any(classes == k)]
            if unknown:
                raise InvalidParameterError(f"The classes {unknown} of class_weight are not in the training labels {list(classes.tolist())}!")
            return np.array([float(cw.get(c, 1.0)) for c in classes])
        raise InvalidParameterError(f'class_weight must be None, "balanced" or a dict, but is {cw!r}!')

    # ------------------------------------------------------------------ fit / predict / score
    def fit(self, X, y, sample_weight=None):
        """Fit the SVM model to the training data; ``sample_weight`` (one value >= 0 per point) times the class weight is the point's weight in the solve."""
        X = np.asarray(X)
        y = np.asarray(y)
        if X.ndim != 2 or y.ndim != 1 or y.shape[0] != X.shape[0]:
            raise InvalidParameterError(f"X must be a matrix and y a vector of as many labels as X has rows, but their shapes are {X.shape} and {y.shape}!")
        params = self._params()
        classes = np.array(sorted(set(y.tolist())))  # (the order of DataSet's label mapping)
        class_weight = self._class_weight(classes, y)
        weights = None
        if sample_weight is not None or self.class_weight is not None:
            sw = np.ones(y.size) if sample_weight is None else np.asarray(sample_weight, dtype=np.float64)
            if sw.shape != y.shape:
                raise InvalidParameterError(f"The number of data points ({y.size}) and the number of sample weights ({sw.size}) must be the same!")
            weights = sw * class_weight[np.searchsorted(classes, y)]
        svm = make_csvm(params=params)
        if len(classes) > 2:
            return self._fit_one_vs_all(svm, params, X, y, classes, class_weight, weights)
        data = DataSet(X, y.tolist(), real_type=self.real_type)
        max_iter = None if self.max_iter is None or self.max_iter < 0 else self.max_iter
        model = svm.fit(data, epsilon=self.tol, max_iter=max_iter, sample_weight=weights)
        return self._set_binary_fit(svm, model, data, X, y, class_weight, weights, int(svm.last_cg_info["iterations"]))

    def _set_binary_fit(self, svm, model, data, X, y, class_weight, weights, n_iter):
        """The fitted state of a two-class model (``fit``, and ``fit_cost_path`` for each cost)."""
        support = np.arange(y.size, dtype=np.int32) if weights is None else np.flatnonzero(weights > 0).astype(np.int32)
        alpha = np.asarray(model.alpha)
        sv_labels = np.asarray(model.labels())
        nonzero = alpha != 0  # the reference's counting rule (sklearn.cpp:381-410): support vectors of non-zero weight, per class
        self._svm, self._model = svm, model
        self._fit = {
            "classes_": np.array(data.different_labels()),
            "class_weight_": class_weight,
            "fit_status_": 0,
            "n_features_in_": int(X.shape[1]),
            "shape_fit_": tuple(int(v) for v in X.shape),
            "n_iter_": n_iter,
            "support_": support,
            "support_vectors_": model.support_vectors(),
            "n_support_": np.array([np.count_nonzero(nonzero & (sv_labels == c)) for c in data.different_labels()], dtype=np.int32),
            "dual_coef_": alpha.reshape(1, -1),
            "intercept_": np.array([-model.rho], dtype=alpha.dtype),
        }
        return self

    def _fit_one_vs_all(self, svm, params, X, y, classes, class_weight, weights):
        """More than two classes: one classifier per class on the same points (plssvm_amd.multiclass)."""
        max_iter = None if self.max_iter is None or self.max_iter < 0 else self.max_iter
        model = _multiclass.fit_one_vs_all(svm, params, np.ascontiguousarray(X, dtype=self.real_type), y, classes, self.tol, max_iter, weights)
        return self._set_one_vs_all_fit(svm, model, X, y, classes, class_weight, weights)

    def _set_one_vs_all_fit(self, svm, model, X, y, classes, class_weight, weights):
        """The fitted state of a one-vs-all model (``fit``, and ``fit_cost_path`` for each cost)."""
        support = np.arange(y.size, dtype=np.int32) if weights is None else np.flatnonzero(weights > 0).astype(np.int32)
        sv_labels = y[support]
        nonzero = np.any(model.alpha != 0, axis=0)  # a support vector counts where ANY classifier gives it a non-zero coefficient
        self._svm, self._model = svm, model
        self._fit = {
            "classes_": classes,
            "class_weight_": class_weight,
            "fit_status_": 0,
            "n_features_in_": int(X.shape[1]),
            "shape_fit_": tuple(int(v) for v in X.shape),
            "n_iter_": np.array([int(info["iterations"]) for info in model.infos], dtype=np.int64),
            "support_": support,
            "support_vectors_": model.support_vectors,
            "n_support_": np.array([np.count_nonzero(nonzero & (sv_labels == c)) for c in classes], dtype=np.int32),
            "dual_coef_": model.alpha,
            "intercept_": -model.rho,
        }
        return self

    def __sklearn_is_fitted__(self):
        return self._fit is not None

    def _check_fitted(self):
        if self._fit is None:
            raise AttributeError("This SVC instance is not fitted yet. Call 'fit' with appropriate arguments before using this estimator.")  # sklearn.cpp:236

    def decision_function(self, X):
        """sum_i dual_coef_[0, i] k(support_vectors_[i], x) + intercept_[0] for every row x of X (an extension: the reference's raises); more than two classes: shape
        (n, n_classes), column c the value of classifier c (class c against the rest)."""
        self._check_fitted()
        m = self._model
        if isinstance(m, _multiclass.OneVsAllModel):
            return _multiclass.decision_values(self._svm, m, X)
        values, w = self._svm.predict_values(m.params, m.support_vectors(), m.alpha, float(m.rho), m.w, np.asarray(X, dtype=self.real_type))
        if w is not None:
            m.w = w
        return values

    def predict(self, X):
        """Perform classification on samples in X."""
        classes = self.classes_
        if len(classes) > 2:
            return _multiclass.predict_classes(classes, self.decision_function(X))
        return np.where(self.decision_function(X) > 0, classes[1], classes[0])

    def score(self, X, y, sample_weight=None):
        """The (sample_weight-weighted) mean accuracy on the given test data and labels."""
        return float(np.average(self.predict(X) == np.asarray(y), weights=sample_weight))

    # ------------------------------------------------------------------ fitted attributes
    classes_ = _fitted_attribute("classes_", "The class labels, ndarray of shape (n_classes,).")
    class_weight_ = _fitted_attribute("class_weight_", "The multiplier of each class's weights, ndarray of shape (n_classes,).")
    fit_status_ = _fitted_attribute("fit_status_", "0 if correctly fitted.")
    n_features_in_ = _fitted_attribute("n_features_in_", "Number of features seen during fit.")
    shape_fit_ = _fitted_attribute("shape_fit_", "Array dimensions of the training matrix X.")
    n_iter_ = _fitted_attribute("n_iter_", "CG iterations of the solve; more than two classes: of every classifier's solve, int ndarray of shape (n_classes,).")
    support_ = _fitted_attribute("support_", "Indices of the support vectors (every point of weight > 0), ndarray of shape (n_SV,).")
    support_vectors_ = _fitted_attribute("support_vectors_", "Support vectors, ndarray of shape (n_SV, n_features).")
    n_support_ = _fitted_attribute("n_support_", "Support vectors of non-zero dual coefficient per class, ndarray of shape (n_classes,), int32.")
    dual_coef_ = _fitted_attribute("dual_coef_", "The dual coefficients alpha, ndarray of shape (1, n_SV); more than two classes: (n_classes, n_SV), row c = class c against the rest.")
    intercept_ = _fitted_attribute("intercept_", "The constant of the decision function (-rho), ndarray of shape (1,); more than two classes: (n_classes,).")

    @property
    def coef_(self):
        """The weights w of the features, ndarray of shape (1, n_features) -- more than two classes: (n_classes, n_features): linear kernel only."""
        if self._fit is None:
            raise _not_fitted("coef_")
        if self._model.params.kernel_type != 0:
            raise AttributeError("coef_ is only available when using a linear kernel")
        if "coef_" not in self._fit:
            from .backend import calculate_w
            if isinstance(self._model, _multiclass.OneVsAllModel):
                self._fit["coef_"] = np.stack([calculate_w(self._model.support_vectors, a) for a in self._model.alpha])
                return self._fit["coef_"]
            self._fit["coef_"] = calculate_w(self._model.support_vectors(), self._model.alpha).reshape(1, -1)
        return self._fit["coef_"]

    predict_proba = _not_implemented("predict_proba", "function")
    predict_log_proba = _not_implemented("predict_log_proba", "function")
    probA_ = _not_implemented("probA_")
    probB_ = _not_implemented("probB_")
    feature_names_in_ = _not_implemented("feature_names_in_")


# ---------------------------------------------------------------------------------------------------------------------
# the cost path: every C of a grid from one Krylov sequence (MI355CSVM.solve_cost_path)
# ---------------------------------------------------------------------------------------------------------------------
def _cost_path_inputs(estimator, X, y, Cs):
    if not isinstance(estimator, SVC):
        raise InvalidParameterError("estimator must be a plssvm_amd.svc.SVC")
    if estimator.class_weight is not None:
        raise InvalidParameterError("the cost path solves the unweighted system: class_weight must be None")
    X, y = np.asarray(X), np.asarray(y)
    if X.ndim != 2 or y.ndim != 1 or y.shape[0] != X.shape[0]:
        raise InvalidParameterError(f"X must be a matrix and y a vector of as many labels as X has rows, but their shapes are {X.shape} and {y.shape}!")
    return X, y, _csvm._checked_costs(Cs)


def fit_cost_path(estimator, X, y, Cs):
    """``estimator`` fitted for every ``C`` of ``Cs``: a list of fitted :class:`SVC` clones (``estimator``'s parameters with ``C`` replaced), in the order of ``Cs``.  Two
    classes: ONE call of the backend's cost path -- every cost from one multi-shift CG sequence, one pass over the Gram tiles per iteration for the whole grid.  More than
    two classes (one-vs-all): one path per class on ONE resident problem (the data uploaded and prepared once, ``MI355CSVM.solve_cost_paths``).  ``tol`` is the path's stop test (the residual in the norm of (I + 1 1^T)^-1 relative to
    the right-hand side, from x0 = 0), not that of ``fit``; ``estimator.C`` is ignored and ``estimator`` itself stays unfitted.  ``class_weight`` must be None."""
    X, y, Cs = _cost_path_inputs(estimator, X, y, Cs)
    params = estimator._params()
    classes = np.array(sorted(set(y.tolist())))
    class_weight = np.ones(len(classes))
    max_iter = None if estimator.max_iter is None or estimator.max_iter < 0 else estimator.max_iter
    svm = make_csvm(params=params)
    clones = [SVC(**{**estimator.get_params(), "C": C}) for C in Cs]
    if len(classes) > 2:
        Xr = np.ascontiguousarray(X, dtype=estimator.real_type)
        resolved = params.resolved(Xr.shape[1])
        B = _multiclass.one_vs_all_targets(classes, y, Xr.dtype)
        solved = svm.solve_cost_paths(resolved, Xr, B, Cs, estimator.tol, Xr.shape[0] if max_iter is None else max_iter)  # [class] -> (alphas[m, N], rhos[m], infos[m])
        for s, (C, clone) in enumerate(zip(Cs, clones)):
            at_cost = Parameter(kernel_type=resolved.kernel_type, degree=resolved.degree, gamma=resolved.gamma, coef0=resolved.coef0, cost=C)
            model = _multiclass.OneVsAllModel(at_cost, classes, Xr, np.stack([np.asarray(c[0][s]) for c in solved]), np.array([c[1][s] for c in solved]), [c[2][s] for c in solved])
            clone._set_one_vs_all_fit(svm, model, X, y, classes, class_weight, None)
        return clones
    data = DataSet(X, y.tolist(), real_type=estimator.real_type)
    models = svm.fit_cost_path(data, Cs, epsilon=estimator.tol, max_iter=max_iter)
    for clone, model, info in zip(clones, models, svm.last_cg_info):
        clone._set_binary_fit(svm, model, data, X, y, class_weight, None, int(info["iterations"]))
    return clones


# ---------------------------------------------------------------------------------------------------------------------
# the fixed-size model: `rank` landmark points as the only support vectors (CSVM.fit_reduced)
# ---------------------------------------------------------------------------------------------------------------------
def fit_reduced(estimator, X, y, rank, landmarks=None, factor="host"):
    """A fitted clone of ``estimator`` whose model has ``rank`` support vectors only (the fixed-size LS-SVM, :meth:`plssvm_amd.csvm.CSVM.fit_reduced`): the library's fixed
    choice of landmark points, the distinct row indices ``landmarks`` (their number is then the rank), or ``"greedy"`` / ``"rpcholesky"`` for ``rank`` points selected from the
    data (``backend.select_landmarks``).  Two classes and one-vs-all alike; one landmark block, one Gram
    matrix and one factorisation serve all classes.  No CG runs: ``tol`` and ``max_iter`` play no part and ``n_iter_`` is 0.  ``support_`` holds the landmarks,
    ``dual_coef_`` has shape ``(n_classifiers, rank)``.  ``class_weight`` must be None; ``estimator`` itself stays unfitted.  ``factor="device"`` (opt-in): the dense
    solve on the device instead of one host thread (not the same bits)."""
    _capi.factor_on_device(factor)
    if not isinstance(estimator, SVC):
        raise InvalidParameterError("estimator must be a plssvm_amd.svc.SVC")
    if estimator.class_weight is not None:
        raise InvalidParameterError("the reduced model is fitted to the unweighted objective: class_weight must be None")
    return _fit_reduced(estimator, X, y, rank, landmarks, factor, weighted=False)


def _reduced_point_weights(estimator, classes, y, sample_weight):
    """``(class_weight_, the points' weights)`` of the weighted fixed-size fits, computed as :meth:`SVC.fit` computes them: ``sample_weight x class_weight[y]``."""
    class_weight = estimator._class_weight(classes, y)
    sw = np.ones(y.size) if sample_weight is None else np.asarray(sample_weight, dtype=np.float64)
    if sw.shape != y.shape:
        raise InvalidParameterError(f"The number of data points ({y.size}) and the number of sample weights ({sw.size}) must be the same!")
    return class_weight, sw * class_weight[np.searchsorted(classes, y)]


def _fit_reduced(estimator, X, y, rank, landmarks, factor, weighted, sample_weight=None):
    """What :func:`fit_reduced` and :func:`fit_reduced_weighted` share."""
    X, y = np.asarray(X), np.asarray(y)
    if X.ndim != 2 or y.ndim != 1 or y.shape[0] != X.shape[0]:
        raise InvalidParameterError(f"X must be a matrix and y a vector of as many labels as X has rows, but their shapes are {X.shape} and {y.shape}!")
    params = estimator._params()
    classes = np.array(sorted(set(y.tolist())))
    class_weight, weights = _reduced_point_weights(estimator, classes, y, sample_weight) if weighted else (np.ones(len(classes)), None)
    weight_keyword = _csvm._weight_keyword(weights)
    svm = make_csvm(params=params)
    clone = SVC(**estimator.get_params())
    if len(classes) > 2:
        Xr = np.ascontiguousarray(X, dtype=estimator.real_type)
        resolved = params.resolved(Xr.shape[1])
        betas, rhos, used, info = svm.solve_reduced_systems(resolved, Xr, _multiclass.one_vs_all_targets(classes, y, Xr.dtype), rank, landmarks, **_capi.factor_keyword(factor),
                                                            **weight_keyword)
        rows = np.asarray(used).astype(np.int64)
        infos = [dict(info, iterations=0) for _ in classes]
        model = _multiclass.OneVsAllModel(resolved, classes, np.ascontiguousarray(Xr[rows]), np.asarray(betas).astype(Xr.dtype), np.asarray(rhos).astype(Xr.dtype), infos)
        nonzero = np.any(model.alpha != 0, axis=0)
        clone._svm, clone._model = svm, model
        clone._fit = {
            "classes_": classes, "class_weight_": class_weight, "fit_status_": 0, "n_features_in_": int(X.shape[1]), "shape_fit_": tuple(int(v) for v in X.shape),
            "n_iter_": np.zeros(len(classes), dtype=np.int64), "support_": rows.astype(np.int32), "support_vectors_": model.support_vectors,
            "n_support_": np.array([np.count_nonzero(nonzero & (y[rows] == c)) for c in classes], dtype=np.int32), "dual_coef_": model.alpha, "intercept_": -model.rho,
        }
        return clone
    data = DataSet(X, y.tolist(), real_type=estimator.real_type)
    model = svm.fit_reduced(data, rank, landmarks, **_capi.factor_keyword(factor), **weight_keyword)
    clone._set_binary_fit(svm, model, model.data, X, y, class_weight, None, 0)
    clone._fit["support_"] = _landmarks_of(svm, landmarks)
    return clone


def fit_reduced_weighted(estimator, X, y, rank, sample_weight=None, landmarks=None, factor="host"):
    """:func:`fit_reduced` for the weighted objective ``1/2 beta^T K_mm beta + C/2 sum_i w_i (y_i - f(x_i))^2``.  ``estimator.class_weight`` is
    honoured exactly as :meth:`SVC.fit` honours it: ``w_i = sample_weight[i] x class_weight[y[i]]`` (``sample_weight`` None: ones), and ``class_weight_`` of the clone
    holds the multipliers.  One-vs-all uses the same weights for every classifier, so one Gram matrix and one factorisation still serve all classes.  A point of weight 0
    takes no part in the fit (it may still be a landmark); the weights must have a positive sum.  The landmark rules ignore the weights."""
    _capi.factor_on_device(factor)
    if not isinstance(estimator, SVC):
        raise InvalidParameterError("estimator must be a plssvm_amd.svc.SVC")
    return _fit_reduced(estimator, X, y, rank, landmarks, factor, weighted=True, sample_weight=sample_weight)


# ---------------------------------------------------------------------------------------------------------------------
# class probabilities: the fixed-size kernel logistic regression (CSVM.fit_reduced_logistic)
# ---------------------------------------------------------------------------------------------------------------------
def _sigmoid(d):
    """1 / (1 + exp(-d)) without overflow: exp is taken of -|d| only."""
    d = np.asarray(d, dtype=np.float64)
    e = np.exp(-np.abs(d))
    return np.where(d >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


class ProbabilisticSVC(SVC):
    """An :class:`SVC` whose decision values are log-odds: what :func:`fit_reduced_logistic` returns.  Everything :class:`SVC` offers, and ``predict_proba`` /
    ``predict_log_proba``; ``n_iter_`` counts the passes of the Newton iteration.  Two classes: ``P(classes_[1] | x) = 1 / (1 + exp(-decision_function(x)))``.  More than
    two classes are fitted one-vs-all; the classifiers' probabilities are normalised by their sum per point."""

    def predict_proba(self, X):
        """The class probabilities of every row of X, ndarray of shape (n, n_classes); the columns follow ``classes_``."""
        d = np.asarray(self.decision_function(X), dtype=np.float64)
        if d.ndim == 1:
            return np.column_stack([_sigmoid(-d), _sigmoid(d)])
        p = _sigmoid(d)
        return p / p.sum(axis=1, keepdims=True)

    def predict_log_proba(self, X):
        """log of :meth:`predict_proba`."""
        with np.errstate(divide="ignore"):
            return np.log(self.predict_proba(X))

    def predict(self, X):
        """The class of the largest probability (ties: the lowest class index)."""
        return self.classes_[np.argmax(self.predict_proba(X), axis=1)]

    n_iter_ = _fitted_attribute("n_iter_", "Passes of the Newton iteration, rejected steps included; more than two classes: of every classifier, int ndarray of shape (n_classes,).")


def fit_reduced_logistic(estimator, X, y, rank, sample_weight=None, landmarks=None, tol=1e-8, max_iter=50, factor="host"):
    """A fitted :class:`ProbabilisticSVC` with ``estimator``'s parameters whose model has ``rank`` support vectors (:meth:`plssvm_amd.csvm.CSVM.fit_reduced_logistic`,
    DESIGN.md section 20): the landmarks of :func:`fit_reduced`, fitted to the logistic loss ``C sum_i w_i log(1 + exp(-y_i f(x_i)))`` instead of the squared one, so that
    ``decision_function`` returns log-odds and ``predict_proba`` probabilities.  Two classes and one-vs-all alike; the classifiers of a one-vs-all fit run in lockstep and
    share every evaluation of the landmark block.  ``estimator.class_weight`` is honoured as :func:`fit_reduced_weighted` honours it: ``w_i = sample_weight[i] x
    class_weight[y[i]]``.  ``tol`` and ``max_iter`` here are the Newton iteration's (the relative decrease of the objective at which it stops; passes over the data,
    rejected steps included): ``estimator.tol`` and ``estimator.max_iter`` are the CG solve's and are not used.  ``estimator`` itself stays unfitted."""
    _capi.factor_on_device(factor)
    if not isinstance(estimator, SVC):
        raise InvalidParameterError("estimator must be a plssvm_amd.svc.SVC")
    X, y = np.asarray(X), np.asarray(y)
    if X.ndim != 2 or y.ndim != 1 or y.shape[0] != X.shape[0]:
        raise InvalidParameterError(f"X must be a matrix and y a vector of as many labels as X has rows, but their shapes are {X.shape} and {y.shape}!")
    params = estimator._params()
    classes = np.array(sorted(set(y.tolist())))
    weighted = sample_weight is not None or estimator.class_weight is not None
    class_weight, weights = _reduced_point_weights(estimator, classes, y, sample_weight) if weighted else (np.ones(len(classes)), None)
    svm = make_csvm(params=params)
    clone = ProbabilisticSVC(**estimator.get_params())
    if len(classes) > 2:
        Xr = np.ascontiguousarray(X, dtype=estimator.real_type)
        resolved = params.resolved(Xr.shape[1])
        betas, rhos, used, infos = svm.solve_reduced_logistic_systems(resolved, Xr, _multiclass.one_vs_all_targets(classes, y, Xr.dtype), rank, landmarks, sample_weight=weights,
                                                                      tol=tol, max_iter=max_iter, factor=factor)
        rows = np.asarray(used).astype(np.int64)
        infos = [dict(info, iterations=int(info["passes"])) for info in infos]
        model = _multiclass.OneVsAllModel(resolved, classes, np.ascontiguousarray(Xr[rows]), np.asarray(betas).astype(Xr.dtype), np.asarray(rhos).astype(Xr.dtype), infos)
        nonzero = np.any(model.alpha != 0, axis=0)
        clone._svm, clone._model = svm, model
        clone._fit = {
            "classes_": classes, "class_weight_": class_weight, "fit_status_": 0, "n_features_in_": int(X.shape[1]), "shape_fit_": tuple(int(v) for v in X.shape),
            "n_iter_": np.array([info["iterations"] for info in infos], dtype=np.int64), "support_": rows.astype(np.int32), "support_vectors_": model.support_vectors,
            "n_support_": np.array([np.count_nonzero(nonzero & (y[rows] == c)) for c in classes], dtype=np.int32), "dual_coef_": model.alpha, "intercept_": -model.rho,
        }
        return clone
    data = DataSet(X, y.tolist(), real_type=estimator.real_type)
    model = svm.fit_reduced_logistic(data, rank, landmarks, sample_weight=weights, tol=tol, max_iter=max_iter, factor=factor)
    clone._set_binary_fit(svm, model, model.data, X, y, class_weight, None, int(svm.last_cg_info["iterations"]))
    clone._fit["support_"] = _landmarks_of(svm, landmarks)
    return clone


def fit_reduced_stream(estimator, chunks, landmarks, classes, Cs=None, sample_weight_of=None):
    """:func:`fit_reduced_weighted` / :func:`fit_reduced_cv_weighted` for data that arrives in pieces (:meth:`plssvm_amd.csvm.CSVM.fit_reduced_stream`, DESIGN.md
    section 19).  ``chunks``: a re-iterable of ``(X, y)`` pairs (a list, or an object whose ``__iter__`` reads the pieces again).  ``landmarks``: the landmark ROWS
    ``(m, d)``, or ``(rows, labels)`` -- two classes need the labels, with both classes among them (the model groups its support vectors by class).  ``classes``: every
    label of the stream, known in advance.  Two classes and one-vs-all alike; one stream, one Gram matrix and one factorisation serve all classes.
    ``estimator.class_weight`` is honoured as :func:`fit_reduced_weighted` honours it; ``"balanced"`` takes one more walk over the chunks, reading the labels only, for
    the class counts.  ``sample_weight_of(i, X, y)``: the weights of chunk ``i`` (None: ones).  ``Cs`` None: a fitted clone at ``estimator.C``; else
    ``(loo_accuracy[len(Cs)], clones)`` from a second walk over the chunks -- the (weighted) leave-one-out accuracy of :func:`fit_reduced_cv_weighted`, accumulated
    chunk by chunk.  ``support_`` is empty: the landmarks are rows of their own, not indices."""
    if not isinstance(estimator, SVC):
        raise InvalidParameterError("estimator must be a plssvm_amd.svc.SVC")
    if iter(chunks) is chunks:
        raise InvalidParameterError("The chunks are walked more than once: a list or another re-iterable, not an iterator!")
    rows, row_labels = landmarks if isinstance(landmarks, tuple) else (landmarks, None)
    rows = np.ascontiguousarray(rows, dtype=estimator.real_type)
    classes = np.array(sorted(set(np.asarray(classes).tolist())))
    if rows.ndim != 2 or len(classes) < 2:
        raise InvalidParameterError("The landmarks must be a matrix of rows and the classes at least two labels!")
    binary = len(classes) == 2
    if row_labels is not None:
        row_labels = np.asarray(row_labels)
        if row_labels.shape != (rows.shape[0],):
            raise InvalidParameterError(f"The number of landmark rows ({rows.shape[0]}) and of their labels ({row_labels.size}) must be the same!")
    if binary and (row_labels is None or set(row_labels.tolist()) != set(classes.tolist())):
        raise InvalidParameterError("A two-class model groups its support vectors by class: the landmarks must come with their labels, of both classes!")
    params = estimator._params()
    resolved = params.resolved(rows.shape[1])
    cw = estimator.class_weight
    if isinstance(cw, str) and cw == "balanced":  # the class counts of the whole stream: one walk over the labels
        counts = np.zeros(len(classes))
        for _, y in chunks:
            counts += np.array([np.count_nonzero(np.asarray(y) == c) for c in classes], dtype=np.float64)
        class_weight = counts.sum() / (len(classes) * counts)
    else:
        class_weight = estimator._class_weight(classes, classes)
    weighted = cw is not None or sample_weight_of is not None

    class _Triples:
        def __iter__(_self):
            for i, (X, y) in enumerate(chunks):
                X, y = np.ascontiguousarray(X, dtype=estimator.real_type), np.asarray(y)
                at = np.searchsorted(classes, y)
                if y.ndim != 1 or y.shape[0] != X.shape[0] or not np.all(classes[np.minimum(at, len(classes) - 1)] == y):
                    raise InvalidParameterError(f"Chunk {i}: y must be a vector of as many labels as X has rows, each one of {classes.tolist()}!")
                w = None
                if weighted:
                    sw = None if sample_weight_of is None else sample_weight_of(i, X, y)
                    w = (np.ones(y.size) if sw is None else np.asarray(sw, dtype=np.float64)) * class_weight[at]
                Y = np.where(y == classes[1], 1.0, -1.0).astype(X.dtype).reshape(1, -1) if binary else _multiclass.one_vs_all_targets(classes, y, X.dtype)
                yield X, Y, w

    single = Cs is None
    costs = [float(estimator.C)] if single else _csvm._checked_costs(Cs)
    correct, total = np.zeros(len(costs)), [0.0]

    def on_scores(i, X, Y2, w, h, f, loo):  # the (weighted) number of points whose leave-one-out value names their class
        wv = np.ones(Y2.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
        total[0] += float(wv.sum())
        for s in range(len(costs)):
            right = np.sign(loo[s, 0]) == np.sign(Y2[0]) if binary else np.argmax(loo[s], axis=0) == np.argmax(Y2, axis=0)
            correct[s] += float(wv[right].sum())

    svm = make_csvm(params=params)
    betas, rhos, report = svm.solve_reduced_stream_systems(resolved, rows, _Triples(), costs, num_rhs=1 if binary else len(classes), loo=not single, weighted=weighted,
                                                           on_scores=None if single else on_scores)
    clones = [SVC(**{**estimator.get_params(), "C": C}) for C in costs]
    N = int(report["num_points"])
    for s, (C, clone) in enumerate(zip(costs, clones)):
        at_cost = Parameter(kernel_type=resolved.kernel_type, degree=resolved.degree, gamma=resolved.gamma, coef0=resolved.coef0, cost=C)
        info = dict(report["infos"][s], iterations=0)
        if binary:
            model = Model(at_cost, DataSet(rows, row_labels.tolist(), real_type=estimator.real_type), alpha=np.asarray(betas[s][0]).astype(rows.dtype), rho=rhos[s][0])
            alpha, sv, sv_labels = np.asarray(model.alpha).reshape(1, -1), model.support_vectors(), np.asarray(model.labels())
            intercept = np.array([-model.rho], dtype=alpha.dtype)
        else:
            model = _multiclass.OneVsAllModel(at_cost, classes, rows, np.asarray(betas[s]).astype(rows.dtype), np.asarray(rhos[s]).astype(rows.dtype), [info for _ in classes])
            alpha, sv, sv_labels, intercept = model.alpha, model.support_vectors, row_labels, -model.rho
        nonzero = np.any(alpha != 0, axis=0)
        clone._svm, clone._model = svm, model
        clone._fit = {
            "classes_": classes, "class_weight_": class_weight, "fit_status_": 0, "n_features_in_": int(rows.shape[1]), "shape_fit_": (N, int(rows.shape[1])),
            "n_iter_": 0 if binary else np.zeros(len(classes), dtype=np.int64), "support_": np.zeros(0, dtype=np.int32), "support_vectors_": sv,
            "n_support_": np.array([0 if sv_labels is None else np.count_nonzero(nonzero & (sv_labels == c)) for c in classes], dtype=np.int32), "dual_coef_": alpha,
            "intercept_": intercept,
        }
    if single:
        return clones[0]
    return correct / total[0], clones


def _landmarks_of(svm, landmarks):
    """The rows a reduced two-class fit used: the caller's, or the library's own or selected ones (read back from the backend's report)."""
    return np.asarray(svm.last_cg_info["landmarks"] if landmarks is None or isinstance(landmarks, str) else landmarks).astype(np.int32)


def fit_reduced_cv(estimator, X, y, rank, Cs, landmarks=None, factor="host"):
    """The exact leave-one-out accuracy of the fixed-size model of ``estimator`` at every ``C`` of ``Cs`` -- leave-one-out with the landmark set held fixed
    (:meth:`plssvm_amd.csvm.CSVM.fit_reduced_path`).  Returns ``(loo_accuracy[len(Cs)], fitted clones)``: the clones are what :func:`fit_reduced`
    gives at each ``C``, the accuracy is over ALL training points, each predicted by the model refitted without it -- no validation split, no refit, one more pass over the
    landmark block per cost.  Two classes: the sign of the leave-one-out value; more (one-vs-all): the argmax over the classes' leave-one-out values, compared with the
    label.  ``estimator.C`` is ignored, ``class_weight`` must be None, ``estimator`` itself stays unfitted.  ``factor="device"`` (opt-in): each cost's factorisation,
    inverse and solves on the device (not the same bits)."""
    _capi.factor_on_device(factor)
    if not isinstance(estimator, SVC):
        raise InvalidParameterError("estimator must be a plssvm_amd.svc.SVC")
    if estimator.class_weight is not None:
        raise InvalidParameterError("the reduced model is fitted to the unweighted objective: class_weight must be None")
    return _fit_reduced_cv(estimator, X, y, rank, Cs, landmarks, factor, weighted=False)


def _fit_reduced_cv(estimator, X, y, rank, Cs, landmarks, factor, weighted, sample_weight=None):
    """What :func:`fit_reduced_cv` and :func:`fit_reduced_cv_weighted` share."""
    X, y = np.asarray(X), np.asarray(y)
    if X.ndim != 2 or y.ndim != 1 or y.shape[0] != X.shape[0]:
        raise InvalidParameterError(f"X must be a matrix and y a vector of as many labels as X has rows, but their shapes are {X.shape} and {y.shape}!")
    Cs = _csvm._checked_costs(Cs)
    params = estimator._params()
    classes = np.array(sorted(set(y.tolist())))
    class_weight, weights = _reduced_point_weights(estimator, classes, y, sample_weight) if weighted else (np.ones(len(classes)), None)
    weight_keyword = _csvm._weight_keyword(weights)
    svm = make_csvm(params=params)
    clones = [SVC(**{**estimator.get_params(), "C": C}) for C in Cs]
    if len(classes) > 2:
        Xr = np.ascontiguousarray(X, dtype=estimator.real_type)
        resolved = params.resolved(Xr.shape[1])
        betas, rhos, used, report = svm.solve_reduced_loo_systems(resolved, Xr, _multiclass.one_vs_all_targets(classes, y, Xr.dtype), rank, Cs, landmarks, **_capi.factor_keyword(factor),
                                                                  **weight_keyword)
        rows = np.asarray(used).astype(np.int64)
        scores = np.array([float(np.average(classes[np.argmax(report["loo"][s], axis=0)] == y, weights=weights)) for s in range(len(Cs))])
        for s, (C, clone) in enumerate(zip(Cs, clones)):
            at_cost = Parameter(kernel_type=resolved.kernel_type, degree=resolved.degree, gamma=resolved.gamma, coef0=resolved.coef0, cost=C)
            infos = [dict(report["infos"][s], iterations=0) for _ in classes]
            model = _multiclass.OneVsAllModel(at_cost, classes, np.ascontiguousarray(Xr[rows]), np.asarray(betas[s]).astype(Xr.dtype), np.asarray(rhos[s]).astype(Xr.dtype), infos)
            nonzero = np.any(model.alpha != 0, axis=0)
            clone._svm, clone._model = svm, model
            clone._fit = {
                "classes_": classes, "class_weight_": class_weight, "fit_status_": 0, "n_features_in_": int(X.shape[1]), "shape_fit_": tuple(int(v) for v in X.shape),
                "n_iter_": np.zeros(len(classes), dtype=np.int64), "support_": rows.astype(np.int32), "support_vectors_": model.support_vectors,
                "n_support_": np.array([np.count_nonzero(nonzero & (y[rows] == c)) for c in classes], dtype=np.int32), "dual_coef_": model.alpha, "intercept_": -model.rho,
            }
        return scores, clones
    data = DataSet(X, y.tolist(), real_type=estimator.real_type)
    models, report = svm.fit_reduced_path(data, rank, Cs, landmarks, **_capi.factor_keyword(factor), **weight_keyword)
    for clone, model in zip(clones, models):
        clone._set_binary_fit(svm, model, model.data, X, y, class_weight, None, 0)
        clone._fit["support_"] = np.asarray(report["landmarks"]).astype(np.int32)
    return np.asarray(report["loo_accuracy"], dtype=np.float64), clones


def fit_reduced_cv_weighted(estimator, X, y, rank, Cs, sample_weight=None, landmarks=None, factor="host"):
    """:func:`fit_reduced_cv` under the weighting the model will be used with: the weights are those of :func:`fit_reduced_weighted`
    (``sample_weight x class_weight[y]``), the clones are what it gives at each ``C`` and carry ``class_weight_``, and the score is the WEIGHTED leave-one-out accuracy
    ``np.average(correct, weights=w)``.  A point of weight 0 does not count in the score; its leave-one-out value is the prediction of a model that never saw it."""
    _capi.factor_on_device(factor)
    if not isinstance(estimator, SVC):
        raise InvalidParameterError("estimator must be a plssvm_amd.svc.SVC")
    return _fit_reduced_cv(estimator, X, y, rank, Cs, landmarks, factor, weighted=True, sample_weight=sample_weight)


def fit_reduced_grid_cv(estimator, X, y, rank, Cs, gammas, sample_weight=None, landmarks=None, factor="host", product="matrix"):
    """:func:`fit_reduced_cv_weighted` at every ``C`` of ``Cs`` AND every kernel width of ``gammas`` from one call on one resident problem
    (:meth:`plssvm_amd.csvm.CSVM.fit_reduced_grid`; rbf and polynomial kernels).  Returns ``(loo_accuracy[G, S], clones[g][s])``: the
    leave-one-out accuracy over all training points, each predicted by the model refitted without it, and fitted clones that carry ``gamma = gammas[g]`` and
    ``C = Cs[s]``.  Two classes and one-vs-all follow the rules of :func:`fit_reduced_cv_weighted`; ``class_weight`` is honoured as there
    (``w_i = sample_weight[i] x class_weight[y[i]]``, the score is the weighted accuracy); with ``sample_weight`` None and ``class_weight`` None the fit is the unweighted
    one.  ``estimator.C`` is ignored; ``estimator.gamma`` only decides how the problem holds the data -- give it a value from ``gammas``.  ``estimator`` itself stays
    unfitted.  ``len(gammas) * len(Cs) <= 64``."""
    _capi.factor_on_device(factor)
    _capi.product_argument(product)
    if not isinstance(estimator, SVC):
        raise InvalidParameterError("estimator must be a plssvm_amd.svc.SVC")
    X, y = np.asarray(X), np.asarray(y)
    if X.ndim != 2 or y.ndim != 1 or y.shape[0] != X.shape[0]:
        raise InvalidParameterError(f"X must be a matrix and y a vector of as many labels as X has rows, but their shapes are {X.shape} and {y.shape}!")
    Cs = _csvm._checked_costs(Cs)
    gammas = [float(g) for g in np.asarray(gammas, dtype=np.float64).reshape(-1)]
    params = estimator._params()
    classes = np.array(sorted(set(y.tolist())))
    weighted = sample_weight is not None or estimator.class_weight is not None
    class_weight, weights = _reduced_point_weights(estimator, classes, y, sample_weight) if weighted else (np.ones(len(classes)), None)
    weight_keyword = _csvm._weight_keyword(weights)
    svm = make_csvm(params=params)
    clones = [[SVC(**{**estimator.get_params(), "C": C, "gamma": g}) for C in Cs] for g in gammas]
    if len(classes) > 2:
        Xr = np.ascontiguousarray(X, dtype=estimator.real_type)
        resolved = params.resolved(Xr.shape[1])
        betas, rhos, used, report = svm.solve_reduced_grid_systems(resolved, Xr, _multiclass.one_vs_all_targets(classes, y, Xr.dtype), rank, gammas, Cs, landmarks, product=product,
                                                                   **_capi.factor_keyword(factor), **weight_keyword)
        rows = np.asarray(used).astype(np.int64)
        scores = np.array([[float(np.average(classes[np.argmax(report["loo"][g][s], axis=0)] == y, weights=weights)) for s in range(len(Cs))] for g in range(len(gammas))])
        for g, gamma in enumerate(gammas):
            for s, C in enumerate(Cs):
                clone = clones[g][s]
                cell = Parameter(kernel_type=resolved.kernel_type, degree=resolved.degree, gamma=gamma, coef0=resolved.coef0, cost=C)
                infos = [dict(report["infos"][g][s], iterations=0) for _ in classes]
                model = _multiclass.OneVsAllModel(cell, classes, np.ascontiguousarray(Xr[rows]), np.asarray(betas[g][s]).astype(Xr.dtype), np.asarray(rhos[g][s]).astype(Xr.dtype), infos)
                nonzero = np.any(model.alpha != 0, axis=0)
                clone._svm, clone._model = make_csvm(params=cell), model
                clone._fit = {
                    "classes_": classes, "class_weight_": class_weight, "fit_status_": 0, "n_features_in_": int(X.shape[1]), "shape_fit_": tuple(int(v) for v in X.shape),
                    "n_iter_": np.zeros(len(classes), dtype=np.int64), "support_": rows.astype(np.int32), "support_vectors_": model.support_vectors,
                    "n_support_": np.array([np.count_nonzero(nonzero & (y[rows] == c)) for c in classes], dtype=np.int32), "dual_coef_": model.alpha, "intercept_": -model.rho,
                }
        return scores, clones
    data = DataSet(X, y.tolist(), real_type=estimator.real_type)
    models, report = svm.fit_reduced_grid(data, rank, gammas, Cs, landmarks, product=product, **_capi.factor_keyword(factor), **weight_keyword)
    for g in range(len(gammas)):
        for s in range(len(Cs)):
            model = models[g][s]
            clones[g][s]._set_binary_fit(make_csvm(params=model.params), model, model.data, X, y, class_weight, None, 0)
            clones[g][s]._fit["support_"] = np.asarray(report["landmarks"]).astype(np.int32)
    return np.asarray(report["loo_accuracy"], dtype=np.float64), clones


def fit_reduced_rank_cv(estimator, X, y, ranks, Cs, sample_weight=None, landmarks="rpcholesky", factor="host"):
    """:func:`fit_reduced_cv_weighted` at every ``C`` of ``Cs`` AND every prefix rank of ``ranks`` from ONE fit at ``max(ranks)`` landmarks
    (:meth:`plssvm_amd.csvm.CSVM.fit_reduced_rank_path`): accuracy against model size without a fit per size.  Returns
    ``(loo_accuracy[len(Cs), len(ranks)], clones[s][q])``: the leave-one-out accuracy over all training points, each predicted by the model on the first ``ranks[q]``
    landmarks refitted without it, and fitted clones of ``ranks[q]`` support vectors.  The landmark list is ordered: ``"rpcholesky"`` (the default) and ``"greedy"`` deliver
    their pivots in the order they were chosen; distinct row indices are taken in the order given (their number is then the rank of the fit); None is the library's fixed
    rule.  Two classes score by the sign of the leave-one-out value, more (one-vs-all) by the argmax over the classes' values, as :func:`fit_reduced_cv`;
    ``class_weight`` is honoured as in :func:`fit_reduced_cv_weighted` (``w_i = sample_weight[i] x class_weight[y[i]]``, the score is the weighted accuracy); with
    ``sample_weight`` None and ``class_weight`` None the fit is the unweighted one.  Every prefix model of a cost takes the jitter of the full rank.  ``estimator.C`` is
    ignored; ``estimator`` itself stays unfitted.  ``len(ranks) <= 16`` and ``len(ranks) * len(Cs) <= 64``."""
    _capi.factor_on_device(factor)
    if not isinstance(estimator, SVC):
        raise InvalidParameterError("estimator must be a plssvm_amd.svc.SVC")
    X, y = np.asarray(X), np.asarray(y)
    if X.ndim != 2 or y.ndim != 1 or y.shape[0] != X.shape[0]:
        raise InvalidParameterError(f"X must be a matrix and y a vector of as many labels as X has rows, but their shapes are {X.shape} and {y.shape}!")
    Cs = _csvm._checked_costs(Cs)
    try:
        ranks = [int(r) for r in np.asarray(ranks).reshape(-1).tolist()]
    except (TypeError, ValueError):
        raise InvalidParameterError("The checkpoints must be a list of integers!") from None
    if not ranks:
        raise InvalidParameterError("The rank path takes between 1 and 16 checkpoints, but got 0!")
    params = estimator._params()
    classes = np.array(sorted(set(y.tolist())))
    weighted = sample_weight is not None or estimator.class_weight is not None
    class_weight, weights = _reduced_point_weights(estimator, classes, y, sample_weight) if weighted else (np.ones(len(classes)), None)
    weight_keyword = _csvm._weight_keyword(weights)
    svm = make_csvm(params=params)
    clones = [[SVC(**{**estimator.get_params(), "C": C}) for _ in ranks] for C in Cs]
    if len(classes) > 2:
        Xr = np.ascontiguousarray(X, dtype=estimator.real_type)
        resolved = params.resolved(Xr.shape[1])
        rank = max(ranks) if landmarks is None or isinstance(landmarks, str) else len(landmarks)
        betas, rhos, used, report = svm.solve_reduced_rank_path_systems(resolved, Xr, _multiclass.one_vs_all_targets(classes, y, Xr.dtype), rank, ranks, Cs, landmarks,
                                                                        **_capi.factor_keyword(factor), **weight_keyword)
        used = np.asarray(used).astype(np.int64)
        scores = np.array([[float(np.average(classes[np.argmax(report["loo"][s][q], axis=0)] == y, weights=weights)) for q in range(len(ranks))] for s in range(len(Cs))])
        for s, C in enumerate(Cs):
            for q, r in enumerate(ranks):
                clone, rows = clones[s][q], used[:r]
                at_cost = Parameter(kernel_type=resolved.kernel_type, degree=resolved.degree, gamma=resolved.gamma, coef0=resolved.coef0, cost=C)
                infos = [dict(report["infos"][s][q], iterations=0) for _ in classes]
                model = _multiclass.OneVsAllModel(at_cost, classes, np.ascontiguousarray(Xr[rows]), np.asarray(betas[s][q][:, :r]).astype(Xr.dtype), np.asarray(rhos[s][q]).astype(Xr.dtype), infos)
                nonzero = np.any(model.alpha != 0, axis=0)
                clone._svm, clone._model = svm, model
                clone._fit = {
                    "classes_": classes, "class_weight_": class_weight, "fit_status_": 0, "n_features_in_": int(X.shape[1]), "shape_fit_": tuple(int(v) for v in X.shape),
                    "n_iter_": np.zeros(len(classes), dtype=np.int64), "support_": rows.astype(np.int32), "support_vectors_": model.support_vectors,
                    "n_support_": np.array([np.count_nonzero(nonzero & (y[rows] == c)) for c in classes], dtype=np.int32), "dual_coef_": model.alpha, "intercept_": -model.rho,
                }
        return scores, clones
    data = DataSet(X, y.tolist(), real_type=estimator.real_type)
    models, report = svm.fit_reduced_rank_path(data, ranks, Cs, landmarks, **_capi.factor_keyword(factor), **weight_keyword)
    for s in range(len(Cs)):
        for q, r in enumerate(ranks):
            model = models[s][q]
            clones[s][q]._set_binary_fit(svm, model, model.data, X, y, class_weight, None, 0)
            clones[s][q]._fit["support_"] = np.asarray(report["landmarks"])[:r].astype(np.int32)
    return np.asarray(report["loo_accuracy"], dtype=np.float64), clones


def cost_path_scores(estimator, X, y, Cs, X_val, y_val):
    """The validation accuracy of a TWO-class ``estimator`` at every ``C`` of ``Cs``: one cost path (:func:`fit_cost_path`), then ONE resident predictor over all the
    models -- they share their support vectors, so the predictor takes their weight vectors two per pass over the Gram tiles.  Returns ``(scores[m], fitted clones)``."""
    if not isinstance(estimator, SVC):
        raise InvalidParameterError("estimator must be a plssvm_amd.svc.SVC")
    num_classes = len(set(np.asarray(y).reshape(-1).tolist()))
    if num_classes != 2:  # (before anything is fitted)
        raise InvalidParameterError(f"cost_path_scores scores two-class models, but the labels have {num_classes} classes")
    y_val = np.asarray(y_val)
    clones = fit_cost_path(estimator, X, y, Cs)  # (checks its inputs)
    classes = clones[0].classes_
    models = [c._model for c in clones]
    alphas = np.stack([np.asarray(m.alpha) for m in models])
    rhos = np.array([float(m.rho) for m in models], dtype=np.float64)
    from . import backend
    with backend.Predictor(models[0].params, models[0].support_vectors(), alphas, rhos, options=getattr(clones[0]._svm, "_options", None)) as predictor:
        values = predictor.predict(np.asarray(X_val, dtype=estimator.real_type))  # [n_val, m]
    predicted = np.where(values > 0, classes[1], classes[0])
    return np.array([float(np.mean(predicted[:, s] == y_val)) for s in range(len(Cs))]), clones
