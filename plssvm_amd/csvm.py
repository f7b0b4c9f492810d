"""``CSVM`` -- the Python mirror of ``plssvm::csvm`` and of the reference's Python bindings
(bindings/Python/csvm.cpp:26-52, :95-181): ``fit`` / ``predict`` / ``score`` on top of the backend boundary, plus
``make_csvm`` (csvm_factory.hpp:123-171) with this repository's single backend."""

from __future__ import annotations

import enum
import sys
import time
from dataclasses import replace

import numpy as np

from . import _capi, backend
from .data_set import DataSet
from .exceptions import BackendError, InvalidParameterError, UnsupportedBackendError
from .model import Model
from .parameter import KernelFunctionType, Parameter

__all__ = ["CSVM", "MI355CSVM", "make_csvm", "BackendType", "TargetPlatform"]

# plssvm::verbosity (logger.hpp), as far as this mirror logs: "full" prints the solve's summary line in fit (csvm.cpp:167-173); "quiet" (default) prints nothing.
# The reference's Python SVC sets it from its `verbose` keyword (bindings/Python/sklearn.cpp:88-94), plssvm_amd.svc.SVC too.
verbosity = "quiet"


class BackendType(enum.Enum):
    """plssvm::backend_type (backend_types.hpp:30-43) + ``mi355``."""
    AUTOMATIC = "automatic"
    OPENMP = "openmp"
    CUDA = "cuda"
    HIP = "hip"
    OPENCL = "opencl"
    SYCL = "sycl"
    MI355 = "mi355"


class TargetPlatform(enum.Enum):
    AUTOMATIC = "automatic"
    CPU = "cpu"
    GPU_NVIDIA = "gpu_nvidia"
    GPU_AMD = "gpu_amd"
    GPU_INTEL = "gpu_intel"


class CSVM:
    """Abstract base: subclasses implement the two boundary methods (csvm.hpp:188-208)."""

    def __init__(self, params: Parameter | None = None, **kwargs):
        if params is not None and kwargs:
            raise InvalidParameterError("Provide either a Parameter object or keyword arguments, not both!")
        self.params = params if params is not None else Parameter(**kwargs)
        self.target_platform = TargetPlatform.AUTOMATIC
        self.last_cg_info = None

    # --- boundary (pure virtual in the reference) ---
    def solve_system_of_linear_equations(self, params, A, b, eps, max_iter):
        raise NotImplementedError

    def predict_values(self, params, support_vectors, alpha, rho, w, predict_points):
        raise NotImplementedError

    # --- several classifiers over one data set (one-vs-all, plssvm_amd.multiclass): defaults on top of the two boundary methods ---
    def solve_systems_of_linear_equations(self, params, A, B, eps, max_iter, sample_weight=None):
        """One solve per row of ``B`` (``k x N`` right-hand sides) on the same matrix: ``(alphas[k, N], rhos[k], [info, ...])``."""
        B = np.asarray(B)
        if B.ndim != 2 or B.shape[0] == 0:
            raise InvalidParameterError("The right-hand sides must be a matrix with one row per system and at least one row!")
        kw = {} if sample_weight is None else {"sample_weight": sample_weight}
        solved = [self.solve_system_of_linear_equations(params, A, b, eps, max_iter, **kw) for b in B]
        return np.stack([np.asarray(s[0]) for s in solved]), np.array([s[1] for s in solved]), [s[2] for s in solved]

    def predict_values_multi(self, params, support_vectors, alphas, rhos, ws, predict_points):
        """``predict_values`` per row of ``alphas``: ``(values[n, k], ws[k, d] or None)``."""
        alphas = np.asarray(alphas)
        done = [self.predict_values(params, support_vectors, alphas[v], float(rhos[v]), None if ws is None else ws[v], predict_points) for v in range(alphas.shape[0])]
        values = np.stack([np.asarray(d[0]) for d in done], axis=1)
        return values, (None if any(d[1] is None for d in done) else np.stack([np.asarray(d[1]) for d in done]))

    def solve_cost_path(self, params, A, b, costs, eps, max_iter):
        """One right-hand side for every cost of ``costs``: ``(alphas[m, N], rhos[m], [info, ...])``.  The default is one solve per cost; a backend with a cost path
        (the MI355X backend) serves the whole grid from one Krylov sequence."""
        solved = []
        for cost in costs:
            at_cost = replace(params, cost=float(cost))
            solved.append(self.solve_system_of_linear_equations(at_cost, A, b, eps, max_iter))
        return np.stack([np.asarray(s[0]) for s in solved]), np.array([s[1] for s in solved]), [s[2] for s in solved]

    def solve_cost_paths(self, params, A, B, costs, eps, max_iter):
        """:meth:`solve_cost_path` for every row of ``B`` (``k x N`` right-hand sides, one-vs-all) on the same matrix: a list of k ``(alphas[m, N], rhos[m], [info, ...])``."""
        B = np.asarray(B)
        if B.ndim != 2 or B.shape[0] == 0:
            raise InvalidParameterError("The right-hand sides must be a matrix with one row per system and at least one row!")
        return [self.solve_cost_path(params, A, b, costs, eps, max_iter) for b in B]

    def get_params(self):
        return self.params

    def set_params(self, params: Parameter | None = None, **kwargs):
        """csvm::set_params (csvm.hpp:236-261): named arguments override only what they name."""
        if params is not None:
            self.params = params
        for k, v in kwargs.items():
            if k not in ("kernel_type", "degree", "gamma", "coef0", "cost"):
                raise InvalidParameterError(f"Invalid argument {k} provided!")
            setattr(self.params, k, v)
        self.params.__post_init__()

    def get_target_platform(self):
        return self.target_platform

    # --- fit / predict / score (csvm.hpp:263-375) ---
    def fit(self, data: DataSet, epsilon: float = 0.001, max_iter: int | None = None, sample_weight=None) -> Model:
        """csvm::fit (csvm.hpp:263-320).  ``sample_weight`` (no counterpart in the reference): one weight >= 0 per data point, scikit-learn's semantics -- the
        weighted LS-SVM system (point i regularised by 1 / (C w_i)) over the points of weight > 0; points of weight 0 are left out of the solve and out of the
        model.  The model is an ordinary one (file format, predict)."""
        if epsilon <= 0.0:
            raise InvalidParameterError(f"epsilon must be less than 0.0, but is {epsilon}!")  # csvm.hpp:283 (message verbatim)
        if max_iter is not None and max_iter <= 0:
            raise InvalidParameterError(f"max_iter must be greater than 0, but is {max_iter}!")  # csvm.hpp:291
        if not data.has_labels():
            raise InvalidParameterError("No labels given for training! Maybe the data is only usable for prediction?")  # csvm.hpp:298
        weights = None
        if sample_weight is not None:
            data, weights = _drop_zero_weights(data, sample_weight)
        if max_iter is None:
            max_iter = data.num_data_points()  # csvm.hpp:269
        params = self.params.resolved(data.num_features())  # csvm.hpp:303-307
        t0 = time.perf_counter()
        if weights is None:
            alpha, rho, info = self.solve_system_of_linear_equations(params, data.data(), data.mapped_labels(), epsilon, max_iter)
        else:
            alpha, rho, info = self.solve_system_of_linear_equations(params, data.data(), data.mapped_labels(), epsilon, max_iter, sample_weight=weights)
        info["total_runtime_ms"] = (time.perf_counter() - t0) * 1e3  # cg/total_runtime (csvm.hpp:318-320)
        self.last_cg_info = info
        if verbosity == "full":
            its = int(info.get("iterations", 0))
            print(f"Finished after {its}/{int(max_iter)} iterations with a residuum of {info.get('residuum', 0.0)} (target: {info.get('target_residuum', 0.0)}) and an average "
                  f"iteration time of {info.get('avg_iteration_ms', 0.0):.3f}ms.", flush=True)
        return Model(params, data, alpha=alpha, rho=rho)

    def fit_cost_path(self, data: DataSet, costs, epsilon: float = 0.001, max_iter: int | None = None) -> list:
        """``fit`` for every cost of ``costs`` (no counterpart in the reference): one :class:`Model` per cost, in the order of ``costs``, each with its ``params.cost``
        set; this object's own cost is ignored.  The models share the data set, so they share their support vectors.  ``last_cg_info`` keeps the list of per-cost
        reports."""
        if epsilon <= 0.0:
            raise InvalidParameterError(f"epsilon must be less than 0.0, but is {epsilon}!")  # csvm.hpp:283 (message verbatim)
        if max_iter is not None and max_iter <= 0:
            raise InvalidParameterError(f"max_iter must be greater than 0, but is {max_iter}!")  # csvm.hpp:291
        if not data.has_labels():
            raise InvalidParameterError("No labels given for training! Maybe the data is only usable for prediction?")  # csvm.hpp:298
        costs = _checked_costs(costs)
        if max_iter is None:
            max_iter = data.num_data_points()  # csvm.hpp:269
        params = self.params.resolved(data.num_features())
        alphas, rhos, infos = self.solve_cost_path(params, data.data(), data.mapped_labels(), costs, epsilon, max_iter)
        self.last_cg_info = infos
        models = []
        for s, cost in enumerate(costs):
            at_cost = replace(params, cost=float(cost))
            models.append(Model(at_cost, data, alpha=np.asarray(alphas[s]), rho=rhos[s]))
        return models

    def solve_reduced_systems(self, params, A, Y, rank, landmarks=None, factor="host", sample_weight=None):
        """The fixed-size model of every row of ``Y`` over the same landmarks: ``(betas[k, m] float64, rhos[k] float64, landmarks[m], info)``.  Boundary of
        :meth:`fit_reduced`; the MI355X backend implements it."""
        raise NotImplementedError

    def fit_reduced(self, data: DataSet, rank: int, landmarks=None, factor: str = "host", sample_weight=None) -> Model:
        """A fixed-size (reduced) LS-SVM model of ``rank`` support vectors (no counterpart in the reference): the decision function is expanded over
        ``rank`` landmark points only -- the library's fixed choice (the preconditioner's rule), the distinct point indices ``landmarks``, whose number is then the rank, or
        ``"greedy"`` / ``"rpcholesky"`` for ``rank`` points selected from the data (``backend.select_landmarks``; fewer where the kernel matrix's rank is exhausted first) --
        and fitted to ALL points by one pass over the N x rank kernel block and a dense solve, without CG.  The model is an ordinary :class:`Model` whose data set is
        the landmark rows of ``data`` (file format, predict, score); it trades accuracy for size.  A two-class model file groups its support vectors by class, so the
        landmarks must hold points of both classes.  ``last_cg_info`` keeps the ``lssvm_reduced_info`` report with ``iterations`` = 0.  ``factor="device"`` (opt-in;
        DESIGN.md section 15) runs the dense solve on the device instead of one host thread: not the same bits, and the report gains the ``lssvm_dense_info`` fields.
        ``sample_weight``: one weight >= 0 per data point with a positive sum, the weight of the point's squared error; unlike :meth:`fit` nothing
        is dropped -- a point of weight 0 takes no part in the fit but may still be a landmark.  The landmark rules ignore the weights."""
        _capi.factor_on_device(factor)
        if not data.has_labels():
            raise InvalidParameterError("No labels given for training! Maybe the data is only usable for prediction?")  # csvm.hpp:298
        labels = data.labels()
        if landmarks is not None and not isinstance(landmarks, str):  # (a selection rule's points are checked once they are known)
            _check_landmark_classes(data, landmarks)  # (before anything is computed)
        params = self.params.resolved(data.num_features())
        t0 = time.perf_counter()
        betas, rhos, used, info = self.solve_reduced_systems(params, data.data(), data.mapped_labels().reshape(1, -1), rank, landmarks, **_capi.factor_keyword(factor),
                                                              **_weight_keyword(sample_weight))
        info = dict(info, iterations=0, landmarks=np.asarray(used), total_runtime_ms=(time.perf_counter() - t0) * 1e3)
        self.last_cg_info = info
        rows = _check_landmark_classes(data, used)
        reduced = DataSet(data.data()[rows], [labels[i] for i in rows.tolist()], real_type=data.real_type)
        return Model(params, reduced, alpha=np.asarray(betas[0]).astype(data.real_type), rho=rhos[0])

    def solve_reduced_logistic_systems(self, params, A, Y, rank, landmarks=None, sample_weight=None, tol=1e-8, max_iter=50, factor="host", start=None):
        """The fixed-size logistic regression of every row of ``Y`` (labels of -1 / +1) over the same landmarks: ``(betas[k, m] float64, rhos[k] float64, landmarks[m],
        infos[k])``.  Boundary of :meth:`fit_reduced_logistic`; the MI355X backend implements it."""
        raise NotImplementedError

    def fit_reduced_logistic(self, data: DataSet, rank: int, landmarks=None, sample_weight=None, tol: float = 1e-8, max_iter: int = 50, factor: str = "host", start=None) -> Model:
        """A fixed-size kernel logistic regression of ``rank`` support vectors (no counterpart in the reference): the model of :meth:`fit_reduced` --
        the same landmarks, the same file format, predict and score -- fitted to the logistic loss ``C sum_i a_i log(1 + exp(-y_i f(x_i)))`` instead of the squared one, by
        Newton's method with a step-halving safeguard, every step a weighted fixed-size fit.  Its decision values are the log-odds of the class the positive label maps
        to: ``P = 1 / (1 + exp(-f(x)))``.  ``sample_weight``: the prior weights ``a_i`` as :meth:`fit_reduced` takes them; ``tol``: the relative decrease of the objective
        at which the iteration stops; ``max_iter``: passes over the data, rejected steps included; ``start``: ``(betas0, rho0)`` or None for zeros.  The model file carries
        no probability field.  ``last_cg_info`` keeps the ``lssvm_reduced_logistic_info`` report with ``iterations`` = its passes."""
        _capi.factor_on_device(factor)
        if not data.has_labels():
            raise InvalidParameterError("No labels given for training! Maybe the data is only usable for prediction?")  # csvm.hpp:298
        labels = data.labels()
        if landmarks is not None and not isinstance(landmarks, str):  # (a selection rule's points are checked once they are known)
            _check_landmark_classes(data, landmarks)  # (before anything is computed)
        params = self.params.resolved(data.num_features())
        t0 = time.perf_counter()
        betas, rhos, used, infos = self.solve_reduced_logistic_systems(params, data.data(), data.mapped_labels().reshape(1, -1), rank, landmarks, sample_weight=sample_weight, tol=tol,
                                                                        max_iter=max_iter, factor=factor, start=start)
        info = dict(infos[0], iterations=int(infos[0]["passes"]), landmarks=np.asarray(used), total_runtime_ms=(time.perf_counter() - t0) * 1e3)
        self.last_cg_info = info
        rows = _check_landmark_classes(data, used)
        reduced = DataSet(data.data()[rows], [labels[i] for i in rows.tolist()], real_type=data.real_type)
        return Model(params, reduced, alpha=np.asarray(betas[0]).astype(data.real_type), rho=rhos[0])

    def solve_reduced_loo_systems(self, params, A, Y, rank, costs, landmarks=None, factor="host", sample_weight=None):
        """The fixed-size models of every row of ``Y`` at every cost of ``costs`` with their leave-one-out report: ``(betas[S, k, m], rhos[S, k], landmarks[m], report)``.
        Boundary of :meth:`fit_reduced_path`; the MI355X backend implements it."""
        raise NotImplementedError

    def solve_reduced_stream_systems(self, params, landmark_rows, chunks, costs, num_rhs=1, factor="host", loo=False, weighted=False, on_scores=None):
        """The fixed-size models over the landmark ROWS ``landmark_rows`` from a stream of ``(X, Y, w)`` chunks at every cost: ``(betas[S, k, m], rhos[S, k], report)``.
        Boundary of :meth:`fit_reduced_stream`; the MI355X backend implements it."""
        raise NotImplementedError

    def fit_reduced_stream(self, landmarks: DataSet, chunks, costs=None, factor: str = "host", loo: bool = False):
        """:meth:`fit_reduced` / :meth:`fit_reduced_path` for data that arrives in pieces (no counterpart in the reference): the N points are never
        held at once and no resident problem is built.  ``landmarks``: a labelled :class:`DataSet` of the landmark ROWS (both classes present; e.g. rows chosen on a
        sample with ``backend.select_landmarks``) -- it becomes the data set of the returned models and its label mapping maps the chunks' labels.  ``chunks``: an
        iterable of :class:`DataSet` or of ``(X, y)`` pairs; with ``loo=True`` it is walked twice and must be re-iterable (a list, not a generator).  ``costs`` None: ONE
        ordinary :class:`Model` at this object's cost; else a list with one model per cost.  ``loo=True`` returns ``(model(s), report)`` with the report of
        :meth:`fit_reduced_path` -- ``press``, ``loo_errors``, ``loo_accuracy``, ``max_leverage``, ``jitter`` per cost, summed over the chunks in row order; nothing of
        size N is kept.  The result does not depend on how the rows are cut into chunks.  No sample weights, no landmark selection from the stream."""
        _capi.factor_on_device(factor)
        if not isinstance(landmarks, DataSet) or not landmarks.has_labels():
            raise InvalidParameterError("The landmarks must be a DataSet of the landmark rows with their labels!")
        labels = landmarks.different_labels()
        single = costs is None
        costs = [float(self.params.cost)] if single else _checked_costs(costs)
        params = self.params.resolved(landmarks.num_features())
        real_type = landmarks.real_type

        class _Triples:
            def __iter__(_self):
                for chunk in chunks:
                    X, y = (chunk.data(), chunk.labels()) if isinstance(chunk, DataSet) else chunk
                    y = np.asarray(y)
                    known = (y == labels[0]) | (y == labels[1])
                    if y.ndim != 1 or not np.all(known):
                        raise InvalidParameterError(f"Every label of a chunk must be one of the landmarks' labels {labels}!")
                    yield np.asarray(X, dtype=real_type), np.where(y == labels[1], 1.0, -1.0).astype(real_type).reshape(1, -1), None

        t0 = time.perf_counter()
        betas, rhos, report = self.solve_reduced_stream_systems(params, landmarks.data(), _Triples() if iter(chunks) is not chunks else iter(_Triples()), costs,
                                                                **_capi.factor_keyword(factor), loo=loo)
        models = [Model(replace(params, cost=float(cost)), landmarks, alpha=np.asarray(betas[s][0]).astype(real_type), rho=rhos[s][0]) for s, cost in enumerate(costs)]
        self.last_cg_info = [dict(info, iterations=0, total_runtime_ms=(time.perf_counter() - t0) * 1e3) for info in report["infos"]]
        result = models[0] if single else models
        if not loo:
            return result
        N = report["num_points"]
        report = {name: (value[:, 0] if name in ("press", "loo_errors") else value) for name, value in report.items()}
        report["loo_accuracy"] = 1.0 - report["loo_errors"].astype(np.float64) / N
        return result, report

    def fit_reduced_path(self, data: DataSet, rank: int, costs, landmarks=None, factor: str = "host", sample_weight=None):
        """:meth:`fit_reduced` for every cost of ``costs`` together with exact leave-one-out scores -- leave-one-out with the landmark set held fixed (no counterpart in
        the reference).  Returns ``(models, report)``: one ordinary :class:`Model` per cost, in the order of ``costs``, each with its ``params.cost``
        set and equal to what :meth:`fit_reduced` gives at that cost; this object's own cost is ignored.  ``report`` (float64, over ALL training points, no validation split
        and no refit): ``costs``, ``leverage[S, N]``, ``fitted[S, N]``, ``loo[S, N]`` (the value the model refitted without point i has at point i), ``press[S]``,
        ``loo_errors[S]``, ``loo_accuracy[S]`` = 1 - loo_errors / N, ``max_leverage[S]``, ``jitter[S]``, ``infos``.  ``last_cg_info`` keeps the per-cost reports.
        ``factor="device"`` (opt-in): each cost's factorisation, inverse and solves run on the device; the models then equal what :meth:`fit_reduced`
        gives with ``factor="device"``.
        ``sample_weight``: the weights of :meth:`fit_reduced`; then ``press`` is weighted, ``loo_errors`` counts the points of positive weight and
        ``loo_accuracy`` is the weighted mean of the correct leave-one-out signs.  A point of weight 0 has leverage 0 and its ``loo`` value is the prediction of a model
        that never saw it."""
        _capi.factor_on_device(factor)
        if not data.has_labels():
            raise InvalidParameterError("No labels given for training! Maybe the data is only usable for prediction?")  # csvm.hpp:298
        labels = data.labels()
        if landmarks is not None and not isinstance(landmarks, str):  # (a selection rule's points are checked once they are known)
            _check_landmark_classes(data, landmarks)  # (before anything is computed)
        costs = _checked_costs(costs)
        params = self.params.resolved(data.num_features())
        betas, rhos, used, report = self.solve_reduced_loo_systems(params, data.data(), data.mapped_labels().reshape(1, -1), rank, costs, landmarks, **_capi.factor_keyword(factor),
                                                                    **_weight_keyword(sample_weight))
        rows = _check_landmark_classes(data, used)
        reduced = DataSet(data.data()[rows], [labels[i] for i in rows.tolist()], real_type=data.real_type)
        models = [Model(replace(params, cost=float(cost)), reduced, alpha=np.asarray(betas[s][0]).astype(data.real_type), rho=rhos[s][0]) for s, cost in enumerate(costs)]
        report = {name: (value[:, 0] if name in ("fitted", "loo", "press", "loo_errors") else value) for name, value in report.items()}
        report["landmarks"] = np.asarray(used)
        report["loo_accuracy"] = 1.0 - report["loo_errors"].astype(np.float64) / data.num_data_points()
        if sample_weight is not None:
            correct = np.sign(report["loo"]) == np.sign(np.asarray(data.mapped_labels(), dtype=np.float64))[None, :]
            report["loo_accuracy"] = np.array([float(np.average(row, weights=np.asarray(sample_weight, dtype=np.float64))) for row in correct])
        self.last_cg_info = [dict(info, iterations=0) for info in report["infos"]]
        return models, report

    def solve_reduced_grid_systems(self, params, A, Y, rank, gammas, costs, landmarks=None, factor="host", sample_weight=None, product="matrix"):
        """The fixed-size models of every row of ``Y`` at every ``(gamma, cost)`` of the grid with their leave-one-out report:
        ``(betas[G, S, k, m], rhos[G, S, k], landmarks[m], report)``.  Boundary of :meth:`fit_reduced_grid`; the MI355X backend implements it."""
        raise NotImplementedError

    def fit_reduced_grid(self, data: DataSet, rank: int, gammas, costs, landmarks=None, factor: str = "host", sample_weight=None, product: str = "matrix"):
        """:meth:`fit_reduced_path` for every kernel width of ``gammas`` AND every cost of ``costs`` in one call on one resident problem (no counterpart in the reference;
        DESIGN.md section 17; rbf and polynomial kernels).  Returns ``(models, report)``: ``models[g][s]`` is an ordinary :class:`Model` whose parameters carry
        ``gammas[g]`` and ``costs[s]`` -- predict, score, the resident predictors and :meth:`Model.save` take it unchanged.  This object's own cost is ignored; its own
        gamma only decides how the resident problem holds the data (and selects the landmarks for ``"greedy"`` / ``"rpcholesky"``): give it a gamma from the grid.
        ``report``: as for :meth:`fit_reduced_path` with a leading gamma axis on every array (``loo[G, S, N]``, ``loo_accuracy[G, S]`` ...), ``gammas``, and
        ``infos[g][s]``.  ``product="matrix"`` (the default) forms what the gammas share on the fp64 matrix cores, ``"ordered"`` with the loop of
        :meth:`fit_reduced_path` (then a grid of this object's one gamma returns that call's bits).  ``len(gammas) * len(costs) <= 64``."""
        _capi.factor_on_device(factor)
        _capi.product_argument(product)
        if not data.has_labels():
            raise InvalidParameterError("No labels given for training! Maybe the data is only usable for prediction?")  # csvm.hpp:298
        labels = data.labels()
        if landmarks is not None and not isinstance(landmarks, str):  # (a selection rule's points are checked once they are known)
            _check_landmark_classes(data, landmarks)  # (before anything is computed)
        costs = _checked_costs(costs)
        params = self.params.resolved(data.num_features())
        betas, rhos, used, report = self.solve_reduced_grid_systems(params, data.data(), data.mapped_labels().reshape(1, -1), rank, gammas, costs, landmarks, product=product,
                                                                     **_capi.factor_keyword(factor), **_weight_keyword(sample_weight))
        rows = _check_landmark_classes(data, used)
        reduced = DataSet(data.data()[rows], [labels[i] for i in rows.tolist()], real_type=data.real_type)
        models = [[Model(replace(params, gamma=float(gamma), cost=float(cost)), reduced, alpha=np.asarray(betas[g][s][0]).astype(data.real_type), rho=rhos[g][s][0])
                   for s, cost in enumerate(costs)] for g, gamma in enumerate(report["gammas"])]
        report = {name: (value[:, :, 0] if name in ("fitted", "loo", "press", "loo_errors") else value) for name, value in report.items()}
        report["landmarks"] = np.asarray(used)
        report["loo_accuracy"] = 1.0 - report["loo_errors"].astype(np.float64) / data.num_data_points()
        if sample_weight is not None:
            correct = np.sign(report["loo"]) == np.sign(np.asarray(data.mapped_labels(), dtype=np.float64))[None, None, :]
            report["loo_accuracy"] = np.average(correct, axis=2, weights=np.asarray(sample_weight, dtype=np.float64))
        self.last_cg_info = [[dict(info, iterations=0) for info in row] for row in report["infos"]]
        return models, report

    def solve_reduced_rank_path_systems(self, params, A, Y, rank, ranks, costs, landmarks=None, factor="host", sample_weight=None):
        """The fixed-size models of every row of ``Y`` at every cost of ``costs`` and every prefix rank of ``ranks`` with their leave-one-out report:
        ``(betas[S, R, k, m], rhos[S, R, k], landmarks[m], report)``.  Boundary of :meth:`fit_reduced_rank_path`; the MI355X backend implements it."""
        raise NotImplementedError

    def fit_reduced_rank_path(self, data: DataSet, ranks, costs, landmarks=None, factor: str = "host", sample_weight=None):
        """:meth:`fit_reduced_path` for every PREFIX RANK of ``ranks`` and every cost of ``costs`` from one fit at ``rank = max(ranks)`` (no counterpart in the reference;
        DESIGN.md section 18): the landmark list is ordered, and the model on its first ``r`` entries, its leverages and its leave-one-out values are prefixes of what the
        full-rank fit forms.  Returns ``(models, report)``: ``models[s][q]`` is an ordinary :class:`Model` of ``ranks[q]`` support vectors -- the first ``ranks[q]``
        landmark rows -- with ``params.cost = costs[s]``; it saves, loads and predicts like a :meth:`fit_reduced` model.  ``ranks``: 1 to 16 strictly ascending prefix
        lengths; ``len(ranks) * len(costs) <= 64``; ``landmarks``: None, at least ``max(ranks)`` distinct point indices in the order that matters (their number is the
        rank the fit runs at), or ``"greedy"`` / ``"rpcholesky"``.  Every prefix model of a cost uses the jitter of the full rank at that cost, which is no smaller than the one
        :meth:`fit_reduced` on ``landmarks[:r]`` would take (``report["jitter"]``).  A two-class model file groups its support vectors by class, so every prefix must
        hold points of both classes.  ``report``: as for :meth:`fit_reduced_path` with a rank axis behind the cost axis (``loo[S, R, N]``, ``loo_accuracy[S, R]`` ...),
        ``ranks``, ``cond_hint[S, R]`` and ``infos[s][q]``.  ``factor`` and ``sample_weight``: as for :meth:`fit_reduced_path`."""
        _capi.factor_on_device(factor)
        if not data.has_labels():
            raise InvalidParameterError("No labels given for training! Maybe the data is only usable for prediction?")  # csvm.hpp:298
        labels = data.labels()
        try:
            prefix = [int(r) for r in np.asarray(ranks).reshape(-1).tolist()]
        except (TypeError, ValueError):
            raise InvalidParameterError("The checkpoints must be a list of integers!") from None
        if not prefix:
            raise InvalidParameterError("The rank path takes between 1 and 16 checkpoints, but got 0!")
        if landmarks is not None and not isinstance(landmarks, str):  # (a selection rule's points are checked once they are known)
            for r in prefix:
                _check_landmark_classes(data, np.asarray(landmarks)[:max(r, 0)])  # (before anything is computed)
        costs = _checked_costs(costs)
        params = self.params.resolved(data.num_features())
        rank = max(prefix) if landmarks is None or isinstance(landmarks, str) else len(landmarks)
        betas, rhos, used, report = self.solve_reduced_rank_path_systems(params, data.data(), data.mapped_labels().reshape(1, -1), rank, prefix, costs, landmarks,
                                                                          **_capi.factor_keyword(factor), **_weight_keyword(sample_weight))
        models = []
        for s, cost in enumerate(costs):
            row = []
            for q, r in enumerate(prefix):
                rows = _check_landmark_classes(data, np.asarray(used)[:r])
                reduced = DataSet(data.data()[rows], [labels[i] for i in rows.tolist()], real_type=data.real_type)
                row.append(Model(replace(params, cost=float(cost)), reduced, alpha=np.asarray(betas[s][q][0][:r]).astype(data.real_type), rho=rhos[s][q][0]))
            models.append(row)
        report = {name: (value[:, :, 0] if name in ("fitted", "loo", "press", "loo_errors") else value) for name, value in report.items()}
        report["landmarks"] = np.asarray(used)
        report["loo_accuracy"] = 1.0 - report["loo_errors"].astype(np.float64) / data.num_data_points()
        if sample_weight is not None:
            correct = np.sign(report["loo"]) == np.sign(np.asarray(data.mapped_labels(), dtype=np.float64))[None, None, :]
            report["loo_accuracy"] = np.average(correct, axis=2, weights=np.asarray(sample_weight, dtype=np.float64))
        self.last_cg_info = [[dict(info, iterations=0) for info in row] for row in report["infos"]]
        return models, report

    def predict(self, model: Model, data: DataSet):
        if model.num_features() != data.num_features():
            raise InvalidParameterError(f"Number of features per data point ({data.num_features()}) must match the number of features per support vector of the "
                                        f"provided model ({model.num_features()})!")
        values, w = self.predict_values(model.params, model.support_vectors(), model.alpha, float(model.rho), model.w, data.data())
        if w is not None:
            model.w = w
        mapper = model.data.mapping
        return [mapper.label_of(1 if v > 0 else -1) for v in values]  # operators.hpp:180-182 sign, csvm.hpp:337-340

    def score(self, model: Model, data: DataSet | None = None) -> float:
        data = model.data if data is None else data
        if not data.has_labels():
            raise InvalidParameterError("The data set to score must have labels!")
        if model.num_features() != data.num_features():
            raise InvalidParameterError(f"Number of features per data point ({data.num_features()}) must match the number of features per support vector of the "
                                        f"provided model ({model.num_features()})!")
        predicted = self.predict(model, data)
        correct = sum(1 for p, c in zip(predicted, data.labels()) if p == c)
        return correct / len(predicted)


def _checked_costs(costs) -> list:
    """The costs of a cost path as a list of floats: at least one, each finite and > 0."""
    costs = [float(c) for c in np.asarray(costs, dtype=np.float64).reshape(-1)]
    if not costs:
        raise InvalidParameterError("The number of costs must be greater than 0!")
    if not all(np.isfinite(c) and c > 0.0 for c in costs):
        raise InvalidParameterError("Every cost of the path must be finite and greater than 0.0!")
    return costs


def _check_landmark_classes(data: DataSet, landmarks) -> np.ndarray:
    """The landmarks of a two-class fixed-size model as row indices; raises where they are no valid list of rows or miss one of the two classes."""
    try:
        rows = np.asarray(landmarks).astype(np.int64).reshape(-1)
    except (TypeError, ValueError):
        raise InvalidParameterError("The landmarks must be a non-empty list of point indices!") from None
    if rows.size == 0 or np.asarray(landmarks).ndim != 1:
        raise InvalidParameterError("The landmarks must be a non-empty list of point indices!")
    N = data.num_data_points()
    if rows.min() < 0 or rows.max() >= N:
        raise InvalidParameterError(f"Every landmark must be the index of a data point (< {N}), but one is {int(rows.max() if rows.max() >= N else rows.min())}!")
    if np.unique(rows).size != rows.size:
        raise InvalidParameterError("The landmarks must be distinct!")
    y = data.mapped_labels()[rows]
    for sign in (-1, 1):
        if not np.any(y == sign):
            raise InvalidParameterError(f'The landmarks hold no point of the class "{data.mapping.label_of(sign)}": a model file groups its support vectors by class, '
                                        "so the landmarks of a two-class model must include both classes!")
    return rows


def _weight_keyword(sample_weight) -> dict:
    """``sample_weight`` as a keyword for the backend boundary of the fixed-size fits -- only where there are weights, so that a backend object written before the
    keyword existed still serves the unweighted fit."""
    return {} if sample_weight is None else {"sample_weight": sample_weight}


def _drop_zero_weights(data: DataSet, sample_weight):
    """``(data of the points of weight > 0, their weights)``: scikit-learn's sample_weight semantics -- finite weights >= 0, a point of weight 0 takes no part."""
    w = np.asarray(sample_weight, dtype=np.float64)
    if w.shape != (data.num_data_points(),):
        raise InvalidParameterError(f"The number of data points ({data.num_data_points()}) and the number of sample weights ({w.size}) must be the same!")
    if not (np.all(np.isfinite(w)) and np.all(w >= 0.0)):
        raise InvalidParameterError("Every sample weight must be finite and greater than or equal to 0.0!")
    keep = np.flatnonzero(w > 0.0)
    if keep.size == w.size:
        return data, np.ascontiguousarray(w)
    labels = data.labels()
    kept_labels = [labels[i] for i in keep.tolist()]
    if keep.size < 2 or len(set(kept_labels)) < 2:
        raise InvalidParameterError(f"The points of weight > 0 ({keep.size} of {w.size}) must include at least two points of two different classes!")
    kept = DataSet(data.data()[keep], kept_labels, real_type=data.real_type)
    return kept, np.ascontiguousarray(w[keep])


class MI355CSVM(CSVM):
    """The MI355X backend (counterpart of plssvm::hip::csvm, HIP/csvm.hpp:39-99, csvm.hip.cpp:47-85)."""

    def __init__(self, target=TargetPlatform.AUTOMATIC, params: Parameter | None = None, num_devices: int = 1, solver: str = "cg", precond_rank: int = 256, precond_landmarks=None,
                 **kwargs):
        """``solver``: ``"cg"`` (default) = the CG of the data's real type; ``"refined"`` = float64 data on ONE device is solved by mixed-precision refinement
        (``backend.solve_refined``: float32 CG iterations on the matrix cores inside a float64 residual loop, same stop test; the gain grows with the iteration
        count) and ``last_refine_info`` keeps the per-solve reports -- float32 data or several devices solve as with ``"cg"`` and leave it None;
        ``"pcg"`` = CG preconditioned with a Nystrom approximation of ``precond_rank`` landmarks (``backend.solve_pcg``), same stop test, built once per
        data set and shared by all right-hand sides -- opt-in: it saves iterations where the kernel matrix has spectral decay and costs some where it has none; one device
        and no sample weights (both raise).  ``precond_landmarks``: None = the library's fixed choice of landmarks, ``"greedy"`` / ``"rpcholesky"`` = ``precond_rank`` points
        selected from the data (``backend.select_landmarks``).

        ``num_devices``: devices ONE solve is sharded over -- 1 (default) = device 0 only, k = devices 0 .. k-1 (gpu_csvm.hpp:283-299),
        0 = automatic (every visible device, at least 4096 points each, as the reference's backends take every device they find,
        csvm.hip.cpp:66-75).  Several devices are OPT-IN: results then depend on the device count through the order of the sums, the exchange
        bootstraps RCCL inside the process, and that path has not run on a multi-GPU box yet."""
        if isinstance(target, Parameter):
            target, params = TargetPlatform.AUTOMATIC, target
        if solver not in ("cg", "refined", "pcg"):
            raise InvalidParameterError(f"solver must be 'cg' or 'refined' or 'pcg', but is {solver!r}!")
        if solver == "pcg" and not (isinstance(precond_rank, (int, np.integer)) and 1 <= int(precond_rank) <= _capi.PRECOND_MAX_RANK):
            raise InvalidParameterError(f"precond_rank must lie in [1, {_capi.PRECOND_MAX_RANK}], but is {precond_rank!r}!")
        if precond_landmarks is not None and precond_landmarks not in _capi.LANDMARK_METHODS:
            raise InvalidParameterError(f"precond_landmarks must be None or one of {sorted(_capi.LANDMARK_METHODS)}, but is {precond_landmarks!r}!")
        super().__init__(params, **kwargs)
        self.solver = solver
        self.precond_rank = int(precond_rank) if solver == "pcg" else None
        self.precond_landmarks = precond_landmarks if solver == "pcg" else None
        self.last_refine_info = None
        if target not in (TargetPlatform.AUTOMATIC, TargetPlatform.GPU_AMD):
            raise BackendError(f"Invalid target platform '{target.value}' for the MI355 backend!")
        self.target_platform = TargetPlatform.GPU_AMD
        self.num_devices = _capi.device_count()
        if self.num_devices <= 0:
            raise BackendError("MI355 backend selected but no HIP capable devices were found!")
        if not 0 <= int(num_devices) <= self.num_devices:
            raise BackendError(f"Requested {num_devices} devices, but only {self.num_devices} are available!")
        self.use_devices = int(num_devices)
        self._options = None  # this object's own tuning knobs (ABI 4): created by the first set_option, None = the process defaults

    def set_option(self, name: str, value: int) -> None:
        """A tuning knob of THIS backend object (``lssvm_mi355_options``; names as ``lssvm_mi355_set_option``): other objects and the process defaults are not touched --
        the reference's backend objects share no state beyond ``verbosity`` either (csvm.hpp:50-83)."""
        if self._options is None:
            self._options = _capi.Options()
        self._options.set(name, value)

    def get_option(self, name: str) -> int:
        return self._options.get(name) if self._options is not None else _capi.get_option(name)

    def solve_system_of_linear_equations(self, params, A, b, eps, max_iter, sample_weight=None):
        self.last_refine_info = None
        if self.solver == "pcg":
            self._pcg_applies(sample_weight)
            return backend.solve_pcg(params, A, b, eps, max_iter, rank=self._pcg_rank(A), landmarks=self.precond_landmarks, options=self._options)
        if self._refines(A):
            alpha, rho, info, refine = backend.solve_refined(params, A, b, eps, max_iter, sample_weight=sample_weight, options=self._options)
            self.last_refine_info = [refine]
            return alpha, rho, info
        # all devices of this process behind ONE call (gpu_csvm::solve_system_of_linear_equations_impl, gpu_csvm.hpp:477-654)
        return backend.solve_system_of_linear_equations(params, A, b, eps, max_iter, num_devices=self.use_devices, options=self._options, sample_weight=sample_weight)

    def solve_cost_path(self, params, A, b, costs, eps, max_iter):
        """Every cost from ONE multi-shift CG sequence on device 0 (``backend.solve_cost_path``): one pass over the Gram tiles per iteration for the whole grid.  The stop
        test is the path's own (``include/plssvm_amd.h``); every cost's true residual is verified and reported in its info.  A backend object of several devices raises, as the library does: the path does not run on a sharded problem."""
        self._one_device_path()
        alphas, rhos, infos, passes = backend.solve_cost_path(params, A, b, costs, eps, max_iter, verify=True, options=self._options)
        for info in infos:
            info["path_passes"] = passes
        return alphas, rhos, infos

    def solve_cost_paths(self, params, A, B, costs, eps, max_iter):
        """One cost path per row of ``B`` on ONE resident problem (``ResidentProblem.solve_cost_path``): the data is uploaded and prepared (q, operand planes) once for all
        the right-hand sides, as :meth:`solve_systems_of_linear_equations` does.  Each path gives the bits of a one-shot :meth:`solve_cost_path`."""
        self._one_device_path()
        A = backend._as_matrix(A)
        B = np.ascontiguousarray(B, dtype=A.dtype)
        if B.ndim != 2 or B.shape[0] == 0 or B.shape[1] != A.shape[0]:
            raise InvalidParameterError(f"The number of data points in the matrix A ({A.shape[0]}) and the values in every right hand side vector ({B.shape[-1] if B.ndim else 0}) must be the same!")
        solved = []
        with backend.ResidentProblem(params, A, devices=[0], options=self._options) as prob:  # (device 0 alone, as the one-shot path creates it)
            for b in B:
                alphas, rhos, infos, passes = prob.solve_cost_path(b, costs, eps, max_iter, verify=True)
                for info in infos:
                    info["path_passes"] = passes
                solved.append((alphas, rhos, infos))
        return solved

    def solve_reduced_systems(self, params, A, Y, rank, landmarks=None, factor="host", sample_weight=None):
        """``backend.fit_reduced`` on device 0: one landmark block, one Gram matrix on the fp64 matrix cores and one factorisation for all rows of ``Y``.  A backend object of
        several devices raises, as the library does on a sharded problem."""
        if self.use_devices != 1:
            raise InvalidParameterError(f"The reduced model is fitted on one device, but this backend object shards a solve over {'every visible device' if self.use_devices == 0 else self.use_devices}"
                                        f"{'' if self.use_devices == 0 else ' devices'} (num_devices={self.use_devices})!")
        return backend.fit_reduced(params, A, Y, rank, landmarks=landmarks, options=self._options, factor=factor, sample_weight=sample_weight)

    def solve_reduced_logistic_systems(self, params, A, Y, rank, landmarks=None, sample_weight=None, tol=1e-8, max_iter=50, factor="host", start=None):
        """``backend.fit_reduced_logistic`` on device 0: the rows of ``Y`` in lockstep, one evaluation of the landmark block per pass for all of them.  A backend object of
        several devices raises, as :meth:`solve_reduced_systems` does."""
        if self.use_devices != 1:
            raise InvalidParameterError(f"The reduced model is fitted on one device, but this backend object shards a solve over {'every visible device' if self.use_devices == 0 else self.use_devices}"
                                        f"{'' if self.use_devices == 0 else ' devices'} (num_devices={self.use_devices})!")
        return backend.fit_reduced_logistic(params, A, Y, rank, landmarks=landmarks, sample_weight=sample_weight, tol=tol, max_iter=max_iter, factor=factor, start=start,
                                            options=self._options)

    def solve_reduced_loo_systems(self, params, A, Y, rank, costs, landmarks=None, factor="host", sample_weight=None):
        """``backend.fit_reduced_loo`` on device 0: one landmark block and one Gram matrix for all costs and rows of ``Y``, then one leverage pass per cost on the fp64
        matrix cores.  A backend object of several devices raises, as :meth:`solve_reduced_systems` does."""
        if self.use_devices != 1:
            raise InvalidParameterError(f"The reduced model is fitted on one device, but this backend object shards a solve over {'every visible device' if self.use_devices == 0 else self.use_devices}"
                                        f"{'' if self.use_devices == 0 else ' devices'} (num_devices={self.use_devices})!")
        return backend.fit_reduced_loo(params, A, Y, rank, costs, landmarks=landmarks, options=self._options, factor=factor, sample_weight=sample_weight)

    def solve_reduced_stream_systems(self, params, landmark_rows, chunks, costs, num_rhs=1, factor="host", loo=False, weighted=False, on_scores=None):
        """``backend.fit_reduced_stream`` on device 0: one reduced stream fed chunk by chunk, one solve for all costs, and for ``loo`` a second walk.  A backend object of
        several devices raises, as :meth:`solve_reduced_systems` does."""
        if self.use_devices != 1:
            raise InvalidParameterError(f"The reduced model is fitted on one device, but this backend object shards a solve over {'every visible device' if self.use_devices == 0 else self.use_devices}"
                                        f"{'' if self.use_devices == 0 else ' devices'} (num_devices={self.use_devices})!")
        return backend.fit_reduced_stream(params, landmark_rows, chunks, costs, num_rhs=num_rhs, factor=factor, loo=loo, weighted=weighted, options=self._options, on_scores=on_scores)

    def solve_reduced_grid_systems(self, params, A, Y, rank, gammas, costs, landmarks=None, factor="host", sample_weight=None, product="matrix"):
        """``backend.fit_reduced_grid`` on device 0: per slab and pass the feature sums once for all gammas, one Gram matrix per gamma, one leverage pass per
        ``(gamma, cost)``.  A backend object of several devices raises, as :meth:`solve_reduced_systems` does."""
        if self.use_devices != 1:
            raise InvalidParameterError(f"The reduced model is fitted on one device, but this backend object shards a solve over {'every visible device' if self.use_devices == 0 else self.use_devices}"
                                        f"{'' if self.use_devices == 0 else ' devices'} (num_devices={self.use_devices})!")
        return backend.fit_reduced_grid(params, A, Y, rank, gammas, costs, landmarks=landmarks, options=self._options, factor=factor, sample_weight=sample_weight, product=product)

    def solve_reduced_rank_path_systems(self, params, A, Y, rank, ranks, costs, landmarks=None, factor="host", sample_weight=None):
        """``backend.fit_reduced_rank_path`` on device 0: one Gram matrix, one factorisation per cost, one prefix leverage pass per cost.  A backend object of several
        devices raises, as :meth:`solve_reduced_systems` does."""
        if self.use_devices != 1:
            raise InvalidParameterError(f"The reduced model is fitted on one device, but this backend object shards a solve over {'every visible device' if self.use_devices == 0 else self.use_devices}"
                                        f"{'' if self.use_devices == 0 else ' devices'} (num_devices={self.use_devices})!")
        return backend.fit_reduced_rank_path(params, A, Y, rank, ranks, costs, landmarks=landmarks, options=self._options, factor=factor, sample_weight=sample_weight)

    def _one_device_path(self) -> None:
        if self.use_devices != 1:
            raise InvalidParameterError(f"The cost path runs on one device, but this backend object shards a solve over {'every visible device' if self.use_devices == 0 else self.use_devices}"
                                        f"{'' if self.use_devices == 0 else ' devices'} (num_devices={self.use_devices})!")

    def _pcg_applies(self, sample_weight) -> None:
        if self.use_devices != 1:
            raise InvalidParameterError(f"solver='pcg' runs on one device, but this backend object shards a solve over {'every visible device' if self.use_devices == 0 else self.use_devices}"
                                        f"{'' if self.use_devices == 0 else ' devices'} (num_devices={self.use_devices})!")
        if sample_weight is not None:
            raise InvalidParameterError("solver='pcg' solves the unweighted system: sample weights need solver='cg'!")

    def _pcg_rank(self, A) -> int:
        """``precond_rank``, but never more landmarks than the reduced system has rows."""
        return max(1, min(self.precond_rank, backend._as_matrix(A).shape[0] - 1))

    def _refines(self, A) -> bool:
        """solver="refined" applies: float64 data on one device."""
        return self.solver == "refined" and self.use_devices == 1 and backend._as_matrix(A).dtype == np.float64

    def predict_values(self, params, support_vectors, alpha, rho, w, predict_points):
        return backend.predict_values(params, support_vectors, alpha, rho, w, predict_points, options=self._options)

    def solve_systems_of_linear_equations(self, params, A, B, eps, max_iter, sample_weight=None):
        """The systems in LOCKSTEP on ONE resident problem (``ResidentProblem.solve_lockstep``): the data is uploaded and prepared (q, operand planes) once, the weights are
        set once, and every right-hand side runs the recipe of the one-shot solve (begin / step / finish) on it -- the same alpha, rho and iteration count as a fresh
        one-shot solve.  In fp64 on the symmetric resident-row-panel kernel, and in fp32 on 129 ... 512 features (polynomial, or rbf with folded records, on the symmetric
        one-pass split kernels), one pass over the Gram tiles serves two right-hand sides per iteration; elsewhere they are solved one after the other.  Several devices: the base class's loop of one-shot solves."""
        self.last_refine_info = None
        if self.solver == "pcg":  # ONE preconditioner for all right-hand sides
            self._pcg_applies(sample_weight)
            B = np.asarray(B)
            if B.ndim != 2 or B.shape[0] == 0:
                raise InvalidParameterError("The right-hand sides must be a matrix with one row per system and at least one row!")
            return backend.solve_pcg(params, A, B, eps, max_iter, rank=self._pcg_rank(A), landmarks=self.precond_landmarks, options=self._options)
        if self.use_devices != 1:
            return super().solve_systems_of_linear_equations(params, A, B, eps, max_iter, sample_weight=sample_weight)
        if self._refines(A):
            B = np.asarray(B)
            if B.ndim != 2 or B.shape[0] == 0:
                raise InvalidParameterError("The right-hand sides must be a matrix with one row per system and at least one row!")
            alphas, rhos, infos, refine = backend.solve_refined(params, A, B, eps, max_iter, sample_weight=sample_weight, options=self._options)
            self.last_refine_info = refine
            return alphas, rhos, infos
        A = backend._as_matrix(A)
        N = A.shape[0]
        B = np.ascontiguousarray(B, dtype=A.dtype)
        if B.ndim != 2 or B.shape[0] == 0 or B.shape[1] != N:
            raise InvalidParameterError(f"The number of data points in the matrix A ({N}) and the values in every right hand side vector ({B.shape[-1] if B.ndim else 0}) must be the same!")
        if not eps > 0.0:
            raise InvalidParameterError(f"The stopping criterion in the CG algorithm must be greater than 0.0, but is {eps}!")
        if not max_iter > 0:
            raise InvalidParameterError("The number of CG iterations must be greater than 0!")
        with backend.ResidentProblem(params, A, devices=[0], options=self._options) as prob:  # (device 0 alone, as the one-shot solve creates it)
            if sample_weight is not None:
                prob.set_weights(sample_weight)
            alphas, rhos, infos, _ = prob.solve_lockstep(B, eps, max_iter)  # (one device: option rebalance_after has nothing to move)
        return alphas, rhos, infos

    def predict_values_multi(self, params, support_vectors, alphas, rhos, ws, predict_points):
        return backend.predict_values_multi(params, support_vectors, alphas, rhos, ws, predict_points, options=self._options)

    def decision_values_resident(self, model, X):
        """The decision values ``f[i, c]`` of a :class:`plssvm_amd.multiclass.OneVsAllModel` with the model RESIDENT in HBM from the first call on
        (``lssvm_mi355_predictor_create_panels``: every resident form the library has, float64 and the models beyond the one-pass kernels included): later calls with the same model upload only their points.  The predictor is cached on the model and made again (the old
        one closed) under the rule of :meth:`predict`: another backend object, changed option values, kernel parameters, another support-vector array (by identity),
        ``alpha`` (by value) or ``rho``."""
        sv = model.support_vectors
        opts = tuple(self._options.get(n) if self._options is not None else _capi.get_option(n) for n in _capi.OPTION_NAMES)
        prm = model.params
        params = (int(prm.kernel_type), prm.degree, prm.gamma, prm.coef0)
        cached = getattr(model, "_predictor", None)
        if (cached is None or cached["owner"] is not self or cached["options"] != opts or cached["params"] != params or cached["sv"] is not sv
                or not np.array_equal(cached["alpha"], model.alpha) or not np.array_equal(cached["rho"], model.rho)):
            if cached is not None:
                cached["predictor"].close()  # (its HBM: nothing else holds it)
            alpha, rho = np.array(model.alpha, copy=True), np.array(model.rho, copy=True)
            cached = {"owner": self, "options": opts, "params": params, "sv": sv, "alpha": alpha, "rho": rho,
                      "predictor": backend.Predictor(model.params, sv, alpha, rho, options=self._options, panels=True)}
            model._predictor = cached
        return cached["predictor"].predict(np.asarray(X, dtype=sv.dtype))

    def predict(self, model: Model, data: DataSet):
        """csvm::predict (csvm.hpp:322-342) with the model RESIDENT in HBM from the first call on (``lssvm_mi355_predictor_create_panels``): later calls with the same model upload only
        their points.  Same labels as the base class's one-shot ``predict_values`` with the state of the moment: the resident predictor is made again (and the old one
        closed) when this object's options -- or, without options of its own, the process defaults --, the model's parameters, its support-vector array (by identity),
        ``alpha`` (compared by value, in place edits included) or ``rho`` have changed since it was made.  Editing the support-vector matrix IN PLACE is not detected."""
        if model.num_features() != data.num_features():
            raise InvalidParameterError(f"Number of features per data point ({data.num_features()}) must match the number of features per support vector of the "
                                        f"provided model ({model.num_features()})!")
        t0 = time.perf_counter()
        sv = model.support_vectors()
        opts = tuple(self._options.get(n) if self._options is not None else _capi.get_option(n) for n in _capi.OPTION_NAMES)
        prm = model.params
        params = (int(prm.kernel_type), prm.degree, prm.gamma, prm.coef0)
        cached = getattr(model, "_predictor", None)
        if (cached is None or cached["owner"] is not self or cached["options"] != opts or cached["params"] != params or cached["sv"] is not sv
                or not np.array_equal(cached["alpha"], model.alpha) or cached["rho"] != float(model.rho)):
            if cached is not None:
                cached["predictor"].close()  # (its HBM: nothing else holds it)
            alpha = np.array(model.alpha, copy=True)
            cached = {"owner": self, "options": opts, "params": params, "sv": sv, "alpha": alpha, "rho": float(model.rho),
                      "predictor": backend.Predictor(model.params, sv, alpha, float(model.rho), options=self._options, panels=True)}
            model._predictor = cached
        t1 = time.perf_counter()
        info = {}
        values = cached["predictor"].predict(data.data(), info_out=info)
        t2 = time.perf_counter()
        mapper = model.data.mapping
        pos, neg = mapper.label_of(1), mapper.label_of(-1)
        labels = [pos if p else neg for p in (np.asarray(values) > 0).tolist()]  # operators.hpp:180-182 sign, csvm.hpp:337-340
        # where the call's time went, in seconds (the command line's timing block and bench.py's `e2e` print it)
        self.last_predict_phases = {"model_to_hbm_s": t1 - t0, "values_s": t2 - t1, "library_total_ms": float(info.get("total_ms", 0.0)), "kernel_ms": float(info.get("kernel_ms", 0.0)),
                                    "resident": int(info.get("resident", 0)), "labels_s": time.perf_counter() - t2}
        return labels


def make_csvm(backend_type=BackendType.AUTOMATIC, *args, **kwargs) -> CSVM:
    """plssvm::make_csvm (csvm_factory.hpp:123-171).  ``automatic`` / ``mi355`` / ``hip`` select the MI355X backend; every other
    enumerator raises UnsupportedBackendError("No {} backend available!") like a reference build without that backend."""
    if isinstance(backend_type, str):
        try:
            backend_type = BackendType(backend_type.lower())
        except ValueError:
            raise UnsupportedBackendError("Unrecognized backend provided!") from None
    if not isinstance(backend_type, BackendType):
        args = (backend_type,) + args
        backend_type = BackendType.AUTOMATIC
    if backend_type in (BackendType.AUTOMATIC, BackendType.MI355, BackendType.HIP):
        return MI355CSVM(*args, **kwargs)
    raise UnsupportedBackendError(f"No {backend_type.value} backend available!")
