"""CPU: the cost path (lssvm_mi355_problem_solve_cost_path, lssvm_mi355_solve_cost_path_f32 / _f64) without a GPU --

  * the three entry points are declared, bound and exported, and ``lssvm_path_info`` has one size in the header, the library and the binding;
  * every rejected argument is LSSVM_ERR_INVALID_ARGUMENT (InvalidParameterError) before a device is touched, never LSSVM_ERR_NO_DEVICE;
  * ``CSVM.fit_cost_path``, ``svc.fit_cost_path`` and ``svc.cost_path_scores`` against a dense stand-in backend;
  * the numpy model of the recurrences (tests/cost_path_model.py) against dense float64 solves: every cost's true residual meets the stop test,
    |P (b - Abar x)| <= eps |P b| -- the precondition of the bound tests/test_gpu_cost_path.py asserts on the device (2 eps)."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cost_path_model as cpm
from conftest import ROOT
from plssvm_amd import _capi, backend, csvm, svc
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter

NAMES = ["lssvm_mi355_problem_solve_cost_path", "lssvm_mi355_solve_cost_path_f32", "lssvm_mi355_solve_cost_path_f64"]
COSTS = [100.0, 0.1, 1.0, 10.0, 1000.0]


def costs_of(kernel, dtype, d=20):
    """The grid of a case.  float32 with the linear kernel: costs up to 10 on 20 features and up to 1 on 200 (whose Gram matrix is ten times larger) -- beyond that the
    ridge 1 / C lies below float32's resolution of a rank-d matrix, and float32 CG drifts with or without shifts."""
    if kernel == "linear" and dtype == np.float32:
        return [0.1, 1.0, 10.0] if d <= 20 else [0.01, 0.1, 1.0]
    return COSTS


def path_inputs(N, d=20, seed=7):
    """The inputs of the model and of the GPU tests: uniform(-1, 1) points, +-1 labels."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (N, d)), np.where(rng.uniform(size=N) < 0.5, -1.0, 1.0)


# ------------------------------------------------------------------ the C surface
@pytest.mark.parametrize("name", NAMES)
def test_symbol_in_header_binding_and_library(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plssvm_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", header), "not declared in include/plssvm_amd.h"
    assert name in _capi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T " + name + r"$", out, flags=re.M), "not exported by the built library"
    assert _capi.cost_path_entry(name).restype is C.c_int


def test_path_info_has_one_size_everywhere():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plssvm_amd.h")).read(), flags=re.S)
    body = re.search(r"typedef struct lssvm_path_info \{(.*?)\} lssvm_path_info;", header, flags=re.S).group(1)
    sizes = {"uint64_t": 8, "int32_t": 4, "double": 8}
    fields = [(t, n.strip()) for t, names in re.findall(r"(uint64_t|int32_t|double)\s+([^;]+);", body) for n in names.split(",")]
    assert [n for _, n in fields] == [n for n, _ in _capi.LssvmPathInfo._fields_]
    assert sum(sizes[t] for t, _ in fields) == C.sizeof(_capi.LssvmPathInfo) == 48  # (no padding: 8 | 4 4 | 8 8 8 | 8)
    capi = open(os.path.join(ROOT, "plssvm_amd", "csrc", "capi.hip")).read()
    assert "static_assert(sizeof(lssvm_path_info) == 48" in capi


def test_problem_call_refuses_a_null_handle():
    """Without a device there is no live problem, and a made-up handle would be dereferenced as soon as the order of the checks changed: only the NULL handle is tried
    here.  The argument checks the two calls share (check_cost_path_arguments) are tried through the one-shot entry points below, and on a live problem in
    tests/test_gpu_cost_path.py."""
    y, costs, alphas, rhos, infos = np.ones(8), np.array([1.0, 10.0]), np.zeros((2, 8)), np.zeros(2), (_capi.LssvmPathInfo * 2)()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    with pytest.raises(InvalidParameterError, match="problem handle must not be NULL"):
        _capi.check(_capi.cost_path_entry(NAMES[0])(None, _capi.ptr(y), dp(costs), 2, 1e-3, 10, 1, _capi.ptr(alphas), dp(rhos), infos, None))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_shot_call_refuses_invalid_arguments_before_any_device(dtype):
    """LSSVM_ERR_INVALID_ARGUMENT (-1), not LSSVM_ERR_NO_DEVICE (-2), on a machine with or without a GPU -- through the raw entry point, past the Python checks."""
    X, y = path_inputs(12, 3)
    X, y = X.astype(dtype), y.astype(dtype)
    ps = backend._params_struct(Parameter(kernel_type="rbf"), 3)
    fn = _capi.cost_path_entry(f"lssvm_mi355_solve_cost_path_{_capi.suffix_of(dtype)}")
    alphas, rhos, infos = np.zeros((2, 12), dtype), np.zeros(2), (_capi.LssvmPathInfo * 2)()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    op = lambda a: None if a is None else _capi.ptr(a)  # noqa: E731

    def status(costs=np.array([1.0, 10.0]), m=2, eps=1e-3, max_iter=10, params=ps, N=12, d=3, y_=y, alphas_=alphas, rhos_=rhos, infos_=infos):
        return fn(None if params is None else C.byref(params), _capi.ptr(X), N, d, op(y_), dp(costs), m, eps, max_iter, 1, op(alphas_), dp(rhos_), infos_, None, None)

    assert status(m=0) == -1 and "number of costs must be greater than 0" in _capi.last_error()
    assert status(costs=np.ones(65), m=65) == -1 and "at most 64 costs" in _capi.last_error()
    assert status(costs=None) == -1 and "costs must not be NULL" in _capi.last_error()
    for bad in ([1.0, 0.0], [-1.0, 1.0], [1.0, np.inf], [np.nan, 1.0]):
        assert status(costs=np.array(bad)) == -1 and "finite and greater than 0.0" in _capi.last_error(), bad
    for bad in (0.0, -1e-3, float("nan")):
        assert status(eps=bad) == -1 and "stopping criterion in the CG algorithm must be greater than 0.0" in _capi.last_error(), bad
    assert status(max_iter=0) == -1 and "number of CG iterations must be greater than 0" in _capi.last_error()
    assert status(alphas_=None) == -1 and "must not be NULL" in _capi.last_error()
    assert status(rhos_=None) == -1 and "must not be NULL" in _capi.last_error()
    assert status(infos_=None) == -1 and "must not be NULL" in _capi.last_error()
    assert status(params=None) == -1
    assert status(y_=None) == -1 and "right hand side" in _capi.last_error()
    assert status(N=0) == -1 and "must not be empty" in _capi.last_error()
    assert status(d=0) == -1 and "feature" in _capi.last_error()


def test_python_checks_come_before_the_library():
    X, y = path_inputs(12, 3)
    p = Parameter(kernel_type="rbf")
    for costs, message in (([], "number of costs"), (np.ones(65), "at most 64"), ([1.0, 0.0], "finite and greater"), ([1.0, np.nan], "finite and greater"), ([[1.0, 2.0]], "number of costs")):
        with pytest.raises(InvalidParameterError, match=message):
            backend.solve_cost_path(p, X, y, costs, 1e-3, 10)
    with pytest.raises(InvalidParameterError, match="stopping criterion"):
        backend.solve_cost_path(p, X, y, [1.0], 0.0, 10)
    with pytest.raises(InvalidParameterError, match="CG iterations"):
        backend.solve_cost_path(p, X, y, [1.0], 1e-3, 0)
    with pytest.raises(InvalidParameterError, match="right hand side"):
        backend.solve_cost_path(p, X, y[:-1], [1.0], 1e-3, 10)
    assert "solve_cost_path" in backend.__all__ and hasattr(backend.ResidentProblem, "solve_cost_path")


# ------------------------------------------------------------------ fit_cost_path / cost_path_scores against a dense stand-in backend
def cross_kernel(params, A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    G = A @ B.T
    kt = int(params.kernel_type)
    if kt == 0:
        return G
    if kt == 1:
        return (params.gamma * G + params.coef0) ** params.degree
    return np.exp(-params.gamma * np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * G, 0.0))


class DenseBackend(csvm.CSVM):
    """The two boundary methods by dense float64 algebra; the cost path is the base class's loop of solves -- and counts its calls."""

    def __init__(self, params=None, **kwargs):
        super().__init__(params, **kwargs)
        self.solves, self.path_calls, self.paths_calls = [], 0, 0

    def solve_system_of_linear_equations(self, params, A, b, eps, max_iter):
        self.solves.append(params.cost)
        K, q, k_ll, rhs, y_last = cpm.reduced_parts(cross_kernel(params, A, A), b)
        x = cpm.dense_solve(K, q, k_ll, rhs, params.cost)
        alpha_last, rho = cpm.finish(x, q, k_ll, y_last, params.cost)
        return np.append(x, alpha_last), rho, {"iterations": 7}

    def solve_cost_path(self, params, A, b, costs, eps, max_iter):
        self.path_calls += 1
        return super().solve_cost_path(params, A, b, costs, eps, max_iter)

    def solve_cost_paths(self, params, A, B, costs, eps, max_iter):
        self.paths_calls += 1
        return super().solve_cost_paths(params, A, B, costs, eps, max_iter)

    def predict_values(self, params, support_vectors, alpha, rho, w, predict_points):
        return cross_kernel(params, predict_points, support_vectors) @ np.asarray(alpha, dtype=np.float64) - rho, None


class DensePredictor:
    """backend.Predictor's surface for a matrix of weight vectors."""
    made = 0

    def __init__(self, params, support_vectors, alpha, rho, options=None, every_form=False):
        type(self).made += 1
        self.params, self.sv, self.alpha, self.rho = params, support_vectors, np.asarray(alpha), np.asarray(rho)

    def predict(self, points, info_out=None):
        return cross_kernel(self.params, points, self.sv) @ self.alpha.T.astype(np.float64) - self.rho

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


def test_csvm_fit_cost_path_returns_one_model_per_cost():
    X, y = path_inputs(40, 5)
    data = DataSet(X, y.tolist())
    svm = DenseBackend(Parameter(kernel_type="rbf", cost=123.0))
    models = svm.fit_cost_path(data, COSTS, epsilon=1e-6)
    assert svm.path_calls == 1 and svm.solves == COSTS  # (the object's own cost is ignored)
    assert [m.params.cost for m in models] == COSTS and all(m.params.gamma == 1.0 / 5 for m in models)
    assert len(svm.last_cg_info) == len(COSTS)
    for m, cost in zip(models, COSTS):
        one = DenseBackend(Parameter(kernel_type="rbf", cost=cost)).fit(data, epsilon=1e-6)
        assert np.array_equal(m.alpha, one.alpha) and m.rho == one.rho
        assert m.support_vectors() is models[0].support_vectors()  # the models share their support vectors
    with pytest.raises(InvalidParameterError, match="number of costs"):
        svm.fit_cost_path(data, [])
    with pytest.raises(InvalidParameterError, match="finite and greater"):
        svm.fit_cost_path(data, [1.0, -1.0])
    with pytest.raises(InvalidParameterError, match="epsilon"):
        svm.fit_cost_path(data, [1.0], epsilon=0.0)
    with pytest.raises(InvalidParameterError, match="max_iter"):
        svm.fit_cost_path(data, [1.0], max_iter=0)


@pytest.mark.parametrize("num_classes", [2, 3])
def test_svc_fit_cost_path_gives_fitted_clones(monkeypatch, num_classes):
    made = []

    def make(params=None):
        made.append(DenseBackend(params))
        return made[-1]

    monkeypatch.setattr(svc, "make_csvm", make)
    X, y = path_inputs(60, 4)
    labels = np.array(["a", "b", "c"])[np.arange(60) % num_classes]
    est = svc.SVC(kernel="rbf", C=5.0, tol=1e-6)
    fitted = svc.fit_cost_path(est, X, labels, COSTS)
    assert est._fit is None  # (the estimator itself stays unfitted)
    assert len(made) == 1 and made[0].path_calls == (1 if num_classes == 2 else 3)  # binary: one call; one-vs-all: one per class ...
    assert made[0].paths_calls == (0 if num_classes == 2 else 1)  # ... behind ONE call of the backend for all the classes
    assert [f.C for f in fitted] == COSTS and all(f.kernel == "rbf" and f.tol == 1e-6 for f in fitted)
    for f, cost in zip(fitted, COSTS):
        one = svc.SVC(kernel="rbf", C=cost, tol=1e-6).fit(X, labels)
        assert np.allclose(f.dual_coef_, one.dual_coef_, rtol=0, atol=1e-12) and np.allclose(f.intercept_, one.intercept_, rtol=0, atol=1e-12)
        assert f.dual_coef_.shape == ((1, 60) if num_classes == 2 else (3, 60))
        assert np.array_equal(f.classes_, one.classes_) and np.array_equal(f.predict(X[:9]), one.predict(X[:9]))
    with pytest.raises(InvalidParameterError, match="class_weight"):
        svc.fit_cost_path(svc.SVC(class_weight="balanced"), X, labels, COSTS)
    with pytest.raises(InvalidParameterError, match="SVC"):
        svc.fit_cost_path(object(), X, labels, COSTS)


class CountingProblem:
    """backend.ResidentProblem's surface as MI355CSVM.solve_cost_paths uses it: counts the problems created and the paths solved on each."""
    created = []

    def __init__(self, params, A, devices=None, options=None):
        type(self).created.append(self)
        self.params, self.A, self.devices, self.paths, self.open = params, np.asarray(A), devices, 0, True

    def solve_cost_path(self, y, costs, eps, max_iter, verify=True):
        assert self.open
        self.paths += 1
        K, q, k_ll, rhs, y_last = cpm.reduced_parts(cross_kernel(self.params, self.A, self.A), np.asarray(y, dtype=np.float64))
        xs = [cpm.dense_solve(K, q, k_ll, rhs, c) for c in costs]
        ends = [cpm.finish(x, q, k_ll, y_last, c) for x, c in zip(xs, costs)]
        infos = [{"iterations": 7, "converged": 1, "verified": 1} for _ in costs]
        return np.stack([np.append(x, e[0]) for x, e in zip(xs, ends)]), np.array([e[1] for e in ends]), infos, (7, len(costs))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.open = False


def one_shot_must_not_run(*args, **kwargs):
    raise AssertionError("the one-shot cost path uploads and prepares the data again: one-vs-all must stay on its resident problem")


def test_one_vs_all_cost_paths_share_one_resident_problem(monkeypatch):
    """More than two classes: ONE problem is created (one upload, one preparation) and every class's path runs on it -- through MI355CSVM itself, the library behind it
    replaced by a dense stand-in."""
    monkeypatch.setattr(_capi, "device_count", lambda: 1)
    monkeypatch.setattr(backend, "ResidentProblem", CountingProblem)
    monkeypatch.setattr(backend, "solve_cost_path", one_shot_must_not_run)
    monkeypatch.setattr(svc, "make_csvm", lambda params=None: csvm.MI355CSVM(params=params))
    CountingProblem.created = []
    X, y = path_inputs(60, 4)
    labels = np.array(["a", "b", "c", "d"])[np.arange(60) % 4]
    fitted = svc.fit_cost_path(svc.SVC(kernel="rbf", tol=1e-6), X, labels, COSTS)
    assert len(CountingProblem.created) == 1 and CountingProblem.created[0].paths == 4 and CountingProblem.created[0].devices == [0]
    assert not CountingProblem.created[0].open  # (and it is closed again)
    assert [f.C for f in fitted] == COSTS and all(f.dual_coef_.shape == (4, 60) for f in fitted)
    dense = DenseBackend(Parameter(kernel_type="rbf", gamma=0.25))
    for f, cost in zip(fitted, COSTS):
        for c in range(4):
            alpha, rho, _ = dense.solve_system_of_linear_equations(Parameter(kernel_type="rbf", gamma=0.25, cost=cost), X, np.where(labels == "abcd"[c], 1.0, -1.0), 1e-6, 60)
            assert np.allclose(f.dual_coef_[c], alpha, rtol=0, atol=1e-12) and np.isclose(f.intercept_[c], -rho, rtol=0, atol=1e-12)


def test_a_backend_of_several_devices_refuses_the_cost_path(monkeypatch):
    """The library rejects a sharded problem; the backend object says so too, and does not fall back to solves with another stop test."""
    monkeypatch.setattr(_capi, "device_count", lambda: 2)
    monkeypatch.setattr(backend, "solve_cost_path", one_shot_must_not_run)
    X, y = path_inputs(12, 3)
    for num_devices in (0, 2):
        svm = csvm.MI355CSVM(params=Parameter(kernel_type="rbf"), num_devices=num_devices)
        with pytest.raises(InvalidParameterError, match="runs on one device"):
            svm.fit_cost_path(DataSet(X, y.tolist()), [1.0, 10.0])
        with pytest.raises(InvalidParameterError, match="runs on one device"):
            svm.solve_cost_paths(svm.params, X, np.stack([y, -y]), [1.0, 10.0], 1e-3, 10)


def test_cost_path_scores_checks_the_class_count_before_it_fits(monkeypatch):
    def make(params=None):
        raise AssertionError("nothing is fitted for labels of three classes")

    monkeypatch.setattr(svc, "make_csvm", make)
    X, y = path_inputs(30, 4)
    with pytest.raises(InvalidParameterError, match="two-class"):
        svc.cost_path_scores(svc.SVC(), X, np.arange(30) % 3, COSTS, X[:5], np.arange(5) % 3)


def test_svc_cost_path_scores_uses_one_predictor_for_all_costs(monkeypatch):
    monkeypatch.setattr(svc, "make_csvm", lambda params=None: DenseBackend(params))
    monkeypatch.setattr(backend, "Predictor", DensePredictor)
    X, y = path_inputs(80, 4)
    Xv, yv = path_inputs(30, 4, seed=8)
    est = svc.SVC(kernel="polynomial", tol=1e-6)
    before = DensePredictor.made
    scores, fitted = svc.cost_path_scores(est, X, y, COSTS, Xv, yv)
    assert DensePredictor.made == before + 1 and scores.shape == (len(COSTS),) and len(fitted) == len(COSTS)
    for s, cost in enumerate(COSTS):
        assert scores[s] == svc.SVC(kernel="polynomial", C=cost, tol=1e-6).fit(X, y).score(Xv, yv)
    with pytest.raises(InvalidParameterError, match="two-class"):
        svc.cost_path_scores(est, X, np.arange(80) % 3, COSTS, Xv, yv)


# ------------------------------------------------------------------ the model against dense solves
@pytest.mark.parametrize("kernel", ["linear", "polynomial", "rbf"])
@pytest.mark.parametrize("N,d,dtype,eps", [(N, 20, dtype, eps) for N in (130, 700) for dtype, eps in ((np.float64, 1e-9), (np.float32, 1e-3))]
                         + [(700, 200, np.float32, 1e-3), (700, 300, np.float64, 1e-9)])  # (the shapes of tests/test_gpu_cost_path.py)
def test_model_meets_the_stop_test_in_the_true_residual(N, d, dtype, eps, kernel):
    """Every cost's true |P (b - Abar x)| <= eps |P b|, the seed takes the most iterations, and a looser cost never freezes later than a harder one.  (float32, linear
    kernel: the smaller grids of costs_of.)"""
    X, y = path_inputs(N, d)
    costs = costs_of(kernel, dtype, d)
    K, q, k_ll, b, _ = cpm.reduced_parts(cpm.kernel_matrix(kernel, X.astype(dtype)), y)
    xs, iterations, converged, seed_iterations = cpm.multi_shift_cg(K, q, k_ll, b, costs, eps, 2000, dtype)
    assert converged.all() and xs.dtype == dtype
    norm_b = np.linalg.norm(cpm.apply_P(b))
    for s, cost in enumerate(costs):
        assert cpm.true_residual_norm(K, q, k_ll, b, cost, xs[s]) <= eps * norm_b, (cost, cpm.true_residual_norm(K, q, k_ll, b, cost, xs[s]) / norm_b)
    assert seed_iterations == iterations.max() == iterations[int(np.argmax(costs))]
    order = np.argsort(costs)
    assert np.all(np.diff(iterations[order]) >= 0)
    if dtype == np.float64:  # ... and the solutions are the dense ones
        kappa = cpm.condition_numbers(K, q, k_ll, costs)
        for s, cost in enumerate(costs):
            z, z_star = cpm.apply_P_inv(xs[s]), cpm.apply_P_inv(cpm.dense_solve(K, q, k_ll, b, cost))
            assert np.linalg.norm(z - z_star) <= 2 * eps * kappa[s] * np.linalg.norm(z_star)


def test_model_handles_duplicates_order_and_max_iter():
    X, y = path_inputs(130)
    K, q, k_ll, b, _ = cpm.reduced_parts(cpm.kernel_matrix("rbf", X), y)
    xs, its, conv, _ = cpm.multi_shift_cg(K, q, k_ll, b, [10.0, 1.0, 10.0], 1e-9, 2000)
    assert np.array_equal(xs[0], xs[2]) and its[0] == its[2]
    xs2, its2, _, _ = cpm.multi_shift_cg(K, q, k_ll, b, [1.0, 10.0, 10.0], 1e-9, 2000)
    assert np.array_equal(xs2[0], xs[1]) and np.array_equal(xs2[1], xs[0]) and its2[0] == its[1]
    xs3, its3, conv3, seed3 = cpm.multi_shift_cg(K, q, k_ll, b, [10.0, 1.0], 1e-9, 3)
    assert seed3 == 3 and not conv3.any() and np.all(its3 == 3) and np.all(np.isfinite(xs3))
