"""CPU: the weighted LS-SVM system (lssvm_mi355_solve_weighted_*, lssvm_mi355_problem_set_weights) -- the reduction of the bordered weighted dual that
the library solves, restated in float64 numpy on the oracle's kernel values, and the argument checks the entry points make before they touch a device."""

import ctypes as C

import numpy as np
import pytest

from plssvm_amd import _capi, backend
from plssvm_amd.csvm import CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.datagen import make_blobs_pm1
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter

KW = dict(degree=3, gamma=1.0 / 8, coef0=0.5)


def oracle_kernel_matrix(orc, kernel, X):
    N = X.shape[0]
    K = np.empty((N, N))
    for i in range(N):
        for j in range(i, N):
            K[i, j] = K[j, i] = orc.kernel_function(kernel, X[i], X[j], **KW)
    return K


def reduced_system(K, y, cost, v):
    """Abar(v), b and QA_cost(v) of the weighted system with b eliminated through the last point (include/plssvm_amd.h)."""
    n = K.shape[0] - 1
    q = K[:n, n]
    QA = K[n, n] + 1.0 / (cost * v[n])
    A = K[:n, :n] + np.diag(1.0 / (cost * v[:n])) + QA - q[:, None] - q[None, :]
    return A, y[:n] - y[n], q, QA


def solve_reduced(K, y, cost, v):
    A, b, q, QA = reduced_system(K, y, cost, v)
    x = np.linalg.solve(A, b)
    bias = y[-1] + QA * x.sum() - q @ x
    return np.append(x, -x.sum()), -bias


def solve_bordered(K, y, cost, v):
    """[0 1^T; 1 K + diag(1 / (C v))] [b; alpha] = [0; y]: the weighted LS-SVM dual (Suykens et al. 2002)."""
    N = K.shape[0]
    M = np.zeros((N + 1, N + 1))
    M[0, 1:] = M[1:, 0] = 1.0
    M[1:, 1:] = K + np.diag(1.0 / (cost * v))
    sol = np.linalg.solve(M, np.concatenate([[0.0], y]))
    return sol[1:], -sol[0]


@pytest.mark.parametrize("kernel", ["linear", "polynomial", "rbf"])
def test_reduction_of_the_weighted_dual(oracle, kernel):
    X, y = make_blobs_pm1(300, 8, seed=5, dtype=np.float64)
    K = oracle_kernel_matrix(oracle, kernel, X)
    rng = np.random.default_rng(7)
    cost = 0.7
    for v in (np.exp(rng.uniform(np.log(0.1), np.log(10.0), 300)), np.where(np.arange(300) == 299, 7.5, 1.0)):
        a_red, rho_red = solve_reduced(K, y, cost, v)
        a_full, rho_full = solve_bordered(K, y, cost, v)
        scale = np.abs(a_full).max()
        assert np.abs(a_red - a_full).max() <= 1e-10 * scale, kernel
        assert abs(rho_red - rho_full) <= 1e-10 * max(1.0, abs(rho_full)), kernel
    # v == 1 is the unweighted system (csvm.cpp:86, :297), v == 2 the unweighted system at cost 2C
    A1, _, _, QA1 = reduced_system(K, y, cost, np.ones(300))
    assert QA1 == K[-1, -1] + 1.0 / cost
    A2, _, _, _ = reduced_system(K, y, cost, np.full(300, 2.0))
    A2c, _, _, _ = reduced_system(K, y, 2.0 * cost, np.ones(300))
    assert np.array_equal(A2, A2c)


def _solve_weighted_status(w, dtype=np.float64, weights_null=False, X_null=False, y_null=False, alpha_null=False):
    X = np.ones((4, 3), dtype=dtype)
    y = np.array([1.0, -1, 1, -1], dtype=dtype)
    alpha = np.zeros(4, dtype=dtype)
    ct = _capi.ctype_of(dtype)
    rho = ct(0)
    info = _capi.LssvmCgInfo()
    ps = _capi.LssvmParams(0, 3, 1.0, 0.0, 1.0)
    fn = _capi.weighted_entry(f"lssvm_mi355_solve_weighted_{_capi.suffix_of(dtype)}")
    w = np.ascontiguousarray(w, dtype=np.float64)
    return fn(C.byref(ps), None if X_null else _capi.ptr(X), 4, 3, None if y_null else _capi.ptr(y), None if weights_null else _capi.weights_ptr(w), 1e-3, 4,
              None if alpha_null else _capi.ptr(alpha), C.byref(rho), C.byref(info), None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weight_arguments_are_checked_before_any_device(dtype):
    """LSSVM_ERR_INVALID_ARGUMENT (-1), not LSSVM_ERR_NO_DEVICE, on a machine with or without a GPU."""
    good = np.array([1.0, 2.0, 0.5, 1.0])
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
        for pos in (0, 3):  # (a point of the reduced system, and the last point: QA_cost)
            w = good.copy()
            w[pos] = bad
            assert _solve_weighted_status(w, dtype) == -1, (bad, pos)
            assert "weight" in _capi.last_error()
    assert _solve_weighted_status(good, dtype, weights_null=True) == -1 and "weights must not be NULL" in _capi.last_error()
    assert _solve_weighted_status(good, dtype, X_null=True) == -1
    assert _solve_weighted_status(good, dtype, y_null=True) == -1
    assert _solve_weighted_status(good, dtype, alpha_null=True) == -1
    if dtype == np.float32:  # positive in double, zero in float: 1 / (C w) is formed in the real type
        assert _solve_weighted_status(np.array([1.0, 1e-300, 1.0, 1.0]), dtype) == -1
    # set_weights: a NULL handle; the length is checked against the handle's (tests/test_gpu_weighted.py)
    w = np.ones(4)
    assert _capi.weighted_entry("lssvm_mi355_problem_set_weights")(None, _capi.weights_ptr(w), 4) == -1 and "handle" in _capi.last_error()
    assert _capi.weighted_entry("lssvm_mi355_problem_set_weights")(None, None, 0) == -1
    # the Python mirror: a length mismatch, weights <= 0
    X, y = np.ones((4, 3), dtype=dtype), np.array([1.0, -1, 1, -1], dtype=dtype)
    with pytest.raises(InvalidParameterError, match="number of weights"):
        backend.solve_system_of_linear_equations(Parameter(), X, y, 1e-3, 4, sample_weight=np.ones(3))
    with pytest.raises(InvalidParameterError, match="greater than 0.0"):
        backend.solve_system_of_linear_equations(Parameter(), X, y, 1e-3, 4, sample_weight=[1.0, 0.0, 1.0, 1.0])


def test_fit_drops_points_of_weight_zero():
    """CSVM.fit(sample_weight=...): scikit-learn's semantics -- weights >= 0, points of weight 0 leave the solve and the model (a canned backend, as the
    reference's mock_csvm)."""
    seen = {}

    class Fake(CSVM):
        def solve_system_of_linear_equations(self, params, A, b, eps, max_iter, sample_weight=None):
            seen.update(A=np.array(A), b=np.array(b), max_iter=max_iter, w=None if sample_weight is None else np.array(sample_weight))
            return np.arange(1.0, A.shape[0] + 1.0), 0.5, {"iterations": 1}

    X = np.arange(24.0).reshape(6, 4)
    labels = [1, 1, -1, -1, -1, 1]
    svm = Fake(kernel_type="linear")
    model = svm.fit(DataSet(X, labels), sample_weight=[1.0, 0.0, 2.0, 0.0, 3.0, 0.5])
    assert np.array_equal(seen["A"], X[[0, 2, 4, 5]]) and list(seen["b"]) == [1, -1, -1, 1] and seen["max_iter"] == 4
    assert list(seen["w"]) == [1.0, 2.0, 3.0, 0.5]
    assert model.num_support_vectors() == 4 and list(model.labels()) == [1, -1, -1, 1] and list(model.alpha) == [1, 2, 3, 4]
    svm.fit(DataSet(X, labels))
    assert seen["w"] is None and seen["A"].shape == (6, 4)  # no weights: the unweighted call, unchanged
    for bad, what in (([1.0, -1.0, 1, 1, 1, 1], "greater than or equal to 0.0"), ([1.0, np.nan, 1, 1, 1, 1], "finite"), ([1.0] * 5, "number of sample weights"),
                      ([1.0, 0, 0, 0, 0, 0], "at least two points"), ([1.0, 1.0, 0, 0, 0, 0], "two different classes")):
        with pytest.raises(InvalidParameterError, match=what):
            svm.fit(DataSet(X, labels), sample_weight=bad)
