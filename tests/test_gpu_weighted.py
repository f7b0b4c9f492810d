"""GPU: the weighted LS-SVM system (lssvm_mi355_solve_weighted_*, lssvm_mi355_problem_set_weights) and the scikit-learn SVC on top of it.

The guarantees of include/plssvm_amd.h: weights == 1 give exactly the bits of the unweighted solve, weights == 2 exactly those of the unweighted solve at
cost 2C; other weights solve Abar(w) = K + diag(1 / (C w)) + QA_cost(w) - q 1^T - 1 q^T, checked against a float64 numpy direct solve of that matrix."""

import numpy as np
import pytest

from plssvm_amd import _capi, backend
from plssvm_amd.datagen import make_blobs_pm1
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter
from plssvm_amd.svc import SVC

pytestmark = pytest.mark.gpu

KERNELS = ["linear", "polynomial", "rbf"]
FP32_BOUND = {"log-uniform": 0.25, "last only": 1e-2}  # about twice what the GPU measured (test_log_uniform_weights_against_the_direct_solve)
DTYPES = [np.float32, np.float64]


def kernel_matrix(kernel, A, B, gamma, degree=3, coef0=0.0):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if kernel == "linear":
        return A @ B.T
    if kernel == "polynomial":
        return (gamma * (A @ B.T) + coef0) ** degree
    return np.exp(-gamma * (np.sum(A * A, 1)[:, None] + np.sum(B * B, 1)[None, :] - 2.0 * (A @ B.T)).clip(min=0.0))


def reduced_system(K, y, cost, w):
    n = K.shape[0] - 1
    q = K[:n, n]
    QA = K[n, n] + 1.0 / (cost * w[n])
    return K[:n, :n] + np.diag(1.0 / (cost * w[:n])) + QA - q[:, None] - q[None, :], q, QA


def direct_solve(K, y, cost, w):
    """float64: alpha (N entries) and rho of the weighted system, the recipe of csvm.cpp:179-182 on the exact solution of Abar(w)."""
    A, q, QA = reduced_system(K, y, cost, w)
    x = np.linalg.solve(A, y[:-1] - y[-1])
    return np.append(x, -x.sum()), -(y[-1] + QA * x.sum() - q @ x)


def rel_inf(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(np.max(np.abs(b)), 1e-300))


def bits_equal(a, b):
    return np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8))


def params_of(kernel, cost=1.0):
    return Parameter(kernel_type=kernel, degree=3, gamma=0.05, coef0=1.0, cost=cost)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_unit_weights_and_doubled_weights_are_bit_exact(kernel, dtype):
    X, y = make_blobs_pm1(1500, 16, seed=21, dtype=dtype)
    eps = 1e-10 if dtype == np.float64 else 1e-5
    a0, r0, i0 = backend.solve_system_of_linear_equations(params_of(kernel), X, y, eps, 1500)
    a1, r1, i1 = backend.solve_system_of_linear_equations(params_of(kernel), X, y, eps, 1500, sample_weight=np.ones(1500))
    assert bits_equal(a1, a0) and bits_equal(r1, r0) and i1["iterations"] == i0["iterations"], (kernel, dtype)
    a2, r2, i2 = backend.solve_system_of_linear_equations(params_of(kernel, cost=0.5), X, y, eps, 1500, sample_weight=np.full(1500, 2.0))
    a2c, r2c, i2c = backend.solve_system_of_linear_equations(params_of(kernel, cost=1.0), X, y, eps, 1500)
    assert bits_equal(a2, a2c) and bits_equal(r2, r2c) and i2["iterations"] == i2c["iterations"], (kernel, dtype)
    # a resident problem: weights set and cleared again -> today's bits
    w = np.exp(np.random.default_rng(3).uniform(np.log(0.1), np.log(10.0), 1500))
    with backend.ResidentProblem(params_of(kernel), X) as prob:
        prob.set_weights(w)
        prob.cg_begin(y, eps)
        prob.cg_step(1500)
        aw, rw, _ = prob.cg_finish()
        assert not bits_equal(aw, a0)
        prob.set_weights(None)
        prob.cg_begin(y, eps)
        prob.cg_step(1500)
        a3, r3, i3 = prob.cg_finish()
    assert bits_equal(a3, a0) and bits_equal(r3, r0) and i3["iterations"] == i0["iterations"], (kernel, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_log_uniform_weights_against_the_direct_solve(kernel, dtype):
    """fp64: within 1e-8 (rel-inf, alpha and rho) of the float64 direct solve.  At eps = 1e-14: the stop test is relative to r0 = b - Abar 1 (x0 = 1,
    csvm.cpp:95-108), and weights in [0.1, 10] give Abar a condition number of ~1e5 here, so a float64 numpy CG of the same recipe stops 1.3e-5 from the
    exact solution at eps = 1e-10, 1.5e-9 at 1e-14 (the GPU: up to 1.3e-9).  fp32 (eps = 1e-6) is as far from float64 as an fp32 CG on a condition number of
    1e5 gets; the GPU measured, alpha (linear / polynomial / rbf) and rho: log-uniform weights 9.4e-2 / 1.2e-1 / 1.1e-1, rho <= 7.0e-3; only the last
    weight != 1: 8.7e-4 / 5.0e-3 / 1.9e-3, rho <= 8.6e-4.  The bounds (FP32_BOUND) are twice the largest of each case."""
    N, d = 2000, 16
    X, y = make_blobs_pm1(N, d, seed=8, dtype=dtype)
    prm = params_of(kernel, cost=0.8)
    K = kernel_matrix(kernel, X, X, prm.gamma, prm.degree, prm.coef0)
    y64 = y.astype(np.float64)
    rng = np.random.default_rng(11)
    last_only = np.ones(N)
    last_only[-1] = 6.5
    for name, w in (("log-uniform", np.exp(rng.uniform(np.log(0.1), np.log(10.0), N))), ("last only", last_only)):
        a_ref, rho_ref = direct_solve(K, y64, 0.8, w)
        eps = 1e-14 if dtype == np.float64 else 1e-6
        alpha, rho, info = backend.solve_system_of_linear_equations(prm, X, y, eps, N, sample_weight=w)
        e_a, e_r = rel_inf(alpha, a_ref), abs(float(rho) - rho_ref) / max(abs(rho_ref), 1.0)
        print(f"{kernel:10s} {np.dtype(dtype).name} {name:11s}: {info['iterations']} its, alpha {e_a:.2e}, rho {e_r:.2e}")
        bound = 1e-8 if dtype == np.float64 else FP32_BOUND[name]
        assert e_a <= bound and e_r <= bound, (kernel, dtype, name, e_a, e_r)


@pytest.mark.parametrize("kernel", KERNELS)
def test_matvec_after_set_weights(kernel):
    N, d = 2000, 16
    X, _ = make_blobs_pm1(N, d, seed=4, dtype=np.float64)
    prm = params_of(kernel, cost=1.5)
    w = np.exp(np.random.default_rng(5).uniform(np.log(0.1), np.log(10.0), N))
    A, _, QA = reduced_system(kernel_matrix(kernel, X, X, prm.gamma, prm.degree, prm.coef0), None, 1.5, w)
    dvec = np.random.default_rng(6).uniform(-1.0, 1.0, N - 1)
    with backend.ResidentProblem(prm, X) as prob:
        prob.set_weights(w)
        assert abs(prob.q()[1] - QA) <= 1e-14 * abs(QA)
        out = prob.matvec(dvec, np.zeros(N - 1))
        assert rel_inf(out, A @ dvec) <= 1e-12, kernel
        # checked against the handle: the length, bad values, and no change while a CG solve is open
        for bad in (np.ones(N - 1), np.ones(N + 1)):
            assert _capi.weighted_entry("lssvm_mi355_problem_set_weights")(prob._h, _capi.weights_ptr(bad), bad.size) == -1
        for v in (0.0, -2.0, np.nan, np.inf):
            wb = w.copy()
            wb[17] = v
            assert _capi.weighted_entry("lssvm_mi355_problem_set_weights")(prob._h, _capi.weights_ptr(wb), N) == -1
        prob.cg_begin(np.where(np.arange(N) % 2 == 0, 1.0, -1.0), 1e-3)
        with pytest.raises(InvalidParameterError, match="between cg_begin and cg_finish"):
            prob.set_weights(None)
        prob.cg_step(3)
        prob.cg_finish()
        prob.set_weights(None)  # (allowed again)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sharded_weighted_solve_is_bit_equal(dtype):
    N = 3000
    X, y = make_blobs_pm1(N, 16, seed=9, dtype=dtype)
    w = np.exp(np.random.default_rng(12).uniform(np.log(0.1), np.log(10.0), N))
    eps = 1e-10 if dtype == np.float64 else 1e-5
    for kernel in ("linear", "rbf"):
        one = backend.solve_system_of_linear_equations(params_of(kernel), X, y, eps, N, options=_capi.Options(symmetric=0), sample_weight=w)
        two = backend.solve_system_of_linear_equations(params_of(kernel), X, y, eps, N, devices=[0, 0], options=_capi.Options(symmetric=0), sample_weight=w)
        assert two[2]["local_devices"] == 2
        assert bits_equal(one[0], two[0]) and bits_equal(one[1], two[1]) and one[2]["iterations"] == two[2]["iterations"], (kernel, dtype)


def test_svc_zero_weights_and_fitted_coefficients():
    X, y = make_blobs_pm1(600, 10, seed=13, dtype=np.float64)
    sw = np.ones(600)
    sw[::7] = 0.0
    keep = sw > 0
    for kernel in ("linear", "poly", "rbf"):
        est = SVC(kernel=kernel, tol=1e-10, gamma=0.1, coef0=1.0).fit(X, y, sample_weight=sw)
        ref = SVC(kernel=kernel, tol=1e-10, gamma=0.1, coef0=1.0).fit(X[keep], y[keep])
        assert np.array_equal(est.support_, np.flatnonzero(keep)) and not np.any(np.isin(np.arange(0, 600, 7), est.support_))
        assert bits_equal(est.dual_coef_, ref.dual_coef_) and bits_equal(est.intercept_, ref.intercept_)
        assert np.array_equal(est.support_vectors_, X[keep]) and est.dual_coef_.shape == (1, int(keep.sum()))
        assert est.shape_fit_ == (600, 10) and est.n_features_in_ == 10 and est.fit_status_ == 0 and list(est.classes_) == [-1.0, 1.0]
        assert est.n_support_.sum() == int(np.count_nonzero(est.dual_coef_)) and est.n_support_.dtype == np.int32
        # decision_function == dual_coef_ @ K(support_vectors_, X) + intercept_
        Xt = make_blobs_pm1(200, 10, seed=14, dtype=np.float64)[0]
        Kt = kernel_matrix("polynomial" if kernel == "poly" else kernel, est.support_vectors_, Xt, 0.1, 3, 1.0)
        expect = est.dual_coef_ @ Kt + est.intercept_
        scale = np.abs(est.dual_coef_) @ np.abs(Kt) + abs(est.intercept_[0])
        assert np.max(np.abs(est.decision_function(Xt) - expect[0]) / scale[0]) <= 1e-10, kernel
        if kernel == "linear":
            assert np.allclose(est.coef_, est.dual_coef_ @ est.support_vectors_, rtol=1e-12, atol=1e-12)
        else:
            assert not hasattr(est, "coef_")
        assert est.score(Xt, np.where(Xt @ np.ones(10) > 0, 1.0, -1.0), sample_weight=np.ones(200)) >= 0.0


def imbalanced_blobs(n_maj, n_min, seed, d=4, sep=1.5):
    rng = np.random.default_rng(seed)
    X = np.vstack([rng.normal(0.0, 1.0, (n_maj, d)), rng.normal(0.0, 1.0, (n_min, d)) + sep / np.sqrt(d)])
    y = np.concatenate([-np.ones(n_maj), np.ones(n_min)])
    p = rng.permutation(y.size)
    return X[p], y[p]


def balanced_accuracy(values, y):
    return 0.5 * (np.mean(values[y > 0] > 0) + np.mean(values[y < 0] < 0))


def test_svc_class_weight_balanced():
    """Overlapping blobs, 9:1: the float64 numpy model of the linear LS-SVM gains about 0.27 of balanced accuracy from "balanced" weights (0.50 -> 0.77)."""
    X, y = imbalanced_blobs(900, 100, 1)
    Xt, yt = imbalanced_blobs(2000, 2000, 2)
    counts = {c: np.count_nonzero(y == c) for c in (-1.0, 1.0)}
    w_bal = y.size / (2 * np.array([counts[c] for c in y], dtype=np.float64))
    K, Kt = kernel_matrix("linear", X, X, 0.0), kernel_matrix("linear", Xt, X, 0.0)
    model = {}
    for name, w in (("none", np.ones(y.size)), ("balanced", w_bal)):
        a, rho = direct_solve(K, y, 1.0, w)
        model[name] = balanced_accuracy(Kt @ a - rho, yt)
    margin = model["balanced"] - model["none"]
    assert margin > 0.2, model
    plain = SVC(kernel="linear", tol=1e-10).fit(X, y)
    bal = SVC(kernel="linear", tol=1e-10, class_weight="balanced").fit(X, y)
    same = SVC(kernel="linear", tol=1e-10).fit(X, y, sample_weight=w_bal)
    assert np.allclose(bal.class_weight_, [1000 / 1800, 5.0]) and np.allclose(plain.class_weight_, [1.0, 1.0])
    assert bits_equal(bal.dual_coef_, same.dual_coef_) and bits_equal(bal.intercept_, same.intercept_)
    gpu = {"none": balanced_accuracy(plain.decision_function(Xt), yt), "balanced": balanced_accuracy(bal.decision_function(Xt), yt)}
    assert abs(gpu["none"] - model["none"]) <= 0.005 and abs(gpu["balanced"] - model["balanced"]) <= 0.005, (gpu, model)
    assert gpu["balanced"] - gpu["none"] >= margin - 0.01, (gpu, model)
    # a dict of class weights is the same as the sample weights it stands for
    d = SVC(kernel="linear", tol=1e-10, class_weight={1.0: 3.0}).fit(X, y)
    s = SVC(kernel="linear", tol=1e-10).fit(X, y, sample_weight=np.where(y > 0, 3.0, 1.0))
    assert bits_equal(d.dual_coef_, s.dual_coef_) and bits_equal(d.intercept_, s.intercept_)


def test_svc_in_scikit_learn_tooling():
    pytest.importorskip("sklearn")
    from sklearn.model_selection import GridSearchCV
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler

    X, y = make_blobs_pm1(300, 6, seed=17, dtype=np.float64)
    grid = GridSearchCV(SVC(real_type=np.float64), {"C": [0.1, 1, 10], "kernel": ["linear", "rbf"]}, cv=3).fit(X, y)
    assert grid.best_params_["C"] in (0.1, 1, 10) and grid.best_score_ > 0.9
    assert np.mean(grid.predict(X) == y) > 0.9
    pipe = Pipeline([("scale", StandardScaler()), ("svc", SVC())]).fit(X, y)
    assert np.mean(pipe.predict(X) == y) > 0.9 and pipe.score(X, y) > 0.9
