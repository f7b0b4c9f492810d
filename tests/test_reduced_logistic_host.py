"""CPU: the fixed-size kernel logistic regression -- the numpy model tests/reduced_logistic_model.py against independent routes, the conditions the
bounds of tests/test_gpu_reduced_logistic.py rest on, and every refusal that needs no device.

  * every case the GPU tests use: converged without a halving, e_model (against a Newton iteration that solves each step by SVD least squares) of the recorded order of
    magnitude, the gradient of J at the returned point small against the gradient at the start, J non-increasing over the accepted passes;
  * integer prior weights equal duplicated rows, rows of weight 0 equal removed rows;
  * one pass from zeros is twice the weighted least-squares model at cost C / 4 (v = 1/4 and z = 2 y exactly);
  * the safeguard: from -1 x the optimum the loop without its rejection rule does not come back, the loop with it halves and reaches the optimum;
  * the new entry points are declared, exported and bound, and each new refusal is raised without a device.
"""

import ctypes as C
import os

import numpy as np
import pytest

import reduced_logistic_model as lg
import reduced_model as rm
import reduced_weighted_model as wm
from conftest import ROOT
from plssvm_amd import _capi, backend, svc
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter

EPS64 = rm.EPS64
TOL = 1e-12


def _model(p, cost, **more):
    return lg.LogisticModel(p["kernel"], p["X"], p["y"], cost, p["landmarks"], held=p["held"], **{"tol": TOL, **more}, **p["kw"])


@pytest.fixture(scope="module")
def optimum():
    """rbf 600 x 4 at C = 100 from zeros: shared by the tests that start somewhere else."""
    p = lg.case("rbf_600x4")
    return p, _model(p, 100.0)


# ---------------------------------------------------------------- the conditions of the GPU tests ----------------------------------------------------------------
@pytest.mark.parametrize("cost", lg.COSTS)
@pytest.mark.parametrize("name", lg.CASE_NAMES)
def test_cases_converge_to_a_stationary_point_of_the_recorded_accuracy(name, cost):
    p = lg.case(name)
    model = _model(p, cost)
    r = model.result
    points = np.vstack([p["X"], p["points"]])
    e = lg.e_model(p, cost, points)
    ones = np.ones(p["y"].size)
    g0 = lg.gradient(model.Phi, model.K_mm, model.y, ones, cost, np.zeros(model.beta.size), 0.0)
    g1 = lg.gradient(model.Phi, model.K_mm, model.y, ones, cost, model.beta, -model.rho)
    rel = float(np.linalg.norm(g1) / np.linalg.norm(g0))
    print(f"{name} C={cost}: passes {r['passes']}, halvings {r['halvings']}, J {r['objective']:.6g}, e_model {e:.1e} (recorded {lg.RECORDED[name, cost]:.1e}), gradient {rel:.1e}, "
          f"cond eps64 {model.cond * EPS64:.1e}")
    assert r["converged"] == 1 and r["halvings"] == 0 and 5 <= r["passes"] <= 20
    assert e <= 10.0 * lg.RECORDED[name, cost]
    assert rel < 1e-8
    assert np.all(np.diff(r["accepted"]) <= 0.0)
    assert abs(r["objective"] - lg.objective(model.Phi, model.K_mm, model.y, ones, cost, model.beta, -model.rho)) <= 4 * EPS64 * r["objective"]
    # the bound of the GPU test says something: it is far below the decision values themselves
    f = model.decision_values(points)
    assert lg.fit_tolerance(model, e, f, linear=name.startswith("linear")) < 1e-3 * np.max(np.abs(f))
    if name == "rbf_600x4":  # the overlapping case: a classifier, not an interpolant
        assert 0.95 <= np.mean(np.sign(model.decision_values(p["X"])) == p["y"]) < 1.0


def test_row_quantities_are_free_of_cancellation_and_overflow():
    eta = np.array([-800.0, -40.0, -1e-300, 0.0, 1e-300, 3.0, 40.0, 800.0])
    for y in (1.0, -1.0):
        q, z, loss, mu, g = lg.row_quantities(np.full(eta.size, y), np.ones(eta.size), eta)
        assert np.all(np.isfinite(q)) and np.all(np.isfinite(z)) and np.all(np.isfinite(loss)) and np.all(q >= 2.0 ** -16)
        # another cancellation-free route: (y + 1) / 2 - p = y sigmoid(-y eta) and p (1 - p) = sigmoid(eta) sigmoid(-eta), each sigmoid as exp(-log(1 + exp(.)))
        assert np.allclose(g, y * np.exp(-np.logaddexp(0.0, y * eta)), rtol=1e-13, atol=0.0)
        assert np.allclose(mu, np.exp(-np.logaddexp(0.0, eta) - np.logaddexp(0.0, -eta)), rtol=1e-13, atol=0.0)
        assert np.allclose(loss, np.logaddexp(0.0, -y * eta), rtol=1e-15, atol=0.0)
    q, z, *_ = lg.row_quantities([1.0, -1.0], [1.0, 4.0], [0.0, 0.0])
    assert q.tolist() == [0.5, 1.0] and z.tolist() == [2.0, -2.0]  # v = a / 4 and z = 2 y exactly at eta = 0


def test_integer_weights_equal_duplicated_rows_and_zero_weights_removed_rows():
    p = lg.case("rbf_600x4")
    N = p["y"].size
    rng = np.random.default_rng(5)
    a = rng.integers(0, 4, N).astype(np.float64)
    a[p["landmarks"].astype(np.int64)] = np.maximum(a[p["landmarks"].astype(np.int64)], 1.0)  # (the landmarks stay: their rows define K_mm)
    for weights in (a, (a > 0).astype(np.float64)):
        Xd, yd, first = wm.expand(p["X"], p["y"][None, :], weights.astype(np.int64))
        lm_d = first[p["landmarks"].astype(np.int64)]
        # to rounding: ONE step of both formulations from the same iterate (three passes in), and the objective there.  Two iterations stopped by `tol` agree only as far
        # as `tol` takes them, so the converged runs are compared through their objectives: each lies within tol J of the minimum it stopped at
        mid = lg.LogisticModel(p["kernel"], p["X"], p["y"], 10.0, p["landmarks"], a=weights, tol=TOL, max_iter=3, **p["kw"])
        start = (mid.beta, mid.rho)
        weighted = lg.LogisticModel(p["kernel"], p["X"], p["y"], 10.0, p["landmarks"], a=weights, tol=TOL, max_iter=1, start=start, **p["kw"])
        plain = lg.LogisticModel(p["kernel"], Xd, yd[0], 10.0, lm_d, tol=TOL, max_iter=1, start=start, **p["kw"])
        fw, fp = weighted.decision_values(p["points"]), plain.decision_values(p["points"])
        assert np.max(np.abs(fw - fp)) <= 8.0 * max(weighted.cond, plain.cond) * EPS64 * np.max(np.abs(fp))
        assert abs(weighted.result["objective"] - plain.result["objective"]) <= (yd.shape[1] + 16) * EPS64 * plain.result["objective"]
        weighted = lg.LogisticModel(p["kernel"], p["X"], p["y"], 10.0, p["landmarks"], a=weights, tol=TOL, **p["kw"])
        plain = lg.LogisticModel(p["kernel"], Xd, yd[0], 10.0, lm_d, tol=TOL, **p["kw"])
        assert weighted.result["converged"] == plain.result["converged"] == 1
        assert abs(weighted.result["objective"] - plain.result["objective"]) <= 2.0 * TOL * plain.result["objective"]


@pytest.mark.parametrize("cost", lg.COSTS)
@pytest.mark.parametrize("name", ["rbf_777x5", "poly_600x8"])
def test_one_pass_from_zeros_is_twice_the_least_squares_model_at_a_quarter_of_the_cost(name, cost):
    p = lg.case(name)
    one = _model(p, cost, max_iter=1)
    assert one.result["passes"] == 1 and one.result["converged"] == 0
    ls = wm.WeightedReducedModel(p["kernel"], p["X"], p["y"][None, :], cost / 4.0, p["landmarks"], np.ones(p["y"].size), held=p["held"], **p["kw"])
    f1, f2 = one.decision_values(p["points"]), 2.0 * ls.decision_values(p["points"])[0]
    assert np.max(np.abs(f1 - f2)) <= 8.0 * ls.cond * EPS64 * np.max(np.abs(f2))
    # the objective reported with it is that of the iterate before: J(0, 0) = C N log 2
    assert abs(one.result["objective"] - cost * p["y"].size * np.log(2.0)) <= 4 * EPS64 * one.result["objective"]


def test_the_safeguard_brings_a_bad_start_back(optimum):
    p, best = optimum
    start = (-best.beta, -best.rho)
    free = _model(p, 100.0, start=start, halving=False)
    print(f"without the rejection rule: J {free.result['objective']:.3g} after {free.result['passes']} passes, against the optimum's {best.result['objective']:.6g}")
    assert free.result["converged"] == 0 or free.result["objective"] > 10.0 * best.result["objective"]
    assert not np.all(np.diff(free.result["accepted"]) <= 0.0)
    safe = _model(p, 100.0, start=start)
    r = safe.result
    print(f"with it: {r['halvings']} halvings, {r['passes']} passes, J {r['objective']:.6g}")
    assert r["converged"] == 1 and r["halvings"] > 0
    assert np.all(np.diff(r["accepted"]) <= 0.0)
    points = np.vstack([p["X"], p["points"]])
    f0, f1 = best.decision_values(points), safe.decision_values(points)
    assert np.max(np.abs(f0 - f1)) <= lg.fit_tolerance(best, lg.RECORDED["rbf_600x4", 100.0], f0)
    assert abs(r["objective"] - best.result["objective"]) <= 1e-10 * best.result["objective"]


def test_max_iter_and_the_halving_limit_end_the_loop(optimum):
    p, best = optimum
    for max_iter in (1, 2, 5):
        r = _model(p, 100.0, max_iter=max_iter).result
        assert r["passes"] == max_iter and r["converged"] == 0
    # a rejected last pass returns the last accepted iterate and its objective
    r = _model(p, 100.0, start=(-best.beta, -best.rho), max_iter=2).result
    assert r["passes"] == 2 and r["halvings"] == 1 and r["converged"] == 0
    assert np.array_equal(r["beta"], -best.beta) and r["objective"] == r["accepted"][0]


def test_convergence_returns_the_older_iterate_only_where_the_newer_is_worse_beyond_rounding(optimum):
    p, best = optimum
    start = (best.beta, best.rho)
    N = p["y"].size

    def worse_by(rel):
        """A `step` that answers the optimum with a point whose objective is larger by about rel x J (found by bisection on the shift of the intercept)."""
        J0 = best.result["objective"]
        ones = np.ones(N)
        lo, hi = 0.0, 1.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if lg.objective(best.Phi, best.K_mm, best.y, ones, 100.0, best.beta, -(best.rho + mid)) - J0 < rel * J0 else (lo, mid)
        return lambda Phi, K_mm, q, z, cost: (best.beta.copy(), best.rho + hi, 0.0, 0.0, None)

    # worse by 1e-6 J, inside tol = 1e-3: converged, and the OLDER iterate (the optimum) with its objective comes back
    r = lg.fit(best.Phi, best.K_mm, best.y, None, 100.0, tol=1e-3, start=start, step=worse_by(1e-6))
    assert r["converged"] == 1 and r["passes"] == 2 and r["last_decrease"] < 0.0
    assert np.array_equal(r["beta"], best.beta) and r["rho"] == best.rho and r["objective"] == r["accepted"][0]
    # worse by less than the rounding of the two sums, 2 (N + 16) eps64 J: they count as equal and the NEWER iterate comes back
    r = lg.fit(best.Phi, best.K_mm, best.y, None, 100.0, tol=1e-3, start=start, step=worse_by(0.5 * (N + 16) * EPS64))
    assert r["converged"] == 1 and r["passes"] == 2 and r["rho"] != best.rho
    assert 0.0 <= r["objective"] - r["accepted"][0] <= 2.0 * (N + 16) * EPS64 * r["accepted"][0]


# ---------------------------------------------------------------- the boundary ----------------------------------------------------------------
PUBLIC = ("lssvm_mi355_problem_fit_reduced_logistic", "lssvm_mi355_fit_reduced_logistic_f32", "lssvm_mi355_fit_reduced_logistic_f64")


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "plssvm_amd.h")).read()
    testing = open(os.path.join(ROOT, "include", "plssvm_amd_testing.h")).read()
    for name in PUBLIC:
        assert name in _capi.EXPORTED_SYMBOLS and name + "(" in header and hasattr(_capi.lib, name)
    name = "lssvm_mi355_problem_reduced_logistic_step"
    assert name in _capi.EXPORTED_SYMBOLS and name + "(" in testing and name + "(" not in header and hasattr(_capi.lib, name)
    assert _capi.ABI_VERSION == 4 and C.sizeof(_capi.LssvmReducedLogisticInfo) == 104
    assert issubclass(svc.ProbabilisticSVC, svc.SVC)
    with pytest.raises(AttributeError):  # SVC itself is untouched
        svc.SVC().predict_proba


def test_new_refusals_are_raised_before_a_device_is_touched():
    N = 12
    X = np.arange(36, dtype=np.float64).reshape(N, 3) / 7.0
    y = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    prm = Parameter(kernel_type="rbf")
    good_start = (np.zeros(4), 0.0)
    # the Python surface, which checks as the library does
    for labels, match in ((np.r_[y[:-1], 0.5], "exactly -1 or"), (np.r_[y[:-1], 0.0], "exactly -1 or"), (np.r_[y[:-1], np.nan], "exactly -1 or")):
        with pytest.raises(InvalidParameterError, match=match):
            backend.fit_reduced_logistic(prm, X, labels, 4)
    for tol in (0.0, -1e-8, np.inf, np.nan, "small"):
        with pytest.raises(InvalidParameterError, match="tol"):
            backend.fit_reduced_logistic(prm, X, y, 4, tol=tol)
    for max_iter in (0, -3, 2.5):
        with pytest.raises(InvalidParameterError, match="max_iter"):
            backend.fit_reduced_logistic(prm, X, y, 4, max_iter=max_iter)
    for start in ((np.full(4, np.nan), 0.0), (np.zeros(4), np.inf), (np.zeros(3), 0.0), 7):
        with pytest.raises(InvalidParameterError, match="start"):
            backend.fit_reduced_logistic(prm, X, y, 4, start=start)
    with pytest.raises(InvalidParameterError, match="factor"):
        backend.fit_reduced_logistic(prm, X, y, 4, factor="gpu", start=good_start)
    with pytest.raises(InvalidParameterError, match="not less than 0.0"):
        backend.fit_reduced_logistic(prm, X, y, 4, sample_weight=np.r_[np.ones(N - 1), -1.0])
    with pytest.raises(InvalidParameterError, match="estimator"):
        svc.fit_reduced_logistic(object(), X, y, 4)
    # the library itself: the one-shot entry points reach every check that needs no device
    ps = _capi.LssvmParams(2, 3, 1.0 / 3, 0.0, 1.0)
    dp = C.POINTER(C.c_double)
    for suffix, dtype in (("f32", np.float32), ("f64", np.float64)):
        data, target = X.astype(dtype), y.astype(dtype)
        fit = _capi.reduced_logistic_entry(f"lssvm_mi355_fit_reduced_logistic_{suffix}")
        betas, rhos = np.zeros(4), np.zeros(1)

        def call(labels=target, w=None, rank=4, slab_rows=0, factor=0, tol=1e-8, max_iter=50, b0=None, r0=None, b=betas):
            return fit(C.byref(ps), _capi.ptr(data), N, 3, _capi.ptr(np.ascontiguousarray(labels, dtype=dtype)), 1, _capi.weights_ptr(w), rank, None, slab_rows, factor, tol, max_iter,
                       _capi.weights_ptr(b0), _capi.weights_ptr(r0), _capi.weights_ptr(b), rhos.ctypes.data_as(dp), None, None, None)

        with pytest.raises(InvalidParameterError, match="exactly -1 or"):
            _capi.check(call(labels=np.r_[target[:-1], 0.5]))
        for tol in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(InvalidParameterError, match="tol must be finite"):
                _capi.check(call(tol=tol))
        with pytest.raises(InvalidParameterError, match="max_iter"):
            _capi.check(call(max_iter=0))
        with pytest.raises(InvalidParameterError, match="start value"):
            _capi.check(call(b0=np.r_[np.zeros(3), np.nan], r0=np.zeros(1)))
        with pytest.raises(InvalidParameterError, match="start value"):
            _capi.check(call(b0=np.zeros(4), r0=np.array([np.inf])))
        with pytest.raises(InvalidParameterError, match="both"):
            _capi.check(call(b0=np.zeros(4)))
        # the refusals of the weighted fit, reached through this entry point
        with pytest.raises(InvalidParameterError, match="not less than 0.0"):
            _capi.check(call(w=np.r_[np.ones(N - 1), -1.0]))
        with pytest.raises(InvalidParameterError, match="factor must be 0"):
            _capi.check(call(factor=2))
        with pytest.raises(InvalidParameterError, match="rank of the reduced model"):
            _capi.check(call(rank=N + 1))
        with pytest.raises(InvalidParameterError, match="slab_rows"):
            _capi.check(call(slab_rows=300))
        with pytest.raises(InvalidParameterError, match="must not be NULL"):
            _capi.check(call(b=None))
    # a NULL handle
    bp = betas.ctypes.data_as(dp)
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(_capi.reduced_logistic_entry("lssvm_mi355_problem_fit_reduced_logistic")(None, _capi.ptr(y), 1, None, 4, None, 0, 0, 1e-8, 50, None, None, bp, bp, None, None))
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(_capi.reduced_logistic_entry("lssvm_mi355_problem_reduced_logistic_step")(None, _capi.ptr(y), 1, None, 4, None, 0, bp, bp, bp, bp, bp, bp, None))
