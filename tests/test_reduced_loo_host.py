"""CPU: the numpy model of the exact leave-one-out scores of the fixed-size LS-SVM (tests/reduced_loo_model.py) -- leave-one-out with the landmark
set held fixed -- the conditions on the inputs of tests/test_gpu_reduced_loo.py, and the host side of the new entry points.

  * the identity against N brute-force refits: 255 x 5 rbf and 255 x 16 polynomial at rank 16, each at the costs 0.1, 1, 100 and 1e4, within
    8 max(e_loo, cond(M) eps64) max |f| -- the model ALONE stays within the bound the GPU test asserts (test_gpu_reduced_loo.py compares the device with the same refits);
  * h in (1 / N, 1), sum h = 1 + tr(M^-1 Phic^T Phic);
  * press and loo_errors against their definitions;
  * every refusal that needs no device; the base CSVM raises; argument checks of backend / CSVM / SVC.
"""

import ctypes as C
import functools
import os

import numpy as np
import pytest

import reduced_loo_model as lm
import reduced_model as rm
from conftest import ROOT
from plssvm_amd import _capi, backend, svc
from plssvm_amd.csvm import CSVM, MI355CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter


@functools.lru_cache(maxsize=None)
def identity_reference(name, cost):
    p = lm.identity_case(name)
    model = lm.LooModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], **p["kw"])
    stable = lm.stable(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], **p["kw"])
    brute = lm.brute_force(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], **p["kw"])
    return p, model, stable, brute


@pytest.mark.parametrize("cost", lm.IDENTITY_COSTS)
@pytest.mark.parametrize("name", [c[0] for c in lm.IDENTITY_CASES])
def test_the_identity_against_brute_force_refits(name, cost):
    p, model, (h_s, f_s, loo_s), brute = identity_reference(name, cost)
    e = lm.e_loo(model, loo_s)
    tol = lm.tolerance(model, e, np.max(np.abs(model.f)))
    diff, diff_stable = float(np.max(np.abs(model.loo - brute))), float(np.max(np.abs(loo_s - brute)))
    print(f"identity {name} C={cost:g}: |loo - refits| {diff:.2e} (stable route {diff_stable:.2e}), tolerance {tol:.2e} (e_loo {e:.1e}, cond(M) {model.cond:.1e}), "
          f"max h {model.max_leverage:.3f}, retries {model.retries}")
    assert model.retries == 0
    assert diff <= tol and diff_stable <= tol, (name, cost, diff, diff_stable, tol)
    # the two routes agree on h and f under the same rule
    assert np.max(np.abs(model.h - h_s)) <= lm.tolerance(model, e, 1.0) and np.max(np.abs(model.f - f_s)) <= tol
    # the leave-one-out values are not the fitted values: the test above is not vacuous
    assert np.max(np.abs(model.loo - model.f)) > 1e3 * tol


@pytest.mark.parametrize("cost", lm.IDENTITY_COSTS)
@pytest.mark.parametrize("name", [c[0] for c in lm.IDENTITY_CASES])
def test_leverages_lie_in_their_range_and_sum_to_the_degrees_of_freedom(name, cost):
    _, model, _, _ = identity_reference(name, cost)
    N = model.h.size
    assert np.all(model.h > 1.0 / N) and np.all(model.h < 1.0)
    m = model.M.shape[0]
    dof = 1.0 + np.trace(np.linalg.solve(model.M + model.nu * np.eye(m), model.Phic.T @ model.Phic))
    assert abs(model.h.sum() - dof) <= 8.0 * max(model.cond * lm.EPS64, N * lm.EPS64) * dof
    assert dof < 1.0 + m


@pytest.mark.parametrize("name", [c[0] for c in lm.IDENTITY_CASES])
def test_press_and_errors_follow_their_definitions(name):
    p, model, _, _ = identity_reference(name, 1.0)
    y, loo = p["Y"][0].astype(np.float64), model.loo[0]
    assert model.press[0] == pytest.approx(sum((a - b) ** 2 for a, b in zip(y, loo)), rel=1e-12)
    assert model.loo_errors[0] == sum(1 for a, b in zip(y, loo) if (b > 0) != (a > 0) or b == 0)
    assert 0 < model.loo_errors[0] < y.size  # (random labels: some points are predicted wrongly, not all)
    # press in its other form: sum (residual / (1 - h))^2
    assert model.press[0] == pytest.approx((((y - model.f[0]) / (1.0 - model.h)) ** 2).sum(), rel=1e-12)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", [c[0] for c in rm.FIT_CASES])
def test_e_loo_is_a_condition_on_the_inputs_of_the_gpu_tests(name, dtype, k):
    p = rm.fit_case(name, dtype, k)
    for cost in lm.FIT_COSTS:
        model = lm.LooModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], held=p["held"], **p["kw"])
        e = lm.e_loo(model, lm.stable(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], held=p["held"], **p["kw"])[2])
        print(f"e_loo {name} {np.dtype(dtype).name} k={k} C={cost:g}: {e:.2e} cond {model.cond:.2e} max h {model.max_leverage:.3f}")
        assert model.retries == 0 and e <= 1e-7 and model.max_leverage < 0.9
        assert lm.tolerance(model, e, np.max(np.abs(model.loo))) <= 1e-2 * np.max(np.abs(model.loo))


def test_overlapping_blobs_move_the_score_with_the_cost():
    """The data of the GPU surface test: the numpy leave-one-out accuracy is not constant over Cs = (1e-3, 1, 1e3)."""
    X, labels = lm.overlapping_blobs(600, 4, 2, seed=41)
    Y = np.where(labels == 1, 1.0, -1.0)[None, :]
    lms = rm.library_landmarks(600, 32)
    scores = [1.0 - lm.LooModel("rbf", X, Y, C, lms, gamma=0.25).loo_errors[0] / 600 for C in (1e-3, 1.0, 1e3)]
    print("numpy loo accuracy on overlapping blobs:", scores)
    assert len(set(scores)) > 1 and max(scores) < 1.0


# ---------------------------------------------------------------- the host side of the entry points ----------------------------------------------------------------
NAMES = ["lssvm_mi355_problem_fit_reduced_loo", "lssvm_mi355_fit_reduced_loo_f32", "lssvm_mi355_fit_reduced_loo_f64"]
TESTING_NAMES = ["lssvm_mi355_problem_reduced_leverage", "lssvm_mi355_problem_time_leverage_kernel"]


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "plssvm_amd.h")).read()
    testing = open(os.path.join(ROOT, "include", "plssvm_amd_testing.h")).read()
    for name in NAMES:
        assert name in _capi.EXPORTED_SYMBOLS and name + "(" in header and hasattr(_capi.lib, name)
    for name in TESTING_NAMES:
        assert name in _capi.EXPORTED_SYMBOLS and name + "(" in testing and name + "(" not in header and hasattr(_capi.lib, name)
    assert C.sizeof(_capi.LssvmReducedLooInfo) == 56
    assert "static_assert(sizeof(lssvm_reduced_loo_info) == 56" in open(os.path.join(ROOT, "plssvm_amd", "csrc", "capi.hip")).read()
    assert _capi.ABI_VERSION == 4 and _capi.REDUCED_LOO_MAX_COSTS == lm.MAX_COSTS == 64
    assert C.sizeof(_capi.LssvmReducedInfo) == 64  # (no existing struct changed)


def test_bad_arguments_are_refused_before_a_device_is_touched():
    """(this box has no GPU: whatever reaches a device fails with another error)"""
    X = np.random.default_rng(0).uniform(-1, 1, (12, 3))
    y = np.where(np.arange(12) % 2 == 0, 1.0, -1.0)
    prm = Parameter()
    # the binding's checks: the cost grid ...
    for costs, match in (([], "between 1 and 64 costs"), (np.ones(65), "between 1 and 64 costs"), ([1.0, 0.0], "finite and greater than 0"), ([-1.0], "finite and greater than 0"),
                         ([float("nan")], "finite and greater than 0"), ([float("inf")], "finite and greater than 0"), ([[1.0, 2.0]], "between 1 and 64 costs")):
        with pytest.raises(InvalidParameterError, match=match):
            backend.fit_reduced_loo(prm, X, y, 4, costs)
    # ... and everything fit_reduced refuses
    with pytest.raises(InvalidParameterError, match="right hand side"):
        backend.fit_reduced_loo(prm, X, y[:5], 4, [1.0])
    for rank in (0, 13, 1025):
        with pytest.raises(InvalidParameterError, match="rank of the reduced model"):
            backend.fit_reduced_loo(prm, X, y, rank, [1.0])
    with pytest.raises(InvalidParameterError, match="landmarks"):
        backend.fit_reduced_loo(prm, X, y, 4, [1.0], landmarks=[])
    for slab_rows in (100, -256, 256.0):
        with pytest.raises(InvalidParameterError, match="slab_rows"):
            backend.fit_reduced_loo(prm, X, y, 4, [1.0], slab_rows=slab_rows)
    with pytest.raises(InvalidParameterError, match="distinct"):
        backend.fit_reduced_loo(prm, X, y, 4, [1.0], landmarks=[3, 7, 3])
    with pytest.raises(InvalidParameterError, match="index of a data point"):
        backend.fit_reduced_loo(prm, X, y, 4, [1.0], landmarks=[3, 12])
    # the library's checks through the raw entry points
    ps = _capi.LssvmParams(0, 3, 1.0, 0.0, 1.0)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    betas, rhos, used, infos = np.zeros(4 * 65), np.zeros(65), np.zeros(4, dtype=np.uint64), (_capi.LssvmReducedLooInfo * 65)()
    bp, rp, lp = betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp), used.ctypes.data_as(up)
    grid = np.array([1.0, 10.0])
    gp = grid.ctypes.data_as(dp)

    def outs(b=bp, r=rp):
        return (b, r, None, None, None, None, None, lp, infos)

    for suffix, data, target in (("f64", X, y), ("f32", X.astype(np.float32), y.astype(np.float32))):
        fn = _capi.reduced_loo_entry(f"lssvm_mi355_fit_reduced_loo_{suffix}")
        head = (C.byref(ps), _capi.ptr(data), 12, 3, _capi.ptr(target), 1)
        for num in (0, 65):
            with pytest.raises(InvalidParameterError, match="between 1 and 64 costs"):
                _capi.check(fn(*head, 4, None, 0, np.ones(65).ctypes.data_as(dp), num, *outs(), None))
        for bad in (0.0, -2.0, float("nan"), float("inf")):
            with pytest.raises(InvalidParameterError, match="finite and greater than 0"):
                _capi.check(fn(*head, 4, None, 0, np.array([1.0, bad]).ctypes.data_as(dp), 2, *outs(), None))
        with pytest.raises(InvalidParameterError, match="costs must not be NULL"):
            _capi.check(fn(*head, 4, None, 0, None, 2, *outs(), None))
        for rank in (0, 13, 1025):
            with pytest.raises(InvalidParameterError, match="rank of the reduced model"):
                _capi.check(fn(*head, rank, None, 0, gp, 2, *outs(), None))
        with pytest.raises(InvalidParameterError, match="slab_rows"):
            _capi.check(fn(*head, 4, None, 300, gp, 2, *outs(), None))
        with pytest.raises(InvalidParameterError, match="right hand sides"):
            _capi.check(fn(C.byref(ps), _capi.ptr(data), 12, 3, _capi.ptr(target), 0, 4, None, 0, gp, 2, *outs(), None))
        for b, r in ((None, rp), (bp, None)):
            with pytest.raises(InvalidParameterError, match="must not be NULL"):
                _capi.check(fn(*head, 4, None, 0, gp, 2, *outs(b, r), None))
        with pytest.raises(InvalidParameterError, match="data must not be empty"):
            _capi.check(fn(C.byref(ps), None, 12, 3, _capi.ptr(target), 1, 4, None, 0, gp, 2, *outs(), None))
        dup = np.array([1, 2, 2, 3], dtype=np.uint64)
        with pytest.raises(InvalidParameterError, match="distinct"):
            _capi.check(fn(*head, 4, dup.ctypes.data_as(up), 0, gp, 2, *outs(), None))
    # NULL handles, and the checks that come before the handle is used
    fit, lev, timing = (_capi.reduced_loo_entry(n) for n in ("lssvm_mi355_problem_fit_reduced_loo", "lssvm_mi355_problem_reduced_leverage", "lssvm_mi355_problem_time_leverage_kernel"))
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(fit(None, _capi.ptr(y), 1, 4, None, 0, gp, 2, *outs()))
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(lev(None, 4, None, 0, bp, bp, None, 0, bp, None))
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(timing(None, 4, 0, 1, 1, bp, bp))


class NumpyCSVM(CSVM):
    """The base class's fit_reduced_path on top of the numpy model: what the method itself does with a backend's answer."""

    def solve_reduced_loo_systems(self, params, A, Y, rank, costs, landmarks=None):
        lms = rm.library_landmarks(A.shape[0], rank) if landmarks is None else np.asarray(landmarks, dtype=np.uint64)
        models = [lm.LooModel("rbf", A, Y, C, lms, gamma=params.gamma) for C in costs]
        report = {"costs": np.array(costs), "leverage": np.stack([m.h for m in models]), "fitted": np.stack([m.f for m in models]), "loo": np.stack([m.loo for m in models]),
                  "press": np.stack([m.press for m in models]), "loo_errors": np.stack([m.loo_errors for m in models]).astype(np.uint64),
                  "max_leverage": np.array([m.max_leverage for m in models]), "jitter": np.array([m.nu for m in models]), "infos": [{"cost": C} for C in costs]}
        return np.stack([m.betas for m in models]), np.stack([m.rhos for m in models]), lms, report


def test_csvm_fit_reduced_path_builds_ordinary_models_and_validates():
    X, labels = rm.blobs(120, 4, 2, seed=5)
    names = ["cat" if v else "dog" for v in labels]
    data = DataSet(X, names, real_type=np.float32, label_type=str)
    svm = NumpyCSVM(kernel_type="rbf", cost=77.0)
    models, report = svm.fit_reduced_path(data, 16, [0.5, 50.0])
    rows = rm.library_landmarks(120, 16).astype(int)
    assert [m.params.cost for m in models] == [0.5, 50.0] and all(m.num_support_vectors() == 16 and m.alpha.dtype == np.float32 for m in models)
    assert np.array_equal(models[0].support_vectors(), data.data()[rows]) and not np.array_equal(models[0].alpha, models[1].alpha)
    assert report["loo"].shape == (2, 120) and report["leverage"].shape == (2, 120) and report["press"].shape == (2,) and np.array_equal(report["landmarks"], rows)
    y = data.mapped_labels().astype(np.float64)
    assert np.allclose(report["loo_accuracy"], [np.mean(np.sign(report["loo"][s]) == y) for s in range(2)])
    assert [i["iterations"] for i in svm.last_cg_info] == [0, 0]
    for bad, match in (([], "greater than 0"), ([1.0, -1.0], "finite and greater"), ([float("nan")], "finite and greater")):
        with pytest.raises(InvalidParameterError, match=match):
            svm.fit_reduced_path(data, 16, bad)
    with pytest.raises(InvalidParameterError, match="No labels"):
        svm.fit_reduced_path(DataSet(X), 4, [1.0])
    with pytest.raises(InvalidParameterError, match="distinct"):
        svm.fit_reduced_path(data, 2, [1.0], landmarks=[1, 1])
    with pytest.raises(NotImplementedError):
        CSVM().fit_reduced_path(data, 4, [1.0])
    sharded = object.__new__(MI355CSVM)
    sharded.use_devices, sharded._options = 2, None
    with pytest.raises(InvalidParameterError, match="one device"):
        sharded.solve_reduced_loo_systems(Parameter(), X, np.ones((1, 120)), 4, [1.0])


def test_svc_fit_reduced_cv_validates_its_arguments():
    X, labels = rm.blobs(30, 3, 2, seed=6)
    with pytest.raises(InvalidParameterError, match="plssvm_amd.svc.SVC"):
        svc.fit_reduced_cv(object(), X, labels, 4, [1.0])
    with pytest.raises(InvalidParameterError, match="class_weight"):
        svc.fit_reduced_cv(svc.SVC(class_weight="balanced"), X, labels, 4, [1.0])
    with pytest.raises(InvalidParameterError, match="shapes"):
        svc.fit_reduced_cv(svc.SVC(), X, labels[:-1], 4, [1.0])
    with pytest.raises(InvalidParameterError, match="greater than 0"):
        svc.fit_reduced_cv(svc.SVC(), X, labels, 4, [])
    for text in (backend.fit_reduced_loo.__doc__, CSVM.fit_reduced_path.__doc__, svc.fit_reduced_cv.__doc__, backend.ResidentProblem.fit_reduced_loo.__doc__):
        assert "leave-one-out with the landmark set held fixed" in " ".join(text.split())
