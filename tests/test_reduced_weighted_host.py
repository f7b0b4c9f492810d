"""CPU: the weighted fixed-size LS-SVM -- the numpy model tests/reduced_weighted_model.py against independent routes, the conditions the bounds of
tests/test_gpu_reduced_weighted.py rest on, and every refusal that needs no device.

  * every case the GPU tests use: no jitter retry, e_model finite, cond(M) eps64 of the recorded order of magnitude;
  * the weighted leave-one-out identity against 255 brute-force refits (the same model with w_i set to 0) within reduced_loo_model.tolerance;
  * integer weights equal the unweighted model on duplicated rows; weight 0 equals the unweighted model on the rows that are left;
  * the new entry points are declared, exported and bound, and each new refusal is raised without a device;
  * svc.fit_reduced_weighted / fit_reduced_cv_weighted compute their weights as SVC.fit does (on a numpy backend).
"""

import ctypes as C
import os

import numpy as np
import pytest

import pcg_model as pm
import reduced_loo_model as lm
import reduced_model as rm
import reduced_weighted_model as wm
from conftest import ROOT
from plssvm_amd import _capi, backend, svc
from plssvm_amd.csvm import CSVM, MI355CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter

EPS64 = rm.EPS64


# ---------------------------------------------------------------- the conditions of the GPU tests ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name, k", [("rbf_777x5", 1), ("rbf_777x5", 3), ("poly_777x16", 1), ("poly_777x16", 3), ("rbf_200x4", 1)])
def test_gpu_cases_meet_the_conditions_of_their_bounds(name, k, dtype):
    p = wm.fit_case(name, dtype, k)
    w = p["w"]
    assert w.shape == (p["X"].shape[0],) and np.all(w >= 0.0) and np.count_nonzero(w == 1024.0) == 3
    assert (np.count_nonzero(w == 0.0) > 0) == (name != "rbf_200x4")
    model = wm.WeightedReducedModel(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], w, held=p["held"], **p["kw"])
    e = wm.e_model(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], w, p["points"], held=p["held"], **p["kw"])
    cond_eps, e_rec = wm.RECORDED[name]
    print(f"{name} {np.dtype(dtype).name} k={k}: retries {model.retries}, cond(M) eps64 {model.cond * EPS64:.1e} (recorded {cond_eps:.1e}), e_model {e:.1e} (recorded {e_rec:.1e})")
    assert model.retries == 0 and np.isfinite(e)
    assert cond_eps / 10.0 <= model.cond * EPS64 <= cond_eps * 10.0
    # the bound of the GPU test, 8 max(e_model, cond eps64) max|f|, says something: it is far below the decision values themselves
    assert 8.0 * max(e, model.cond * EPS64) <= 1e-3


def test_the_linear_case_is_singular_by_construction_as_without_weights():
    p = wm.fit_case("linear_300x6")
    model = wm.WeightedReducedModel(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], p["w"], **p["kw"])
    e = wm.e_model(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], p["w"], p["points"], **p["kw"])
    full = wm.dense_full_solution(p["kernel"], p["X"], p["Y"][0], p["cost"], p["w"], p["points"], **p["kw"])
    print(f"linear: cond(M) eps64 {model.cond * EPS64:.2f}, on the range of Phi {model.cond_range * EPS64:.1e}, e_model {e:.1e}")
    assert model.retries == 0 and 0.05 <= model.cond * EPS64 <= 10.0 and e <= 1e-10
    assert np.max(np.abs(model.decision_values(p["points"])[0] - full)) <= 8.0 * max(e, model.cond_range * EPS64) * np.max(np.abs(full))


def test_every_point_a_landmark_is_the_weighted_full_solution():
    p = wm.fit_case("rbf_200x4")
    model = wm.WeightedReducedModel(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], p["w"], held=p["held"], **p["kw"])
    e = wm.e_model(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], p["w"], p["points"], held=p["held"], **p["kw"])
    full = wm.dense_full_solution(p["kernel"], p["X"], p["Y"][0], p["cost"], p["w"], p["points"], held=p["held"], **p["kw"])
    assert np.min(p["w"]) >= 0.01
    assert np.max(np.abs(model.decision_values(p["points"])[0] - full)) <= rm.fit_tolerance(model, e, full)


# ---------------------------------------------------------------- leave-one-out ----------------------------------------------------------------
@pytest.mark.parametrize("rank", [16, 130])
def test_the_weighted_identity_against_brute_force_refits(rank):
    p = wm.loo_case(rank=rank)
    w = p["w"]
    assert np.max(w) == 64.0 and np.count_nonzero(w == 0.0) > 0
    cost = wm.LOO_COSTS[0]
    model = wm.WeightedLooModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], w, held=p["held"], **p["kw"])
    h_s, f_s, loo_s = wm.stable(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], w, held=p["held"], **p["kw"])
    brute = wm.brute_force(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], w, held=p["held"], **p["kw"])
    e = wm.e_loo(model, loo_s)
    tol = lm.tolerance(model, e, np.max(np.abs(brute)))
    print(f"rank {rank}: |loo - refits| {np.max(np.abs(model.loo - brute)):.1e}, tolerance {tol:.1e}, largest leverage {model.max_leverage:.2f}, e_loo {e:.1e}")
    assert model.retries == 0 and model.max_leverage < 1.0
    assert np.max(np.abs(model.loo - brute)) <= tol and np.max(np.abs(loo_s - brute)) <= tol
    assert np.max(np.abs(model.h - h_s)) <= tol
    zero = w == 0.0
    assert np.all(model.h[zero] == 0.0) and np.array_equal(model.loo[:, zero], model.f[:, zero])
    assert np.all(model.h >= 0.0)
    assert model.press[0] == pytest.approx(np.sum(w * (p["Y"][0] - model.loo[0]) ** 2)) and model.loo_errors[0] == np.sum((np.sign(model.loo[0]) != np.sign(p["Y"][0])) & (w > 0))


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("rank", [16, 130])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_loo_cases_meet_the_conditions_of_their_bounds(dtype, rank, k):
    p = wm.loo_case(dtype, k, rank)
    for cost in wm.LOO_COSTS:
        model = wm.WeightedLooModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], p["w"], held=p["held"], **p["kw"])
        e = wm.e_loo(model, wm.stable(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], p["w"], held=p["held"], **p["kw"])[2])
        assert model.retries == 0 and model.max_leverage < 0.99 and np.isfinite(e)
        assert 8.0 * max(e, model.cond * EPS64) <= 1e-2  # (the tolerance of the GPU test says something)


def test_unit_weights_are_the_unweighted_models():
    p = wm.loo_case(k=3)
    ones = np.ones(p["X"].shape[0])
    a = wm.WeightedLooModel(p["kernel"], p["X"], p["Y"], 10.0, p["landmarks"], ones, held=p["held"], **p["kw"])
    b = lm.LooModel(p["kernel"], p["X"], p["Y"], 10.0, p["landmarks"], held=p["held"], **p["kw"])
    tol = lm.tolerance(b, 0.0, 1.0)
    for x, y in ((a.h, b.h), (a.f, b.f), (a.loo, b.loo), (a.betas, b.betas), (a.rhos, b.rhos)):
        assert np.max(np.abs(x - y)) <= tol * max(1.0, np.max(np.abs(y)))
    c = wm.WeightedReducedModel(p["kernel"], p["X"], p["Y"], 10.0, p["landmarks"], ones, held=p["held"], **p["kw"])
    d = rm.ReducedModel(p["kernel"], p["X"], p["Y"], 10.0, p["landmarks"], held=p["held"], **p["kw"])
    assert np.max(np.abs(c.betas - d.betas)) <= tol * np.max(np.abs(d.betas)) and c.nu == pytest.approx(d.nu, rel=1e-12)


# ---------------------------------------------------------------- duplication and removal ----------------------------------------------------------------
def duplication_case():
    N, d, rank = 255, 5, 16
    X, y = pm.make_data(N, d, pm.DATA_SEED, np.float64)
    w = np.random.default_rng(41).integers(0, 4, N)
    lms = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
    w[np.asarray(lms[:2], dtype=np.int64)] = (0, 3)  # a landmark of weight 0 (it stays a basis centre) and a duplicated one
    points = pm.make_data(rm.HELD_OUT, d, rm.HELD_OUT_SEED, np.float64)[0]
    return X, y[None, :], w, lms, points, dict(gamma=0.2)


def test_integer_weights_are_duplicated_rows_and_weight_zero_is_removal():
    X, Y, w, lms, points, kw = duplication_case()
    assert set(np.unique(w).tolist()) == {0, 1, 2, 3}
    weighted = wm.WeightedReducedModel("rbf", X, Y, 10.0, lms, w.astype(np.float64), **kw)
    e = wm.e_model("rbf", X, Y, 10.0, lms, w.astype(np.float64), points, **kw)
    f = weighted.decision_values(points)
    tol = rm.fit_tolerance(weighted, e, f)
    # duplication: the unweighted model on the expanded rows.  A landmark of weight 0 is no row of that set, so Phi is evaluated against the landmark POINTS
    Xd, Yd, first = wm.expand(X, Y, w)
    Phi = pm.kernel_matrix("rbf", Xd, X[lms.astype(np.int64)], **kw)
    K_mm = pm.kernel_matrix("rbf", X[lms.astype(np.int64)], X[lms.astype(np.int64)], **kw)
    beta, b = wm._stacked(Phi, K_mm, Yd, 10.0, np.ones(Xd.shape[0]))
    g = rm.decision_values("rbf", X[lms.astype(np.int64)], beta.T, -b, points, **kw)
    assert np.max(np.abs(f - g)) <= tol
    # removal: weights in {0, 1} against the unweighted ReducedModel on the rows that are left, its landmarks mapped to the rows' new places
    w01 = (w > 0).astype(np.float64)
    keep_lm = lms[w01[lms.astype(np.int64)] > 0]
    Xr, Yr, first = wm.expand(X, Y, w01.astype(np.int64))
    a = wm.WeightedReducedModel("rbf", X, Y, 10.0, keep_lm, w01, **kw)
    c = rm.ReducedModel("rbf", Xr, Yr, 10.0, first[keep_lm.astype(np.int64)], **kw)
    assert np.all(first[keep_lm.astype(np.int64)] >= 0)
    fa, fc = a.decision_values(points), c.decision_values(points)
    assert np.max(np.abs(fa - fc)) <= rm.fit_tolerance(c, rm.e_model("rbf", Xr, Yr, 10.0, first[keep_lm.astype(np.int64)], points, **kw), fc)


# ---------------------------------------------------------------- the boundary ----------------------------------------------------------------
PUBLIC = ("lssvm_mi355_problem_fit_reduced_weighted", "lssvm_mi355_fit_reduced_weighted_f32", "lssvm_mi355_fit_reduced_weighted_f64",
          "lssvm_mi355_problem_fit_reduced_loo_weighted", "lssvm_mi355_fit_reduced_loo_weighted_f32", "lssvm_mi355_fit_reduced_loo_weighted_f64")


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "plssvm_amd.h")).read()
    testing = open(os.path.join(ROOT, "include", "plssvm_amd_testing.h")).read()
    for name in PUBLIC:
        assert name in _capi.EXPORTED_SYMBOLS and name + "(" in header and hasattr(_capi.lib, name)
    name = "lssvm_mi355_problem_landmark_gram_weighted"
    assert name in _capi.EXPORTED_SYMBOLS and name + "(" in testing and name + "(" not in header and hasattr(_capi.lib, name)
    assert _capi.ABI_VERSION == 4 and C.sizeof(_capi.LssvmReducedInfo) == 64 and C.sizeof(_capi.LssvmReducedLooInfo) == 56 and C.sizeof(_capi.LssvmDenseInfo) == 72


def test_new_refusals_are_raised_before_a_device_is_touched():
    N = 12
    X = np.arange(36, dtype=np.float64).reshape(N, 3) / 7.0
    y = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    prm = Parameter(kernel_type="rbf")
    good = np.ones(N)
    bad_weights = [(np.r_[good[:-1], -1.0], "not less than 0.0"), (np.r_[good[:-1], np.nan], "finite"), (np.r_[good[:-1], np.inf], "finite"), (np.zeros(N), "sum greater than 0.0"),
                   (np.full(N, 1e308), "sum"), (good[:-1], "number of weights"), ("abc", "numbers")]
    # the Python surface, which checks as the library does
    for w, match in bad_weights:
        with pytest.raises(InvalidParameterError, match=match):
            backend.fit_reduced(prm, X, y, 4, sample_weight=w)
        with pytest.raises(InvalidParameterError, match=match):
            backend.fit_reduced_loo(prm, X, y, 4, [1.0], sample_weight=w)
    with pytest.raises(InvalidParameterError, match="factor"):
        backend.fit_reduced(prm, X, y, 4, sample_weight=good, factor="gpu")
    # the library itself: the one-shot entry points reach every check that needs no device
    ps = _capi.LssvmParams(2, 3, 1.0 / 3, 0.0, 1.0)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    costs = np.array([1.0, 10.0])
    for suffix, dtype in (("f32", np.float32), ("f64", np.float64)):
        data, target = X.astype(dtype), y.astype(dtype)
        fit = _capi.reduced_weighted_entry(f"lssvm_mi355_fit_reduced_weighted_{suffix}")
        loo = _capi.reduced_weighted_entry(f"lssvm_mi355_fit_reduced_loo_weighted_{suffix}")
        betas, rhos = np.zeros(2 * 4), np.zeros(2)

        def call_fit(w, factor=0, rank=4, slab_rows=0, b=betas, lms=None):
            return fit(C.byref(ps), _capi.ptr(data), N, 3, _capi.ptr(target), 1, None if w is None else w.ctypes.data_as(dp), rank, lms, slab_rows, factor,
                       None if b is None else b.ctypes.data_as(dp), rhos.ctypes.data_as(dp), None, None, None, None)

        def call_loo(w, factor=0, num_costs=2):
            return loo(C.byref(ps), _capi.ptr(data), N, 3, _capi.ptr(target), 1, None if w is None else w.ctypes.data_as(dp), 4, None, 0, costs.ctypes.data_as(dp), num_costs, factor,
                       betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp), None, None, None, None, None, None, None, None, None)

        for call in (call_fit, call_loo):
            for w, match in bad_weights[:5]:
                with pytest.raises(InvalidParameterError, match=match):
                    _capi.check(call(np.ascontiguousarray(w)))
            for factor in (-1, 2):
                with pytest.raises(InvalidParameterError, match="factor must be 0"):
                    _capi.check(call(good, factor=factor))
        # the refusals of the unweighted forms, reached through the weighted entry point
        with pytest.raises(InvalidParameterError, match="rank of the reduced model"):
            _capi.check(call_fit(good, rank=N + 1))
        with pytest.raises(InvalidParameterError, match="slab_rows"):
            _capi.check(call_fit(good, slab_rows=300))
        with pytest.raises(InvalidParameterError, match="must not be NULL"):
            _capi.check(call_fit(good, b=None))
        with pytest.raises(InvalidParameterError, match="distinct"):
            _capi.check(call_fit(good, lms=np.array([1, 2, 2, 3], dtype=np.uint64).ctypes.data_as(up)))
        with pytest.raises(InvalidParameterError, match="between 1 and 64 costs"):
            _capi.check(call_loo(good, num_costs=0))
    # a NULL handle
    bp = betas.ctypes.data_as(dp)
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(_capi.reduced_weighted_entry("lssvm_mi355_problem_fit_reduced_weighted")(None, _capi.ptr(y), 1, good.ctypes.data_as(dp), 4, None, 0, 0, bp, bp, None, None, None))
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(_capi.reduced_weighted_entry("lssvm_mi355_problem_fit_reduced_loo_weighted")(None, _capi.ptr(y), 1, good.ctypes.data_as(dp), 4, None, 0, costs.ctypes.data_as(dp), 2, 0, bp, bp,
                                                                                                  None, None, None, None, None, None, None, None))
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(_capi.reduced_weighted_entry("lssvm_mi355_problem_landmark_gram_weighted")(None, _capi.ptr(y), 1, good.ctypes.data_as(dp), 4, None, 0, bp))


# ---------------------------------------------------------------- the surface on a numpy backend ----------------------------------------------------------------
class NumpyCSVM(CSVM):
    """The base class's fit_reduced / fit_reduced_path on top of the numpy model; records the weights it was given."""

    seen = None

    def solve_reduced_systems(self, params, A, Y, rank, landmarks=None, sample_weight=None):
        NumpyCSVM.seen = None if sample_weight is None else np.array(sample_weight)
        lms = rm.library_landmarks(A.shape[0], rank) if landmarks is None else np.asarray(landmarks, dtype=np.uint64)
        w = np.ones(A.shape[0]) if sample_weight is None else sample_weight
        model = wm.WeightedReducedModel("rbf", A, Y, params.cost, lms, w, gamma=params.gamma)
        return model.betas, model.rhos, lms, {"rank": rank, "jitter": model.nu}

    def solve_reduced_loo_systems(self, params, A, Y, rank, costs, landmarks=None, sample_weight=None):
        NumpyCSVM.seen = None if sample_weight is None else np.array(sample_weight)
        lms = rm.library_landmarks(A.shape[0], rank) if landmarks is None else np.asarray(landmarks, dtype=np.uint64)
        w = np.ones(A.shape[0]) if sample_weight is None else sample_weight
        models = [wm.WeightedLooModel("rbf", A, Y, cost, lms, w, gamma=params.gamma) for cost in costs]
        report = {"costs": np.array(costs), "leverage": np.stack([m.h for m in models]), "fitted": np.stack([m.f for m in models]), "loo": np.stack([m.loo for m in models]),
                  "press": np.stack([m.press for m in models]), "loo_errors": np.stack([m.loo_errors for m in models]).astype(np.uint64),
                  "max_leverage": np.array([m.max_leverage for m in models]), "jitter": np.array([m.nu for m in models]), "infos": [{"cost": cost} for cost in costs]}
        return np.stack([m.betas for m in models]), np.stack([m.rhos for m in models]), lms, report


@pytest.mark.parametrize("classes", [2, 3])
def test_svc_weighted_fits_compute_their_weights_like_svc_fit(classes, monkeypatch):
    monkeypatch.setattr(svc, "make_csvm", lambda params=None: NumpyCSVM(params=params))
    N = 180
    X, labels = lm.overlapping_blobs(N, 4, classes, seed=9)
    labels = np.where(np.random.default_rng(8).random(N) < 0.7, 0, labels)  # imbalanced: most points in class 0
    sw = np.random.default_rng(4).uniform(0.5, 2.0, N)
    sw[::17] = 0.0
    counts = np.array([np.count_nonzero(labels == c) for c in range(classes)], dtype=np.float64)
    balanced = N / (classes * counts)
    for class_weight, multipliers in (("balanced", balanced), ({1: 5.0}, np.r_[1.0, 5.0, np.ones(classes - 2)]), (None, np.ones(classes))):
        est = svc.SVC(kernel="rbf", C=10.0, gamma=0.25, class_weight=class_weight)
        expected = sw * multipliers[labels]
        fitted = svc.fit_reduced_weighted(est, X, labels, 16, sample_weight=sw)
        assert np.array_equal(NumpyCSVM.seen, expected) and np.allclose(fitted.class_weight_, multipliers) and est._fit is None
        assert fitted.dual_coef_.shape == (1 if classes == 2 else classes, 16)
        svc.fit_reduced_weighted(est, X, labels, 16)  # no sample_weight: the class weights alone
        assert np.array_equal(NumpyCSVM.seen, multipliers[labels])
        scores, clones = svc.fit_reduced_cv_weighted(est, X, labels, 16, [0.5, 50.0], sample_weight=sw)
        assert np.array_equal(NumpyCSVM.seen, expected) and [c.C for c in clones] == [0.5, 50.0] and all(np.allclose(c.class_weight_, multipliers) for c in clones)
        # the score: np.average of the correct leave-one-out predictions under these weights
        Y = np.where(labels[None, :] == np.arange(classes)[:, None], 1.0, -1.0)[(1 if classes == 2 else 0):]
        for s, cost in enumerate((0.5, 50.0)):
            loo = wm.WeightedLooModel("rbf", X, Y, cost, rm.library_landmarks(N, 16), expected, gamma=0.25).loo
            predicted = (loo[0] > 0).astype(int) if classes == 2 else np.argmax(loo, axis=0)
            correct = (np.sign(loo[0]) == np.sign(Y[0])) if classes == 2 else predicted == labels
            assert scores[s] == pytest.approx(np.average(correct, weights=expected), abs=1e-12)
    # the unweighted functions stay as they are, refusal included
    with pytest.raises(InvalidParameterError, match="class_weight"):
        svc.fit_reduced(svc.SVC(class_weight="balanced"), X, labels, 16)
    with pytest.raises(InvalidParameterError, match="class_weight"):
        svc.fit_reduced_cv(svc.SVC(class_weight="balanced"), X, labels, 16, [1.0])
    svc.fit_reduced(svc.SVC(kernel="rbf", gamma=0.25), X, labels, 16)
    assert NumpyCSVM.seen is None
    with pytest.raises(InvalidParameterError, match="plssvm_amd.svc.SVC"):
        svc.fit_reduced_weighted(object(), X, labels, 4)
    with pytest.raises(InvalidParameterError, match="sample weights"):
        svc.fit_reduced_weighted(svc.SVC(), X, labels, 4, sample_weight=sw[:-1])
    with pytest.raises(InvalidParameterError, match="factor"):
        svc.fit_reduced_cv_weighted(svc.SVC(), X, labels, 4, [1.0], factor="gpu")


def test_csvm_keywords_and_documents():
    X, labels = rm.blobs(120, 4, 2, seed=5)
    data = DataSet(X, labels.tolist())
    w = np.random.default_rng(2).uniform(0.0, 2.0, 120)
    svm = NumpyCSVM(kernel_type="rbf", cost=3.0)
    model = svm.fit_reduced(data, 16, sample_weight=w)
    assert np.array_equal(NumpyCSVM.seen, w) and model.num_support_vectors() == 16
    models, report = svm.fit_reduced_path(data, 16, [0.5, 50.0], sample_weight=w)
    y = data.mapped_labels().astype(np.float64)
    assert np.allclose(report["loo_accuracy"], [np.average(np.sign(report["loo"][s]) == y, weights=w) for s in range(2)])
    svm.fit_reduced(data, 16)
    assert NumpyCSVM.seen is None  # (no keyword where there are no weights: a backend written before it existed still serves)
    sharded = object.__new__(MI355CSVM)
    sharded.use_devices, sharded._options = 2, None
    with pytest.raises(InvalidParameterError, match="one device"):
        sharded.solve_reduced_systems(Parameter(), X, np.ones((1, 120)), 4, sample_weight=w)
    for text in (backend.fit_reduced.__doc__, svc.fit_reduced_weighted.__doc__, CSVM.fit_reduced.__doc__):
        assert "landmark rules ignore the weights" in " ".join(text.split())
