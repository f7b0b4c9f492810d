"""CPU: the numpy model of the fixed-size LS-SVM (tests/reduced_model.py), the conditions on the inputs of tests/test_gpu_reduced.py, and the
host side of the new entry points.

  * every point a landmark: the model is the full dual LS-SVM (200 x 4 rbf, gamma 0.5, C 10).  The issue measured 5e-11 of the values' scale on data it did not record; on
    this project's uniform data (pcg_model.make_data, seed 20) M = K^2 + K / C - ... has the condition number 1.4e9 and the agreement is 1.4e-9 (standard normal data:
    2e7 and 1.7e-10), so the assertion is the rule of the GPU test -- 8 max(e_model, cond(M) eps64) -- and a flat 1e-8;
  * linear kernel, m >= d: again the full model, nu carrying the singular M (the issue: 1e-13 on its data; here 6e-13 at 300 x 6, m = 8, against the bound
    8 max(e_model, cond eps64) with the condition number taken on the range of Phi -- cond(M + nu I) itself is ~ 1 / eps64 and bounds nothing);
  * e_model -- the normal equations against a stacked least-squares solve of the same objective -- at every shape the GPU tests fit, asserted as a CONDITION ON THE INPUTS:
    <= 1e-7 at rank <= 64; no jitter retries on any of them;
  * the library's landmark rule restated; every refusal of include/plssvm_amd.h that needs no device; backend / CSVM / SVC argument checks.
"""

import ctypes as C
import os

import numpy as np
import pytest

import pcg_model as pm
import reduced_model as rm
from conftest import ROOT
from plssvm_amd import _capi, backend, svc
from plssvm_amd.csvm import CSVM, MI355CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter


# ---------------------------------------------------------------- the model ----------------------------------------------------------------
def test_all_points_as_landmarks_reproduce_the_full_dual_solution():
    p = rm.fit_case("rbf_200x4")
    model = rm.ReducedModel(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], **p["kw"])
    full = rm.dense_full_solution(p["kernel"], p["X"], p["Y"][0], p["cost"], p["points"], **p["kw"])
    f = model.decision_values(p["points"])[0]
    err = np.max(np.abs(f - full)) / np.max(np.abs(full))
    e = rm.e_model(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], p["points"], **p["kw"])
    print(f"all landmarks: {err:.2e} (e_model {e:.2e}, cond {model.cond:.2e}, nu {model.nu:.2e}, retries {model.retries})")
    assert err * np.max(np.abs(full)) <= rm.fit_tolerance(model, e, full) and err <= 1e-8 and model.retries == 0


def test_linear_kernel_with_at_least_d_landmarks_reproduces_the_full_solution():
    p = rm.fit_case("linear_300x6")
    assert len(p["landmarks"]) >= p["X"].shape[1]
    model = rm.ReducedModel(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], **p["kw"])
    full = rm.dense_full_solution(p["kernel"], p["X"], p["Y"][0], p["cost"], p["points"], **p["kw"])
    f = model.decision_values(p["points"])[0]
    err = np.max(np.abs(f - full)) / np.max(np.abs(full))
    e = rm.e_model(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], p["points"], **p["kw"])
    print(f"linear: {err:.2e} (e_model {e:.2e}, cond {model.cond:.2e}, on the range of Phi {model.cond_range:.2e}, nu {model.nu:.2e}, retries {model.retries})")
    # M is singular: m = 8 landmarks span d = 6 directions, nu carries the rest (cond(M + nu I) ~ 4e15) -- the bound is the one on the range of Phi
    assert model.cond > 1e14 and model.cond_range < 1e3
    assert err * np.max(np.abs(full)) <= rm.range_tolerance(model, e, full) and err <= 1e-11 and model.retries == 0


@pytest.mark.parametrize("name", [c[0] for c in rm.FIT_CASES] + ["rbf_200x4", "linear_300x6"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [1, 3])
def test_e_model_is_a_condition_on_the_inputs_of_the_gpu_tests(name, dtype, k):
    p = rm.fit_case(name, dtype, k)
    model = rm.ReducedModel(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], held=p["held"], **p["kw"])
    e = rm.e_model(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], p["points"], held=p["held"], **p["kw"])
    print(f"e_model {name} {np.dtype(dtype).name} k={k}: {e:.2e} cond {model.cond:.2e} retries {model.retries}")
    assert model.retries == 0
    if len(p["landmarks"]) <= 64:
        assert e <= 1e-7, (name, e)
    # the tolerance of the GPU test is finite and far below the values it compares
    f = model.decision_values(p["points"])
    tolerance = rm.range_tolerance if p["kernel"] == "linear" else rm.fit_tolerance
    assert tolerance(model, e, f) <= 1e-2 * np.max(np.abs(f))


def test_the_issues_table_of_e_model():
    """The rbf rows of the issue's table (777 x 5 uniform, gamma 0.2, C 100) on this project's seeds: e_model grows with the rank as the table shows (1e-12 ... 4e-6) and the
    conditioning of M with it -- the method's limit, reported through `jitter`."""
    p = rm.fit_case("rbf_777x5")
    seen = []
    for m, ceiling in ((16, 1e-10), (64, 1e-7), (256, 1e-4), (512, 1e-4)):
        lm = pm.draw_landmarks(777, m, pm.LANDMARK_SEED)
        e = rm.e_model(p["kernel"], p["X"], p["Y"], p["cost"], lm, p["points"], **p["kw"])
        cond = rm.ReducedModel(p["kernel"], p["X"], p["Y"], p["cost"], lm, **p["kw"]).cond
        print(f"rank {m}: e_model {e:.1e} cond(M) {cond:.1e}")
        assert e <= ceiling
        seen.append(cond)
    assert seen == sorted(seen)


def test_surface_data_is_separated_enough_for_the_label_test():
    """tests/test_gpu_reduced.py excepts points with |f| below the decision-value tolerance from its label comparison, at most 1 % of them: the numpy model alone stays
    within that on the data it uses (2 000 x 8 blobs, rank 64; three classes likewise)."""
    for classes in (2, 3):
        X, labels = rm.blobs(2000, 8, classes, seed=31)
        lm = rm.library_landmarks(2000, 64)
        Y = np.where(labels[None, :] == np.arange(classes)[:, None], 1.0, -1.0)
        if classes == 2:
            Y = Y[1:]
        model = rm.ReducedModel("rbf", X, Y, 10.0, lm, gamma=1.0 / 8)
        e = rm.e_model("rbf", X, Y, 10.0, lm, X, gamma=1.0 / 8)
        f = model.decision_values(X)
        tol = rm.fit_tolerance(model, e, f)
        margin = np.abs(f[0]) if classes == 2 else np.sort(f, axis=0)[-1] - np.sort(f, axis=0)[-2]
        predicted = (f[0] > 0).astype(int) if classes == 2 else np.argmax(f, axis=0)
        print(f"{classes} classes: tolerance {tol:.2e}, points below it {np.mean(margin <= 2 * tol):.4f}, accuracy {np.mean(predicted == labels):.4f}")
        assert np.mean(margin <= 2 * tol) <= 0.01
        assert np.mean(predicted == labels) >= 0.97
        assert len(set(labels[lm.astype(int)].tolist())) == classes


def test_held_data_is_the_given_data_up_to_float32_roundings():
    """The float32 rbf problem's centred and scaled data (reduced_model.held_data) gives the kernel of the data as given to a few float32 roundings of the exponent's
    terms -- and is the data as given everywhere else."""
    X = pm.make_data(300, 5, pm.DATA_SEED, np.float32)[0]
    kw = rm.rounded_parameters(np.float32, gamma=0.2)
    held, kw_held = rm.held_data("rbf", X, **kw)
    assert held.dtype == np.float32 and abs(held.mean()) < 1e-6
    a, b = pm.kernel_matrix("rbf", X, X[:40], **kw), pm.kernel_matrix("rbf", held, held[:40], **kw_held)
    assert 0.0 < np.max(np.abs(a - b)) <= 64 * rm.EPS32
    for kernel, data in (("rbf", X.astype(np.float64)), ("polynomial", X), ("linear", X)):
        assert rm.held_data(kernel, data, **kw)[0] is data
    assert rm.held_data("rbf", X, direct=True, **kw)[0] is X


def test_model_refuses_bad_landmarks():
    X, y = pm.make_data(20, 3, 1)
    for lm in ([], [1, 1], [20], [-1]):
        with pytest.raises(ValueError):
            rm.ReducedModel("rbf", X, y, 1.0, lm, gamma=0.5)
    rm.ReducedModel("rbf", X, y, 1.0, list(range(20)), gamma=0.5)  # (every point, the last one included)


def test_the_landmark_rule_restated():
    own = rm.library_landmarks(777, 64)
    assert len(set(own.tolist())) == 64 and own.max() < 777
    assert np.array_equal(rm.library_landmarks(777, 16), own[:16])  # a prefix rule
    assert np.array_equal(np.sort(rm.library_landmarks(50, 50)), np.arange(50))


# ---------------------------------------------------------------- the host side of the entry points ----------------------------------------------------------------
NAMES = ["lssvm_mi355_problem_fit_reduced", "lssvm_mi355_fit_reduced_f32", "lssvm_mi355_fit_reduced_f64"]
TESTING_NAMES = ["lssvm_mi355_problem_landmark_gram", "lssvm_mi355_problem_time_gram_kernels"]


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "plssvm_amd.h")).read()
    testing = open(os.path.join(ROOT, "include", "plssvm_amd_testing.h")).read()
    for name in NAMES:
        assert name in _capi.EXPORTED_SYMBOLS and name + "(" in header and hasattr(_capi.lib, name)
    for name in TESTING_NAMES:
        assert name in _capi.EXPORTED_SYMBOLS and name + "(" in testing and name + "(" not in header and hasattr(_capi.lib, name)
    assert C.sizeof(_capi.LssvmReducedInfo) == 64
    assert "static_assert(sizeof(lssvm_reduced_info) == 64" in open(os.path.join(ROOT, "plssvm_amd", "csrc", "capi.hip")).read()
    assert _capi.ABI_VERSION == 4 and len(_capi.OPTION_NAMES) == 16 and _capi.REDUCED_MAX_RANK == rm.MAX_RANK == 1024
    assert "lssvm_reduced.hip" in open(os.path.join(ROOT, "plssvm_amd", "csrc", "Makefile")).read()


def test_bad_arguments_are_refused_before_a_device_is_touched():
    """(this box has no GPU: whatever reaches a device fails with another error)"""
    X = np.random.default_rng(0).uniform(-1, 1, (12, 3))
    y = np.where(np.arange(12) % 2 == 0, 1.0, -1.0)
    prm = Parameter()
    # the binding's checks
    with pytest.raises(InvalidParameterError, match="right hand side"):
        backend.fit_reduced(prm, X, y[:5], 4)
    with pytest.raises(InvalidParameterError, match="right hand side"):
        backend.fit_reduced(prm, X, np.ones((0, 12)), 4)
    for rank in (0, 13, 1025):
        with pytest.raises(InvalidParameterError, match="rank of the reduced model"):
            backend.fit_reduced(prm, X, y, rank)
    with pytest.raises(InvalidParameterError, match="rank of the reduced model"):
        backend.fit_reduced(prm, X, y, 2.5)
    with pytest.raises(InvalidParameterError, match="landmarks"):
        backend.fit_reduced(prm, X, y, 4, landmarks=[])
    for slab_rows in (100, 255, -256, 256.0):
        with pytest.raises(InvalidParameterError, match="slab_rows"):
            backend.fit_reduced(prm, X, y, 4, slab_rows=slab_rows)
    # duplicate and out-of-range landmarks: the library's own check, before the problem is created
    with pytest.raises(InvalidParameterError, match="distinct"):
        backend.fit_reduced(prm, X, y, 4, landmarks=[3, 7, 3])
    with pytest.raises(InvalidParameterError, match="index of a data point"):
        backend.fit_reduced(prm, X, y, 4, landmarks=[3, 12])
    # the library's checks through the raw entry point
    ps = _capi.LssvmParams(0, 3, 1.0, 0.0, 1.0)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    betas, rhos, used, info = np.zeros(4), np.zeros(1), np.zeros(4, dtype=np.uint64), _capi.LssvmReducedInfo()
    bp, rp, lp = betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp), used.ctypes.data_as(up)
    for suffix, data, target in (("f64", X, y), ("f32", X.astype(np.float32), y.astype(np.float32))):
        fn = _capi.reduced_entry(f"lssvm_mi355_fit_reduced_{suffix}")
        for rank in (0, 13, 1025):
            with pytest.raises(InvalidParameterError, match="rank of the reduced model"):
                _capi.check(fn(C.byref(ps), _capi.ptr(data), 12, 3, _capi.ptr(target), 1, rank, None, 0, bp, rp, lp, C.byref(info), None))
        with pytest.raises(InvalidParameterError, match="slab_rows"):
            _capi.check(fn(C.byref(ps), _capi.ptr(data), 12, 3, _capi.ptr(target), 1, 4, None, 300, bp, rp, lp, C.byref(info), None))
        with pytest.raises(InvalidParameterError, match="right hand sides"):
            _capi.check(fn(C.byref(ps), _capi.ptr(data), 12, 3, _capi.ptr(target), 0, 4, None, 0, bp, rp, lp, C.byref(info), None))
        with pytest.raises(InvalidParameterError, match="right hand side"):
            _capi.check(fn(C.byref(ps), _capi.ptr(data), 12, 3, None, 1, 4, None, 0, bp, rp, lp, C.byref(info), None))
        for b, r in ((None, rp), (bp, None)):
            with pytest.raises(InvalidParameterError, match="must not be NULL"):
                _capi.check(fn(C.byref(ps), _capi.ptr(data), 12, 3, _capi.ptr(target), 1, 4, None, 0, b, r, lp, C.byref(info), None))
        with pytest.raises(InvalidParameterError, match="data must not be empty"):
            _capi.check(fn(C.byref(ps), None, 12, 3, _capi.ptr(target), 1, 4, None, 0, bp, rp, lp, C.byref(info), None))
        bad = np.array([1, 2, 2, 3], dtype=np.uint64)
        with pytest.raises(InvalidParameterError, match="distinct"):
            _capi.check(fn(C.byref(ps), _capi.ptr(data), 12, 3, _capi.ptr(target), 1, 4, bad.ctypes.data_as(up), 0, bp, rp, lp, C.byref(info), None))
    # NULL handles, and the checks that come before the handle is used
    fit, gram, timing = (_capi.reduced_entry(n) for n in ("lssvm_mi355_problem_fit_reduced", "lssvm_mi355_problem_landmark_gram", "lssvm_mi355_problem_time_gram_kernels"))
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(fit(None, _capi.ptr(y), 1, 4, None, 0, bp, rp, lp, C.byref(info)))
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(gram(None, _capi.ptr(y), 1, 4, None, 0, bp))
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(timing(None, 1, bp, bp, None))


class NumpyCSVM(CSVM):
    """The base class's fit_reduced on top of the numpy model: what the method itself does with a backend's answer."""

    def solve_reduced_systems(self, params, A, Y, rank, landmarks=None):
        lm = rm.library_landmarks(A.shape[0], rank) if landmarks is None else np.asarray(landmarks, dtype=np.uint64)
        model = rm.ReducedModel("rbf", A, Y, params.cost, lm, gamma=params.gamma)
        return model.betas, model.rhos, lm, {"rank": len(lm), "jitter": model.nu}


def test_csvm_fit_reduced_builds_an_ordinary_model_and_validates(tmp_path):
    X, labels = rm.blobs(120, 4, 2, seed=5)
    names = ["cat" if v else "dog" for v in labels]
    data = DataSet(X, names, real_type=np.float32, label_type=str)
    svm = NumpyCSVM(kernel_type="rbf", cost=10.0)
    model = svm.fit_reduced(data, 16)
    lm = rm.library_landmarks(120, 16).astype(int)
    assert model.num_support_vectors() == 16 and np.array_equal(model.support_vectors(), data.data()[lm])
    assert model.labels() == [names[i] for i in lm] and model.different_labels() == data.different_labels()
    assert model.alpha.dtype == np.float32 and svm.last_cg_info["iterations"] == 0 and svm.last_cg_info["rank"] == 16
    assert np.array_equal(svm.last_cg_info["landmarks"], lm)
    # an ordinary model file
    from plssvm_amd.model import Model
    path = tmp_path / "reduced.model"
    model.save(str(path))
    loaded = Model.load(str(path), real_type=np.float32, label_type=str)
    assert loaded.num_support_vectors() == 16 and sorted(loaded.different_labels()) == sorted(data.different_labels())
    # the landmarks of a two-class fit must hold both classes
    dogs = [i for i, n in enumerate(names) if n == "dog"][:5]
    with pytest.raises(InvalidParameterError, match='no point of the class "cat"'):
        svm.fit_reduced(data, 5, landmarks=dogs)
    for bad, match in (([], "non-empty"), ([1, 1], "distinct"), ([0, 120], "index of a data point"), ([[0, 1]], "non-empty")):
        with pytest.raises(InvalidParameterError, match=match):
            svm.fit_reduced(data, 2, landmarks=bad)
    with pytest.raises(InvalidParameterError, match="No labels"):
        svm.fit_reduced(DataSet(X), 4)
    with pytest.raises(NotImplementedError):
        CSVM().fit_reduced(data, 4)
    # a backend object of several devices raises (the constructor needs a device: the method is called on a bare object)
    sharded = object.__new__(MI355CSVM)
    sharded.use_devices, sharded._options = 2, None
    with pytest.raises(InvalidParameterError, match="one device"):
        sharded.solve_reduced_systems(Parameter(), X, np.ones((1, 120)), 4)


def test_svc_fit_reduced_validates_its_arguments():
    X, labels = rm.blobs(30, 3, 2, seed=6)
    with pytest.raises(InvalidParameterError, match="plssvm_amd.svc.SVC"):
        svc.fit_reduced(object(), X, labels, 4)
    with pytest.raises(InvalidParameterError, match="class_weight"):
        svc.fit_reduced(svc.SVC(class_weight="balanced"), X, labels, 4)
    with pytest.raises(InvalidParameterError, match="shapes"):
        svc.fit_reduced(svc.SVC(), X, labels[:-1], 4)
    with pytest.raises(InvalidParameterError, match="not supported"):
        svc.fit_reduced(svc.SVC(kernel="sigmoid"), X, labels, 4)
    assert "rank" not in svc.SVC().get_params() and sorted(svc.SVC().get_params()) == sorted(svc._PARAM_NAMES)
