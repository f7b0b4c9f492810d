"""Host side of the multi-class support (no GPU): the one-vs-all logic of ``SVC`` through a test double of the backend whose two boundary methods are dense float64
numpy (the LS-SVM system solved directly, the kernel evaluated directly) and that inherits ``CSVM``'s default loops, the two-class path as it was, and the argument
validation of the new C entry points."""

import ctypes as C

import numpy as np
import pytest

from plssvm_amd import _capi, backend, multiclass
from plssvm_amd import svc as svc_module
from plssvm_amd.csvm import CSVM
from plssvm_amd.data_set import DataSetError
from plssvm_amd.datagen import make_blobs_multiclass
from plssvm_amd.exceptions import BackendError, InvalidParameterError
from plssvm_amd.parameter import Parameter
from plssvm_amd.svc import SVC


def gram(params, A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    G = A @ B.T
    kt = int(params.kernel_type)
    if kt == 0:
        return G
    if kt == 1:
        return (params.gamma * G + params.coef0) ** params.degree
    sq = np.einsum("ij,ij->i", A, A)[:, None] + np.einsum("ij,ij->i", B, B)[None, :] - 2.0 * G
    return np.exp(-params.gamma * np.maximum(sq, 0.0))


class DenseCSVM(CSVM):
    """The two boundary methods in dense float64: [[K + diag(1 / (C w)), 1], [1^T, 0]] [alpha; b] = [y; 0], rho = -b; f(x) = sum_i alpha_i k(x_i, x) - rho."""

    instances = []

    def __init__(self, params=None, **kwargs):
        super().__init__(params, **kwargs)
        self.solves = []
        DenseCSVM.instances.append(self)

    def solve_system_of_linear_equations(self, params, A, b, eps, max_iter, sample_weight=None):
        A = np.asarray(A)
        n = A.shape[0]
        w = np.ones(n) if sample_weight is None else np.asarray(sample_weight, dtype=np.float64)
        self.solves.append({"b": np.array(b), "w": None if sample_weight is None else w.copy(), "n": n})
        M = np.zeros((n + 1, n + 1))
        M[:n, :n] = gram(params, A, A) + np.diag(1.0 / (params.cost * w))
        M[:n, n] = M[n, :n] = 1.0
        sol = np.linalg.solve(M, np.concatenate([np.asarray(b, dtype=np.float64), [0.0]]))
        return sol[:n].astype(A.dtype), A.dtype.type(-sol[n]), {"iterations": 3 + len(self.solves)}

    def predict_values(self, params, support_vectors, alpha, rho, w, predict_points):
        values = gram(params, predict_points, support_vectors) @ np.asarray(alpha, dtype=np.float64) - float(rho)
        return values.astype(np.asarray(support_vectors).dtype), None


@pytest.fixture
def dense(monkeypatch):
    DenseCSVM.instances = []
    monkeypatch.setattr(svc_module, "make_csvm", lambda params=None, **kw: DenseCSVM(params=params, **kw))
    return DenseCSVM


def blobs(k, seed, n=240, d=6, held=120):
    X, y = make_blobs_multiclass(n + held, d, k, seed=seed, dtype=np.float64)
    return X[:n], y[:n], X[n:], y[n:]


@pytest.mark.parametrize("kernel", ["linear", "poly", "rbf"])
@pytest.mark.parametrize("k, seed", [(3, 11), (5, 7)])
def test_svc_one_vs_all_through_a_dense_backend(dense, k, seed, kernel):
    Xt, yt, Xh, yh = blobs(k, seed)
    clf = SVC(kernel=kernel, C=1.0).fit(Xt, yt)
    n = Xt.shape[0]
    assert np.array_equal(clf.classes_, np.arange(k)) and clf.classes_.shape == (k,)
    assert clf.dual_coef_.shape == (k, n) and clf.intercept_.shape == (k,) and clf.class_weight_.shape == (k,)
    assert isinstance(clf.n_iter_, np.ndarray) and clf.n_iter_.shape == (k,) and np.issubdtype(clf.n_iter_.dtype, np.integer)
    assert clf.n_iter_.tolist() == [4 + c for c in range(k)]  # (the double counts its solves: one per class, in class order)
    assert clf.n_support_.shape == (k,) and clf.n_support_.dtype == np.int32 and clf.n_support_.tolist() == [np.count_nonzero(yt == c) for c in range(k)]
    assert np.array_equal(clf.support_, np.arange(n)) and clf.support_vectors_.shape == Xt.shape and clf.shape_fit_ == Xt.shape and clf.n_features_in_ == Xt.shape[1]
    # classifier c: y = +1 for class c, -1 for the rest; unweighted
    svm = dense.instances[-1]
    assert len(svm.solves) == k
    for c in range(k):
        assert np.array_equal(svm.solves[c]["b"], np.where(yt == c, 1.0, -1.0)) and svm.solves[c]["w"] is None
    # the decision values are the double's per-class values, the prediction is their argmax
    values = clf.decision_function(Xh)
    assert values.shape == (Xh.shape[0], k)
    params = clf._model.params
    for c in range(k):
        want, _ = svm.predict_values(params, Xt, clf.dual_coef_[c], -clf.intercept_[c], None, Xh)
        assert np.array_equal(values[:, c], want)
    assert np.array_equal(clf.predict(Xh), clf.classes_[np.argmax(values, axis=1)])
    assert np.array_equal(clf.predict(Xh), yh) and clf.score(Xh, yh) == 1.0


def test_string_and_non_contiguous_integer_labels(dense):
    Xt, yt, Xh, yh = blobs(3, 11)
    names = np.array(["pear", "apple", "quince"])  # (sorted: apple, pear, quince)
    clf = SVC(kernel="rbf").fit(Xt, names[yt])
    assert clf.classes_.tolist() == ["apple", "pear", "quince"]
    assert np.array_equal(clf.predict(Xh), names[yh])
    assert np.array_equal(dense.instances[-1].solves[0]["b"], np.where(yt == 1, 1.0, -1.0))  # classifier 0 is "apple" = class 1 of the recipe
    codes = np.array([40, -7, 1000])
    clf = SVC(kernel="linear").fit(Xt, codes[yt])
    assert clf.classes_.tolist() == [-7, 40, 1000]
    assert np.array_equal(clf.predict(Xh), codes[yh]) and clf.score(Xh, codes[yh]) == 1.0


def test_an_exact_tie_goes_to_the_lower_class_index(dense, monkeypatch):
    Xt, yt, Xh, _ = blobs(3, 11)
    clf = SVC(kernel="rbf").fit(Xt, yt)
    tied = np.array([[0.25, 0.5, 0.5], [0.5, 0.5, 0.25], [-1.0, -1.0, -1.0], [0.0, 0.1, 0.2]])
    monkeypatch.setattr(multiclass, "decision_values", lambda svm, model, X: tied)
    assert clf.predict(Xh[:4]).tolist() == [1, 0, 0, 2]
    assert multiclass.predict_classes(np.array(["a", "b", "c"]), tied).tolist() == ["b", "a", "a", "c"]


def test_class_weight_and_sample_weight_are_the_same_in_every_classifier(dense):
    Xt, yt, _, _ = blobs(3, 11, n=200)
    yt = yt.copy()
    yt[:50] = 0  # unbalanced
    clf = SVC(kernel="rbf", class_weight="balanced").fit(Xt, yt)
    counts = np.array([np.count_nonzero(yt == c) for c in range(3)])
    want = (yt.size / (3 * counts))[yt]
    assert np.allclose(clf.class_weight_, yt.size / (3 * counts), rtol=1e-15)
    solves = dense.instances[-1].solves
    assert len(solves) == 3 and all(np.array_equal(s["w"], want) for s in solves)
    # a dict, times sample_weight; points of weight 0 are dropped from every classifier and from the model
    sw = np.ones(yt.size)
    sw[::4] = 0.0
    sw[1::4] = 2.5
    clf = SVC(kernel="linear", class_weight={1: 3.0}).fit(Xt, yt, sample_weight=sw)
    keep = np.flatnonzero(sw > 0)
    want = (sw * np.array([1.0, 3.0, 1.0])[yt])[keep]
    solves = dense.instances[-1].solves
    assert all(s["n"] == keep.size and np.array_equal(s["w"], want) for s in solves)
    assert np.array_equal(clf.support_, keep) and clf.dual_coef_.shape == (3, keep.size) and clf.support_vectors_.shape == (keep.size, Xt.shape[1])
    assert clf.n_support_.tolist() == [np.count_nonzero(yt[keep] == c) for c in range(3)]


def test_clone_and_grid_search(dense):
    sklearn_base = pytest.importorskip("sklearn.base")
    model_selection = pytest.importorskip("sklearn.model_selection")
    Xt, yt, Xh, yh = blobs(3, 11)
    clf = sklearn_base.clone(SVC(kernel="rbf", C=2.0))
    assert clf.fit(Xt, yt).score(Xh, yh) == 1.0
    assert clf.__sklearn_tags__().classifier_tags.multi_class is True
    search = model_selection.GridSearchCV(SVC(kernel="rbf"), {"C": [0.5, 2.0]}, cv=3).fit(Xt, yt)
    assert search.best_estimator_.dual_coef_.shape[0] == 3 and search.score(Xh, yh) == 1.0


def test_two_classes_keep_their_shapes_and_a_single_class_stays_an_error(dense):
    Xt, yt, Xh, yh = blobs(2, 5)
    clf = SVC(kernel="rbf").fit(Xt, yt)
    n = Xt.shape[0]
    svm = dense.instances[-1]
    assert len(svm.solves) == 1 and np.array_equal(svm.solves[0]["b"], np.where(yt == 1, 1.0, -1.0))
    assert clf.dual_coef_.shape == (1, n) and clf.intercept_.shape == (1,) and isinstance(clf.n_iter_, int) and clf.n_iter_ == 4
    assert clf.classes_.tolist() == [0, 1] and clf.n_support_.shape == (2,) and clf.class_weight_.shape == (2,)
    values = clf.decision_function(Xh)
    assert values.shape == (Xh.shape[0],)
    want, _ = svm.predict_values(clf._model.params, Xt, clf.dual_coef_[0], -clf.intercept_[0], None, Xh)
    assert np.array_equal(values, want)
    assert np.array_equal(clf.predict(Xh), np.where(values > 0, 1, 0)) and clf.score(Xh, yh) == 1.0
    with pytest.raises(DataSetError, match="binary classification"):
        SVC().fit(Xt, np.zeros(n, dtype=int))


def test_default_loops_of_the_base_class():
    svm = DenseCSVM(params=Parameter(kernel_type="rbf", gamma=0.5))
    Xt, yt, Xh, _ = blobs(3, 11, n=60, held=20)
    p = svm.params.resolved(Xt.shape[1])
    B = multiclass.one_vs_all_targets(np.arange(3), yt, np.float64)
    assert B.shape == (3, 60) and set(np.unique(B).tolist()) == {-1.0, 1.0} and np.all(B.sum(axis=0) == -1.0)
    alphas, rhos, infos = svm.solve_systems_of_linear_equations(p, Xt, B, 1e-3, 60)
    assert alphas.shape == (3, 60) and rhos.shape == (3,) and len(infos) == 3
    values, ws = svm.predict_values_multi(p, Xt, alphas, rhos, None, Xh)
    assert values.shape == (20, 3) and ws is None
    for c in range(3):
        a, rho, _ = svm.solve_system_of_linear_equations(p, Xt, B[c], 1e-3, 60)
        assert np.array_equal(alphas[c], a) and rhos[c] == rho
        assert np.array_equal(values[:, c], svm.predict_values(p, Xt, a, rho, None, Xh)[0])
    with pytest.raises(InvalidParameterError, match="right-hand sides"):
        svm.solve_systems_of_linear_equations(p, Xt, B[0], 1e-3, 60)


# ------------------------------------------------------------------------------------------------------------------ the C entry points, without a device
def call_multi(dt, alpha="ok", rho="ok", out="ok", k=2):
    X = np.ones((4, 3), dtype=dt)
    ps = _capi.LssvmParams(2, 3, 1.0 / 3, 0.0, 1.0)
    a, r, o, w = np.ones((2, 4), dtype=dt), np.zeros(2, dtype=dt), np.zeros((4, 2), dtype=dt), np.zeros((2, 3), dtype=dt)
    w_valid = C.c_int(0)
    return _capi.predict_multi_entry(dt)(C.byref(ps), _capi.ptr(X), 4, 3, _capi.ptr(a) if alpha == "ok" else None, _capi.ptr(r) if rho == "ok" else None, k, _capi.ptr(w),
                                         C.byref(w_valid), _capi.ptr(X), 4, _capi.ptr(o) if out == "ok" else None, None, None)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_predict_values_multi_validates_its_arguments_without_a_device(dt):
    with pytest.raises(InvalidParameterError, match="number of weights"):
        _capi.check(call_multi(dt, alpha=None))
    with pytest.raises(InvalidParameterError, match="rho"):
        _capi.check(call_multi(dt, rho=None))
    with pytest.raises(InvalidParameterError, match="out"):
        _capi.check(call_multi(dt, out=None))
    with pytest.raises(InvalidParameterError, match="number of weight vectors"):
        _capi.check(call_multi(dt, k=0))
    # the Python mirror checks the shapes before it calls
    X = np.ones((4, 3), dtype=dt)
    with pytest.raises(InvalidParameterError, match="number of weights"):
        backend.predict_values_multi(Parameter(), X, np.ones((2, 5)), np.zeros(2), None, X)
    with pytest.raises(InvalidParameterError, match="rho values"):
        backend.predict_values_multi(Parameter(), X, np.ones((2, 4)), np.zeros(3), None, X)
    with pytest.raises(InvalidParameterError, match="one row per weight vector"):
        backend.predict_values_multi(Parameter(), X, np.ones(4), np.zeros(1), None, X)
    with pytest.raises(InvalidParameterError, match="w must be empty"):
        backend.predict_values_multi(Parameter(), X, np.ones((2, 4)), np.zeros(2), np.ones((2, 2)), X)


def test_predict_info_reports_vectors_per_launch():
    assert C.sizeof(_capi.LssvmPredictInfo) == 56
    assert [name for name, _ in _capi.LssvmPredictInfo._fields_][-1] == "vectors_per_launch"
    assert _capi.LssvmPredictInfo().as_dict()["vectors_per_launch"] == 0


@pytest.mark.skipif(_capi.device_count() > 0, reason="only meaningful on a box without a GPU")
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_predict_values_multi_without_a_device_is_a_loud_error(dt):
    with pytest.raises(BackendError, match="no HIP capable devices"):
        _capi.check(call_multi(dt))
    X = np.ones((4, 3), dtype=dt)
    with pytest.raises(BackendError, match="no HIP capable devices"):
        backend.predict_values_multi(Parameter(kernel_type="linear"), X, np.ones((2, 4)), np.zeros(2), None, X)
