"""Host side of the resident predictor of a one-vs-all model (no GPU): the Python shape checks of ``backend.Predictor`` with ``alpha`` of shape ``(k, n)``, the argument
validation of ``lssvm_mi355_predictor_create_multi`` / ``_predict_multi`` before any device is touched (LSSVM_ERR_INVALID_ARGUMENT, never LSSVM_ERR_NO_DEVICE), the loud
no-device error for valid arguments on a machine without a GPU, and ``multiclass.decision_values`` with a backend object that does not offer the resident call."""

import ctypes as C

import numpy as np
import pytest

from plssvm_amd import _capi, backend, multiclass
from plssvm_amd.exceptions import BackendError, InvalidParameterError
from plssvm_amd.parameter import Parameter

K, NSV, D = 3, 5, 4


def model(dtype=np.float32):
    rng = np.random.default_rng(1)
    return rng.uniform(-1, 1, (NSV, D)).astype(dtype), rng.uniform(-1, 1, (K, NSV)).astype(dtype), np.array([0.125, 0.25, 0.5])


def create_multi_status(dtype=np.float32, dtype_code=None, params_null=False, out_null=False, sv_null=False, nsv=NSV, nfeat=D, alphas_null=False, rhos_null=False, k=K, kernel="rbf"):
    sv, alpha, rho = model(dtype)
    ps = backend._params_struct(Parameter(kernel_type=kernel), D)
    h = C.c_void_p(None)
    fn = _capi.predictor_multi_entry("lssvm_mi355_predictor_create_multi")
    status = fn(None if out_null else C.byref(h), None if params_null else C.byref(ps), _capi.dtype_code(dtype) if dtype_code is None else dtype_code, None if sv_null else _capi.ptr(sv), nsv,
                nfeat, None if alphas_null else _capi.ptr(alpha), None if rhos_null else rho.ctypes.data_as(C.POINTER(C.c_double)), k, None)
    if h:
        _capi.lib.lssvm_mi355_predictor_destroy(h)
    return status


@pytest.mark.parametrize("kernel", ["linear", "polynomial", "rbf"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_create_multi_refuses_bad_arguments_before_any_device(dtype, kernel):
    """LSSVM_ERR_INVALID_ARGUMENT (-1), not LSSVM_ERR_NO_DEVICE (-2), on a machine with or without a GPU."""
    assert create_multi_status(dtype, kernel=kernel, k=0) == -1 and "weight vectors" in _capi.last_error()
    assert create_multi_status(dtype, kernel=kernel, alphas_null=True) == -1 and "weights" in _capi.last_error()
    assert create_multi_status(dtype, kernel=kernel, rhos_null=True) == -1 and "rhos" in _capi.last_error()
    assert create_multi_status(dtype, kernel=kernel, sv_null=True) == -1 and "support vectors" in _capi.last_error()
    assert create_multi_status(dtype, kernel=kernel, nsv=0) == -1 and "support vectors" in _capi.last_error()
    assert create_multi_status(dtype, kernel=kernel, nfeat=0) == -1 and "feature" in _capi.last_error()
    assert create_multi_status(dtype, kernel=kernel, out_null=True) == -1
    assert create_multi_status(dtype, kernel=kernel, params_null=True) == -1
    assert create_multi_status(dtype, kernel=kernel, dtype_code=7) == -1 and "dtype" in _capi.last_error()
    assert create_multi_status(dtype, kernel=kernel, k=(1 << 20) + 1) == -1


def test_predict_multi_refuses_a_null_handle():
    fn = _capi.predictor_multi_entry("lssvm_mi355_predictor_predict_multi")
    out = np.zeros((2, K), np.float32)
    pts = np.zeros((2, D), np.float32)
    assert fn(None, _capi.ptr(pts), _capi.LSSVM_MEM_HOST, 2, _capi.ptr(out), None) == -1 and "handle" in _capi.last_error()


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_valid_arguments_without_a_device_raise_the_no_device_error(kernel):
    """... and nothing else: with a device the same arguments make a predictor."""
    sv, alpha, rho = model()
    if _capi.device_count() > 0:
        assert create_multi_status(kernel=kernel) == 0, _capi.last_error()
        backend.Predictor(Parameter(kernel_type=kernel), sv, alpha, rho).close()
        return
    assert create_multi_status(kernel=kernel) == -2, _capi.last_error()
    with pytest.raises(BackendError, match="LSSVM_ERR_NO_DEVICE"):
        backend.Predictor(Parameter(kernel_type=kernel), sv, alpha, rho)


def test_python_shape_checks_come_before_the_library():
    """Every one of these raises InvalidParameterError -- on a machine without a GPU a call that reached the library would raise the no-device BackendError instead."""
    sv, alpha, rho = model()
    p = Parameter(kernel_type="rbf")
    with pytest.raises(InvalidParameterError, match="at least one row"):
        backend.Predictor(p, sv, np.zeros((0, NSV), np.float32), np.zeros(0))
    with pytest.raises(InvalidParameterError, match="number of weights"):
        backend.Predictor(p, sv, alpha[:, :-1], rho)
    with pytest.raises(InvalidParameterError, match="rho values"):
        backend.Predictor(p, sv, alpha, rho[:-1])
    with pytest.raises(InvalidParameterError, match="rho values"):
        backend.Predictor(p, sv, alpha, 0.125)
    with pytest.raises(InvalidParameterError, match="rho values"):
        backend.Predictor(p, sv, alpha, rho.reshape(1, K))
    with pytest.raises(InvalidParameterError, match="number of weights"):  # one weight vector, as before
        backend.Predictor(p, sv, alpha[0, :-1], 0.125)
    with pytest.raises(InvalidParameterError, match="same number of features"):
        backend.Predictor(p, sv[0], alpha, rho)


def test_both_entry_points_are_declared_and_exported():
    for name in ("lssvm_mi355_predictor_create_multi", "lssvm_mi355_predictor_predict_multi"):
        assert name in _capi.EXPORTED_SYMBOLS
        assert getattr(_capi.lib, name) is not None


class LoopOnlyBackend:
    """A backend object without the resident call: what the dense stand-ins of tests/test_multiclass_host.py are to multiclass.decision_values."""

    def __init__(self):
        self.calls = 0

    def predict_values_multi(self, params, support_vectors, alphas, rhos, ws, predict_points):
        self.calls += 1
        values = np.asarray(predict_points, dtype=np.float64) @ (np.asarray(alphas, dtype=np.float64) @ np.asarray(support_vectors, dtype=np.float64)).T - np.asarray(rhos)
        return values, np.asarray(alphas) @ np.asarray(support_vectors)


def test_decision_values_without_the_resident_call_takes_the_default_loop():
    sv, alpha, rho = model(np.float64)
    m = multiclass.OneVsAllModel(Parameter(kernel_type="linear").resolved(D), np.arange(K), sv, alpha, rho, [])
    svm = LoopOnlyBackend()
    X = np.random.default_rng(2).uniform(-1, 1, (7, D))
    values = multiclass.decision_values(svm, m, X)
    assert svm.calls == 1 and values.shape == (7, K)
    assert np.allclose(values, X @ (alpha @ sv).T - rho)
    assert m.w is not None and np.allclose(m.w, alpha @ sv)  # the cached w of the default loop is still kept on the model
    assert not hasattr(m, "_predictor")


class ResidentBackend(LoopOnlyBackend):
    def __init__(self):
        super().__init__()
        self.resident_calls = 0

    def decision_values_resident(self, model, X):
        self.resident_calls += 1
        return np.full((np.shape(X)[0], len(model.classes)), 7.0)


def test_decision_values_prefers_the_resident_call_where_the_backend_offers_it():
    sv, alpha, rho = model(np.float64)
    m = multiclass.OneVsAllModel(Parameter(kernel_type="rbf").resolved(D), np.arange(K), sv, alpha, rho, [])
    svm = ResidentBackend()
    values = multiclass.decision_values(svm, m, np.zeros((4, D)))
    assert svm.resident_calls == 1 and svm.calls == 0 and np.all(values == 7.0) and values.shape == (4, K)
