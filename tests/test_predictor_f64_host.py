"""Host side of ``lssvm_mi355_predictor_create_resident`` (no GPU): the symbol is declared and exported, its argument validation is that of
``lssvm_mi355_predictor_create_multi`` -- the same messages, LSSVM_ERR_INVALID_ARGUMENT before any device is touched, never LSSVM_ERR_NO_DEVICE --, valid arguments on a
machine without a GPU give the loud no-device error, and the Python shape checks of ``backend.Predictor`` come before the library with ``every_form=True`` too."""

import ctypes as C
import os

import numpy as np
import pytest

from plssvm_amd import _capi, backend
from plssvm_amd.exceptions import BackendError, InvalidParameterError
from plssvm_amd.parameter import Parameter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lssvm_mi355_predictor_create_resident"
K, NSV, D = 3, 5, 4


def model(dtype=np.float64):
    rng = np.random.default_rng(1)
    return rng.uniform(-1, 1, (NSV, D)).astype(dtype), rng.uniform(-1, 1, (K, NSV)).astype(dtype), np.array([0.125, 0.25, 0.5])


def create_status(name, dtype=np.float64, dtype_code=None, params_null=False, out_null=False, sv_null=False, nsv=NSV, nfeat=D, alphas_null=False, rhos_null=False, k=K, kernel="rbf"):
    """(status, message) of a creation entry point"""
    sv, alpha, rho = model(dtype)
    ps = backend._params_struct(Parameter(kernel_type=kernel), D)
    h = C.c_void_p(None)
    fn = _capi.predictor_multi_entry(name)
    status = fn(None if out_null else C.byref(h), None if params_null else C.byref(ps), _capi.dtype_code(dtype) if dtype_code is None else dtype_code, None if sv_null else _capi.ptr(sv), nsv,
                nfeat, None if alphas_null else _capi.ptr(alpha), None if rhos_null else rho.ctypes.data_as(C.POINTER(C.c_double)), k, None)
    message = _capi.last_error() if status != 0 else ""
    if h:
        _capi.lib.lssvm_mi355_predictor_destroy(h)
    return status, message


def test_the_entry_point_is_declared_and_exported():
    assert NAME in _capi.EXPORTED_SYMBOLS
    assert getattr(_capi.lib, NAME) is not None
    with open(os.path.join(ROOT, "include", "plssvm_amd.h")) as f:
        header = f.read()
    assert f"int {NAME}(lssvm_mi355_predictor **out, const lssvm_params *params, int dtype, const void *support_vectors" in header
    assert _capi.lib.lssvm_mi355_abi_version() == 4  # (additive: the version stays)


BAD = [dict(k=0), dict(alphas_null=True), dict(rhos_null=True), dict(sv_null=True), dict(nsv=0), dict(nfeat=0), dict(out_null=True), dict(params_null=True), dict(dtype_code=7),
       dict(k=(1 << 20) + 1)]
WORDS = ["weight vectors", "weights", "rhos", "support vectors", "support vectors", "feature", "out", "", "dtype", "too many weight vectors"]


@pytest.mark.parametrize("kernel", ["linear", "polynomial", "rbf"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bad_arguments_are_refused_before_any_device_with_the_messages_of_create_multi(dtype, kernel):
    for bad, word in zip(BAD, WORDS):
        status, message = create_status(NAME, dtype, kernel=kernel, **bad)
        want_status, want_message = create_status("lssvm_mi355_predictor_create_multi", dtype, kernel=kernel, **bad)
        assert status == -1 and want_status == -1, (bad, status, message)
        assert message == want_message and word in message, (bad, message, want_message)


@pytest.mark.parametrize("kernel", ["linear", "polynomial", "rbf"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_valid_arguments_without_a_device_raise_the_no_device_error(dtype, kernel):
    """... and nothing else: with a device the same arguments make a predictor."""
    sv, alpha, rho = model(dtype)
    prm = Parameter(kernel_type=kernel)
    if _capi.device_count() > 0:
        assert create_status(NAME, dtype, kernel=kernel)[0] == 0
        backend.Predictor(prm, sv, alpha, rho, every_form=True).close()
        backend.Predictor(prm, sv, alpha[0], 0.125, every_form=True).close()
        return
    status, message = create_status(NAME, dtype, kernel=kernel)
    assert status == -2, message
    with pytest.raises(BackendError, match="LSSVM_ERR_NO_DEVICE"):
        backend.Predictor(prm, sv, alpha, rho, every_form=True)
    with pytest.raises(BackendError, match="LSSVM_ERR_NO_DEVICE"):
        backend.Predictor(prm, sv, alpha[0], 0.125, every_form=True)


def test_python_shape_checks_come_before_the_library_with_every_form_too():
    """Every one of these raises InvalidParameterError -- on a machine without a GPU a call that reached the library would raise the no-device BackendError instead."""
    sv, alpha, rho = model()
    p = Parameter(kernel_type="rbf")
    with pytest.raises(InvalidParameterError, match="at least one row"):
        backend.Predictor(p, sv, np.zeros((0, NSV)), np.zeros(0), every_form=True)
    with pytest.raises(InvalidParameterError, match="number of weights"):
        backend.Predictor(p, sv, alpha[:, :-1], rho, every_form=True)
    with pytest.raises(InvalidParameterError, match="rho values"):
        backend.Predictor(p, sv, alpha, rho[:-1], every_form=True)
    with pytest.raises(InvalidParameterError, match="rho values"):
        backend.Predictor(p, sv, alpha, 0.125, every_form=True)
    with pytest.raises(InvalidParameterError, match="rho values"):
        backend.Predictor(p, sv, alpha, rho.reshape(1, K), every_form=True)
    with pytest.raises(InvalidParameterError, match="number of weights"):  # one weight vector
        backend.Predictor(p, sv, alpha[0, :-1], 0.125, every_form=True)
    with pytest.raises(InvalidParameterError, match="same number of features"):
        backend.Predictor(p, sv[0], alpha, rho, every_form=True)
