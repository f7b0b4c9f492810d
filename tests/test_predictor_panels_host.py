"""Host side of ``lssvm_mi355_predictor_create_panels`` (no GPU): the symbol is declared and exported, its argument validation is that of
``lssvm_mi355_predictor_create_multi`` -- the same messages, LSSVM_ERR_INVALID_ARGUMENT before any device is touched, never LSSVM_ERR_NO_DEVICE --, valid arguments on a
machine without a GPU give the loud no-device error, and the Python shape checks of ``backend.Predictor`` come before the library with ``panels=True`` too."""

import ctypes as C
import os

import numpy as np
import pytest

from plssvm_amd import _capi, backend
from plssvm_amd.exceptions import BackendError, InvalidParameterError
from plssvm_amd.parameter import Parameter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lssvm_mi355_predictor_create_panels"
K, NSV, D = 3, 5, 4  # (the validation does not look at the width: a panel-wide model is refused and accepted alike)


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
        backend.Predictor(prm, sv, alpha, rho, panels=True).close()
        backend.Predictor(prm, sv, alpha[0], 0.125, panels=True).close()
        return
    status, message = create_status(NAME, dtype, kernel=kernel)
    assert status == -2, message
    with pytest.raises(BackendError, match="LSSVM_ERR_NO_DEVICE"):
        backend.Predictor(prm, sv, alpha, rho, panels=True)
    with pytest.raises(BackendError, match="LSSVM_ERR_NO_DEVICE"):
        backend.Predictor(prm, sv, alpha[0], 0.125, panels=True)


def test_python_shape_checks_come_before_the_library_with_panels_too():
    """Every one of these raises InvalidParameterError -- on a machine without a GPU a call that reached the library would raise the no-device BackendError instead."""
    sv, alpha, rho = model()
    p = Parameter(kernel_type="rbf")
    with pytest.raises(InvalidParameterError, match="at least one row"):
        backend.Predictor(p, sv, np.zeros((0, NSV)), np.zeros(0), panels=True)
    with pytest.raises(InvalidParameterError, match="number of weights"):
        backend.Predictor(p, sv, alpha[:, :-1], rho, panels=True)
    with pytest.raises(InvalidParameterError, match="rho values"):
        backend.Predictor(p, sv, alpha, rho[:-1], panels=True)
    with pytest.raises(InvalidParameterError, match="rho values"):
        backend.Predictor(p, sv, alpha, 0.125, panels=True)
    with pytest.raises(InvalidParameterError, match="rho values"):
        backend.Predictor(p, sv, alpha, rho.reshape(1, K), panels=True)
    with pytest.raises(InvalidParameterError, match="number of weights"):  # one weight vector
        backend.Predictor(p, sv, alpha[0, :-1], 0.125, panels=True)
    with pytest.raises(InvalidParameterError, match="same number of features"):
        backend.Predictor(p, sv[0], alpha, rho, panels=True)


USAGE = {"f32": os.path.join(ROOT, "plssvm_amd", "lib", "asm", "resource_usage_tile_launch_f32xv2.txt"), "f64": os.path.join(ROOT, "plssvm_amd", "lib", "asm", "resource_usage_tile_launch_f64xv2.txt")}
KT_POLY, KT_RBF, KT_POLY2, KT_POLY3, KT_RBFF = 1, 2, 3, 4, 5  # (lssvm_types.hpp)


def kernels_of(path):
    """{kernel name: {resource: value}} of a unit's resource-usage remarks"""
    import re

    found, name = {}, None
    with open(path) as f:
        for line in f:
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                found[name] = {}
            for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
                m = re.search(pat, line)
                if m and name is not None:
                    found[name][key] = int(m.group(1))
    return found


@pytest.mark.parametrize("unit", ["f32", "f64"])
def test_the_two_vector_panel_units_hold_their_kernels_without_scratch_at_two_waves_per_simd(unit):
    """The register budget of the NV = 1 siblings, read from the cross-compile: eight fp32 kernels (four kernel functions x two plane kinds), four fp64 ones."""
    if not os.path.isfile(USAGE[unit]):
        pytest.skip("no build tree here (the resource-usage files do not travel to the GPU box)")
    found = kernels_of(USAGE[unit])
    if unit == "f32":
        want = {f"_ZN5lssvm24tile_matvec_f32_wide_nv2ILi{kt}ELi{pl}EEEvNS_8TileArgsIfEE" for kt in (KT_POLY, KT_POLY2, KT_POLY3, KT_RBFF) for pl in (2, 3)}
    else:
        want = {f"_ZN5lssvm20tile_matvec_f64_wideILi{kt}ELb0ELi2EEEvNS_8TileArgsIdEE" for kt in (KT_POLY, KT_RBF, KT_POLY2, KT_POLY3)}
    assert set(found) == want, sorted(set(found) ^ want)
    for name, res in found.items():
        assert res == {"scratch": 0, "occupancy": 2, "vgpr_spill": 0, "sgpr_spill": 0}, (name, res)
