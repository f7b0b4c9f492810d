"""Host side of the resident fp32 predictor beyond 128 features (no GPU): the translation unit of the wide two-vector kernels (plssvm_amd/csrc/tile_launch_f32v2w.hip)
holds exactly the 38 instantiations the routing function of lssvm_problem.hip may dispatch, every one without scratch at one wave per SIMD -- read from the
resource-usage file the build leaves beside the ISA of the library that ships --, and the Python shape checks of ``backend.Predictor(..., every_form=True)`` still come
before the library for a 192-feature float32 model."""

import os
import re

import numpy as np
import pytest

from plssvm_amd import backend
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE = os.path.join(ROOT, "plssvm_amd", "lib", "asm", "resource_usage_tile_launch_f32v2w.txt")
KT_POLY, KT_POLY2, KT_POLY3, KT_RBFF = 1, 3, 4, 5  # (lssvm_types.hpp)


def expected_kernels():
    """(wrapper, kernel type, 64-feature chunks): f16x3 planes -- polynomial forms on 3 ... 8 chunks, folded rbf on 3 ... 6 --, bf16x6 planes -- all four on 3 ... 6"""
    want = set()
    for kt in (KT_POLY, KT_POLY2, KT_POLY3, KT_RBFF):
        want.update(("f3w_nv2w", kt, n) for n in range(3, (6 if kt == KT_RBFF else 8) + 1))
        want.update(("s6w_nv2w", kt, n) for n in range(3, 7))
    return want


def test_the_wide_two_vector_unit_holds_the_38_kernels_without_scratch_at_one_wave_per_simd():
    if not os.path.isfile(USAGE):
        pytest.skip("no build tree here (the resource-usage files do not travel to the GPU box)")
    lib = os.path.join(ROOT, "plssvm_amd", "lib", "libplssvm_amd.so")
    assert os.path.getmtime(USAGE) <= os.path.getmtime(lib) + 1, "lib/asm is newer than the library: run make"
    found = {}
    name = None
    with open(USAGE) as f:
        for line in f:
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                found[name] = {}
                continue
            m = re.search(r"remark: \S+\s+(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
            if m and name is not None:
                found[name][m.group(1).split()[0]] = int(m.group(2))
    kernels = {}
    for name, usage in found.items():
        m = re.fullmatch(r"_ZN5lssvm\d+tile_matvec_f32_(f3w_nv2w|s6w_nv2w)ILi(\d+)ELi(\d+)EEEvNS_8TileArgsIfEE", name)
        assert m, f"a kernel that is no wide two-vector instantiation: {name}"
        kernels[(m.group(1), int(m.group(2)), int(m.group(3)))] = usage
    assert set(kernels) == expected_kernels() and len(kernels) == 38, sorted(set(kernels) ^ expected_kernels())
    for key, usage in sorted(kernels.items()):
        assert usage == {"ScratchSize": 0, "Occupancy": 1, "SGPRs": 0, "VGPRs": 0}, (key, usage)


def test_python_shape_checks_come_before_the_library_for_a_192_feature_float32_model():
    """Every one of these raises InvalidParameterError -- on a machine without a GPU a call that reached the library would raise the no-device BackendError instead."""
    rng = np.random.default_rng(2)
    nsv, d, k = 7, 192, 3
    sv = rng.uniform(-1, 1, (nsv, d)).astype(np.float32)
    alpha = rng.uniform(-1, 1, (k, nsv)).astype(np.float32)
    rho = np.array([0.125, 0.25, 0.5])
    for kernel in ("rbf", "polynomial"):
        p = Parameter(kernel_type=kernel, gamma=1.0 / d, coef0=0.5)
        with pytest.raises(InvalidParameterError, match="at least one row"):
            backend.Predictor(p, sv, np.zeros((0, nsv), np.float32), np.zeros(0), every_form=True)
        with pytest.raises(InvalidParameterError, match="number of weights"):
            backend.Predictor(p, sv, alpha[:, :-1], rho, every_form=True)
        with pytest.raises(InvalidParameterError, match="rho values"):
            backend.Predictor(p, sv, alpha, rho[:-1], every_form=True)
        with pytest.raises(InvalidParameterError, match="rho values"):
            backend.Predictor(p, sv, alpha, 0.125, every_form=True)
        with pytest.raises(InvalidParameterError, match="number of weights"):  # one weight vector
            backend.Predictor(p, sv, alpha[0, :-1], 0.125, every_form=True)
        with pytest.raises(InvalidParameterError, match="same number of features"):
            backend.Predictor(p, sv[0], alpha, rho, every_form=True)
