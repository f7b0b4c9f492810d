"""CPU: the two entry points of the lockstep CG (lssvm_mi355_problem_solve_lockstep, lssvm_mi355_problem_matvec_pair) are declared, bound and exported, and refuse
invalid arguments before any device is touched -- this file runs on a machine without a GPU."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from plssvm_amd import _capi
from plssvm_amd.exceptions import InvalidParameterError

NAMES = ["lssvm_mi355_problem_solve_lockstep", "lssvm_mi355_problem_matvec_pair"]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_in_header_binding_and_library(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plssvm_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", header), "not declared in include/plssvm_amd.h"
    assert name in _capi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T " + name + r"$", out, flags=re.M), "not exported by the built library"
    assert _capi.lockstep_entry(name).restype is C.c_int


def lockstep(handle, Y, k, eps, max_iter, alphas, rhos):
    rho_ptr = None if rhos is None else rhos.ctypes.data_as(C.POINTER(C.c_double))
    return _capi.lockstep_entry(NAMES[0])(handle, None if Y is None else _capi.ptr(Y), k, eps, max_iter, None if alphas is None else _capi.ptr(alphas), rho_ptr, None, None)


def test_solve_lockstep_refuses_invalid_arguments_without_a_device():
    Y, alphas, rhos = np.ones((2, 8)), np.zeros((2, 8)), np.zeros(2)
    fake = C.c_void_p(1)  # never dereferenced: every call below fails its argument checks first
    with pytest.raises(InvalidParameterError, match="problem handle must not be NULL"):
        _capi.check(lockstep(None, Y, 2, 1e-3, 10, alphas, rhos))
    with pytest.raises(InvalidParameterError, match="number of right hand sides must be greater than 0"):
        _capi.check(lockstep(fake, Y, 0, 1e-3, 10, alphas, rhos))
    with pytest.raises(InvalidParameterError, match="right hand side"):
        _capi.check(lockstep(fake, None, 2, 1e-3, 10, alphas, rhos))
    for eps in (0.0, -1e-3):
        with pytest.raises(InvalidParameterError, match="stopping criterion in the CG algorithm must be greater than 0.0"):
            _capi.check(lockstep(fake, Y, 2, eps, 10, alphas, rhos))
    with pytest.raises(InvalidParameterError, match="number of CG iterations must be greater than 0"):
        _capi.check(lockstep(fake, Y, 2, 1e-3, 0, alphas, rhos))
    with pytest.raises(InvalidParameterError, match="must not be NULL"):
        _capi.check(lockstep(fake, Y, 2, 1e-3, 10, None, rhos))
    with pytest.raises(InvalidParameterError, match="must not be NULL"):
        _capi.check(lockstep(fake, Y, 2, 1e-3, 10, alphas, None))


def test_matvec_pair_refuses_invalid_arguments_without_a_device():
    fn = _capi.lockstep_entry(NAMES[1])
    d, ret = np.ones(7), np.zeros(7)
    fake = C.c_void_p(1)
    with pytest.raises(InvalidParameterError, match="problem handle must not be NULL"):
        _capi.check(fn(None, _capi.ptr(d), _capi.ptr(d), _capi.ptr(ret), _capi.ptr(ret), 1.0, None))
    for args in ((None, _capi.ptr(d), _capi.ptr(ret), _capi.ptr(ret)), (_capi.ptr(d), None, _capi.ptr(ret), _capi.ptr(ret)), (_capi.ptr(d), _capi.ptr(d), None, _capi.ptr(ret)),
                 (_capi.ptr(d), _capi.ptr(d), _capi.ptr(ret), None)):
        with pytest.raises(InvalidParameterError, match="may not be empty"):
            _capi.check(fn(fake, *args, 1.0, None))
    with pytest.raises(InvalidParameterError, match="add must either be -1.0 or 1.0"):
        _capi.check(fn(fake, _capi.ptr(d), _capi.ptr(d), _capi.ptr(ret), _capi.ptr(ret), 0.5, None))
