"""CPU: the two entry points of the factored linear-kernel operator (lssvm_mi355_problem_matvec_factored, _solve_lockstep_factored) are declared, bound, exported and
typed, and refuse invalid arguments before any device is touched; lockstep="factored" is a value of the backend object -- this file runs on a machine without a GPU."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from plssvm_amd import _capi
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.exceptions import BackendError, InvalidParameterError

NAMES = ["lssvm_mi355_problem_matvec_factored", "lssvm_mi355_problem_solve_lockstep_factored"]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_in_header_binding_and_library(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plssvm_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", header), "not declared in include/plssvm_amd.h"
    assert name in _capi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T " + name + r"$", out, flags=re.M), "not exported by the built library"
    entry = _capi.lockstep_entry(name)
    assert entry.restype is C.c_int and entry.argtypes[0] is C.c_void_p
    assert int(re.search(r"#define\s+LSSVM_FACTORED_SLAB_ROWS\s+(\d+)", header).group(1)) == _capi.FACTORED_SLAB_ROWS


def test_the_entry_points_refuse_invalid_arguments_without_a_device():
    matvec, solve = (_capi.lockstep_entry(name) for name in NAMES)
    Y, alphas, rhos = np.ones((2, 8), np.float32), np.zeros((2, 8), np.float32), np.zeros(2)
    y, a, rho = _capi.ptr(Y), _capi.ptr(alphas), rhos.ctypes.data_as(C.POINTER(C.c_double))
    fake = C.c_void_p(1)  # never dereferenced: every call below fails its argument checks first
    for args, message in (((None, y, 2, 1e-3, 10, a, rho), "problem handle must not be NULL"), ((fake, y, 0, 1e-3, 10, a, rho), "number of right hand sides must be greater than 0"),
                          ((fake, None, 2, 1e-3, 10, a, rho), "right hand side"), ((fake, y, 2, 0.0, 10, a, rho), "stopping criterion in the CG algorithm must be greater than 0.0"),
                          ((fake, y, 2, -1e-3, 10, a, rho), "stopping criterion in the CG algorithm must be greater than 0.0"),
                          ((fake, y, 2, 1e-3, 0, a, rho), "number of CG iterations must be greater than 0"), ((fake, y, 2, 1e-3, 10, None, rho), "must not be NULL"),
                          ((fake, y, 2, 1e-3, 10, a, None), "must not be NULL")):
        with pytest.raises(InvalidParameterError, match=message):
            _capi.check(solve(*args, None, None))
    for args, message in (((None, y, 2, a, 1.0), "problem handle must not be NULL"), ((fake, y, 0, a, 1.0), "number of vectors must be greater than 0"),
                          ((fake, None, 2, a, 1.0), "may not be empty"), ((fake, y, 2, None, 1.0), "may not be empty"), ((fake, y, 2, a, 0.5), "add must either be -1.0 or 1.0")):
        with pytest.raises(InvalidParameterError, match=message):
            _capi.check(matvec(*args, None))


def test_csvm_accepts_the_factored_lockstep_and_still_refuses_a_misspelt_one():
    try:
        assert MI355CSVM(lockstep="factored").lockstep == "factored"
    except BackendError:  # (no device here: the argument check, which comes first, has passed)
        pass
    with pytest.raises(InvalidParameterError, match="lockstep must be 'pair', 'block' or 'block32' or 'factored', but is 'factord'"):
        MI355CSVM(lockstep="factord")
