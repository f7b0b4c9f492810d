"""CPU: the entry point of the mixed-precision refinement (lssvm_mi355_solve_refined_f64) is declared, bound and exported, its report struct has the same layout in
header and binding, and it refuses invalid arguments before any device is touched -- this file runs on a machine without a GPU."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from plssvm_amd import _capi, backend
from plssvm_amd.csvm import MI355CSVM, make_csvm
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter

NAME = "lssvm_mi355_solve_refined_f64"
HEADER = os.path.join(ROOT, "include", "plssvm_amd.h")
C_TYPES = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double}


def test_symbol_in_header_binding_and_library():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", header), "not declared in include/plssvm_amd.h"
    assert NAME in _capi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T " + NAME + r"$", out, flags=re.M), "not exported by the built library"
    fn = _capi.refined_entry()
    assert fn.restype is C.c_int and len(fn.argtypes) == 15


def test_refine_info_layout_agrees_with_the_header():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct lssvm_refine_info \{(.*?)\} lssvm_refine_info;", header, flags=re.S).group(1)
    declared = []
    for statement in body.split(";"):
        words = statement.replace(",", " ").split()
        if words:
            declared += [(name, C_TYPES[words[0]]) for name in words[1:]]
    assert declared == list(_capi.LssvmRefineInfo._fields_)
    assert C.sizeof(_capi.LssvmRefineInfo) == 104  # (static_assert in capi.hip)
    assert C.sizeof(_capi.LssvmCgInfo) == 168 and _capi.lib.lssvm_mi355_abi_version() == 4  # only additions


def refined(params, X, Y, k, w, eps, max_iter, alphas, rhos, N=8, d=3):
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda a: None if a is None else _capi.ptr(a)
    return _capi.refined_entry()(None if params is None else C.byref(params), vp(X), N, d, vp(Y), k, dp(w), eps, max_iter, vp(alphas), dp(rhos), None, None, None, None)


def test_refuses_invalid_arguments_without_a_device():
    ps = _capi.LssvmParams(0, 3, 0.5, 0.0, 1.0)
    X, Y, alphas, rhos = np.ones((8, 3)), np.ones((2, 8)), np.zeros((2, 8)), np.zeros(2)
    with pytest.raises(InvalidParameterError, match="params must not be NULL"):
        _capi.check(refined(None, X, Y, 2, None, 1e-3, 10, alphas, rhos))
    with pytest.raises(InvalidParameterError, match="data must not be empty"):
        _capi.check(refined(ps, None, Y, 2, None, 1e-3, 10, alphas, rhos))
    with pytest.raises(InvalidParameterError, match="at least one feature"):
        _capi.check(refined(ps, X, Y, 2, None, 1e-3, 10, alphas, rhos, d=0))
    with pytest.raises(InvalidParameterError, match="number of right hand sides must be greater than 0"):
        _capi.check(refined(ps, X, Y, 0, None, 1e-3, 10, alphas, rhos))
    with pytest.raises(InvalidParameterError, match="right hand side"):
        _capi.check(refined(ps, X, None, 2, None, 1e-3, 10, alphas, rhos))
    for eps in (0.0, -1e-3):
        with pytest.raises(InvalidParameterError, match="stopping criterion in the CG algorithm must be greater than 0.0"):
            _capi.check(refined(ps, X, Y, 2, None, eps, 10, alphas, rhos))
    with pytest.raises(InvalidParameterError, match="number of CG iterations must be greater than 0"):
        _capi.check(refined(ps, X, Y, 2, None, 1e-3, 0, alphas, rhos))
    with pytest.raises(InvalidParameterError, match="must not be NULL"):
        _capi.check(refined(ps, X, Y, 2, None, 1e-3, 10, None, rhos))
    with pytest.raises(InvalidParameterError, match="must not be NULL"):
        _capi.check(refined(ps, X, Y, 2, None, 1e-3, 10, alphas, None))
    # the weights, as check_weights refuses them for the weighted solve
    for bad in (0.0, -1.0, np.nan, np.inf):
        w = np.ones(8)
        w[3] = bad
        with pytest.raises(InvalidParameterError, match="weight"):
            _capi.check(refined(ps, X, Y, 2, w, 1e-3, 10, alphas, rhos))
    with pytest.raises(InvalidParameterError, match="gamma"):
        _capi.check(refined(_capi.LssvmParams(2, 3, -1.0, 0.0, 1.0), X, Y, 2, None, 1e-3, 10, alphas, rhos))


def test_backend_solve_refined_checks_its_arguments_without_a_device():
    X, y = np.ones((8, 3)), np.ones(8)
    with pytest.raises(InvalidParameterError, match="float64"):
        backend.solve_refined(Parameter(), X.astype(np.float32), y, 1e-3, 10)
    with pytest.raises(InvalidParameterError, match="right hand side"):
        backend.solve_refined(Parameter(), X, y[:7], 1e-3, 10)
    with pytest.raises(InvalidParameterError, match="right hand side"):
        backend.solve_refined(Parameter(), X, np.ones((0, 8)), 1e-3, 10)
    with pytest.raises(InvalidParameterError, match="weights"):
        backend.solve_refined(Parameter(), X, y, 1e-3, 10, sample_weight=np.ones(7))
    with pytest.raises(InvalidParameterError, match="stopping criterion"):
        backend.solve_refined(Parameter(), X, y, 0.0, 10)
    with pytest.raises(InvalidParameterError, match="CG iterations"):
        backend.solve_refined(Parameter(), X, np.ones((2, 8)), 1e-3, 0)


def test_csvm_refuses_an_unknown_solver_before_it_looks_for_a_device():
    for word in ("refine", "", "CG", None):
        with pytest.raises(InvalidParameterError, match="solver must be 'cg' or 'refined'"):
            MI355CSVM(solver=word)
        with pytest.raises(InvalidParameterError, match="solver must be 'cg' or 'refined'"):
            make_csvm("mi355", solver=word)
