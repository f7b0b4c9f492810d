"""CPU: the numpy model of the Nystrom preconditioner and of PCG on it (tests/pcg_model.py), the host side of the new entry points, and the proof
that every input of tests/test_gpu_pcg.py is solvable: the model, run in the input's dtype, meets the stop test and the true-residual bound the GPU test asserts."""

import ctypes as C
import functools
import os

import numpy as np
import pytest

import pcg_model as pm
from conftest import ROOT
from plssvm_amd import _capi, backend
from plssvm_amd.csvm import MI355CSVM, make_csvm
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter

# the issue's table: (CG at eps 1e-4, 1e-8), (PCG at eps 1e-4, 1e-8); None where it gives no figure; the 2000 x 128 row is its single eps = 1e-10 figure
ISSUE_TABLE = {
    "rbf_777x5": ((54, 155), (10, 23)),
    "poly_777x16": ((27, 84), (4, 13)),
    "rbf_1025x5": ((151, 460), (36, 75)),
    "linear_777x8": ((None, 11), (None, 1)),
    "rbf_777x300_flat": ((10, 32), (25, 43)),
}


@functools.lru_cache(maxsize=None)
def table_setup(name):
    p = pm.table_problem(name)
    A = pm.reduced_matrix(p["kernel"], p["X"], p["cost"], **p["kw"])
    b = pm.reduced_rhs(p["y"])
    pc = pm.Preconditioner(p["kernel"], p["X"], p["cost"], p["landmarks"], **p["kw"])
    A.setflags(write=False)
    b.setflags(write=False)
    return p, A, b, pc


def near(count, issue):
    """The issue's seeds are not recorded, so its counts are reproduced on this project's seeds (pcg_model.DATA_SEED / LANDMARK_SEED) to within a fifth, or 3 iterations."""
    return issue is None or abs(count - issue) <= max(3, 0.2 * issue)


@pytest.mark.parametrize("name", ["rbf_777x5", "poly_777x16", "linear_777x8"])
def test_P_is_the_congruence_of_the_nystrom_matrix_and_positive_definite(name):
    p, A, b, pc = table_setup(name)
    n = A.shape[0]
    # P = Bhat Bhat^T + sigma I equals E (Khat + sigma I) E^T built densely: the identity sigma E E^T = sigma (I + 1 1^T)
    P, Pb = pc.dense_f64(), pc.dense_from_bhat()
    assert np.linalg.norm(P - Pb) <= 1e-13 * np.linalg.norm(P)
    E = np.hstack([np.eye(n), -np.ones((n, 1))])
    Khat = pc.B_f @ pc.B_f.T
    assert np.linalg.norm(E @ (Khat + pc.sigma * np.eye(n + 1)) @ E.T - P) <= 1e-13 * np.linalg.norm(P)
    w = np.linalg.eigvalsh(0.5 * (P + P.T))
    # P - sigma I = Btilde Btilde^T + sigma 1 1^T is positive semi-definite: the smallest eigenvalue is sigma, up to the eigensolver's backward error eps |P|
    assert w[0] > 0.0 and w[0] >= pc.sigma - 64 * pm.EPS64 * w[-1]
    # the apply is P^-1 up to the factor sigma
    r = np.random.default_rng(3).standard_normal(n)
    assert pc.apply_residual(pc.apply(r), r) <= 1e-7


def test_exact_rank_linear_kernel_P_is_Abar_up_to_the_jitter():
    p, A, b, pc = table_setup("linear_777x8")  # 32 landmarks of a linear kernel on 8 features: Khat = K up to nu
    assert np.linalg.norm(pc.dense_f64() - A) <= 1e3 * pc.nu * 777 + 1e-10 * np.linalg.norm(A)
    assert pm.solve(A, b, 1e-8, 100, precond=pc)[1] <= 3


@pytest.mark.parametrize("name", sorted(ISSUE_TABLE))
def test_iteration_counts_of_the_issues_table(name):
    p, A, b, pc = table_setup(name)
    (cg4, cg8), (pcg4, pcg8) = ISSUE_TABLE[name]
    got = {}
    for eps, cg_issue, pcg_issue in ((1e-4, cg4, pcg4), (1e-8, cg8, pcg8)):
        x0, it_cg, ok0 = pm.solve(A, b, eps, 2000)
        x1, it_pcg, ok1 = pm.solve(A, b, eps, 2000, precond=pc)
        got[eps] = (it_cg, it_pcg)
        assert ok0 and ok1
        assert pm.true_residual(A, b, x1) <= 2 * eps
        assert near(it_cg, cg_issue) and near(it_pcg, pcg_issue), (name, eps, it_cg, cg_issue, it_pcg, pcg_issue)
    if name == "rbf_777x300_flat":
        assert all(pcg > cg for cg, pcg in got.values()), got  # the row where the preconditioner LOSES: flat spectrum, few landmarks
    else:
        assert all(2 * pcg <= cg for cg, pcg in got.values()), got


def test_iteration_counts_of_the_issues_2000_point_row():
    p, A, b, pc = table_setup("rbf_2000x128")
    it_cg = pm.solve(A, b, 1e-10, 2000)[1]
    it_pcg = pm.solve(A, b, 1e-10, 2000, precond=pc)[1]
    assert near(it_cg, 75) and near(it_pcg, 32), (it_cg, it_pcg)


@pytest.mark.parametrize("name", [c[0] for c in pm.GPU_CASES])
def test_every_gpu_input_is_solvable_in_its_dtype(name):
    """The precondition of tests/test_gpu_pcg.py: on each of its inputs the model in the input's dtype meets the stop test, and its solution the true-residual bound."""
    p = pm.gpu_case(name)
    A = pm.reduced_matrix(p["kernel"], p["X"], p["cost"], **p["kw"])
    b = pm.reduced_rhs(p["y"])
    pc = pm.Preconditioner(p["kernel"], p["X"], p["cost"], p["landmarks"], dtype=p["dtype"], **p["kw"])
    x, its, converged = pm.solve(A, b, p["eps"], 2000, dtype=p["dtype"], precond=pc)
    assert converged and its < 2000
    assert pm.true_residual(A, b, x) <= 2 * p["eps"]
    assert (p["X"].shape[0] - 1 in p["landmarks"]) == (name == "f64_rbf_last")


def test_model_refuses_bad_landmarks():
    X, _ = pm.make_data(20, 3, 1)
    for lm in ([], [1, 1], [20], list(range(20))):
        with pytest.raises(ValueError):
            pm.Preconditioner("rbf", X, 1.0, lm, gamma=0.5)


# ---------------------------------------------------------------- the host side of the entry points ----------------------------------------------------------------
NAMES = ["lssvm_mi355_problem_build_preconditioner", "lssvm_mi355_problem_precond_landmarks", "lssvm_mi355_problem_precond_apply", "lssvm_mi355_problem_solve_pcg",
         "lssvm_mi355_solve_pcg_f32", "lssvm_mi355_solve_pcg_f64"]


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "plssvm_amd.h")).read()
    for name in NAMES:
        assert name in _capi.EXPORTED_SYMBOLS and name + "(" in header and hasattr(_capi.lib, name)
    assert C.sizeof(_capi.LssvmPrecondInfo) == 40 and C.sizeof(_capi.LssvmPcgInfo) == 80
    capi = open(os.path.join(ROOT, "plssvm_amd", "csrc", "capi.hip")).read()
    assert "static_assert(sizeof(lssvm_precond_info) == 40 && sizeof(lssvm_pcg_info) == 80" in capi
    assert _capi.ABI_VERSION == 4 and len(_capi.OPTION_NAMES) == 16 and C.sizeof(_capi.LssvmCgInfo) == 168
    assert "lssvm_precond.hip" in open(os.path.join(ROOT, "plssvm_amd", "csrc", "Makefile")).read()


def test_bad_arguments_are_refused_before_a_device_is_touched():
    """(this box has no GPU: whatever reaches a device fails with another error)"""
    X = np.random.default_rng(0).uniform(-1, 1, (12, 3))
    y = np.where(np.arange(12) % 2 == 0, 1.0, -1.0)
    with pytest.raises(InvalidParameterError, match="stopping criterion"):
        backend.solve_pcg(Parameter(), X, y, 0.0, 10, rank=4)
    with pytest.raises(InvalidParameterError, match="stopping criterion"):
        backend.solve_pcg(Parameter(), X, y, float("nan"), 10, rank=4)
    with pytest.raises(InvalidParameterError, match="CG iterations"):
        backend.solve_pcg(Parameter(), X, y, 1e-3, 0, rank=4)
    with pytest.raises(InvalidParameterError, match="right hand side"):
        backend.solve_pcg(Parameter(), X, y[:5], 1e-3, 10, rank=4)
    with pytest.raises(InvalidParameterError, match="right hand side"):
        backend.solve_pcg(Parameter(), X, np.ones((0, 12)), 1e-3, 10, rank=4)
    with pytest.raises(InvalidParameterError, match="landmarks"):
        backend.solve_pcg(Parameter(), X, y, 1e-3, 10, landmarks=[])
    # the library's own checks, through the raw entry point: rank 0, rank > N - 1, rank > 512, NULL outputs
    ps = _capi.LssvmParams(0, 3, 1.0, 0.0, 1.0)
    fn = _capi.pcg_entry("lssvm_mi355_solve_pcg_f64")
    alphas, rhos, infos = np.zeros(12), np.zeros(1), (_capi.LssvmPcgInfo * 1)()
    rp = rhos.ctypes.data_as(C.POINTER(C.c_double))
    for rank in (0, 12, 513):
        with pytest.raises(InvalidParameterError, match="rank of the preconditioner"):
            _capi.check(fn(C.byref(ps), _capi.ptr(X), 12, 3, _capi.ptr(y), 1, rank, None, 1e-3, 10, _capi.ptr(alphas), rp, infos, None))
    for a, r, i in ((None, rp, infos), (_capi.ptr(alphas), None, infos), (_capi.ptr(alphas), rp, None)):
        with pytest.raises(InvalidParameterError, match="must not be NULL"):
            _capi.check(fn(C.byref(ps), _capi.ptr(X), 12, 3, _capi.ptr(y), 1, 4, None, 1e-3, 10, a, r, i, None))
    with pytest.raises(InvalidParameterError, match="right hand side"):
        _capi.check(fn(C.byref(ps), _capi.ptr(X), 12, 3, None, 1, 4, None, 1e-3, 10, _capi.ptr(alphas), rp, infos, None))
    with pytest.raises(InvalidParameterError, match="right hand sides"):
        _capi.check(fn(C.byref(ps), _capi.ptr(X), 12, 3, _capi.ptr(y), 0, 4, None, 1e-3, 10, _capi.ptr(alphas), rp, infos, None))
    # NULL handles
    for name, args in (("lssvm_mi355_problem_build_preconditioner", (None, 4, None, None)), ("lssvm_mi355_problem_precond_landmarks", (None, None)),
                       ("lssvm_mi355_problem_precond_apply", (None, None, None)), ("lssvm_mi355_problem_solve_pcg", (None, _capi.ptr(y), 1, 1e-3, 10, _capi.ptr(alphas), rp, infos))):
        with pytest.raises(InvalidParameterError, match="handle"):
            _capi.check(_capi.pcg_entry(name)(*args))


def test_csvm_solver_keyword():
    for bad in (0, 513, 2.5, None):
        with pytest.raises(InvalidParameterError, match="precond_rank"):
            MI355CSVM(solver="pcg", precond_rank=bad)
        with pytest.raises(InvalidParameterError, match="precond_rank"):
            make_csvm("mi355", solver="pcg", precond_rank=bad)
    with pytest.raises(InvalidParameterError, match="solver must be"):
        MI355CSVM(solver="nystrom")
