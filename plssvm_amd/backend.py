"""Thin Python mirror of the backend boundary over the C ABI (include/plssvm_amd.h).

Function names and argument meaning follow the reference's backend interface so that the parity tests read like the
reference's own (tests/backends/generic_csvm_tests.hpp):

    solve_system_of_linear_equations(params, A, b, eps, max_iter)   csvm.hpp:188-192
    predict_values(params, support_vectors, alpha, rho, w, points)  csvm.hpp:204-208
    predict_values_multi(params, support_vectors, alphas, rhos, ws, points)   the same for k weight vectors over one set of support vectors (one-vs-all)
    generate_q(params, data)                                        gpu_csvm.hpp:349-384 / OpenMP csvm.cpp:232-251
    run_device_kernel(params, q, ret, d, data, QA_cost, add)        gpu_csvm.hpp:431-447 / OpenMP csvm.cpp:283-306
    calculate_w(support_vectors, alpha)                             gpu_csvm.hpp:386-429 / OpenMP csvm.cpp:255-280

All arithmetic runs in the HIP library; numpy is only the host container.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import LssvmCgInfo, LssvmParams, LssvmPredictInfo, LssvmShard, Options, check, ctype_of, lib, options_ptr, ptr, suffix_of
from .exceptions import InvalidParameterError
from .parameter import Parameter

__all__ = ["Options", "Predictor", "solve_system_of_linear_equations", "solve_refined", "solve_cost_path", "solve_pcg", "fit_reduced", "fit_reduced_loo", "fit_reduced_grid", "ReducedStream", "fit_reduced_stream", "select_landmarks", "predict_values", "predict_values_multi", "generate_q", "run_device_kernel", "calculate_w", "ResidentProblem",
           "comm_get_unique_id", "comm_init", "comm_destroy"]


def _params_struct(params: Parameter, num_features: int) -> LssvmParams:
    p = params.resolved(num_features)
    return LssvmParams(int(p.kernel_type), int(p.degree), float(p.gamma), float(p.coef0), float(p.cost))


def _as_matrix(A, dtype=None) -> np.ndarray:
    A = np.asarray(A)
    if dtype is None:
        dtype = A.dtype if A.dtype in (np.float32, np.float64) else np.float64
    A = np.ascontiguousarray(A, dtype=dtype)
    if A.ndim != 2:
        raise InvalidParameterError("All data points must have the same number of features!")
    return A


def _as_weights(sample_weight, N: int) -> np.ndarray:
    """The per-point weights of a weighted solve as the library takes them: N doubles, each finite and > 0."""
    w = np.ascontiguousarray(sample_weight, dtype=np.float64)
    if w.shape != (N,):
        raise InvalidParameterError(f"The number of data points ({N}) and the number of weights ({w.size}) must be the same!")
    if not (np.all(np.isfinite(w)) and np.all(w > 0.0)):
        raise InvalidParameterError("Every weight of the solve must be finite and greater than 0.0!")
    return w


def solve_system_of_linear_equations(params: Parameter, A, b, eps: float, max_iter: int, devices=None, num_devices: int | None = None, options: Options | None = None,
                                     sample_weight=None):
    """Returns ``(alpha[N], rho, info)`` -- ``csvm::solve_system_of_linear_equations`` (csvm.hpp:188-192).

    ``devices`` (a list of HIP ordinals; the same ordinal may repeat) or ``num_devices`` (0 = every visible device) select the
    single-process multi-device solve ``lssvm_mi355_solve_multi_*``; with neither the solve runs on device 0.  ``options``: this call's own tuning knobs
    (:class:`Options`); None = the process defaults.  ``sample_weight``: N weights > 0 -- the WEIGHTED LS-SVM system (point i regularised by 1 / (C w_i),
    ``lssvm_mi355_solve_weighted_*``; on several devices a resident problem with ``lssvm_mi355_problem_set_weights``); None = the unweighted solve."""
    A = _as_matrix(A)
    N, d = A.shape
    b = np.ascontiguousarray(b, dtype=A.dtype)
    if b.shape != (N,):
        raise InvalidParameterError(f"The number of data points in the matrix A ({N}) and the values in the right hand side vector ({b.size}) must be the same!")
    if sample_weight is not None:
        return _solve_weighted(params, A, b, _as_weights(sample_weight, N), eps, max_iter, devices, num_devices, options)
    ct = ctype_of(A.dtype)
    alpha = np.zeros(N, dtype=A.dtype)
    rho = ct(0)
    info = LssvmCgInfo()
    ps = _params_struct(params, d)
    if devices is None and num_devices is None:
        fn = getattr(lib, f"lssvm_mi355_solve_{suffix_of(A.dtype)}")
        fn.restype = C.c_int
        check(fn(C.byref(ps), ptr(A), C.c_size_t(N), C.c_size_t(d), ptr(b), ct(eps), C.c_uint64(int(max_iter)), ptr(alpha), C.byref(rho), C.byref(info), options_ptr(options)))
    else:
        fn = getattr(lib, f"lssvm_mi355_solve_multi_{suffix_of(A.dtype)}")
        fn.restype = C.c_int
        dev_arr, ndev = _capi.int_array(devices)
        if devices is None:
            ndev = int(num_devices)
        check(fn(C.byref(ps), ptr(A), C.c_size_t(N), C.c_size_t(d), ptr(b), ct(eps), C.c_uint64(int(max_iter)), ptr(alpha), C.byref(rho), C.byref(info),
                 dev_arr, C.c_int(ndev), options_ptr(options)))
    return alpha, A.dtype.type(rho.value), info.as_dict()


def _solve_weighted(params: Parameter, A: np.ndarray, b: np.ndarray, w: np.ndarray, eps: float, max_iter: int, devices, num_devices, options):
    N, d = A.shape
    if devices is None and num_devices in (None, 1):  # device 0 alone (what lssvm_mi355_solve_* and _multi with one device run)
        ct = ctype_of(A.dtype)
        alpha = np.zeros(N, dtype=A.dtype)
        rho = ct(0)
        info = LssvmCgInfo()
        fn = _capi.weighted_entry(f"lssvm_mi355_solve_weighted_{suffix_of(A.dtype)}")
        check(fn(C.byref(_params_struct(params, d)), ptr(A), N, d, ptr(b), _capi.weights_ptr(w), eps, int(max_iter), ptr(alpha), C.byref(rho), C.byref(info),
                 options_ptr(options)))
        return alpha, A.dtype.type(rho.value), info.as_dict()
    # several devices: the recipe of the one-shot solve (capi.hip, solve_one_shot) over a resident problem of all of them
    if not max_iter > 0:
        raise InvalidParameterError("The number of CG iterations must be greater than 0!")
    devs = list(devices) if devices is not None else list(range(int(num_devices)))
    first = options.get("rebalance_after") if options is not None else _capi.get_option("rebalance_after")
    with ResidentProblem(params, A, devices=devs, options=options) as prob:
        prob.set_weights(w)
        prob.cg_begin(b, eps)
        if 0 < first < max_iter:
            prob.cg_step(first)
            prob.rebalance()
            prob.cg_step(max_iter - first)
        else:
            prob.cg_step(max_iter)
        alpha, rho, info = prob.cg_finish()
    info["max_iterations"] = int(max_iter)
    return alpha, rho, info


def solve_refined(params: Parameter, A, B, eps: float, max_iter: int, sample_weight=None, options: Options | None = None, passes_out: list | None = None):
    """The float64 system(s) solved to the float64 stop test by MIXED-PRECISION REFINEMENT (``lssvm_mi355_solve_refined_f64``): the CG iterations run in float32 on the
    matrix-core kernels, the float64 problem supplies the true residual once per outer step, and a step that does not halve it hands the solve to the plain float64 CG.
    ``B``: one right-hand side ``(N,)`` or ``k`` of them ``(k, N)``.  Returns ``(alphas, rhos, infos, refine_infos)`` -- ``alphas`` shaped like ``B``, ``rhos`` a scalar or
    ``(k,)``, one ``lssvm_cg_info`` and one ``lssvm_refine_info`` dict per right-hand side (a single dict each for a single right-hand side).  Column ``c`` of a call with
    several right-hand sides has the bits of the call with ``B[c]`` alone.  Device 0; ``A`` must be float64 (a float32 matrix has nothing to refine).  ``passes_out``: a list
    that receives the call's ``(two-vector, single-vector)`` float64 Gram passes."""
    A = _as_matrix(A)
    if A.dtype != np.float64:
        raise InvalidParameterError(f"solve_refined refines a float64 system; the data is {A.dtype} (solve_system_of_linear_equations solves it as it is)")
    N, d = A.shape
    B = np.ascontiguousarray(B, dtype=np.float64)
    single = B.ndim == 1
    B2 = B.reshape(1, -1) if single else B
    if B2.ndim != 2 or B2.shape[0] == 0 or B2.shape[1] != N:
        raise InvalidParameterError(f"The number of data points in the matrix A ({N}) and the values in every right hand side vector ({B2.shape[-1] if B2.ndim else 0}) must be the same!")
    k = B2.shape[0]
    w = None if sample_weight is None else _as_weights(sample_weight, N)
    alphas = np.zeros_like(B2)
    rhos = np.zeros(k, dtype=np.float64)
    infos = (LssvmCgInfo * k)()
    refine = (_capi.LssvmRefineInfo * k)()
    passes = (C.c_uint64 * 2)()
    check(_capi.refined_entry()(C.byref(_params_struct(params, d)), ptr(A), N, d, ptr(B2), k, _capi.weights_ptr(w), eps, int(max_iter), ptr(alphas),
                                rhos.ctypes.data_as(C.POINTER(C.c_double)), infos, refine, passes, options_ptr(options)))
    if passes_out is not None:
        passes_out[:] = [int(passes[0]), int(passes[1])]
    info_dicts, refine_dicts = [i.as_dict() for i in infos], [r.as_dict() for r in refine]
    if single:
        return alphas[0], np.float64(rhos[0]), info_dicts[0], refine_dicts[0]
    return alphas, rhos, info_dicts, refine_dicts


def _cost_path_arguments(y, N: int, dtype, costs, eps: float, max_iter: int):
    """The arguments of a cost path as the library takes them, checked as it checks them (so that a bad one never reaches a device): ``(y, costs)``."""
    y = np.ascontiguousarray(y, dtype=dtype)
    if y.shape != (N,):
        raise InvalidParameterError(f"The number of data points in the matrix A ({N}) and the values in the right hand side vector ({y.size}) must be the same!")
    costs = np.ascontiguousarray(costs, dtype=np.float64)
    if costs.ndim != 1 or costs.size == 0:
        raise InvalidParameterError("The number of costs must be greater than 0!")
    if costs.size > _capi.PATH_MAX_COSTS:
        raise InvalidParameterError(f"A cost path takes at most {_capi.PATH_MAX_COSTS} costs, but got {costs.size}!")
    if not (np.all(np.isfinite(costs)) and np.all(costs > 0.0)):
        raise InvalidParameterError("Every cost of the path must be finite and greater than 0.0!")
    if not (np.isfinite(eps) and eps > 0.0):
        raise InvalidParameterError(f"The stopping criterion in the CG algorithm must be greater than 0.0, but is {eps}!")
    if not int(max_iter) > 0:
        raise InvalidParameterError("The number of CG iterations must be greater than 0!")
    return y, costs


def _cost_path_call(fn, head, y, costs, N: int, dtype, eps: float, max_iter: int, verify: bool, tail=()):
    m = costs.size
    alphas = np.zeros((m, N), dtype=dtype)
    rhos = np.zeros(m, dtype=np.float64)
    infos = (_capi.LssvmPathInfo * m)()
    passes = (C.c_uint64 * 2)()
    check(fn(*head, ptr(y), costs.ctypes.data_as(C.POINTER(C.c_double)), m, float(eps), int(max_iter), 1 if verify else 0, ptr(alphas), rhos.ctypes.data_as(C.POINTER(C.c_double)),
             infos, passes, *tail))
    return alphas, rhos.astype(dtype), [i.as_dict() for i in infos], (int(passes[0]), int(passes[1]))


def solve_cost_path(params: Parameter, A, b, costs, eps: float, max_iter: int, verify: bool = True, options: Options | None = None):
    """ONE right-hand side solved for EVERY cost of ``costs`` by one multi-shift CG sequence (``lssvm_mi355_solve_cost_path_*``): one pass over the Gram tiles per
    iteration serves the whole grid.  ``params.cost`` is ignored.  Returns ``(alphas[m, N], rhos[m], infos, passes)``: row ``s`` belongs to ``costs[s]``, ``infos`` one
    ``lssvm_path_info`` dict per cost, ``passes = (Gram passes of the iteration, of the verification)``.  The stop test is the path's own -- the residual in the norm of
    M^-1 = (I + 1 1^T)^-1 relative to the right-hand side in that norm, from x0 = 0 -- not that of :func:`solve_system_of_linear_equations`; with ``verify`` the true
    residual of every cost is evaluated afterwards and reported (``true_residuum``, ``verified``).  Device 0; deterministic."""
    A = _as_matrix(A)
    N, d = A.shape
    y, costs = _cost_path_arguments(b, N, A.dtype, costs, eps, max_iter)
    ps = _params_struct(params, d)
    fn = _capi.cost_path_entry(f"lssvm_mi355_solve_cost_path_{suffix_of(A.dtype)}")
    return _cost_path_call(fn, (C.byref(ps), ptr(A), N, d), y, costs, N, A.dtype, eps, max_iter, verify, tail=(options_ptr(options),))


def _pcg_arguments(B, N: int, dtype, eps: float, max_iter: int):
    """The right-hand sides of a PCG solve as the library takes them (``k x N``), checked as it checks them: ``(B2, single)``."""
    B = np.ascontiguousarray(B, dtype=dtype)
    single = B.ndim == 1
    B2 = B.reshape(1, -1) if single else B
    if B2.ndim != 2 or B2.shape[0] == 0 or B2.shape[1] != N:
        raise InvalidParameterError(f"The number of data points in the matrix A ({N}) and the values in every right hand side vector ({B2.shape[-1] if B2.ndim else 0}) must be the same!")
    if not (np.isfinite(eps) and eps > 0.0):
        raise InvalidParameterError(f"The stopping criterion in the CG algorithm must be greater than 0.0, but is {eps}!")
    if not int(max_iter) > 0:
        raise InvalidParameterError("The number of CG iterations must be greater than 0!")
    return B2, single


def _landmarks_argument(rank: int, landmarks):
    """``(rank, array or None, pointer or NULL)`` of a preconditioner's landmarks: ``landmarks`` given -> its length is the rank."""
    if landmarks is None:
        return int(rank), None, None
    lm = np.ascontiguousarray(landmarks, dtype=np.uint64)
    if lm.ndim != 1 or lm.size == 0:
        raise InvalidParameterError("The landmarks must be a non-empty list of point indices!")
    return int(lm.size), lm, lm.ctypes.data_as(C.POINTER(C.c_uint64))


def _select_arguments(N: int, rank, method, pool, seed, tol):
    """The arguments of a landmark selection as the library takes them, checked as it checks them: ``(rank, method code, pool, seed, tol)``."""
    code = _capi.LANDMARK_METHODS.get(method) if isinstance(method, str) else None
    if code is None:
        raise InvalidParameterError(f"The landmark rule must be one of {sorted(_capi.LANDMARK_METHODS)}, but is {method!r}!")
    for name, value in (("rank", rank), ("pool", pool), ("seed", seed)):
        if not (isinstance(value, (int, np.integer)) and not isinstance(value, bool) and 0 <= int(value) < 2 ** 64):
            raise InvalidParameterError(f"{name} must be a non-negative integer, but is {value!r}!")
    rank, pool = int(rank), int(pool)
    if pool > N or 0 < pool < rank:
        raise InvalidParameterError(f"The candidate pool must be 0 (all {N} points) or lie in [rank, {N}], but is {pool} at rank {rank}!")
    most = min(pool if pool > 0 else N, _capi.SELECT_MAX_RANK)
    if not 1 <= rank <= most:
        raise InvalidParameterError(f"The number of landmarks to select must lie in [1, {most}], but is {rank}!")
    try:
        tol = float(tol)
    except (TypeError, ValueError):
        raise InvalidParameterError(f"The tolerance of the landmark selection must be a number, but is {tol!r}!") from None
    if not (np.isfinite(tol) and tol >= 0.0):
        raise InvalidParameterError(f"The tolerance of the landmark selection must be finite and not negative, but is {tol}!")
    return rank, code, pool, int(seed), tol


def _select_call(fn, head, N: int, rank: int, code: int, pool: int, seed: int, tol: float, tail=()):
    lm = np.zeros(rank, dtype=np.uint64)
    trace, residual = np.zeros(rank), np.zeros(N)
    info = _capi.LssvmLandmarkSelectInfo()
    dp = C.POINTER(C.c_double)
    check(fn(*head, rank, code, pool, seed, tol, lm.ctypes.data_as(C.POINTER(C.c_uint64)), trace.ctypes.data_as(dp), residual.ctypes.data_as(dp), C.byref(info), *tail))
    return lm[:int(info.rank_found)].copy(), trace, residual, info.as_dict()


def select_landmarks(params: Parameter, A, rank: int, method: str = "rpcholesky", pool: int = 0, seed: int = 0, tol: float = 0.0, options: Options | None = None):
    """``rank`` landmarks chosen from the data by a pivoted partial Cholesky factorisation of the kernel matrix (``lssvm_mi355_select_landmarks_*``; opt-in, DESIGN.md
    section 14).  ``method``: ``"greedy"`` (the largest residual diagonal entry) or ``"rpcholesky"`` (at random in proportion to the residual diagonal, from ``seed``);
    neither dominates the other or the fixed rule.  ``pool``: 0 = every point is a candidate, else the first ``pool`` points of the library's fixed shuffle (it bounds the
    work space, ``rank x pool`` doubles).  ``tol``: stop once the pivot's residual falls to ``max(tol, 64 eps64)`` times the largest diagonal entry.  Returns
    ``(landmarks[:rank_found], trace[rank], residual[N], info)``: the indices for the ``landmarks`` argument of :func:`solve_pcg` / :func:`fit_reduced`, the trace of the
    Nystrom residual after every step, the final residual diagonal (NaN outside the pool) and the ``lssvm_landmark_select_info`` dict.  Device 0; deterministic."""
    A = _as_matrix(A)
    N, d = A.shape
    rank, code, pool, seed, tol = _select_arguments(N, rank, method, pool, seed, tol)
    ps = _params_struct(params, d)
    fn = _capi.select_entry(f"lssvm_mi355_select_landmarks_{suffix_of(A.dtype)}")
    return _select_call(fn, (C.byref(ps), ptr(A), N, d), N, rank, code, pool, seed, tol, tail=(options_ptr(options),))


def _pcg_call(fn, head, middle, B2, single: bool, N: int, dtype, eps: float, max_iter: int, tail=()):
    k = B2.shape[0]
    alphas = np.zeros((k, N), dtype=dtype)
    rhos = np.zeros(k, dtype=np.float64)
    infos = (_capi.LssvmPcgInfo * k)()
    check(fn(*head, ptr(B2), k, *middle, float(eps), int(max_iter), ptr(alphas), rhos.ctypes.data_as(C.POINTER(C.c_double)), infos, *tail))
    dicts = [i.as_dict() for i in infos]
    if single:
        return alphas[0], np.dtype(dtype).type(rhos[0]), dicts[0]
    return alphas, rhos.astype(dtype), dicts


def solve_pcg(params: Parameter, A, B, eps: float, max_iter: int, rank: int = 256, landmarks=None, options: Options | None = None):
    """The system(s) solved by CG preconditioned with a Nystrom approximation of ``rank`` landmarks (``lssvm_mi355_solve_pcg_*``; opt-in: it pays where the kernel matrix
    has spectral decay and costs iterations where it has none).  ``B``: one right-hand side ``(N,)`` or ``k`` of them ``(k, N)``, solved one after the other on ONE
    preconditioner.  ``landmarks``: distinct point indices (their number is the rank), None for the library's fixed choice, or ``"greedy"`` / ``"rpcholesky"`` for
    ``rank`` points chosen by :func:`select_landmarks` (fewer where the kernel matrix's rank is exhausted first).  The stop test is that of
    :func:`solve_system_of_linear_equations`.  Returns ``(alphas, rhos, infos)`` shaped like ``B`` (``infos``: ``lssvm_pcg_info`` dicts).  Device 0; deterministic."""
    A = _as_matrix(A)
    N, d = A.shape
    B2, single = _pcg_arguments(B, N, A.dtype, eps, max_iter)
    if isinstance(landmarks, str):  # a selection rule: one resident problem selects, builds and solves (the data is uploaded once)
        with ResidentProblem(params, A, options=options) as prob:
            prob.build_preconditioner(rank, landmarks)
            return prob.solve_pcg(B, eps, max_iter)
    rank, lm, lm_ptr = _landmarks_argument(rank, landmarks)
    ps = _params_struct(params, d)
    fn = _capi.pcg_entry(f"lssvm_mi355_solve_pcg_{suffix_of(A.dtype)}")
    return _pcg_call(fn, (C.byref(ps), ptr(A), N, d), (rank, lm_ptr), B2, single, N, A.dtype, eps, max_iter, tail=(options_ptr(options),))


def _reduced_arguments(Y, N: int, dtype, rank, landmarks, slab_rows):
    """The arguments of a fixed-size fit as the library takes them, checked as it checks them: ``(Y2, single, rank, landmarks array or None, pointer or NULL, slab_rows)``."""
    Y = np.ascontiguousarray(Y, dtype=dtype)
    single = Y.ndim == 1
    Y2 = Y.reshape(1, -1) if single else Y
    if Y2.ndim != 2 or Y2.shape[0] == 0 or Y2.shape[1] != N:
        raise InvalidParameterError(f"The number of data points in the matrix A ({N}) and the values in every right hand side vector ({Y2.shape[-1] if Y2.ndim else 0}) must be the same!")
    if landmarks is None and not isinstance(rank, (int, np.integer)):
        raise InvalidParameterError(f"The rank of the reduced model must be an integer, but is {rank!r}!")
    rank, lm, lm_ptr = _landmarks_argument(rank, landmarks)
    most = min(N, _capi.REDUCED_MAX_RANK)
    if not 1 <= rank <= most:
        raise InvalidParameterError(f"The rank of the reduced model must lie in [1, {most}], but is {rank}!")
    if not (isinstance(slab_rows, (int, np.integer)) and slab_rows >= 0 and slab_rows % 256 == 0):
        raise InvalidParameterError(f"slab_rows must be a multiple of 256 (0: the library's default), but is {slab_rows!r}!")
    return Y2, single, rank, lm, lm_ptr, int(slab_rows)


def _reduced_weights(sample_weight, N: int):
    """The per-point weights of a weighted fixed-size fit as the library takes them, checked as it checks them: N doubles, each finite and >= 0, their sum > 0 -- or
    None.  (Exact zeros are allowed here, unlike in the full solve: such a point takes no part in the fit.)"""
    if sample_weight is None:
        return None
    try:
        w = np.ascontiguousarray(sample_weight, dtype=np.float64)
    except (TypeError, ValueError):
        raise InvalidParameterError("The weights must be a list of numbers!") from None
    if w.shape != (N,):
        raise InvalidParameterError(f"The number of data points ({N}) and the number of weights ({w.size}) must be the same!")
    if not (np.all(np.isfinite(w)) and np.all(w >= 0.0)):
        raise InvalidParameterError("Every weight of the reduced model must be finite and not less than 0.0!")
    with np.errstate(over="ignore"):
        total = float(w.sum())
    if not (np.isfinite(total) and total > 0.0):
        raise InvalidParameterError(f"The weights of the reduced model must have a finite sum greater than 0.0, but it is {total}!")
    return w


def _reduced_entry(name: str, on_device: bool, suffix: str = "", weighted: bool = False):
    """``lssvm_mi355_<name><suffix>`` or, for ``factor="device"``, its ``_dev`` form; with weights the ``_weighted`` form, which takes the factor as an argument."""
    if weighted:
        return _capi.reduced_weighted_entry(f"lssvm_mi355_{name}_weighted{suffix}")
    entry = _capi.reduced_loo_entry if "loo" in name else _capi.reduced_entry
    return entry(f"lssvm_mi355_{name}{'_dev' if on_device else ''}{suffix}")


def _reduced_call(fn, head, Y2, single: bool, rank: int, lm_ptr, slab_rows: int, tail=(), on_device: bool = False, weights=None):
    k = Y2.shape[0]
    betas = np.zeros((k, rank), dtype=np.float64)
    rhos = np.zeros(k, dtype=np.float64)
    used = np.zeros(rank, dtype=np.uint64)
    info = _capi.LssvmReducedInfo()
    dp = C.POINTER(C.c_double)
    dense = _capi.LssvmDenseInfo()
    if weights is not None:  # (``fn`` is the weighted entry point)
        check(fn(*head, ptr(Y2), k, weights.ctypes.data_as(dp), rank, lm_ptr, slab_rows, int(on_device), betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp),
                 used.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info), C.byref(dense), *tail))
    else:
        if on_device:
            tail = tuple(tail) + (C.byref(dense),)
        check(fn(*head, ptr(Y2), k, rank, lm_ptr, slab_rows, betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp), used.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info), *tail))
    report = dict(dense.as_dict(), **info.as_dict()) if on_device else info.as_dict()  # (rank and jitter are the same in both records)
    if single:
        return betas[0], float(rhos[0]), used, report
    return betas, rhos, used, report


def fit_reduced(params: Parameter, A, Y, rank: int, landmarks=None, slab_rows: int = 0, options: Options | None = None, factor: str = "host", sample_weight=None):
    """The fixed-size (reduced) LS-SVM over ``rank`` landmark points (``lssvm_mi355_fit_reduced_*``; opt-in: it trades accuracy for a model of ``rank`` support vectors):
    ``f(x) = sum_j beta_j k(x, x_L[j]) - rho`` minimises ``1/2 beta^T K_mm beta + C/2 sum_i (y_i - f(x_i))^2``.  ``Y``: one right-hand side ``(N,)`` or ``k`` of them
    ``(k, N)`` -- one landmark block, one Gram matrix and one factorisation serve all.  ``landmarks``: distinct point indices (their number is the rank), None for the
    preconditioner's fixed rule, or ``"greedy"`` / ``"rpcholesky"`` for ``rank`` points chosen by :func:`select_landmarks`.  ``slab_rows``: rows of the landmark block held at a time (a multiple of 256; 0: 65 536).  Returns ``(betas, rhos, landmarks, info)``,
    ``betas`` and ``rhos`` float64 whatever the data's type and shaped like ``Y``; ``info``: the ``lssvm_reduced_info`` dict.  Device 0; deterministic; no CG.
    ``factor="device"`` (opt-in; ``lssvm_mi355_fit_reduced_dev_*``): assembly, factorisation and solves run on the device instead of one host
    thread -- not the host path's bits -- and ``info`` gains the ``lssvm_dense_info`` fields (``block``, ``attempts``, ``launches``, ``assemble_ms`` ...).
    ``sample_weight`` (``lssvm_mi355_fit_reduced_weighted_*``): ``N`` weights ``w_i >= 0`` with a positive sum for the objective
    ``1/2 beta^T K_mm beta + C/2 sum_i w_i (y_i - f(x_i))^2``; a point of weight 0 takes no part in the fit.  None: the unweighted entry point, as before.  The landmark
    rules ignore the weights."""
    on_device = _capi.factor_on_device(factor)
    A = _as_matrix(A)
    N, d = A.shape
    w = _reduced_weights(sample_weight, N)
    if isinstance(landmarks, str):  # a selection rule (:func:`select_landmarks`): one resident problem selects and fits
        with ResidentProblem(params, A, options=options) as prob:
            return prob.fit_reduced(Y, rank, landmarks, slab_rows, factor=factor, sample_weight=w)
    Y2, single, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, N, A.dtype, rank, landmarks, slab_rows)
    ps = _params_struct(params, d)
    fn = _reduced_entry("fit_reduced", on_device, f"_{suffix_of(A.dtype)}", weighted=w is not None)
    return _reduced_call(fn, (C.byref(ps), ptr(A), N, d), Y2, single, rank, lm_ptr, slab_rows, tail=(options_ptr(options),), on_device=on_device, weights=w)


def _reduced_logistic_arguments(Y2, rank: int, tol, max_iter, start):
    """What the logistic fit adds to the arguments of a weighted fit, checked as the library checks it: labels of exactly -1 or +1, ``tol`` finite and > 0,
    ``max_iter`` >= 1 and the start values ``(betas0, rhos0)`` -- shaped like the result, all finite -- or None.  Returns ``(tol, max_iter, betas0, rhos0)``."""
    if not np.all(np.abs(Y2) == 1):
        raise InvalidParameterError("Every label of the logistic model must be exactly -1 or +1!")
    if not (isinstance(tol, (int, float, np.floating)) and np.isfinite(tol) and tol > 0):
        raise InvalidParameterError(f"tol must be finite and greater than 0, but is {tol!r}!")
    if not (isinstance(max_iter, (int, np.integer)) and max_iter >= 1):
        raise InvalidParameterError(f"max_iter must be an integer greater than 0, but is {max_iter!r}!")
    if start is None:
        return float(tol), int(max_iter), None, None
    try:
        betas0, rhos0 = start
        betas0 = np.ascontiguousarray(betas0, dtype=np.float64).reshape(Y2.shape[0], -1)
        rhos0 = np.ascontiguousarray(rhos0, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise InvalidParameterError("start must be a pair (betas0, rhos0) of numbers shaped like the result!") from None
    if betas0.shape != (Y2.shape[0], rank) or rhos0.shape != (Y2.shape[0],):
        raise InvalidParameterError(f"start must hold {Y2.shape[0]} x {rank} betas and {Y2.shape[0]} rhos, but their shapes are {betas0.shape} and {rhos0.shape}!")
    if not (np.all(np.isfinite(betas0)) and np.all(np.isfinite(rhos0))):
        raise InvalidParameterError("Every start value must be finite!")
    return float(tol), int(max_iter), betas0, rhos0


def _reduced_logistic_call(fn, head, Y2, single: bool, rank: int, lm_ptr, slab_rows: int, weights, on_device: bool, tol: float, max_iter: int, betas0, rhos0, tail=()):
    k = Y2.shape[0]
    betas = np.zeros((k, rank), dtype=np.float64)
    rhos = np.zeros(k, dtype=np.float64)
    used = np.zeros(rank, dtype=np.uint64)
    infos = (_capi.LssvmReducedLogisticInfo * k)()
    dp = C.POINTER(C.c_double)
    check(fn(*head, ptr(Y2), k, _capi.weights_ptr(weights), rank, lm_ptr, slab_rows, int(on_device), tol, max_iter, _capi.weights_ptr(betas0), _capi.weights_ptr(rhos0),
             betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp), used.ctypes.data_as(C.POINTER(C.c_uint64)), infos, *tail))
    reports = [info.as_dict() for info in infos]
    if single:
        return betas[0], float(rhos[0]), used, reports[0]
    return betas, rhos, used, reports


def fit_reduced_logistic(params: Parameter, A, Y, rank: int, landmarks=None, sample_weight=None, tol: float = 1e-8, max_iter: int = 50, factor: str = "host", start=None,
                         slab_rows: int = 0, options: Options | None = None):
    """The fixed-size kernel logistic regression over ``rank`` landmark points (``lssvm_mi355_fit_reduced_logistic_*``): with labels ``y_i`` of
    exactly -1 or +1 the model ``eta(x) = sum_j beta_j k(x, x_L[j]) - rho`` minimises ``1/2 beta^T K_mm beta + C sum_i a_i log(1 + exp(-y_i eta(x_i)))`` by Newton's
    method, every step a weighted fixed-size fit; ``eta`` is the log-odds of ``y = +1``.  ``Y``: one label vector ``(N,)`` or ``k`` of them ``(k, N)`` (one-vs-all),
    which run in lockstep and share every evaluation of the landmark block.  ``sample_weight``: the prior weights ``a_i`` as :func:`fit_reduced` takes them.
    ``tol``: the relative decrease of the objective at which a class stops; ``max_iter``: passes over the data, rejected steps included; ``start``: ``(betas0, rhos0)``
    shaped like the result, or None for zeros.  ``landmarks``, ``factor``, ``slab_rows``: as in :func:`fit_reduced`.  Returns ``(betas, rhos, landmarks, info)``; ``info``:
    the ``lssvm_reduced_logistic_info`` dict of the class, or a list of them for ``k`` label vectors.  Device 0; deterministic."""
    on_device = _capi.factor_on_device(factor)
    A = _as_matrix(A)
    N, d = A.shape
    w = _reduced_weights(sample_weight, N)
    if isinstance(landmarks, str):  # a selection rule (:func:`select_landmarks`): one resident problem selects and fits
        with ResidentProblem(params, A, options=options) as prob:
            return prob.fit_reduced_logistic(Y, rank, landmarks, w, tol, max_iter, factor, start, slab_rows)
    Y2, single, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, N, A.dtype, rank, landmarks, slab_rows)
    tol, max_iter, betas0, rhos0 = _reduced_logistic_arguments(Y2, rank, tol, max_iter, start)
    ps = _params_struct(params, d)
    fn = _capi.reduced_logistic_entry(f"lssvm_mi355_fit_reduced_logistic_{suffix_of(A.dtype)}")
    return _reduced_logistic_call(fn, (C.byref(ps), ptr(A), N, d), Y2, single, rank, lm_ptr, slab_rows, w, on_device, tol, max_iter, betas0, rhos0, tail=(options_ptr(options),))


def _reduced_loo_costs(costs):
    """The cost grid of the leave-one-out scores, checked as the library checks it."""
    try:
        costs = np.ascontiguousarray(costs, dtype=np.float64)
    except (TypeError, ValueError):
        raise InvalidParameterError("The costs must be a list of numbers!") from None
    if costs.ndim != 1 or not 1 <= costs.size <= _capi.REDUCED_LOO_MAX_COSTS:
        raise InvalidParameterError(f"The leave-one-out scores take between 1 and {_capi.REDUCED_LOO_MAX_COSTS} costs, but got {costs.size if costs.ndim == 1 else costs.shape}!")
    if not (np.all(np.isfinite(costs)) and np.all(costs > 0.0)):
        raise InvalidParameterError("Every cost must be finite and greater than 0!")
    return costs


def _reduced_loo_call(fn, head, Y2, single: bool, N: int, rank: int, lm_ptr, slab_rows: int, costs, tail=(), on_device: bool = False, weights=None):
    k, S = Y2.shape[0], costs.size
    betas, rhos = np.zeros((S, k, rank)), np.zeros((S, k))
    leverage, fitted, loo = np.zeros((S, N)), np.zeros((S, k, N)), np.zeros((S, k, N))
    press, errors, used = np.zeros((S, k)), np.zeros((S, k), dtype=np.uint64), np.zeros(rank, dtype=np.uint64)
    infos = (_capi.LssvmReducedLooInfo * S)()
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    dense = (_capi.LssvmDenseInfo * S)()
    outs = (betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp), leverage.ctypes.data_as(dp), fitted.ctypes.data_as(dp), loo.ctypes.data_as(dp), press.ctypes.data_as(dp),
            errors.ctypes.data_as(up), used.ctypes.data_as(up), infos)
    if weights is not None:  # (``fn`` is the weighted entry point)
        check(fn(*head, ptr(Y2), k, weights.ctypes.data_as(dp), rank, lm_ptr, slab_rows, costs.ctypes.data_as(dp), S, int(on_device), *outs, dense, *tail))
    else:
        if on_device:
            tail = tuple(tail) + (dense,)
        check(fn(*head, ptr(Y2), k, rank, lm_ptr, slab_rows, costs.ctypes.data_as(dp), S, *outs, *tail))
    report = {"costs": costs.copy(), "leverage": leverage, "fitted": fitted[:, 0] if single else fitted, "loo": loo[:, 0] if single else loo,
              "press": press[:, 0] if single else press, "loo_errors": errors[:, 0] if single else errors, "max_leverage": np.array([i.max_leverage for i in infos]),
              "jitter": np.array([i.jitter for i in infos]),
              "infos": [dict(dn.as_dict(), **i.as_dict()) if on_device else i.as_dict() for i, dn in zip(infos, dense)]}
    return (betas[:, 0], rhos[:, 0], used, report) if single else (betas, rhos, used, report)


def fit_reduced_loo(params: Parameter, A, Y, rank: int, costs, landmarks=None, slab_rows: int = 0, options: Options | None = None, factor: str = "host",
                    sample_weight=None):
    """:func:`fit_reduced` at every cost of ``costs`` with its exact leave-one-out values -- leave-one-out with the landmark set held fixed
    (``lssvm_mi355_fit_reduced_loo_*``).  The fit is a linear smoother, so the model refitted without point ``i`` predicts
    ``y_i - (y_i - f(x_i)) / (1 - h_ii)`` at ``x_i``: one more pass over the landmark block per cost gives the leverages ``h`` and these values for ALL ``N`` points, without
    a validation split and without a refit.  ``params.cost`` is ignored; 1 to 64 costs.  Returns ``(betas[S, k, rank], rhos[S, k], landmarks, report)`` (the ``k`` axis
    dropped for a single right-hand side ``(N,)``); ``betas[s]`` / ``rhos[s]`` have the bits of :func:`fit_reduced` at ``costs[s]``.  ``report``: ``leverage[S, N]``,
    ``fitted`` / ``loo`` ``[S, k, N]``, ``press[S, k]`` (sum of squared leave-one-out residuals), ``loo_errors[S, k]`` (points whose leave-one-out value has another sign than
    ``y``), ``max_leverage[S]``, ``jitter[S]``, ``infos`` (``lssvm_reduced_loo_info`` dicts).  Everything float64.  Device 0; deterministic.
    ``factor="device"`` (opt-in; ``lssvm_mi355_fit_reduced_loo_dev_*``): per cost the assembly, the factorisation, the solves and the triangular
    inverse run on the device and the leverage kernel's operand never leaves it -- not the host path's bits; ``betas[s]`` / ``rhos[s]`` then have the bits of
    :func:`fit_reduced` with ``factor="device"`` at ``costs[s]``, and every dict of ``infos`` gains the ``lssvm_dense_info`` fields.
    ``sample_weight`` (``lssvm_mi355_fit_reduced_loo_weighted_*``): the weights of :func:`fit_reduced`; then ``h_ii = w_i (1 / W + ...)``,
    ``press`` is ``sum_i w_i (y_i - loo_i)^2`` and ``loo_errors`` counts over the points with ``w_i > 0``.  A point of weight 0 has leverage 0 and its ``loo`` value is
    the prediction of a model that never saw it: one call scores a validation mask."""
    on_device = _capi.factor_on_device(factor)
    A = _as_matrix(A)
    N, d = A.shape
    w = _reduced_weights(sample_weight, N)
    if isinstance(landmarks, str):  # a selection rule (:func:`select_landmarks`): one resident problem selects and fits
        with ResidentProblem(params, A, options=options) as prob:
            return prob.fit_reduced_loo(Y, rank, costs, landmarks, slab_rows, factor=factor, sample_weight=w)
    Y2, single, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, N, A.dtype, rank, landmarks, slab_rows)
    costs = _reduced_loo_costs(costs)
    ps = _params_struct(params, d)
    fn = _reduced_entry("fit_reduced_loo", on_device, f"_{suffix_of(A.dtype)}", weighted=w is not None)
    return _reduced_loo_call(fn, (C.byref(ps), ptr(A), N, d), Y2, single, N, rank, lm_ptr, slab_rows, costs, tail=(options_ptr(options),), on_device=on_device, weights=w)


def _reduced_grid_gammas(gammas, num_costs: int):
    """The gammas of the (gamma, cost) grid, checked as the library checks them."""
    try:
        gammas = np.ascontiguousarray(gammas, dtype=np.float64)
    except (TypeError, ValueError):
        raise InvalidParameterError("The gammas must be a list of numbers!") from None
    if gammas.ndim != 1 or gammas.size < 1:
        raise InvalidParameterError(f"The grid takes at least 1 gamma, but got {gammas.size if gammas.ndim == 1 else gammas.shape}!")
    if not (np.all(np.isfinite(gammas)) and np.all(gammas > 0.0)):
        raise InvalidParameterError("Every gamma must be finite and greater than 0!")
    if gammas.size * num_costs > _capi.REDUCED_GRID_MAX_CELLS:
        raise InvalidParameterError(f"The grid takes at most {_capi.REDUCED_GRID_MAX_CELLS} (gamma, cost) cells, but got {gammas.size} x {num_costs}!")
    return gammas


def _reduced_grid_kernel(params: Parameter):
    """The grid's refusal of a kernel function without a gamma, as the library words it."""
    if int(params.kernel_type) == 0:
        raise InvalidParameterError("The linear kernel has no gamma to vary: the (gamma, cost) grid takes an rbf or a polynomial problem!")


def _reduced_grid_call(fn, head, Y2, single: bool, N: int, rank: int, lm_ptr, slab_rows: int, gammas, costs, on_device: bool, product: int, weights, tail=()):
    k, G, S = Y2.shape[0], gammas.size, costs.size
    betas, rhos = np.zeros((G, S, k, rank)), np.zeros((G, S, k))
    leverage, fitted, loo = np.zeros((G, S, N)), np.zeros((G, S, k, N)), np.zeros((G, S, k, N))
    press, errors, used = np.zeros((G, S, k)), np.zeros((G, S, k), dtype=np.uint64), np.zeros(rank, dtype=np.uint64)
    infos = (_capi.LssvmReducedGridInfo * (G * S))()
    dense = (_capi.LssvmDenseInfo * (G * S))()
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    check(fn(*head, ptr(Y2), k, _capi.weights_ptr(weights), rank, lm_ptr, slab_rows, gammas.ctypes.data_as(dp), G, costs.ctypes.data_as(dp), S, int(on_device), product,
             betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp), leverage.ctypes.data_as(dp), fitted.ctypes.data_as(dp), loo.ctypes.data_as(dp), press.ctypes.data_as(dp),
             errors.ctypes.data_as(up), used.ctypes.data_as(up), infos, dense, *tail))
    cells = [[dict(dense[g * S + s].as_dict(), **infos[g * S + s].as_dict()) if on_device else infos[g * S + s].as_dict() for s in range(S)] for g in range(G)]
    report = {"gammas": gammas.copy(), "costs": costs.copy(), "leverage": leverage, "fitted": fitted[:, :, 0] if single else fitted, "loo": loo[:, :, 0] if single else loo,
              "press": press[:, :, 0] if single else press, "loo_errors": errors[:, :, 0] if single else errors,
              "max_leverage": np.array([[c["max_leverage"] for c in row] for row in cells]), "jitter": np.array([[c["jitter"] for c in row] for row in cells]), "infos": cells}
    return (betas[:, :, 0], rhos[:, :, 0], used, report) if single else (betas, rhos, used, report)


def fit_reduced_grid(params: Parameter, A, Y, rank: int, gammas, costs, landmarks=None, slab_rows: int = 0, options: Options | None = None, factor: str = "host",
                     sample_weight=None, product: str = "matrix"):
    """:func:`fit_reduced_loo` at every kernel width of ``gammas`` AND every cost of ``costs`` in one call on one resident problem (``lssvm_mi355_fit_reduced_grid_*``;
    DESIGN.md section 17), for rbf and polynomial kernels.  The sums over the features behind every kernel value do not depend on gamma: they are formed once per slab
    and pass and shared by all gammas.  ``params.cost`` and ``params.gamma`` are ignored by the fit, but ``params.gamma`` still decides how the problem holds its data:
    pass a gamma from the grid.  ``gammas.size * costs.size <= 64``.  ``product="matrix"`` (the default) forms the dot products on the fp64 matrix cores (rbf: through the
    norm expansion ``n_i + n_l - 2 x_i . x_l``); ``product="ordered"`` runs the loop of :func:`fit_reduced_loo` -- with the one gamma of ``params`` it returns that
    call's bits.  Returns ``(betas[G, S, k, rank], rhos[G, S, k], landmarks, report)`` (the ``k`` axis dropped for a single right-hand side); ``report`` as for
    :func:`fit_reduced_loo` with a leading gamma axis on every array, ``gammas``, and ``infos[g][s]`` (``lssvm_reduced_grid_info`` dicts).  ``factor`` and
    ``sample_weight``: as for :func:`fit_reduced_loo`."""
    on_device = _capi.factor_on_device(factor)
    code = _capi.product_argument(product)
    A = _as_matrix(A)
    N, d = A.shape
    w = _reduced_weights(sample_weight, N)
    if isinstance(landmarks, str):  # a selection rule (:func:`select_landmarks`): one resident problem selects and fits
        with ResidentProblem(params, A, options=options) as prob:
            return prob.fit_reduced_grid(Y, rank, gammas, costs, landmarks, sample_weight=w, factor=factor, product=product, slab_rows=slab_rows)
    Y2, single, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, N, A.dtype, rank, landmarks, slab_rows)
    costs = _reduced_loo_costs(costs)
    gammas = _reduced_grid_gammas(gammas, costs.size)
    _reduced_grid_kernel(params)
    ps = _params_struct(params, d)
    fn = _capi.reduced_grid_entry(f"lssvm_mi355_fit_reduced_grid_{suffix_of(A.dtype)}")
    return _reduced_grid_call(fn, (C.byref(ps), ptr(A), N, d), Y2, single, N, rank, lm_ptr, slab_rows, gammas, costs, on_device, code, w, tail=(options_ptr(options),))


def _reduced_rank_list(ranks, rank: int, num_costs: int):
    """The checkpoints of the rank path, checked as the library checks them."""
    try:
        arr = np.asarray(ranks)
        if arr.size and arr.dtype.kind not in "iu":
            raise TypeError
        if arr.size and int(arr.min()) < 0:
            raise InvalidParameterError(f"Every checkpoint must lie in [1, {rank}]!")
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
    except (TypeError, ValueError):
        raise InvalidParameterError("The checkpoints must be a list of integers!") from None
    if arr.ndim != 1 or not 1 <= arr.size <= _capi.REDUCED_RANK_PATH_MAX_RANKS:
        raise InvalidParameterError(f"The rank path takes between 1 and {_capi.REDUCED_RANK_PATH_MAX_RANKS} checkpoints, but got {arr.size if arr.ndim == 1 else arr.shape}!")
    if arr.size * num_costs > _capi.REDUCED_GRID_MAX_CELLS:
        raise InvalidParameterError(f"The rank path takes at most {_capi.REDUCED_GRID_MAX_CELLS} (cost, checkpoint) cells, but got {num_costs} x {arr.size}!")
    if not (np.all(arr >= 1) and np.all(arr <= rank)):
        raise InvalidParameterError(f"Every checkpoint must lie in [1, {rank}]!")
    if np.any(arr[1:] <= arr[:-1]):
        raise InvalidParameterError("The checkpoints must be strictly ascending!")
    return arr


def _reduced_rank_path_call(fn, head, Y2, single: bool, N: int, rank: int, lm_ptr, slab_rows: int, ranks, costs, on_device: bool, weights, tail=()):
    k, R, S = Y2.shape[0], ranks.size, costs.size
    betas, rhos = np.zeros((S, R, k, rank)), np.zeros((S, R, k))
    leverage, fitted, loo = np.zeros((S, R, N)), np.zeros((S, R, k, N)), np.zeros((S, R, k, N))
    press, errors, used = np.zeros((S, R, k)), np.zeros((S, R, k), dtype=np.uint64), np.zeros(rank, dtype=np.uint64)
    infos = (_capi.LssvmReducedRankInfo * (S * R))()
    dense = (_capi.LssvmDenseInfo * S)()
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    check(fn(*head, ptr(Y2), k, _capi.weights_ptr(weights), rank, lm_ptr, slab_rows, ranks.ctypes.data_as(up), R, costs.ctypes.data_as(dp), S, int(on_device),
             betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp), press.ctypes.data_as(dp), errors.ctypes.data_as(up), leverage.ctypes.data_as(dp), fitted.ctypes.data_as(dp),
             loo.ctypes.data_as(dp), used.ctypes.data_as(up), infos, dense, *tail))
    cells = [[dict(dense[s].as_dict(), **infos[s * R + q].as_dict()) if on_device else infos[s * R + q].as_dict() for q in range(R)] for s in range(S)]
    report = {"costs": costs.copy(), "ranks": ranks.astype(np.int64), "leverage": leverage, "fitted": fitted[:, :, 0] if single else fitted, "loo": loo[:, :, 0] if single else loo,
              "press": press[:, :, 0] if single else press, "loo_errors": errors[:, :, 0] if single else errors,
              "max_leverage": np.array([[c["max_leverage"] for c in row] for row in cells]), "jitter": np.array([row[0]["jitter"] for row in cells]),
              "cond_hint": np.array([[c["cond_hint"] for c in row] for row in cells]), "infos": cells}
    return (betas[:, :, 0], rhos[:, :, 0], used, report) if single else (betas, rhos, used, report)


def fit_reduced_rank_path(params: Parameter, A, Y, rank: int, ranks, costs, landmarks=None, slab_rows: int = 0, options: Options | None = None, factor: str = "host",
                          sample_weight=None):
    """:func:`fit_reduced_loo` for EVERY PREFIX RANK of ``ranks`` and every cost of ``costs`` from one fit at ``rank`` (``lssvm_mi355_fit_reduced_rank_path_*``; DESIGN.md
    section 18).  The landmark list is ordered; the model on its first ``r`` entries needs only leading blocks of what the rank-``rank`` fit forms, and its leverages and
    fitted values are prefix sums along the rows of the product the leverage kernel forms anyway: one Gram pass, one factorisation per cost and one leverage pass per
    cost score the whole (cost, rank) grid.  ``ranks``: 1 to 16 strictly ascending checkpoints in ``[1, rank]``; ``len(ranks) * len(costs) <= 64``.  Every prefix model of
    a cost uses the jitter of the FULL rank at that cost (reported), which is no smaller than the one a separate fit on ``landmarks[:r]`` would take.
    Returns ``(betas[S, R, k, rank], rhos[S, R, k], landmarks, report)`` (the ``k`` axis dropped for a single right-hand side ``(N,)``); ``betas[s, q]`` is zero from
    ``ranks[q]`` on.  ``report`` as for :func:`fit_reduced_loo` with a rank axis behind the cost axis on every array, ``ranks``, ``jitter[S]``, ``cond_hint[S, R]`` (a
    cheap lower bound of the condition number, off the factor's diagonal) and ``infos[s][q]`` (``lssvm_reduced_rank_info`` dicts).  ``factor`` and ``sample_weight``: as
    for :func:`fit_reduced_loo`; with ``factor="host"``, ``betas[s, q]`` / ``rhos[s, q]`` at ``ranks[q] == rank`` have the bits of that call."""
    on_device = _capi.factor_on_device(factor)
    A = _as_matrix(A)
    N, d = A.shape
    w = _reduced_weights(sample_weight, N)
    if isinstance(landmarks, str):  # a selection rule (:func:`select_landmarks`): one resident problem selects and fits
        with ResidentProblem(params, A, options=options) as prob:
            return prob.fit_reduced_rank_path(Y, rank, ranks, costs, landmarks, slab_rows, factor=factor, sample_weight=w)
    Y2, single, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, N, A.dtype, rank, landmarks, slab_rows)
    costs = _reduced_loo_costs(costs)
    ranks = _reduced_rank_list(ranks, rank, costs.size)
    ps = _params_struct(params, d)
    fn = _capi.reduced_rank_path_entry(f"lssvm_mi355_fit_reduced_rank_path_{suffix_of(A.dtype)}")
    return _reduced_rank_path_call(fn, (C.byref(ps), ptr(A), N, d), Y2, single, N, rank, lm_ptr, slab_rows, ranks, costs, on_device, w, tail=(options_ptr(options),))


def generate_q(params: Parameter, data, options: Options | None = None):
    data = _as_matrix(data)
    N, d = data.shape
    q = np.zeros(N - 1, dtype=data.dtype)
    fn = getattr(lib, f"lssvm_mi355_generate_q_{suffix_of(data.dtype)}")
    fn.restype = C.c_int
    ps = _params_struct(params, d)
    check(fn(C.byref(ps), ptr(data), C.c_size_t(N), C.c_size_t(d), ptr(q), options_ptr(options)))
    return q


def run_device_kernel(params: Parameter, q, ret, d, data, QA_cost: float, add: float, options: Options | None = None):
    """``ret += add * Abar * d``; returns the updated copy of ``ret`` (gpu_csvm.hpp:431-447)."""
    data = _as_matrix(data)
    N, nf = data.shape
    q = np.ascontiguousarray(q, dtype=data.dtype)
    d = np.ascontiguousarray(d, dtype=data.dtype)
    out = np.array(ret, dtype=data.dtype, copy=True)
    if not (q.size == d.size == out.size == N - 1):
        raise InvalidParameterError(f"Sizes mismatch!: {q.size} != {N - 1}")
    ct = ctype_of(data.dtype)
    fn = getattr(lib, f"lssvm_mi355_run_device_kernel_{suffix_of(data.dtype)}")
    fn.restype = C.c_int
    ps = _params_struct(params, nf)
    check(fn(C.byref(ps), ptr(data), C.c_size_t(N), C.c_size_t(nf), ptr(q), ptr(d), ptr(out), ct(QA_cost), ct(add), options_ptr(options)))
    return out


def calculate_w(support_vectors, alpha):
    sv = _as_matrix(support_vectors)
    alpha = np.ascontiguousarray(alpha, dtype=sv.dtype)
    if alpha.size != sv.shape[0]:
        raise InvalidParameterError(f"The number of support vectors ({sv.shape[0]}) and weights ({alpha.size}) must match!")
    w = np.zeros(sv.shape[1], dtype=sv.dtype)
    fn = getattr(lib, f"lssvm_mi355_calculate_w_{suffix_of(sv.dtype)}")
    fn.restype = C.c_int
    check(fn(ptr(sv), C.c_size_t(sv.shape[0]), C.c_size_t(sv.shape[1]), ptr(alpha), ptr(w)))
    return w


def predict_values(params: Parameter, support_vectors, alpha, rho: float, w, predict_points, options: Options | None = None, info_out: dict | None = None):
    """Returns ``(values[num_points], w)``; ``w`` is None for the polynomial / rbf kernels (csvm.hpp:204-208).  ``info_out``: a dict that receives the call's
    ``lssvm_predict_info`` (timings, the Gram mode that ran)."""
    sv = _as_matrix(support_vectors)
    pts = _as_matrix(predict_points, dtype=sv.dtype)
    alpha = np.ascontiguousarray(alpha, dtype=sv.dtype)
    nsv, nf = sv.shape
    if alpha.size != nsv:
        raise InvalidParameterError(f"The number of support vectors ({nsv}) and number of weights ({alpha.size}) must be the same!")
    if pts.shape[1] != nf:
        raise InvalidParameterError(f"The number of features in the support vectors ({nf}) must be the same as in the data points to predict ({pts.shape[1]})!")
    if w is not None and len(w) not in (0, nf):
        raise InvalidParameterError(f"Either w must be empty or contain exactly the same number of values ({len(w)}) as features are present ({nf})!")
    ct = ctype_of(sv.dtype)
    w_valid = C.c_int(1 if (w is not None and len(w) == nf) else 0)
    w_buf = np.array(w, dtype=sv.dtype, copy=True) if w_valid.value else np.zeros(nf, dtype=sv.dtype)
    out = np.zeros(pts.shape[0], dtype=sv.dtype)
    fn = getattr(lib, f"lssvm_mi355_predict_values_{suffix_of(sv.dtype)}")
    fn.restype = C.c_int
    ps = _params_struct(params, nf)
    pinfo = LssvmPredictInfo()
    check(fn(C.byref(ps), ptr(sv), C.c_size_t(nsv), C.c_size_t(nf), ptr(alpha), ct(rho), ptr(w_buf), C.byref(w_valid), ptr(pts), C.c_size_t(pts.shape[0]), ptr(out), C.byref(pinfo), options_ptr(options)))
    if info_out is not None:
        info_out.update(pinfo.as_dict())
    return out, (w_buf if w_valid.value else None)


def predict_values_multi(params: Parameter, support_vectors, alphas, rhos, ws, predict_points, options: Options | None = None, info_out: dict | None = None):
    """``predict_values`` for ``k`` weight vectors over the SAME support vectors (``lssvm_mi355_predict_values_multi_*``): ``alphas`` is ``k x num_support_vectors``,
    ``rhos`` has ``k`` entries, ``ws`` is None or ``k x num_features`` (the cached w of the linear kernel).  Returns ``(values[num_points, k], ws)`` with ``ws`` None for the
    polynomial / rbf kernels; column ``v`` equals ``predict_values(..., alphas[v], rhos[v], ...)`` bit for bit.  Both point sets are uploaded and prepared once;
    ``info_out["vectors_per_launch"]`` says whether one pass over the Gram tiles fed two weight vectors (2) or every vector had a launch of its own (1)."""
    sv = _as_matrix(support_vectors)
    pts = _as_matrix(predict_points, dtype=sv.dtype)
    alphas = np.ascontiguousarray(alphas, dtype=sv.dtype)
    rhos = np.ascontiguousarray(rhos, dtype=sv.dtype)
    nsv, nf = sv.shape
    if alphas.ndim != 2 or alphas.shape[0] == 0:
        raise InvalidParameterError("The weights must be a matrix with one row per weight vector and at least one row!")
    k = alphas.shape[0]
    if alphas.shape[1] != nsv:
        raise InvalidParameterError(f"The number of support vectors ({nsv}) and number of weights ({alphas.shape[1]}) must be the same!")
    if rhos.shape != (k,):
        raise InvalidParameterError(f"The number of weight vectors ({k}) and the number of rho values ({rhos.size}) must be the same!")
    if pts.shape[1] != nf:
        raise InvalidParameterError(f"The number of features in the support vectors ({nf}) must be the same as in the data points to predict ({pts.shape[1]})!")
    have_w = ws is not None and np.size(ws) != 0
    if have_w and np.shape(ws) != (k, nf):
        raise InvalidParameterError(f"Either w must be empty or contain one row of {nf} values per weight vector ({k}), but its shape is {np.shape(ws)}!")
    w_valid = C.c_int(1 if have_w else 0)
    w_buf = np.array(ws, dtype=sv.dtype, copy=True, order="C") if have_w else np.zeros((k, nf), dtype=sv.dtype)
    out = np.zeros((pts.shape[0], k), dtype=sv.dtype)
    ps = _params_struct(params, nf)
    pinfo = LssvmPredictInfo()
    check(_capi.predict_multi_entry(sv.dtype)(C.byref(ps), ptr(sv), nsv, nf, ptr(alphas), ptr(rhos), k, ptr(w_buf), C.byref(w_valid), ptr(pts), pts.shape[0], ptr(out),
                                              C.byref(pinfo), options_ptr(options)))
    if info_out is not None:
        info_out.update(pinfo.as_dict())
    return out, (w_buf if w_valid.value else None)


class Predictor:
    """A model resident in HBM across predict calls (``lssvm_mi355_predictor_*``): the support vectors are uploaded and prepared once, every :meth:`predict` uploads only
    its batch of points.  Same values as :func:`predict_values`; ``info_out["resident"]`` says whether a batch ran against the resident form or took the one-shot path.

    A ONE-VS-ALL model: ``alpha`` of shape ``(k, num_support_vectors)`` with ``rho`` of shape ``(k,)`` (``lssvm_mi355_predictor_create_multi``).  :meth:`predict` then
    returns ``(num_points, k)`` and :meth:`predict_device` writes ``num_points`` x ``k`` values row-major, column ``v`` the bits of a predictor of ``(alpha[v], rho[v])``;
    ``info_out["vectors_per_launch"]`` says whether one pass over the Gram tiles fed two weight vectors (2) or every vector had a launch of its own (1).

    ``every_form=True`` creates the model through ``lssvm_mi355_predictor_create_resident``, for a vector or a matrix of weights: every resident form the library has,
    which adds the float64 one (rbf / polynomial, at most 256 features, two weight vectors per pass) and the float32 one beyond 128 features (rbf up to 384 features,
    polynomial up to 512 on f16 planes and 384 on bf16 planes; two weight vectors per pass).  The default keeps the routing of ``_create`` / ``_create_multi``, where a
    float64 rbf / polynomial model and a float32 model of more than 128 features take the one-shot path.  Float64 and rbf values are the same bits either way; a wide
    float32 polynomial model's differ from the one-shot call's by the rounding of the operand planes' scale (a few eps of the summand scale).

    ``panels=True`` creates the model through ``lssvm_mi355_predictor_create_panels``: every form of ``every_form=True``, and the models beyond those widths on the
    kernels that walk feature panels inside a tile (float32 rbf / polynomial beyond 384 / 512 features, float64 beyond 256; two weight vectors per pass for the
    polynomial kernel, float64 rbf and float32 rbf with folded records).  A model below those widths behaves as with ``every_form=True``."""

    def __init__(self, params: Parameter, support_vectors, alpha, rho, options: Options | None = None, every_form: bool = False, panels: bool = False):
        sv = _as_matrix(support_vectors)
        alpha = np.ascontiguousarray(alpha, dtype=sv.dtype)
        self.dtype, self.num_features = sv.dtype, int(sv.shape[1])
        self._h = C.c_void_p(None)
        if alpha.ndim == 2:
            k = alpha.shape[0]
            if k == 0:
                raise InvalidParameterError("The weights must be a matrix with one row per weight vector and at least one row!")
            if alpha.shape[1] != sv.shape[0]:
                raise InvalidParameterError(f"The number of support vectors ({sv.shape[0]}) and number of weights ({alpha.shape[1]}) must be the same!")
            rhos = np.ascontiguousarray(rho, dtype=np.float64)
            if rhos.shape != (k,):
                raise InvalidParameterError(f"The number of weight vectors ({k}) and the number of rho values ({rhos.size}) must be the same!")
            self.num_vectors = int(k)
        else:
            if alpha.size != sv.shape[0]:
                raise InvalidParameterError(f"The number of support vectors ({sv.shape[0]}) and number of weights ({alpha.size}) must be the same!")
            self.num_vectors = None  # (one weight vector: the values are a vector, not a matrix of one column)
            k, rhos = 1, np.array([float(rho)], dtype=np.float64)  # (every_form / panels: a handle of one vector, used through lssvm_mi355_predictor_predict like any other)
        ps = _params_struct(params, sv.shape[1])
        if alpha.ndim == 2 or every_form or panels:
            create = "lssvm_mi355_predictor_create_panels" if panels else ("lssvm_mi355_predictor_create_resident" if every_form else "lssvm_mi355_predictor_create_multi")
            check(_capi.predictor_multi_entry(create)(C.byref(self._h), C.byref(ps), _capi.dtype_code(sv.dtype), ptr(sv), sv.shape[0], sv.shape[1], ptr(alpha),
                                                      rhos.ctypes.data_as(C.POINTER(C.c_double)), k, options_ptr(options)))
            return
        check(lib.lssvm_mi355_predictor_create(C.byref(self._h), C.byref(ps), C.c_int(_capi.dtype_code(sv.dtype)), ptr(sv), C.c_size_t(sv.shape[0]), C.c_size_t(sv.shape[1]), ptr(alpha),
                                               C.c_double(float(rho)), options_ptr(options)))

    def predict(self, predict_points, info_out: dict | None = None):
        pts = _as_matrix(predict_points, dtype=self.dtype)
        if pts.shape[1] != self.num_features:
            raise InvalidParameterError(f"The number of features in the support vectors ({self.num_features}) must be the same as in the data points to predict ({pts.shape[1]})!")
        pinfo = LssvmPredictInfo()
        if self.num_vectors is None:
            out = np.zeros(pts.shape[0], dtype=self.dtype)
            check(lib.lssvm_mi355_predictor_predict(self._h, ptr(pts), C.c_int(_capi.LSSVM_MEM_HOST), C.c_size_t(pts.shape[0]), ptr(out), C.byref(pinfo)))
        else:
            out = np.zeros((pts.shape[0], self.num_vectors), dtype=self.dtype)
            check(_capi.predictor_multi_entry("lssvm_mi355_predictor_predict_multi")(self._h, ptr(pts), _capi.LSSVM_MEM_HOST, pts.shape[0], ptr(out), C.byref(pinfo)))
        if info_out is not None:
            info_out.update(pinfo.as_dict())
        return out

    def predict_device(self, points_ptr: int, num_points: int, out_ptr: int, info_out: dict | None = None) -> None:
        """The same with the batch AND the values in memory of device 0 (``LSSVM_MEM_DEVICE``): ``points_ptr`` -> ``num_points`` x ``num_features`` row-major of the predictor's
        dtype (e.g. a contiguous torch tensor's ``data_ptr()``, complete when the call is made), ``out_ptr`` -> ``num_points`` values (a one-vs-all model: ``num_points`` x
        ``k``, row-major), written when the call returns."""
        pinfo = LssvmPredictInfo()
        if self.num_vectors is None:
            check(lib.lssvm_mi355_predictor_predict(self._h, C.c_void_p(int(points_ptr)), C.c_int(_capi.LSSVM_MEM_DEVICE), C.c_size_t(int(num_points)), C.c_void_p(int(out_ptr)), C.byref(pinfo)))
        else:
            check(_capi.predictor_multi_entry("lssvm_mi355_predictor_predict_multi")(self._h, int(points_ptr), _capi.LSSVM_MEM_DEVICE, int(num_points), int(out_ptr), C.byref(pinfo)))
        if info_out is not None:
            info_out.update(pinfo.as_dict())

    def close(self):
        if self._h:
            lib.lssvm_mi355_predictor_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ReducedStream:
    """The fixed-size model from a STREAM of chunks (``lssvm_mi355_reduced_stream_*``; opt-in): what :func:`fit_reduced` keeps of the data is
    additive over rows, so the points need never be held at once.  The handle owns the landmark ROWS (``landmark_rows``: ``m x d``, float32 or float64 -- the stream's
    dtype), ``K_mm``, the running sums and one pending slab on device 0.  ``params.cost`` is ignored; ``weighted=True``: chunks may carry weights.

    :meth:`update` appends a chunk; :meth:`solve` fits every cost of a grid without consuming the state; :meth:`loo`, after a solve, scores a chunk that was streamed in
    (leverage, fitted and leave-one-out values per cost); :meth:`export_state` / :meth:`merge` carry the sums between streams of the same landmarks (one stream per
    shard or process, one of them merges).  No result depends on how the rows were cut into chunks."""

    def __init__(self, params: Parameter, landmark_rows, num_rhs: int = 1, weighted: bool = False, slab_rows: int = 0, options: Options | None = None):
        XL = _as_matrix(landmark_rows)
        self.dtype, self.rank, self.num_features, self.num_rhs, self.weighted = XL.dtype, int(XL.shape[0]), int(XL.shape[1]), int(num_rhs), bool(weighted)
        self._h = C.c_void_p(None)
        self._costs = 0
        if not (isinstance(slab_rows, (int, np.integer)) and slab_rows >= 0):
            raise InvalidParameterError(f"slab_rows must be a multiple of 256 (0: the library's default), but is {slab_rows!r}!")
        if not (isinstance(num_rhs, (int, np.integer)) and num_rhs >= 0):
            raise InvalidParameterError(f"The number of right hand sides must be greater than 0, but is {num_rhs!r}!")
        ps = _params_struct(params, XL.shape[1])
        create = _capi.reduced_stream_entry(f"lssvm_mi355_reduced_stream_create_{suffix_of(XL.dtype)}")
        check(create(C.byref(self._h), C.byref(ps), ptr(XL), XL.shape[0], XL.shape[1], self.num_rhs, int(self.weighted), int(slab_rows), options_ptr(options)))

    def _chunk(self, X, Y, sample_weight):
        X = _as_matrix(X, dtype=self.dtype)
        if X.shape[1] != self.num_features:
            raise InvalidParameterError(f"The number of features in the landmark rows ({self.num_features}) must be the same as in the chunk ({X.shape[1]})!")
        n = X.shape[0]
        Y2 = np.ascontiguousarray(Y, dtype=self.dtype)
        if Y2.ndim == 1 and self.num_rhs == 1:
            Y2 = Y2.reshape(1, -1)
        if Y2.shape != (self.num_rhs, n):
            raise InvalidParameterError(f"The right hand sides of a chunk of {n} rows must have the shape ({self.num_rhs}, {n}), but it is {Y2.shape}!")
        w = None
        if sample_weight is not None:
            w = np.ascontiguousarray(sample_weight, dtype=np.float64)
            if w.shape != (n,):
                raise InvalidParameterError(f"The number of rows in the chunk ({n}) and the number of weights ({w.size}) must be the same!")
        return X, Y2, w, n

    def update(self, X, Y, sample_weight=None) -> "ReducedStream":
        """Append the rows ``X`` (``n x d``) with their right-hand sides ``Y`` (``(k, n)``; ``(n,)`` for one) and, on a weighted stream, weights (None: 1.0)."""
        X, Y2, w, n = self._chunk(X, Y, sample_weight)
        check(_capi.reduced_stream_entry("lssvm_mi355_reduced_stream_update")(self._h, ptr(X), ptr(Y2), _capi.weights_ptr(w), n))
        self._costs = 0
        return self

    def solve(self, costs, factor: str = "host"):
        """The fit on every row streamed so far at each cost: ``(betas[S, k, m], rhos[S, k], infos)``, float64.  The state is left as it was: more updates may follow.
        ``factor``: as for :func:`fit_reduced`."""
        on_device = _capi.factor_on_device(factor)
        costs = np.ascontiguousarray(costs, dtype=np.float64).reshape(-1)
        S, dp = costs.size, C.POINTER(C.c_double)
        betas, rhos = np.zeros((S, self.num_rhs, self.rank)), np.zeros((S, self.num_rhs))
        infos = (_capi.LssvmReducedLooInfo * max(S, 1))()
        check(_capi.reduced_stream_entry("lssvm_mi355_reduced_stream_solve")(self._h, costs.ctypes.data_as(dp), S, int(on_device), betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp), infos))
        self._costs = S
        return betas, rhos, [infos[s].as_dict() for s in range(S)]

    def loo(self, X, Y, sample_weight=None):
        """After :meth:`solve` and before the next :meth:`update`: ``(leverage[S, n], fitted[S, k, n], loo[S, k, n])`` of a chunk that was streamed in, per cost of
        that solve.  A row of weight 0 is a held-out point: its ``loo`` value is the prediction of a model that never saw it."""
        X, Y2, w, n = self._chunk(X, Y, sample_weight)
        S, dp = max(self._costs, 1), C.POINTER(C.c_double)
        h, f, loo = np.zeros((S, n)), np.zeros((S, self.num_rhs, n)), np.zeros((S, self.num_rhs, n))
        check(_capi.reduced_stream_entry("lssvm_mi355_reduced_stream_loo")(self._h, ptr(X), ptr(Y2), _capi.weights_ptr(w), n, h.ctypes.data_as(dp), f.ctypes.data_as(dp), loo.ctypes.data_as(dp)))
        return h, f, loo

    def phi(self, X):
        """``K(X, X_L)`` (``n x m``, float64) as the stream evaluates it (a test aid, ``lssvm_mi355_reduced_stream_phi``); the state is left untouched."""
        X = _as_matrix(X, dtype=self.dtype)
        if X.shape[1] != self.num_features:
            raise InvalidParameterError(f"The number of features in the landmark rows ({self.num_features}) must be the same as in the chunk ({X.shape[1]})!")
        out = np.zeros((X.shape[0], self.rank))
        check(_capi.reduced_stream_entry("lssvm_mi355_reduced_stream_phi")(self._h, ptr(X), X.shape[0], out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def time_kernels(self, X, repeats: int = 10):
        """``(cross_ms[repeats], landmark_ms[repeats])``: device time of the stream's product kernel on the chunk ``X`` and of its resident sibling at the same shape (a
        measurement aid, ``lssvm_mi355_reduced_stream_time_kernels``)."""
        X = _as_matrix(X, dtype=self.dtype)
        a, b = np.zeros(repeats), np.zeros(repeats)
        dp = C.POINTER(C.c_double)
        check(_capi.reduced_stream_entry("lssvm_mi355_reduced_stream_time_kernels")(self._h, ptr(X), X.shape[0], int(repeats), a.ctypes.data_as(dp), b.ctypes.data_as(dp)))
        return a, b

    def export_state(self) -> dict:
        """The sums of every row streamed so far: ``{"gram": S~ (m+1+k)^2, "kmm", "num_points", "fingerprint"}`` -- what :meth:`merge` of another stream takes."""
        cols, dp, up = self.rank + 1 + self.num_rhs, C.POINTER(C.c_double), C.POINTER(C.c_uint64)
        gram, kmm = np.zeros((cols, cols)), np.zeros((self.rank, self.rank))
        n, fp = C.c_uint64(0), np.zeros(_capi.REDUCED_STREAM_FINGERPRINT_WORDS, dtype=np.uint64)
        check(_capi.reduced_stream_entry("lssvm_mi355_reduced_stream_export_state")(self._h, gram.ctypes.data_as(dp), kmm.ctypes.data_as(dp), C.byref(n), fp.ctypes.data_as(up)))
        return {"gram": gram, "kmm": kmm, "num_points": int(n.value), "fingerprint": fp}

    def merge(self, state: dict) -> "ReducedStream":
        """Add the exported sums of another stream of the same parameters, landmarks and dtype (refused otherwise) to this one's."""
        cols = self.rank + 1 + self.num_rhs
        gram = np.ascontiguousarray(state["gram"], dtype=np.float64)
        fp = np.ascontiguousarray(state["fingerprint"], dtype=np.uint64)
        if gram.shape != (cols, cols) or fp.shape != (_capi.REDUCED_STREAM_FINGERPRINT_WORDS,):
            raise InvalidParameterError(f"The state to merge must hold a ({cols}, {cols}) matrix and a fingerprint of {_capi.REDUCED_STREAM_FINGERPRINT_WORDS} words!")
        check(_capi.reduced_stream_entry("lssvm_mi355_reduced_stream_merge_state")(self._h, gram.ctypes.data_as(C.POINTER(C.c_double)), int(state["num_points"]),
                                                                                   fp.ctypes.data_as(C.POINTER(C.c_uint64))))
        self._costs = 0
        return self

    def _info(self, centre=None, kmm=None) -> dict:
        dp = C.POINTER(C.c_double)
        info = _capi.LssvmReducedStreamInfo()
        check(_capi.reduced_stream_entry("lssvm_mi355_reduced_stream_info")(self._h, C.byref(info), None if centre is None else centre.ctypes.data_as(dp),
                                                                            None if kmm is None else kmm.ctypes.data_as(dp)))
        return info.as_dict()

    @property
    def info(self) -> dict:
        return self._info()

    @property
    def num_points(self) -> int:
        return int(self._info()["num_points"])

    @property
    def centre(self) -> np.ndarray:
        """What every operand is shifted by as it is staged (rbf: the landmarks' mean; else zeros), ``d`` float64."""
        c = np.zeros(self.num_features)
        self._info(centre=c)
        return c

    @property
    def landmark_gram(self) -> np.ndarray:
        """``K_mm`` (``m x m``, float64): diagonal exactly 1 for rbf, symmetric to the bit."""
        kmm = np.zeros((self.rank, self.rank))
        self._info(kmm=kmm)
        return kmm

    def close(self):
        if self._h:
            _capi.reduced_stream_entry("lssvm_mi355_reduced_stream_destroy")(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _sum_in_row_order(start: float, terms) -> float:
    """``((start + t_0) + t_1) + ...``: one sequential chain, as the library's own sums over the points run."""
    return float(np.cumsum(np.concatenate([[start], np.asarray(terms, dtype=np.float64)]))[-1])


def fit_reduced_stream(params: Parameter, landmark_rows, chunks, costs, num_rhs: int = 1, factor: str = "host", loo: bool = False, weighted: bool = False, slab_rows: int = 0,
                       options: Options | None = None, on_scores=None):
    """:func:`fit_reduced_loo` from a stream of chunks through one :class:`ReducedStream`.  ``chunks``: an iterable of ``(X, Y, w)`` -- ``X``
    ``(n, d)``, ``Y`` ``(num_rhs, n)``, ``w`` ``(n,)`` weights or None (given only with ``weighted=True``).  One walk over ``chunks`` feeds the stream, the solve gives
    ``betas[S, k, m]`` and ``rhos[S, k]``; with ``loo=True`` a SECOND walk (``chunks`` must be re-iterable) scores every chunk and the sums over the points are
    accumulated here in row order: ``press[S, k]``, ``loo_errors[S, k]``, ``max_leverage[S]``, as :func:`fit_reduced_loo` defines them.  ``on_scores(i, X, Y, w, h, f, loo)``
    is called per chunk of the second walk for what else a caller accumulates.  Returns ``(betas, rhos, report)``; nothing of size N is kept."""
    costs = _reduced_loo_costs(costs)
    if loo and iter(chunks) is chunks:
        raise InvalidParameterError("The leave-one-out scores take a second walk over the chunks: a list or another re-iterable, not an iterator!")
    with ReducedStream(params, landmark_rows, num_rhs=num_rhs, weighted=weighted, slab_rows=slab_rows, options=options) as stream:
        fed = 0
        for X, Y, w in chunks:
            stream.update(X, Y, w)
            fed += 1
        if fed == 0:
            raise InvalidParameterError("The stream holds no rows: there was no chunk!")
        betas, rhos, infos = stream.solve(costs, factor=factor)
        S, k = costs.size, stream.num_rhs
        report = {"costs": costs.copy(), "num_points": stream.num_points, "jitter": np.array([i["jitter"] for i in infos]), "infos": infos}
        if loo:
            press, errors, top = np.zeros((S, k)), np.zeros((S, k), dtype=np.uint64), np.zeros(S)
            for i, (X, Y, w) in enumerate(chunks):
                h, f, values = stream.loo(X, Y, w)
                Y2 = np.asarray(Y, dtype=np.float64).reshape(k, -1)
                wrong = np.sign(values) != np.sign(Y2)[None, :, :]
                d2 = (Y2[None, :, :] - values) ** 2
                if w is not None:
                    wv = np.asarray(w, dtype=np.float64)
                    d2, wrong = wv[None, None, :] * d2, wrong & (wv > 0.0)[None, None, :]
                for s in range(S):
                    top[s] = max(top[s], float(h[s].max()))
                    for c in range(k):
                        press[s, c] = _sum_in_row_order(press[s, c], d2[s, c])
                errors += wrong.sum(axis=2).astype(np.uint64)
                if on_scores is not None:
                    on_scores(i, X, Y2, w, h, f, values)
            report.update(press=press, loo_errors=errors, max_leverage=top)
    return betas, rhos, report


# ---------------------------------------------------------------------------------------------------------------------
# communicator + resident problem (bench.py, multi-rank launchers)
# ---------------------------------------------------------------------------------------------------------------------
def comm_get_unique_id() -> bytes:
    buf = (C.c_ubyte * _capi.UNIQUE_ID_BYTES)()
    check(lib.lssvm_mi355_comm_get_unique_id(buf))
    return bytes(buf)


def comm_init(device: int, rank: int, world: int, unique_id: bytes) -> None:
    if len(unique_id) != _capi.UNIQUE_ID_BYTES:
        raise InvalidParameterError("unique id must have 128 bytes")
    buf = (C.c_ubyte * _capi.UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
    check(lib.lssvm_mi355_comm_init(C.c_int(device), C.c_int(rank), C.c_int(world), buf))


def comm_library_path() -> str:
    """The file the library resolved its RCCL entry points from (a measurement / test aid, include/plssvm_amd_testing.h)."""
    buf = C.create_string_buffer(4096)
    check(lib.lssvm_mi355_comm_library_path(buf, C.c_size_t(4096)))
    return buf.value.decode()


def comm_destroy() -> None:
    check(lib.lssvm_mi355_comm_destroy())


class ResidentProblem:
    """A data matrix resident in HBM plus the CG state on it (``lssvm_mi355_problem_*`` / ``lssvm_mi355_cg_*``)."""

    def __init__(self, params: Parameter, X, device: int = 0, rank: int = 0, world: int = 1, device_ptr: int | None = None, shape=None, dtype=None,
                 devices=None, options: Options | None = None):
        """``devices``: a list of HIP ordinals -> ONE process drives all of them (``lssvm_mi355_problem_create_multi``; an empty list = every
        visible device); otherwise ``device`` holds rank ``rank`` of a world of processes (one process per GPU, or a single GPU)."""
        self._h = C.c_void_p(None)
        if device_ptr is not None:
            N, d = shape
            self.dtype = np.dtype(dtype)
            src = C.c_void_p(device_ptr)
            kind = _capi.LSSVM_MEM_DEVICE
            self._keep = None
        else:
            X = _as_matrix(X)
            N, d = X.shape
            self.dtype = X.dtype
            src = ptr(X)
            kind = _capi.LSSVM_MEM_HOST
            self._keep = X
        self.num_points, self.num_features = int(N), int(d)
        self.params = params.resolved(d)
        ps = _params_struct(params, d)
        if devices is not None:
            if (rank, world) != (0, 1):
                raise InvalidParameterError("a device list (one process, several GPUs) and rank/world (one process per GPU) exclude each other")
            dev_arr, ndev = _capi.int_array(list(devices) or None)
            lib.lssvm_mi355_problem_create_multi.restype = C.c_int
            check(lib.lssvm_mi355_problem_create_multi(C.byref(self._h), C.byref(ps), C.c_int(_capi.dtype_code(self.dtype)), src, C.c_int(kind), C.c_size_t(N),
                                                       C.c_size_t(d), dev_arr, C.c_int(ndev), options_ptr(options)))
        else:
            shard = LssvmShard(rank, world)
            lib.lssvm_mi355_problem_create.restype = C.c_int
            check(lib.lssvm_mi355_problem_create(C.byref(self._h), C.byref(ps), C.c_int(_capi.dtype_code(self.dtype)), src, C.c_int(kind), C.c_size_t(N), C.c_size_t(d),
                                                 C.c_int(device), C.byref(shard), options_ptr(options)))
        self._keep = None  # the library copied the data

    def close(self):
        if self._h:
            lib.lssvm_mi355_problem_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def q(self):
        q = np.zeros(self.num_points - 1, dtype=self.dtype)
        qa = C.c_double(0)
        check(lib.lssvm_mi355_problem_get_q(self._h, ptr(q), C.byref(qa)))
        return q, float(qa.value)

    def set_weights(self, weights=None) -> None:
        """Per-point weights of the weighted LS-SVM system (``lssvm_mi355_problem_set_weights``): ``num_points`` values > 0, or None for the unweighted
        system.  Takes effect from the next :meth:`cg_begin` / :meth:`matvec`; not between ``cg_begin`` and ``cg_finish``."""
        w = None if weights is None else _as_weights(weights, self.num_points)
        check(_capi.weighted_entry("lssvm_mi355_problem_set_weights")(self._h, _capi.weights_ptr(w), 0 if w is None else w.size))

    def matvec(self, d, ret, add: float = 1.0):
        d = np.ascontiguousarray(d, dtype=self.dtype)
        out = np.array(ret, dtype=self.dtype, copy=True)
        if not (d.ndim == out.ndim == 1 and d.size == out.size == self.num_points - 1):  # the library reads / writes exactly N - 1 elements of both
            raise InvalidParameterError(f"Sizes mismatch!: {d.size} / {out.size} != {self.num_points - 1}")
        check(lib.lssvm_mi355_problem_matvec(self._h, ptr(d), ptr(out), C.c_double(add)))
        return out

    def matvec_pair(self, d0, d1, ret0, ret1, add: float = 1.0):
        """:meth:`matvec` for two vectors (``lssvm_mi355_problem_matvec_pair``): returns ``(out0, out1, two_vector)`` -- each result the bits of :meth:`matvec` for that
        vector; ``two_vector`` says whether one pass over the Gram tiles served both (one device; fp64: the symmetric resident-row-panel kernel; fp32: the symmetric one-pass split kernels on 129 ... 512 features, polynomial or rbf with folded
        records) or two single passes ran."""
        ds = [np.ascontiguousarray(d, dtype=self.dtype) for d in (d0, d1)]
        outs = [np.array(ret, dtype=self.dtype, copy=True) for ret in (ret0, ret1)]
        for v in ds + outs:
            if not (v.ndim == 1 and v.size == self.num_points - 1):
                raise InvalidParameterError(f"Sizes mismatch!: {v.size} != {self.num_points - 1}")
        two = C.c_int(0)
        check(_capi.lockstep_entry("lssvm_mi355_problem_matvec_pair")(self._h, ptr(ds[0]), ptr(ds[1]), ptr(outs[0]), ptr(outs[1]), add, C.byref(two)))
        return outs[0], outs[1], bool(two.value)

    def solve_lockstep(self, B, eps: float, max_iter: int):
        """``k`` right-hand sides (``B``: ``k x num_points``) in lockstep on this problem (``lssvm_mi355_problem_solve_lockstep``): every one runs the recipe of
        :meth:`cg_begin` / :meth:`cg_step` / :meth:`cg_finish`, and where the two-vector kernel applies (fp64, and fp32 on 129 ... 512 features: see :meth:`matvec_pair`)
        one pass over the Gram tiles serves two of them per iteration.
        Returns ``(alphas[k, num_points], rhos[k], infos, passes)`` -- per right-hand side the bits of a one-shot solve; ``passes = (two-vector, single-vector)`` Gram
        passes."""
        B = np.ascontiguousarray(B, dtype=self.dtype)
        if B.ndim != 2 or B.shape[0] == 0 or B.shape[1] != self.num_points:
            raise InvalidParameterError(f"The number of data points in the matrix A ({self.num_points}) and the values in every right hand side vector ({B.shape[-1] if B.ndim else 0}) must be the same!")
        k = B.shape[0]
        alphas = np.zeros_like(B)
        rhos = np.zeros(k, dtype=np.float64)
        infos = (LssvmCgInfo * k)()
        passes = (C.c_uint64 * 2)()
        check(_capi.lockstep_entry("lssvm_mi355_problem_solve_lockstep")(self._h, ptr(B), k, eps, int(max_iter), ptr(alphas), rhos.ctypes.data_as(C.POINTER(C.c_double)), infos, passes))
        return alphas, rhos.astype(self.dtype), [info.as_dict() for info in infos], (int(passes[0]), int(passes[1]))

    def solve_cost_path(self, y, costs, eps: float, max_iter: int, verify: bool = True):
        """:func:`solve_cost_path` on this resident problem (``lssvm_mi355_problem_solve_cost_path``): every cost of ``costs`` from one multi-shift CG sequence on the
        problem's own single-vector pass.  The problem's own cost is ignored and the problem is left as it was.  Not on a problem of several devices or ranks, not with
        weights set, not between :meth:`cg_begin` and :meth:`cg_finish`."""
        y, costs = _cost_path_arguments(y, self.num_points, self.dtype, costs, eps, max_iter)
        return _cost_path_call(_capi.cost_path_entry("lssvm_mi355_problem_solve_cost_path"), (self._h,), y, costs, self.num_points, self.dtype, eps, max_iter, verify)

    def select_landmarks(self, rank: int, method: str = "rpcholesky", pool: int = 0, seed: int = 0, tol: float = 0.0):
        """:func:`select_landmarks` on this resident problem (``lssvm_mi355_problem_select_landmarks``): ``(landmarks[:rank_found], trace, residual, info)``.  The problem
        is left as it was and keeps its preconditioner.  Not on a problem of several devices or ranks, not with weights set, not between :meth:`cg_begin` and
        :meth:`cg_finish`."""
        rank, code, pool, seed, tol = _select_arguments(self.num_points, rank, method, pool, seed, tol)
        return _select_call(_capi.select_entry("lssvm_mi355_problem_select_landmarks"), (self._h,), self.num_points, rank, code, pool, seed, tol)

    def _selected(self, rank, landmarks):
        """``landmarks`` as the entry points that consume them take it: a selection rule's name becomes the indices :meth:`select_landmarks` finds for ``rank`` (fewer where
        the rank is exhausted first); everything else passes through."""
        return self.select_landmarks(rank, method=landmarks)[0] if isinstance(landmarks, str) else landmarks

    def build_preconditioner(self, rank: int = 256, landmarks=None):
        """The Nystrom preconditioner of this problem at its own cost (``lssvm_mi355_problem_build_preconditioner``): ``rank`` landmarks of the library's fixed choice, or
        the given distinct point indices (their number is the rank), or ``"greedy"`` / ``"rpcholesky"``: ``rank`` points of :meth:`select_landmarks`.  Building again replaces it.  Returns the ``lssvm_precond_info`` dict.  Not on a problem of several
        devices or ranks, not with weights set, not between :meth:`cg_begin` and :meth:`cg_finish`."""
        rank, lm, lm_ptr = _landmarks_argument(rank, self._selected(rank, landmarks))
        info = _capi.LssvmPrecondInfo()
        check(_capi.pcg_entry("lssvm_mi355_problem_build_preconditioner")(self._h, rank, lm_ptr, C.byref(info)))
        self._precond_rank = rank
        return info.as_dict()

    def precond_landmarks(self):
        """The landmarks of the preconditioner in use (``lssvm_mi355_problem_precond_landmarks``)."""
        out = np.zeros(max(int(getattr(self, "_precond_rank", 0)), 1), dtype=np.uint64)
        check(_capi.pcg_entry("lssvm_mi355_problem_precond_landmarks")(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def precond_apply(self, r):
        """``z = r - Bhat G^-1 Bhat^T r = P^-1 r / C`` for a vector of ``num_points - 1`` entries: the preconditioner alone (``lssvm_mi355_problem_precond_apply``)."""
        r = np.ascontiguousarray(r, dtype=self.dtype)
        if not (r.ndim == 1 and r.size == self.num_points - 1):
            raise InvalidParameterError(f"Sizes mismatch!: {r.size} != {self.num_points - 1}")
        z = np.zeros_like(r)
        check(_capi.pcg_entry("lssvm_mi355_problem_precond_apply")(self._h, ptr(r), ptr(z)))
        return z

    def solve_pcg(self, B, eps: float, max_iter: int):
        """:func:`solve_pcg` on this resident problem and the preconditioner :meth:`build_preconditioner` left (``lssvm_mi355_problem_solve_pcg``): one right-hand side
        ``(num_points,)`` or ``k`` of them, one after the other.  Returns ``(alphas, rhos, infos)`` shaped like ``B``; the problem is left as it was."""
        B2, single = _pcg_arguments(B, self.num_points, self.dtype, eps, max_iter)
        return _pcg_call(_capi.pcg_entry("lssvm_mi355_problem_solve_pcg"), (self._h,), (), B2, single, self.num_points, self.dtype, eps, max_iter)

    def fit_reduced(self, Y, rank: int, landmarks=None, slab_rows: int = 0, factor: str = "host", sample_weight=None):
        """:func:`fit_reduced` on this resident problem at its own cost (``lssvm_mi355_problem_fit_reduced``; ``factor="device"``: ``lssvm_mi355_problem_fit_reduced_dev``).
        The problem is left as it was and keeps its preconditioner.
        Not on a problem of several devices or ranks, not with weights set, not between :meth:`cg_begin` and :meth:`cg_finish`.
        ``sample_weight`` (``lssvm_mi355_problem_fit_reduced_weighted``): the weights of :func:`fit_reduced` -- the keyword is the only source of weights, :meth:`set_weights`
        is not consulted (and still refused)."""
        on_device = _capi.factor_on_device(factor)
        w = _reduced_weights(sample_weight, self.num_points)
        Y2, single, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, self.num_points, self.dtype, rank, self._selected(rank, landmarks), slab_rows)
        return _reduced_call(_reduced_entry("problem_fit_reduced", on_device, weighted=w is not None), (self._h,), Y2, single, rank, lm_ptr, slab_rows, on_device=on_device, weights=w)

    def landmark_gram(self, Y, rank: int, landmarks=None, slab_rows: int = 0):
        """The operator of :meth:`fit_reduced` alone (a test aid, ``lssvm_mi355_problem_landmark_gram``): ``[Phi | 1 | Y]^T [Phi | 1 | Y]`` as the device sums it,
        ``(rank + 1 + k, rank + 1 + k)`` float64, both triangles."""
        Y2, _, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, self.num_points, self.dtype, rank, landmarks, slab_rows)
        cols = rank + 1 + Y2.shape[0]
        out = np.zeros((cols, cols), dtype=np.float64)
        check(_capi.reduced_entry("lssvm_mi355_problem_landmark_gram")(self._h, ptr(Y2), Y2.shape[0], rank, lm_ptr, slab_rows, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def landmark_gram_weighted(self, Y, rank: int, sample_weight, landmarks=None, slab_rows: int = 0):
        """The operator of the weighted :meth:`fit_reduced` alone (a test aid, ``lssvm_mi355_problem_landmark_gram_weighted``): ``[Phi | 1 | Y]^T diag(w) [Phi | 1 | Y]``
        as the device sums it, ``(rank + 1 + k, rank + 1 + k)`` float64, both triangles."""
        w = _reduced_weights(sample_weight, self.num_points)
        Y2, _, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, self.num_points, self.dtype, rank, landmarks, slab_rows)
        cols = rank + 1 + Y2.shape[0]
        out = np.zeros((cols, cols), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        check(_capi.reduced_weighted_entry("lssvm_mi355_problem_landmark_gram_weighted")(self._h, ptr(Y2), Y2.shape[0], None if w is None else w.ctypes.data_as(dp), rank, lm_ptr, slab_rows,
                                                                                          out.ctypes.data_as(dp)))
        return out

    def fit_reduced_loo(self, Y, rank: int, costs, landmarks=None, slab_rows: int = 0, factor: str = "host", sample_weight=None):
        """:func:`fit_reduced_loo` on this resident problem (``lssvm_mi355_problem_fit_reduced_loo``; ``factor="device"``: ``lssvm_mi355_problem_fit_reduced_loo_dev``):
        leave-one-out with the landmark set held fixed, at every cost of ``costs``.  The problem's own cost is ignored; the problem is left as it was and keeps its
        preconditioner.  Refused where :meth:`fit_reduced` is.  ``sample_weight`` (``lssvm_mi355_problem_fit_reduced_loo_weighted``): as for :func:`fit_reduced_loo`."""
        on_device = _capi.factor_on_device(factor)
        w = _reduced_weights(sample_weight, self.num_points)
        Y2, single, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, self.num_points, self.dtype, rank, self._selected(rank, landmarks), slab_rows)
        costs = _reduced_loo_costs(costs)
        return _reduced_loo_call(_reduced_entry("problem_fit_reduced_loo", on_device, weighted=w is not None), (self._h,), Y2, single, self.num_points, rank, lm_ptr, slab_rows, costs,
                                 on_device=on_device, weights=w)

    def fit_reduced_grid(self, Y, rank: int, gammas, costs, landmarks=None, sample_weight=None, factor: str = "host", product: str = "matrix", slab_rows: int = 0):
        """:func:`fit_reduced_grid` on this resident problem (``lssvm_mi355_problem_fit_reduced_grid``): leave-one-out with the landmark set held fixed at every
        ``(gamma, cost)`` of the grid, the feature sums behind Phi formed once per slab and pass.  The problem's own cost and gamma are ignored by the fit (its gamma
        decided how it holds its data when it was created); ``landmarks="greedy"`` / ``"rpcholesky"`` select with the problem's own gamma.  The problem is left as it
        was and keeps its preconditioner.  Refused where :meth:`fit_reduced` is, and on a linear-kernel problem."""
        on_device = _capi.factor_on_device(factor)
        code = _capi.product_argument(product)
        _reduced_grid_kernel(self.params)
        w = _reduced_weights(sample_weight, self.num_points)
        costs = _reduced_loo_costs(costs)
        gammas = _reduced_grid_gammas(gammas, costs.size)
        Y2, single, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, self.num_points, self.dtype, rank, self._selected(rank, landmarks), slab_rows)
        return _reduced_grid_call(_capi.reduced_grid_entry("lssvm_mi355_problem_fit_reduced_grid"), (self._h,), Y2, single, self.num_points, rank, lm_ptr, slab_rows, gammas, costs,
                                  on_device, code, w)

    def landmark_acc(self, rank: int, landmarks=None, product: str = "matrix"):
        """The operator of :meth:`fit_reduced_grid` alone (a test aid, ``lssvm_mi355_problem_landmark_acc``): ``D[l, i]`` = the sum over the held features of
        ``(a_f - b_f)^2`` (rbf) or ``a_f b_f`` (polynomial, linear) for landmark ``l`` and point ``i``, ``(rank, num_points)`` float64."""
        code = _capi.product_argument(product)
        _, _, rank, _, lm_ptr, _ = _reduced_arguments(np.zeros(self.num_points, dtype=self.dtype), self.num_points, self.dtype, rank, landmarks, 0)
        out = np.zeros((rank, self.num_points), dtype=np.float64)
        check(_capi.reduced_grid_entry("lssvm_mi355_problem_landmark_acc")(self._h, lm_ptr, rank, code, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def reduced_leverage(self, V, shift, B_extra=None, landmarks=None, slab_rows: int = 0):
        """The operator of :meth:`fit_reduced_loo` alone on the caller's operands (a test aid, ``lssvm_mi355_problem_reduced_leverage``): with ``phic_i = phi_i - shift``,
        ``h[i] = |V phic_i|^2`` for the LOWER triangle of ``V`` (rank x rank; what stands above the diagonal is never used) and ``f[c, i] = phic_i . B_extra[:, c]``
        (``B_extra``: rank x k or None).  Returns ``(h[N], f[k, N])``, float64."""
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.ndim != 2 or V.shape[0] != V.shape[1]:
            raise InvalidParameterError(f"V must be a square matrix, but its shape is {V.shape}!")
        rank = V.shape[0]
        _, _, rank, _, lm_ptr, slab_rows = _reduced_arguments(np.zeros(self.num_points, dtype=self.dtype), self.num_points, self.dtype, rank if landmarks is None else None, landmarks, slab_rows)
        shift = np.ascontiguousarray(shift, dtype=np.float64)
        extra = np.zeros((rank, 0)) if B_extra is None else np.ascontiguousarray(B_extra, dtype=np.float64)
        if V.shape[0] != rank or shift.shape != (rank,) or extra.ndim != 2 or extra.shape[0] != rank:
            raise InvalidParameterError(f"V, shift and B_extra must have {rank} rows, but their shapes are {V.shape}, {shift.shape} and {extra.shape}!")
        k = extra.shape[1]
        h, f = np.zeros(self.num_points), np.zeros((k, self.num_points))
        dp = C.POINTER(C.c_double)
        check(_capi.reduced_loo_entry("lssvm_mi355_problem_reduced_leverage")(self._h, rank, lm_ptr, slab_rows, V.ctypes.data_as(dp), shift.ctypes.data_as(dp),
                                                                                 extra.ctypes.data_as(dp) if k else None, k, h.ctypes.data_as(dp), f.ctypes.data_as(dp) if k else None))
        return h, f

    def fit_reduced_rank_path(self, Y, rank: int, ranks, costs, landmarks=None, slab_rows: int = 0, factor: str = "host", sample_weight=None):
        """:func:`fit_reduced_rank_path` on this resident problem (``lssvm_mi355_problem_fit_reduced_rank_path``): the leave-one-out scores of every prefix rank of
        ``ranks`` at every cost of ``costs`` from one fit at ``rank``.  The problem's own cost is ignored; the problem is left as it was and keeps its preconditioner.
        Refused where :meth:`fit_reduced` is."""
        on_device = _capi.factor_on_device(factor)
        w = _reduced_weights(sample_weight, self.num_points)
        Y2, single, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, self.num_points, self.dtype, rank, self._selected(rank, landmarks), slab_rows)
        costs = _reduced_loo_costs(costs)
        ranks = _reduced_rank_list(ranks, rank, costs.size)
        return _reduced_rank_path_call(_capi.reduced_rank_path_entry("lssvm_mi355_problem_fit_reduced_rank_path"), (self._h,), Y2, single, self.num_points, rank, lm_ptr, slab_rows,
                                       ranks, costs, on_device, w)

    def fit_reduced_logistic(self, Y, rank: int, landmarks=None, sample_weight=None, tol: float = 1e-8, max_iter: int = 50, factor: str = "host", start=None, slab_rows: int = 0):
        """:func:`fit_reduced_logistic` on this resident problem at its own cost (``lssvm_mi355_problem_fit_reduced_logistic``).  The problem is left as it was and keeps
        its preconditioner.  Refused where :meth:`fit_reduced` is."""
        on_device = _capi.factor_on_device(factor)
        w = _reduced_weights(sample_weight, self.num_points)
        Y2, single, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, self.num_points, self.dtype, rank, self._selected(rank, landmarks), slab_rows)
        tol, max_iter, betas0, rhos0 = _reduced_logistic_arguments(Y2, rank, tol, max_iter, start)
        return _reduced_logistic_call(_capi.reduced_logistic_entry("lssvm_mi355_problem_fit_reduced_logistic"), (self._h,), Y2, single, rank, lm_ptr, slab_rows, w, on_device, tol,
                                      max_iter, betas0, rhos0)

    def reduced_logistic_step(self, Y, betas, rhos, landmarks=None, sample_weight=None, slab_rows: int = 0):
        """The step operator of :meth:`fit_reduced_logistic` alone at the caller's coefficients (a test aid, ``lssvm_mi355_problem_reduced_logistic_step``): ``betas``
        ``(k, rank)`` and ``rhos`` ``(k,)`` for the ``k`` label vectors ``Y``.  Returns ``(eta, q, z, loss, floored)``: ``eta = Phi beta - rho``, ``q = sqrt(a max(mu, 2^-32))``
        and the working responses ``z``, ``(k, N)`` float64 each, the ``k`` sums of ``a_i l_i`` and the ``k`` numbers of rows at the floor."""
        betas = np.ascontiguousarray(betas, dtype=np.float64)
        betas = betas.reshape(1, -1) if betas.ndim == 1 else betas
        rhos = np.ascontiguousarray(rhos, dtype=np.float64).reshape(-1)
        w = _reduced_weights(sample_weight, self.num_points)
        Y2, _, rank, _, lm_ptr, slab_rows = _reduced_arguments(Y, self.num_points, self.dtype, betas.shape[1] if landmarks is None else None, landmarks, slab_rows)
        _, _, betas, rhos = _reduced_logistic_arguments(Y2, rank, 1.0, 1, (betas, rhos))
        k, N = Y2.shape
        eta, q, z = np.zeros((k, N)), np.zeros((k, N)), np.zeros((k, N))
        loss, floored = np.zeros(k), np.zeros(k, dtype=np.uint64)
        dp = C.POINTER(C.c_double)
        check(_capi.reduced_logistic_entry("lssvm_mi355_problem_reduced_logistic_step")(self._h, ptr(Y2), k, _capi.weights_ptr(w), rank, lm_ptr, slab_rows, betas.ctypes.data_as(dp),
                                                                                          rhos.ctypes.data_as(dp), eta.ctypes.data_as(dp), q.ctypes.data_as(dp), z.ctypes.data_as(dp),
                                                                                          loss.ctypes.data_as(dp), floored.ctypes.data_as(C.POINTER(C.c_uint64))))
        return eta, q, z, loss, floored

    def reduced_leverage_prefix(self, V, shift, ranks, Z=None, landmarks=None, slab_rows: int = 0):
        """The operator of :meth:`fit_reduced_rank_path` alone on the caller's operands (a test aid, ``lssvm_mi355_problem_reduced_leverage_prefix``): with
        ``u_i = V (phi_i - shift)`` for the LOWER triangle of ``V``, ``h[q, i] = sum_{j < ranks[q]} u_ij^2`` and ``f[q, c, i] = sum_{j < ranks[q]} u_ij Z[c, j]``
        (``Z``: k x rank or None).  Returns ``(h[R, N], f[R, k, N])``, float64."""
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.ndim != 2 or V.shape[0] != V.shape[1]:
            raise InvalidParameterError(f"V must be a square matrix, but its shape is {V.shape}!")
        rank = V.shape[0]
        _, _, rank, _, lm_ptr, slab_rows = _reduced_arguments(np.zeros(self.num_points, dtype=self.dtype), self.num_points, self.dtype, rank if landmarks is None else None, landmarks, slab_rows)
        shift = np.ascontiguousarray(shift, dtype=np.float64)
        Z = np.zeros((0, rank)) if Z is None else np.ascontiguousarray(Z, dtype=np.float64)
        if V.shape[0] != rank or shift.shape != (rank,) or Z.ndim != 2 or Z.shape[1] != rank:
            raise InvalidParameterError(f"V and shift must have {rank} rows and Z {rank} columns, but their shapes are {V.shape}, {shift.shape} and {Z.shape}!")
        ranks = _reduced_rank_list(ranks, rank, 1)
        k, R = Z.shape[0], ranks.size
        h, f = np.zeros((R, self.num_points)), np.zeros((R, k, self.num_points))
        dp = C.POINTER(C.c_double)
        check(_capi.reduced_rank_path_entry("lssvm_mi355_problem_reduced_leverage_prefix")(self._h, rank, lm_ptr, slab_rows, V.ctypes.data_as(dp), shift.ctypes.data_as(dp),
                                                                                            Z.ctypes.data_as(dp) if k else None, k, ranks.ctypes.data_as(C.POINTER(C.c_uint64)), R,
                                                                                            h.ctypes.data_as(dp), f.ctypes.data_as(dp) if k else None))
        return h, f

    def time_leverage_prefix_kernel(self, rank: int, ranks, k: int = 1, slab_rows: int = 0, repeats: int = 10):
        """A measurement aid (``lssvm_mi355_problem_time_leverage_prefix_kernel``): on the slab and operands of :meth:`time_leverage_kernel`, the prefix leverage kernel of
        :meth:`fit_reduced_rank_path` with the checkpoints ``ranks``: ``prefix_ms[repeats]``."""
        ranks = _reduced_rank_list(ranks, int(rank), 1)
        out = np.zeros(int(repeats))
        check(_capi.reduced_rank_path_entry("lssvm_mi355_problem_time_leverage_prefix_kernel")(self._h, int(rank), int(slab_rows), int(k), ranks.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                                                                ranks.size, int(repeats), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def time_leverage_kernel(self, rank: int, k: int = 1, slab_rows: int = 0, repeats: int = 10):
        """A measurement aid (``lssvm_mi355_problem_time_leverage_kernel``): on one slab of this problem, the Gram kernels of :meth:`fit_reduced` and the leverage kernel of
        :meth:`fit_reduced_loo`: ``(gram_ms[repeats], leverage_ms[repeats])``."""
        gram, lev = np.zeros(int(repeats)), np.zeros(int(repeats))
        dp = C.POINTER(C.c_double)
        check(_capi.reduced_loo_entry("lssvm_mi355_problem_time_leverage_kernel")(self._h, int(rank), int(slab_rows), int(k), int(repeats), gram.ctypes.data_as(dp), lev.ctypes.data_as(dp)))
        return gram, lev

    def time_gram_kernels(self, repeats: int = 10):
        """A measurement aid (``lssvm_mi355_problem_time_gram_kernels``): ``Bhat^T Bhat`` of this fp64 problem's preconditioner by the preconditioner's own kernel and by the
        matrix-core kernels of :meth:`fit_reduced`: ``(parent_ms[repeats], mfma_ms[repeats], largest relative difference of the two results)``."""
        parent, mfma, diff = np.zeros(int(repeats)), np.zeros(int(repeats)), C.c_double(0)
        dp = C.POINTER(C.c_double)
        check(_capi.reduced_entry("lssvm_mi355_problem_time_gram_kernels")(self._h, int(repeats), parent.ctypes.data_as(dp), mfma.ctypes.data_as(dp), C.byref(diff)))
        return parent, mfma, float(diff.value)

    def cg_begin(self, y, eps: float):
        y = np.ascontiguousarray(y, dtype=self.dtype)
        if y.size != self.num_points:
            raise InvalidParameterError(f"The number of data points in the matrix A ({self.num_points}) and the values in the right hand side vector ({y.size}) must be the same!")
        check(lib.lssvm_mi355_cg_begin(self._h, ptr(y), C.c_double(eps)))

    def cg_step(self, iterations: int) -> bool:
        done = C.c_int(0)
        check(lib.lssvm_mi355_cg_step(self._h, C.c_uint64(int(iterations)), C.byref(done)))
        return bool(done.value)

    def cg_finish(self):
        alpha = np.zeros(self.num_points, dtype=self.dtype)
        rho = C.c_double(0)
        info = LssvmCgInfo()
        check(lib.lssvm_mi355_cg_finish(self._h, ptr(alpha), C.byref(rho), C.byref(info)))
        return alpha, self.dtype.type(rho.value), info.as_dict()

    def info(self):
        info = LssvmCgInfo()
        check(lib.lssvm_mi355_problem_info(self._h, C.byref(info)))
        return info.as_dict()

    def synchronize(self):
        check(lib.lssvm_mi355_problem_synchronize(self._h))

    def rebalance(self, weights=None) -> bool:
        """New shares for the ranks of a sharded symmetric problem, between two ``cg_step`` calls (``lssvm_mi355_problem_rebalance``): explicit ``weights`` (one per rank,
        the same on every rank) or, ``None``, by the shards' measured pace.  Returns whether the shares changed."""
        w = [float(v) for v in (weights or [])]
        arr = (C.c_double * len(w))(*w) if w else None
        changed = C.c_int(0)
        check(lib.lssvm_mi355_problem_rebalance(self._h, arr, C.c_int(len(w)), C.byref(changed)))
        return bool(changed.value)

    def ipc_export(self) -> bytes:
        """One process per GPU over HIP IPC: this rank's ``LSSVM_IPC_BLOB_BYTES`` blob (``lssvm_mi355_problem_ipc_export``)."""
        buf = (C.c_ubyte * _capi.LSSVM_IPC_BLOB_BYTES)()
        check(lib.lssvm_mi355_problem_ipc_export(self._h, buf, C.c_size_t(_capi.LSSVM_IPC_BLOB_BYTES)))
        return bytes(buf)

    def ipc_connect(self, blobs) -> None:
        """``blobs``: the exports of ALL ranks in rank order (``lssvm_mi355_problem_ipc_connect``)."""
        joined = b"".join(bytes(b) for b in blobs)
        buf = (C.c_ubyte * len(joined)).from_buffer_copy(joined) if joined else None
        check(lib.lssvm_mi355_problem_ipc_connect(self._h, buf, C.c_size_t(len(joined))))
