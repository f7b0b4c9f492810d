"""ctypes binding of the C ABI declared in ``include/plssvm_amd.h`` (libplssvm_amd.so: HIP kernels for gfx950).

The library is the ONLY compute path of this package: if it is missing, importing this module raises -- there is no
CPU or PyTorch fallback (the CPU oracle under ``oracle/`` is test infrastructure and is never imported from here).
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .exceptions import BackendError, InvalidParameterError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PLSSVM_AMD_LIBRARY") or os.path.join(_HERE, "lib", "libplssvm_amd.so")  # (the variable lets a developer A/B two builds)

LSSVM_DTYPE_F32 = 0
LSSVM_DTYPE_F64 = 1
LSSVM_MEM_HOST = 0
LSSVM_MEM_DEVICE = 1
UNIQUE_ID_BYTES = 128

STATUS_NAMES = {0: "LSSVM_SUCCESS", -1: "LSSVM_ERR_INVALID_ARGUMENT", -2: "LSSVM_ERR_NO_DEVICE", -3: "LSSVM_ERR_HIP", -4: "LSSVM_ERR_COMM",
                -5: "LSSVM_ERR_OUT_OF_MEMORY", -6: "LSSVM_ERR_INTERNAL"}

# every symbol include/plssvm_amd.h declares (tests/test_capi_symbols.py checks the built library against this list AND the header)
EXPORTED_SYMBOLS = [
    "lssvm_mi355_abi_version", "lssvm_mi355_device_count", "lssvm_mi355_device_name", "lssvm_mi355_last_error",
    "lssvm_mi355_options_create", "lssvm_mi355_options_set", "lssvm_mi355_options_get", "lssvm_mi355_options_destroy",
    "lssvm_mi355_solve_f32", "lssvm_mi355_solve_f64", "lssvm_mi355_solve_multi_f32", "lssvm_mi355_solve_multi_f64", "lssvm_mi355_predict_values_f32", "lssvm_mi355_predict_values_f64",
    "lssvm_mi355_predict_values_multi_f32", "lssvm_mi355_predict_values_multi_f64",
    "lssvm_mi355_solve_weighted_f32", "lssvm_mi355_solve_weighted_f64", "lssvm_mi355_problem_set_weights", "lssvm_mi355_solve_refined_f64",
    "lssvm_mi355_predictor_create", "lssvm_mi355_predictor_predict", "lssvm_mi355_predictor_destroy", "lssvm_mi355_predictor_create_multi", "lssvm_mi355_predictor_predict_multi",
    "lssvm_mi355_predictor_create_resident", "lssvm_mi355_predictor_create_panels",
    "lssvm_mi355_generate_q_f32", "lssvm_mi355_generate_q_f64", "lssvm_mi355_run_device_kernel_f32", "lssvm_mi355_run_device_kernel_f64",
    "lssvm_mi355_calculate_w_f32", "lssvm_mi355_calculate_w_f64",
    "lssvm_mi355_shard_blocks", "lssvm_mi355_set_shard_weights", "lssvm_mi355_problem_rebalance", "lssvm_mi355_comm_get_unique_id", "lssvm_mi355_comm_init", "lssvm_mi355_comm_destroy",
    "lssvm_mi355_problem_create", "lssvm_mi355_problem_create_multi", "lssvm_mi355_problem_ipc_export", "lssvm_mi355_problem_ipc_connect", "lssvm_mi355_problem_destroy", "lssvm_mi355_problem_get_q", "lssvm_mi355_problem_matvec",
    "lssvm_mi355_problem_matvec_pair", "lssvm_mi355_problem_solve_lockstep",
    "lssvm_mi355_problem_solve_cost_path", "lssvm_mi355_solve_cost_path_f32", "lssvm_mi355_solve_cost_path_f64",
    "lssvm_mi355_problem_build_preconditioner", "lssvm_mi355_problem_precond_landmarks", "lssvm_mi355_problem_precond_apply", "lssvm_mi355_problem_solve_pcg",
    "lssvm_mi355_solve_pcg_f32", "lssvm_mi355_solve_pcg_f64",
    "lssvm_mi355_problem_fit_reduced", "lssvm_mi355_fit_reduced_f32", "lssvm_mi355_fit_reduced_f64", "lssvm_mi355_problem_landmark_gram", "lssvm_mi355_problem_time_gram_kernels",
    "lssvm_mi355_problem_fit_reduced_loo", "lssvm_mi355_fit_reduced_loo_f32", "lssvm_mi355_fit_reduced_loo_f64", "lssvm_mi355_problem_reduced_leverage", "lssvm_mi355_problem_time_leverage_kernel",
    "lssvm_mi355_problem_fit_reduced_dev", "lssvm_mi355_fit_reduced_dev_f32", "lssvm_mi355_fit_reduced_dev_f64",
    "lssvm_mi355_problem_fit_reduced_loo_dev", "lssvm_mi355_fit_reduced_loo_dev_f32", "lssvm_mi355_fit_reduced_loo_dev_f64",
    "lssvm_mi355_problem_fit_reduced_weighted", "lssvm_mi355_fit_reduced_weighted_f32", "lssvm_mi355_fit_reduced_weighted_f64",
    "lssvm_mi355_problem_fit_reduced_loo_weighted", "lssvm_mi355_fit_reduced_loo_weighted_f32", "lssvm_mi355_fit_reduced_loo_weighted_f64",
    "lssvm_mi355_problem_landmark_gram_weighted",
    "lssvm_mi355_problem_fit_reduced_grid", "lssvm_mi355_fit_reduced_grid_f32", "lssvm_mi355_fit_reduced_grid_f64", "lssvm_mi355_problem_landmark_acc",
    "lssvm_mi355_problem_fit_reduced_rank_path", "lssvm_mi355_fit_reduced_rank_path_f32", "lssvm_mi355_fit_reduced_rank_path_f64",
    "lssvm_mi355_problem_reduced_leverage_prefix", "lssvm_mi355_problem_time_leverage_prefix_kernel",
    "lssvm_mi355_dense_cholesky", "lssvm_mi355_dense_solve", "lssvm_mi355_dense_invert_lower",
    "lssvm_mi355_problem_select_landmarks", "lssvm_mi355_select_landmarks_f32", "lssvm_mi355_select_landmarks_f64",
    "lssvm_mi355_reduced_stream_create_f32", "lssvm_mi355_reduced_stream_create_f64", "lssvm_mi355_reduced_stream_update", "lssvm_mi355_reduced_stream_solve",
    "lssvm_mi355_reduced_stream_loo", "lssvm_mi355_reduced_stream_export_state", "lssvm_mi355_reduced_stream_merge_state", "lssvm_mi355_reduced_stream_info",
    "lssvm_mi355_reduced_stream_destroy", "lssvm_mi355_reduced_stream_phi", "lssvm_mi355_reduced_stream_time_kernels",
    "lssvm_mi355_problem_fit_reduced_logistic", "lssvm_mi355_fit_reduced_logistic_f32", "lssvm_mi355_fit_reduced_logistic_f64", "lssvm_mi355_problem_reduced_logistic_step",
    "lssvm_mi355_cg_begin", "lssvm_mi355_cg_step", "lssvm_mi355_cg_finish", "lssvm_mi355_problem_synchronize", "lssvm_mi355_problem_info",
    "lssvm_mi355_measure_bf16_mfma_ceiling", "lssvm_mi355_comm_library_path", "lssvm_mi355_set_io_threads", "lssvm_mi355_set_option", "lssvm_mi355_get_option",
    "lssvm_mi355_libsvm_open", "lssvm_mi355_libsvm_fill_f32", "lssvm_mi355_libsvm_fill_f64", "lssvm_mi355_libsvm_close",
    "lssvm_mi355_libsvm_write_f32", "lssvm_mi355_libsvm_write_f64", "lssvm_mi355_model_write_f32", "lssvm_mi355_model_write_f64",
    "lssvm_mi355_model_open", "lssvm_mi355_model_labels", "lssvm_mi355_model_fill_f32", "lssvm_mi355_model_fill_f64", "lssvm_mi355_model_close",
    "lssvm_mi355_arff_open", "lssvm_mi355_arff_fill_f32", "lssvm_mi355_arff_fill_f64", "lssvm_mi355_arff_close",
]


class LssvmParams(C.Structure):
    """``lssvm_params`` (include/plssvm_amd.h) == plssvm::detail::parameter<T> with gamma resolved."""
    _fields_ = [("kernel_type", C.c_int32), ("degree", C.c_int32), ("gamma", C.c_double), ("coef0", C.c_double), ("cost", C.c_double)]


class LssvmCgInfo(C.Structure):
    _fields_ = [("iterations", C.c_uint64), ("max_iterations", C.c_uint64), ("residuum", C.c_double), ("initial_residuum", C.c_double),
                ("target_residuum", C.c_double), ("epsilon", C.c_double), ("avg_iteration_ms", C.c_double), ("total_ms", C.c_double),
                ("setup_ms", C.c_double), ("matvec_kernel_ms", C.c_double), ("matvec_launches", C.c_uint64), ("devices_used", C.c_int32),
                ("converged", C.c_int32), ("symmetric", C.c_int32), ("gram_mode", C.c_int32), ("local_devices", C.c_int32), ("exchange", C.c_int32), ("tile_launches_per_matvec", C.c_int32), ("rbf_direct", C.c_int32), ("rbf_exponent_scale", C.c_double),
                ("matvec_timed", C.c_uint64), ("matvec_kernel_ms_total", C.c_double), ("rccl_nranks", C.c_int32), ("rccl_rank", C.c_int32), ("rccl_device", C.c_int32), ("persistent_launches", C.c_int32),
                ("f16_row_rel_error", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class LssvmPredictInfo(C.Structure):
    """``lssvm_predict_info``: the timings of one ``predict_values`` call; ``vectors_per_launch``: what ``predict_values_multi`` reports (0 from every other call)."""
    _fields_ = [("total_ms", C.c_double), ("setup_ms", C.c_double), ("kernel_ms", C.c_double), ("rbf_exponent_scale", C.c_double), ("f16_row_rel_error", C.c_double),
                ("gram_mode", C.c_int32), ("rbf_direct", C.c_int32), ("resident", C.c_int32), ("vectors_per_launch", C.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class LssvmRefineInfo(C.Structure):
    """``lssvm_refine_info``: what the mixed-precision refinement (``lssvm_mi355_solve_refined_f64``) did for one right-hand side."""
    _fields_ = [("refined", C.c_int32), ("took_over_f64", C.c_int32), ("outer_steps", C.c_uint64), ("inner_iterations", C.c_uint64), ("f64_cg_iterations", C.c_uint64),
                ("f64_passes", C.c_uint64), ("f32_passes", C.c_uint64), ("initial_residuum", C.c_double), ("residuum", C.c_double), ("target_residuum", C.c_double),
                ("f64_ms", C.c_double), ("f32_ms", C.c_double), ("total_ms", C.c_double), ("inner_gram_mode", C.c_int32), ("inner_rbf_direct", C.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class LssvmPathInfo(C.Structure):
    """``lssvm_path_info``: how one cost of a cost path (``lssvm_mi355_problem_solve_cost_path``) went; the residua are squared norms, ``true_residuum`` -1 without verify."""
    _fields_ = [("iterations", C.c_uint64), ("converged", C.c_int32), ("verified", C.c_int32), ("initial_residuum", C.c_double), ("residuum", C.c_double),
                ("target_residuum", C.c_double), ("true_residuum", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class LssvmPrecondInfo(C.Structure):
    """``lssvm_precond_info``: what building the Nystrom preconditioner of a problem took (``lssvm_mi355_problem_build_preconditioner``)."""
    _fields_ = [("rank", C.c_uint64), ("jitter", C.c_double), ("build_ms", C.c_double), ("host_ms", C.c_double), ("device_bytes", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class LssvmPcgInfo(C.Structure):
    """``lssvm_pcg_info``: how one right-hand side of ``lssvm_mi355_problem_solve_pcg`` went; the residua are squared norms as in ``lssvm_cg_info``."""
    _fields_ = [("iterations", C.c_uint64), ("gram_passes", C.c_uint64), ("converged", C.c_int32), ("rank", C.c_int32), ("initial_residuum", C.c_double),
                ("residuum", C.c_double), ("target_residuum", C.c_double), ("jitter", C.c_double), ("build_ms", C.c_double), ("apply_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class LssvmReducedInfo(C.Structure):
    """``lssvm_reduced_info``: what fitting a fixed-size model took (``lssvm_mi355_problem_fit_reduced``); ``jitter``: the nu added to the diagonal of M."""
    _fields_ = [("rank", C.c_uint64), ("slabs", C.c_uint64), ("jitter", C.c_double), ("landmark_ms", C.c_double), ("gram_ms", C.c_double), ("host_ms", C.c_double),
                ("total_ms", C.c_double), ("workspace_bytes", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class LssvmModelInfo(C.Structure):
    """``lssvm_model_info``: the header of a model file as the native reader reports it."""
    _fields_ = [("kernel_type", C.c_int32), ("has_degree", C.c_int32), ("has_gamma", C.c_int32), ("has_coef0", C.c_int32), ("degree", C.c_int64),
                ("gamma", C.c_double), ("coef0", C.c_double), ("rho", C.c_double), ("nr_class", C.c_uint64), ("total_sv", C.c_uint64),
                ("num_features", C.c_uint64), ("label_text_bytes", C.c_uint64)]


class LssvmShard(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32)]


def _load():
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C plssvm_amd/csrc`. plssvm_amd has no CPU fallback.")
    return C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)


lib = _load()
lib.lssvm_mi355_last_error.restype = C.c_char_p
lib.lssvm_mi355_abi_version.restype = C.c_int
lib.lssvm_mi355_device_count.restype = C.c_int


def weighted_entry(name: str):
    """``lssvm_mi355_solve_weighted_f32 / _f64`` or ``lssvm_mi355_problem_set_weights`` with its argument types (weights are double whatever the real type).
    Bound at the first call, so that an older build named by PLSSVM_AMD_LIBRARY still serves everything else."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        if name == "lssvm_mi355_problem_set_weights":
            fn.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_size_t]
        else:
            ct = C.c_float if name.endswith("_f32") else C.c_double
            fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.POINTER(C.c_double), ct, C.c_uint64, C.c_void_p, C.POINTER(ct),
                           C.POINTER(LssvmCgInfo), C.c_void_p]
        fn.restype = C.c_int
    return fn


def predict_multi_entry(dtype):
    """``lssvm_mi355_predict_values_multi_f32 / _f64`` with its argument types.  Bound at the first call, like the weighted entry points."""
    fn = getattr(lib, f"lssvm_mi355_predict_values_multi_{suffix_of(dtype)}")
    if fn.argtypes is None:
        fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_size_t,
                       C.c_void_p, C.POINTER(LssvmPredictInfo), C.c_void_p]
        fn.restype = C.c_int
    return fn


def predictor_multi_entry(name: str):
    """``lssvm_mi355_predictor_create_multi`` / ``lssvm_mi355_predictor_create_resident`` / ``lssvm_mi355_predictor_create_panels`` / ``lssvm_mi355_predictor_predict_multi`` with its argument types.  Bound at the first call, like the weighted entry points."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        if name in ("lssvm_mi355_predictor_create_multi", "lssvm_mi355_predictor_create_resident", "lssvm_mi355_predictor_create_panels"):
            fn.argtypes = [C.POINTER(C.c_void_p), C.POINTER(LssvmParams), C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.c_void_p]
        else:
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.POINTER(LssvmPredictInfo)]
        fn.restype = C.c_int
    return fn


def lockstep_entry(name: str):
    """``lssvm_mi355_problem_solve_lockstep`` / ``lssvm_mi355_problem_matvec_pair`` with its argument types.  Bound at the first call, like the weighted entry points."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        if name == "lssvm_mi355_problem_solve_lockstep":
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_uint64, C.c_void_p, C.POINTER(C.c_double), C.POINTER(LssvmCgInfo), C.POINTER(C.c_uint64)]
        else:
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_int)]
        fn.restype = C.c_int
    return fn


def refined_entry():
    """``lssvm_mi355_solve_refined_f64`` with its argument types.  Bound at the first call, like the weighted entry points."""
    fn = lib.lssvm_mi355_solve_refined_f64
    if fn.argtypes is None:
        fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.c_double, C.c_uint64, C.c_void_p,
                       C.POINTER(C.c_double), C.POINTER(LssvmCgInfo), C.POINTER(LssvmRefineInfo), C.POINTER(C.c_uint64), C.c_void_p]
        fn.restype = C.c_int
    return fn


PATH_MAX_COSTS = 64


def cost_path_entry(name: str):
    """``lssvm_mi355_problem_solve_cost_path`` / ``lssvm_mi355_solve_cost_path_f32 / _f64`` with its argument types.  Bound at the first call, like the weighted entry points."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        tail = [C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.c_double, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(LssvmPathInfo), C.POINTER(C.c_uint64)]
        if name == "lssvm_mi355_problem_solve_cost_path":
            fn.argtypes = [C.c_void_p] + tail
        else:
            fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t] + tail + [C.c_void_p]
        fn.restype = C.c_int
    return fn


PRECOND_MAX_RANK = 512


def pcg_entry(name: str):
    """The entry points of the Nystrom preconditioner and of PCG (``lssvm_mi355_problem_build_preconditioner`` ... ``lssvm_mi355_solve_pcg_f32 / _f64``) with their
    argument types.  Bound at the first call, like the weighted entry points."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        solve = [C.c_void_p, C.c_size_t]
        tail = [C.c_double, C.c_uint64, C.c_void_p, C.POINTER(C.c_double), C.POINTER(LssvmPcgInfo)]
        if name == "lssvm_mi355_problem_build_preconditioner":
            fn.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(LssvmPrecondInfo)]
        elif name == "lssvm_mi355_problem_precond_landmarks":
            fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        elif name == "lssvm_mi355_problem_precond_apply":
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        elif name == "lssvm_mi355_problem_solve_pcg":
            fn.argtypes = [C.c_void_p] + solve + tail
        else:
            fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t] + solve + [C.c_uint64, C.POINTER(C.c_uint64)] + tail + [C.c_void_p]
        fn.restype = C.c_int
    return fn


class LssvmDenseInfo(C.Structure):
    """``lssvm_dense_info``: the dense steps of one device-factored fit or of one cost of a device-factored leave-one-out grid (``lssvm_mi355_problem_fit_reduced_dev``)."""
    _fields_ = [("rank", C.c_uint64), ("block", C.c_uint64), ("attempts", C.c_uint64), ("launches", C.c_uint64), ("jitter", C.c_double), ("assemble_ms", C.c_double),
                ("factor_ms", C.c_double), ("solve_ms", C.c_double), ("invert_ms", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


REDUCED_MAX_RANK = 1024
DENSE_BLOCK = 64  # lssvm::DENSE_BLOCK (plssvm_amd/csrc/lssvm_dense.hip.hpp): the block width of the device's factorisation, solves and inverse
FACTOR_CHOICES = ("host", "device")


def factor_on_device(factor) -> bool:
    """The ``factor=`` keyword of the fixed-size fits: ``"host"`` (the default) or ``"device"``; anything else is refused before any library call."""
    if not isinstance(factor, str) or factor not in FACTOR_CHOICES:
        raise InvalidParameterError(f'factor must be "host" or "device", but is {factor!r}!')
    return factor == "device"


def factor_keyword(factor) -> dict:
    """``factor`` as a keyword for the backend boundary of ``plssvm_amd.csvm`` -- only where it is not the default, so that a backend object written before the keyword
    existed still serves the default."""
    return {} if factor == "host" else {"factor": factor}


def reduced_entry(name: str):
    """The entry points of the fixed-size model (``lssvm_mi355_problem_fit_reduced``, ``lssvm_mi355_fit_reduced_f32 / _f64``, and the test aids
    ``lssvm_mi355_problem_landmark_gram`` / ``_time_gram_kernels``) with their argument types.  Bound at the first call, like the weighted entry points."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        common = [C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64]  # Y, num_rhs, rank, landmarks, slab_rows
        outs = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(LssvmReducedInfo)]
        dense = [C.POINTER(LssvmDenseInfo)]
        if name == "lssvm_mi355_problem_fit_reduced":
            fn.argtypes = [C.c_void_p] + common + outs
        elif name == "lssvm_mi355_problem_fit_reduced_dev":
            fn.argtypes = [C.c_void_p] + common + outs + dense
        elif name.startswith("lssvm_mi355_fit_reduced_dev_"):
            fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t] + common + outs + [C.c_void_p] + dense
        elif name == "lssvm_mi355_problem_landmark_gram":
            fn.argtypes = [C.c_void_p] + common + [C.POINTER(C.c_double)]
        elif name == "lssvm_mi355_problem_time_gram_kernels":
            fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        else:
            fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t] + common + outs + [C.c_void_p]
        fn.restype = C.c_int
    return fn


class LssvmReducedLooInfo(C.Structure):
    """``lssvm_reduced_loo_info``: one cost of ``lssvm_mi355_problem_fit_reduced_loo``."""
    _fields_ = [("cost", C.c_double), ("jitter", C.c_double), ("max_leverage", C.c_double), ("landmark_ms", C.c_double), ("gram_ms", C.c_double), ("leverage_ms", C.c_double),
                ("host_ms", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


REDUCED_LOO_MAX_COSTS = 64


def reduced_loo_entry(name: str):
    """The entry points of the leave-one-out scores of the fixed-size model (``lssvm_mi355_problem_fit_reduced_loo``, ``lssvm_mi355_fit_reduced_loo_f32 / _f64`` and the
    test aids ``lssvm_mi355_problem_reduced_leverage`` / ``_time_leverage_kernel``) with their argument types.  Bound at the first call."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
        common = [C.c_void_p, C.c_size_t, C.c_uint64, up, C.c_uint64, dp, C.c_size_t]  # Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs
        outs = [dp, dp, dp, dp, dp, dp, up, up, C.POINTER(LssvmReducedLooInfo)]  # betas, rhos, leverage, fitted, loo, press, loo_errors, landmarks, infos
        dense = [C.POINTER(LssvmDenseInfo)]
        if name == "lssvm_mi355_problem_fit_reduced_loo":
            fn.argtypes = [C.c_void_p] + common + outs
        elif name == "lssvm_mi355_problem_fit_reduced_loo_dev":
            fn.argtypes = [C.c_void_p] + common + outs + dense
        elif name.startswith("lssvm_mi355_fit_reduced_loo_dev_"):
            fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t] + common + outs + [C.c_void_p] + dense
        elif name == "lssvm_mi355_problem_reduced_leverage":
            fn.argtypes = [C.c_void_p, C.c_uint64, up, C.c_uint64, dp, dp, dp, C.c_size_t, dp, dp]
        elif name == "lssvm_mi355_problem_time_leverage_kernel":
            fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_size_t, C.c_int, dp, dp]
        else:
            fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t] + common + outs + [C.c_void_p]
        fn.restype = C.c_int
    return fn


class LssvmReducedStreamInfo(C.Structure):
    """``lssvm_reduced_stream_info``: the counts of a reduced stream (``lssvm_mi355_reduced_stream_info``)."""
    _fields_ = [("num_points", C.c_uint64), ("pending", C.c_uint64), ("rank", C.c_uint64), ("num_features", C.c_uint64), ("num_rhs", C.c_uint64), ("slab_rows", C.c_uint64),
                ("weighted", C.c_int32), ("dtype", C.c_int32), ("workspace_bytes", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


REDUCED_STREAM_FINGERPRINT_WORDS = 9


def reduced_stream_entry(name: str):
    """The entry points of the fixed-size model from a stream of chunks (``lssvm_mi355_reduced_stream_*``; the test aid ``_phi``) with their argument types.  Bound at
    the first call."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        dp, up, h = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_void_p
        tail = name[len("lssvm_mi355_reduced_stream_"):]
        fn.argtypes = {
            "create_f32": [C.POINTER(C.c_void_p), C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_uint64, C.c_void_p],
            "create_f64": [C.POINTER(C.c_void_p), C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_uint64, C.c_void_p],
            "update": [h, C.c_void_p, C.c_void_p, dp, C.c_size_t],
            "solve": [h, dp, C.c_size_t, C.c_int, dp, dp, C.POINTER(LssvmReducedLooInfo)],
            "loo": [h, C.c_void_p, C.c_void_p, dp, C.c_size_t, dp, dp, dp],
            "export_state": [h, dp, dp, up, up],
            "merge_state": [h, dp, C.c_uint64, up],
            "info": [h, C.POINTER(LssvmReducedStreamInfo), dp, dp],
            "phi": [h, C.c_void_p, C.c_size_t, dp],
            "time_kernels": [h, C.c_void_p, C.c_size_t, C.c_int, dp, dp],
            "destroy": [h],
        }[tail]
        fn.restype = C.c_int
    return fn


def dense_entry(name: str):
    """The testing aids of the dense toolbox (``lssvm_mi355_dense_cholesky`` / ``_solve`` / ``_invert_lower``; include/plssvm_amd_testing.h) with their argument types."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        dp = C.POINTER(C.c_double)
        if name == "lssvm_mi355_dense_cholesky":
            fn.argtypes = [dp, C.c_size_t, C.c_double, dp, C.POINTER(C.c_uint64), dp]
        elif name == "lssvm_mi355_dense_solve":
            fn.argtypes = [dp, C.c_size_t, dp, C.c_size_t, dp, dp]
        else:
            fn.argtypes = [dp, C.c_size_t, dp, dp]
        fn.restype = C.c_int
    return fn


def reduced_weighted_entry(name: str):
    """The weighted entry points of the fixed-size model (``lssvm_mi355_problem_fit_reduced_weighted``, ``_fit_reduced_loo_weighted``, their one-shot forms and the test
    aid ``lssvm_mi355_problem_landmark_gram_weighted``) with their argument types.  Bound at the first call."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
        common = [C.c_void_p, C.c_size_t, dp, C.c_uint64, up, C.c_uint64]  # Y, num_rhs, weights, rank, landmarks, slab_rows
        if "loo" in name:
            # costs, num_costs, factor, betas, rhos, leverage, fitted, loo, press, loo_errors, landmarks, infos, dense
            common += [dp, C.c_size_t, C.c_int, dp, dp, dp, dp, dp, dp, up, up, C.POINTER(LssvmReducedLooInfo), C.POINTER(LssvmDenseInfo)]
        elif name == "lssvm_mi355_problem_landmark_gram_weighted":
            common += [dp]
        else:
            common += [C.c_int, dp, dp, up, C.POINTER(LssvmReducedInfo), C.POINTER(LssvmDenseInfo)]  # factor, betas, rhos, landmarks, info, dense
        if "problem" in name:
            fn.argtypes = [C.c_void_p] + common
        else:
            fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t] + common + [C.c_void_p]
        fn.restype = C.c_int
    return fn


class LssvmReducedLogisticInfo(C.Structure):
    """``lssvm_reduced_logistic_info``: how one class of ``lssvm_mi355_problem_fit_reduced_logistic`` went."""
    _fields_ = [("passes", C.c_uint64), ("halvings", C.c_uint64), ("floored", C.c_uint64), ("converged", C.c_int32), ("reserved", C.c_int32), ("objective", C.c_double),
                ("last_decrease", C.c_double), ("jitter", C.c_double), ("max_abs_eta", C.c_double), ("landmark_ms", C.c_double), ("step_ms", C.c_double), ("gram_ms", C.c_double),
                ("host_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


def reduced_logistic_entry(name: str):
    """The entry points of the fixed-size logistic regression (``lssvm_mi355_problem_fit_reduced_logistic``, ``lssvm_mi355_fit_reduced_logistic_f32 / _f64`` and the test
    aid ``lssvm_mi355_problem_reduced_logistic_step``) with their argument types.  Bound at the first call."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
        common = [C.c_void_p, C.c_size_t, dp, C.c_uint64, up, C.c_uint64]  # Y, num_rhs, weights, rank, landmarks, slab_rows
        if name == "lssvm_mi355_problem_reduced_logistic_step":
            fn.argtypes = [C.c_void_p] + common + [dp, dp, dp, dp, dp, dp, up]  # betas, rhos, eta, q, z, loss, floored
        else:
            # factor, tol, max_iter, betas0, rhos0, betas, rhos, landmarks, infos
            common += [C.c_int, C.c_double, C.c_uint64, dp, dp, dp, dp, up, C.POINTER(LssvmReducedLogisticInfo)]
            if "problem" in name:
                fn.argtypes = [C.c_void_p] + common
            else:
                fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t] + common + [C.c_void_p]
        fn.restype = C.c_int
    return fn


class LssvmReducedGridInfo(C.Structure):
    """``lssvm_reduced_grid_info``: one (gamma, cost) cell of ``lssvm_mi355_problem_fit_reduced_grid``."""
    _fields_ = [("cost", C.c_double), ("jitter", C.c_double), ("max_leverage", C.c_double), ("landmark_ms", C.c_double), ("gram_ms", C.c_double), ("leverage_ms", C.c_double),
                ("host_ms", C.c_double), ("gamma", C.c_double), ("accumulate_ms", C.c_double), ("values_ms", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


REDUCED_GRID_MAX_CELLS = 64
PRODUCT_CHOICES = ("ordered", "matrix")  # the `product` argument of the grid: 0, 1


def product_argument(product) -> int:
    """The ``product=`` keyword of the (gamma, cost) grid: ``"ordered"`` or ``"matrix"`` (the default); anything else is refused before any library call."""
    if not isinstance(product, str) or product not in PRODUCT_CHOICES:
        raise InvalidParameterError(f'product must be "ordered" or "matrix", but is {product!r}!')
    return PRODUCT_CHOICES.index(product)


def reduced_grid_entry(name: str):
    """The entry points of the (gamma, cost) grid of the fixed-size model (``lssvm_mi355_problem_fit_reduced_grid``, ``lssvm_mi355_fit_reduced_grid_f32 / _f64`` and the
    test aid ``lssvm_mi355_problem_landmark_acc``) with their argument types.  Bound at the first call."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
        if name == "lssvm_mi355_problem_landmark_acc":
            fn.argtypes = [C.c_void_p, up, C.c_uint64, C.c_int, dp]
        else:
            # Y, num_rhs, weights, rank, landmarks, slab_rows, gammas, num_gammas, costs, num_costs, factor, product, then the outputs of the leave-one-out call
            common = [C.c_void_p, C.c_size_t, dp, C.c_uint64, up, C.c_uint64, dp, C.c_size_t, dp, C.c_size_t, C.c_int, C.c_int,
                      dp, dp, dp, dp, dp, dp, up, up, C.POINTER(LssvmReducedGridInfo), C.POINTER(LssvmDenseInfo)]
            if "problem" in name:
                fn.argtypes = [C.c_void_p] + common
            else:
                fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t] + common + [C.c_void_p]
        fn.restype = C.c_int
    return fn


class LssvmReducedRankInfo(C.Structure):
    """``lssvm_reduced_rank_info``: one (cost, checkpoint) cell of ``lssvm_mi355_problem_fit_reduced_rank_path``."""
    _fields_ = [("cost", C.c_double), ("rank", C.c_uint64), ("jitter", C.c_double), ("max_leverage", C.c_double), ("landmark_ms", C.c_double), ("gram_ms", C.c_double),
                ("leverage_ms", C.c_double), ("host_ms", C.c_double), ("cond_hint", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


REDUCED_RANK_PATH_MAX_RANKS = 16


def reduced_rank_path_entry(name: str):
    """The entry points of the rank path of the fixed-size model (``lssvm_mi355_problem_fit_reduced_rank_path``, ``lssvm_mi355_fit_reduced_rank_path_f32 / _f64`` and the
    test aids ``lssvm_mi355_problem_reduced_leverage_prefix`` / ``_time_leverage_prefix_kernel``) with their argument types.  Bound at the first call."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
        if name == "lssvm_mi355_problem_reduced_leverage_prefix":
            fn.argtypes = [C.c_void_p, C.c_uint64, up, C.c_uint64, dp, dp, dp, C.c_size_t, up, C.c_size_t, dp, dp]
        elif name == "lssvm_mi355_problem_time_leverage_prefix_kernel":
            fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_size_t, up, C.c_size_t, C.c_int, dp]
        else:
            # Y, num_rhs, weights, rank, landmarks, slab_rows, ranks, num_ranks, costs, num_costs, factor, betas, rhos, press, loo_errors, leverage, fitted, loo, landmarks, infos, dense
            common = [C.c_void_p, C.c_size_t, dp, C.c_uint64, up, C.c_uint64, up, C.c_size_t, dp, C.c_size_t, C.c_int,
                      dp, dp, dp, up, dp, dp, dp, up, C.POINTER(LssvmReducedRankInfo), C.POINTER(LssvmDenseInfo)]
            if "problem" in name:
                fn.argtypes = [C.c_void_p] + common
            else:
                fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t] + common + [C.c_void_p]
        fn.restype = C.c_int
    return fn


class LssvmLandmarkSelectInfo(C.Structure):
    """``lssvm_landmark_select_info``: how a landmark selection went (``lssvm_mi355_problem_select_landmarks``); the traces are sums of the residual diagonal."""
    _fields_ = [("rank_found", C.c_uint64), ("candidates", C.c_uint64), ("trace0", C.c_double), ("trace", C.c_double), ("max_residual", C.c_double), ("select_ms", C.c_double),
                ("device_bytes", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


SELECT_MAX_RANK = 1024
LANDMARK_METHODS = {"greedy": 1, "rpcholesky": 2}  # LSSVM_LANDMARKS_GREEDY, LSSVM_LANDMARKS_RPCHOLESKY


def select_entry(name: str):
    """The entry points of the landmark selection (``lssvm_mi355_problem_select_landmarks``, ``lssvm_mi355_select_landmarks_f32 / _f64``) with their argument types.
    Bound at the first call, like the weighted entry points."""
    fn = getattr(lib, name)
    if fn.argtypes is None:
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
        common = [C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_double, up, dp, dp, C.POINTER(LssvmLandmarkSelectInfo)]  # rank, method, pool, seed, tol, the outputs
        if name == "lssvm_mi355_problem_select_landmarks":
            fn.argtypes = [C.c_void_p] + common
        else:
            fn.argtypes = [C.POINTER(LssvmParams), C.c_void_p, C.c_size_t, C.c_size_t] + common + [C.c_void_p]
        fn.restype = C.c_int
    return fn


def weights_ptr(w: np.ndarray | None):
    """The ``const double *weights`` argument: NULL for None."""
    return None if w is None else w.ctypes.data_as(C.POINTER(C.c_double))


def last_error() -> str:
    msg = lib.lssvm_mi355_last_error()
    return msg.decode("utf-8", errors="replace") if msg else ""


def check(status: int) -> None:
    """Map a non-zero status to the exception the reference would throw at this point."""
    if status == 0:
        return
    msg = f"{STATUS_NAMES.get(status, status)}: {last_error()}"
    if status == -1:
        raise InvalidParameterError(msg)
    raise BackendError(msg)


def dtype_code(dtype) -> int:
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return LSSVM_DTYPE_F32
    if dtype == np.float64:
        return LSSVM_DTYPE_F64
    raise InvalidParameterError(f"real_type must be float32 or float64, not {dtype}")


def ctype_of(dtype):
    return C.c_float if np.dtype(dtype) == np.float32 else C.c_double


def suffix_of(dtype) -> str:
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def device_count() -> int:
    return int(lib.lssvm_mi355_device_count())


def device_name(device: int = 0) -> str:
    buf = C.create_string_buffer(256)
    check(lib.lssvm_mi355_device_name(C.c_int(device), buf, C.c_size_t(256)))
    return buf.value.decode()


ABI_VERSION = 4
LSSVM_IPC_BLOB_BYTES = 256
# every tuning knob of lssvm_mi355_set_option (include/plssvm_amd.h)
OPTION_NAMES = ["rbf_form", "rbf_fold", "j_chunk_tiles", "j_chunk_head", "symmetric", "tile_kernel", "gram_mode", "mfma_shape", "colslab_band_mb", "colslab_limit_mb", "force_collective", "skip_collective",
                "exchange", "ipc_timeout_s", "enqueue_ahead_below_us", "rebalance_after"]
# accepted with the value 0 everywhere, with other values in development builds only (make DEV=1 / -DLSSVM_ENABLE_ABLATION)
DEV_OPTION_NAMES = ["pair_lag", "debug_ablate", "item_order_dev"]


def int_array(values):
    """A C ``int[]`` (or NULL for None) for the device lists of the ``_multi`` entry points."""
    if values is None:
        return None, 0
    values = [int(v) for v in values]
    return (C.c_int * len(values))(*values), len(values)


def shard_blocks(num_points: int, world: int, rank: int, symmetric: bool):
    """The library's own row-block partition (host only): ``(block_begin, block_end)`` of shard ``rank``."""
    b, e = C.c_int64(0), C.c_int64(0)
    check(lib.lssvm_mi355_shard_blocks(C.c_size_t(num_points), C.c_int(world), C.c_int(rank), C.c_int(1 if symmetric else 0), C.byref(b), C.byref(e)))
    return int(b.value), int(e.value)


def set_shard_weights(weights=None) -> None:
    """Shares of the triangle's area per rank of a sharded symmetric problem (``None`` / empty: equal shares) -- a process-wide default, snapshotted when a
    problem is created; every rank must set the same list (``lssvm_mi355_set_shard_weights``)."""
    w = [float(v) for v in (weights or [])]
    arr = (C.c_double * len(w))(*w) if w else None
    check(lib.lssvm_mi355_set_shard_weights(arr, C.c_int(len(w))))


class Options:
    """``lssvm_mi355_options`` (ABI 4): the tuning knobs held by ONE caller instead of the process -- a private copy of the process defaults of the moment it is
    created, changed with :meth:`set`, handed to the entry points that create a problem (``options=`` of ``plssvm_amd.backend``)."""

    def __init__(self, **values):
        self._h = C.c_void_p(None)
        check(lib.lssvm_mi355_options_create(C.byref(self._h)))
        for name, value in values.items():
            self.set(name, value)

    def set(self, name: str, value: int) -> "Options":
        check(lib.lssvm_mi355_options_set(self._h, name.encode(), C.c_int64(int(value))))
        return self

    def get(self, name: str) -> int:
        v = C.c_int64(0)
        check(lib.lssvm_mi355_options_get(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def close(self):
        if self._h:
            lib.lssvm_mi355_options_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def options_ptr(options):
    """The ``const lssvm_mi355_options *`` argument: NULL (= the process defaults) for None."""
    if options is None:
        return None
    if not isinstance(options, Options):
        raise InvalidParameterError("options must be a plssvm_amd._capi.Options or None")
    return options._h


def set_option(name: str, value: int) -> None:
    check(lib.lssvm_mi355_set_option(name.encode(), C.c_int64(value)))


def get_option(name: str) -> int:
    v = C.c_int64(0)
    check(lib.lssvm_mi355_get_option(name.encode(), C.byref(v)))
    return int(v.value)
