/*
 * capi.hip -- the extern "C" surface of libplssvm_amd.so (declared in include/plssvm_amd.h).
 * No exception crosses this boundary: every entry point maps lssvm::Error / std::exception to a negative status and
 * stores the message in a thread-local string (lssvm_mi355_last_error).
 */
#include "lssvm_problem.hip.hpp"
#include "lssvm_dense.hip.hpp"

#include <dlfcn.h>
#include <cstdlib>
#include <memory>
#include <new>

/* the options of one caller (ABI 4): a private copy of the tuning knobs */
struct lssvm_mi355_options {
    lssvm::Options o;
};

namespace {

using lssvm::guarded;

/* the options by name: ONE rule book for the process defaults (lssvm_mi355_set_option) and for a caller's own object (lssvm_mi355_options_set) */
void set_option_in(lssvm::Options &o, const char *name, int64_t value) {
    const std::string n(name);
    if (n == "rbf_form") {
        LSSVM_REQUIRE(value >= 0 && value <= 3, "rbf_form must be 0 (automatic), 1 (direct), 2 (matrix cores, norm expansion) or 3 (matrix cores, grid planes)");
        o.rbf_form = value;
    } else if (n == "rbf_fold") {
        o.rbf_fold = value != 0 ? 1 : 0;
    } else if (n == "j_chunk_tiles") {
        LSSVM_REQUIRE(value >= 0 && value <= (1 << 20), "j_chunk_tiles out of range");
        o.j_chunk_tiles = value;
    } else if (n == "j_chunk_head") {
        LSSVM_REQUIRE(value >= 0 && value < (1 << 20), "j_chunk_head out of range (1024 count + tiles)");
        o.j_chunk_head = value;
    } else if (n == "symmetric") {
        o.symmetric = value != 0 ? 1 : 0;
    } else if (n == "tile_kernel") {
        LSSVM_REQUIRE(value == 0 || value == 1, "tile_kernel must be 0 (automatic) or 1 (generic kernel)");
        o.tile_kernel = value;
    } else if (n == "debug_ablate") {
#ifdef LSSVM_ENABLE_ABLATION
        o.debug_ablate = value;
#else
        LSSVM_REQUIRE(value == 0, "debug_ablate exists in builds with -DLSSVM_ENABLE_ABLATION only");
#endif
    } else if (n == "force_collective") {
        o.force_collective = value != 0 ? 1 : 0;
    } else if (n == "gram_mode") {
        LSSVM_REQUIRE(value >= 0 && value <= 3, "gram_mode must be 0 (v_mfma_f32), 1 (bf16x6), 2 (f16x3 unchecked) or 3 (f16x3 where the data allows, else bf16x6)");
        o.gram_mode = value;
    } else if (n == "mfma_shape") {
        LSSVM_REQUIRE(value == 2 || value == 3, "mfma_shape must be 2 (128-row workgroups) or 3 (256-row workgroups in the symmetric variant where they apply)");
        o.mfma_shape = value;
    } else if (n == "item_order_dev") {
#ifdef LSSVM_DEV_SUBSET
        LSSVM_REQUIRE(value >= 0 && value <= 7, "item_order_dev must be 0 ... 7");
        o.item_order_dev = value;
#else
        LSSVM_REQUIRE(value == 0, "item_order_dev exists in development builds (make DEV=1) only");
#endif
    } else if (n == "pair_lag") {
#ifdef LSSVM_DEV_SUBSET
        LSSVM_REQUIRE(value >= 0 && value <= 7 && value != 2, "pair_lag must be 0, 1, 3 (steps of lag) or 4 ... 7 (priority experiments)");
        o.pair_lag = value;
#else
        LSSVM_REQUIRE(value == 0, "pair_lag exists in development builds (make DEV=1) only");
#endif
    } else if (n == "colslab_band_mb") {
        LSSVM_REQUIRE(value >= 1, "colslab_band_mb must be positive");
        o.colslab_band_mb = value;
    } else if (n == "colslab_limit_mb") {
        LSSVM_REQUIRE(value >= 0, "colslab_limit_mb must not be negative");
        o.colslab_limit_mb = value;
    } else if (n == "skip_collective") {
        o.skip_collective = value != 0 ? 1 : 0;
    } else if (n == "exchange") {
        LSSVM_REQUIRE(value >= 0 && value <= 2, "exchange must be 0 (automatic), 1 (RCCL) or 2 (peer kernels)");
        o.exchange = value;
    } else if (n == "ipc_timeout_s") {
        LSSVM_REQUIRE(value >= 1, "ipc_timeout_s must be at least 1");
        o.ipc_timeout_s = value;
    } else if (n == "enqueue_ahead_below_us") {
        LSSVM_REQUIRE(value >= 0, "enqueue_ahead_below_us must not be negative");
        o.enqueue_ahead_below_us = value;
    } else if (n == "rebalance_after") {
        LSSVM_REQUIRE(value >= 0, "rebalance_after must not be negative");
        o.rebalance_after = value;
    } else {
        throw lssvm::Error(LSSVM_ERR_INVALID_ARGUMENT, "unknown option '" + n + "'");
    }
}
void get_option_from(const lssvm::Options &o, const char *name, int64_t *value_out) {
    const std::string n(name);
    if (n == "rbf_form") {
        *value_out = o.rbf_form;
    } else if (n == "rbf_fold") {
        *value_out = o.rbf_fold;
    } else if (n == "j_chunk_tiles") {
        *value_out = o.j_chunk_tiles;
    } else if (n == "j_chunk_head") {
        *value_out = o.j_chunk_head;
    } else if (n == "symmetric") {
        *value_out = o.symmetric;
    } else if (n == "tile_kernel") {
        *value_out = o.tile_kernel;
    } else if (n == "debug_ablate") {
        *value_out = o.debug_ablate;
    } else if (n == "force_collective") {
        *value_out = o.force_collective;
    } else if (n == "gram_mode") {
        *value_out = o.gram_mode;
    } else if (n == "mfma_shape") {
        *value_out = o.mfma_shape;
    } else if (n == "item_order_dev") {
        *value_out = o.item_order_dev;
    } else if (n == "pair_lag") {
        *value_out = o.pair_lag;
    } else if (n == "colslab_band_mb") {
        *value_out = o.colslab_band_mb;
    } else if (n == "colslab_limit_mb") {
        *value_out = o.colslab_limit_mb;
    } else if (n == "skip_collective") {
        *value_out = o.skip_collective;
    } else if (n == "exchange") {
        *value_out = o.exchange;
    } else if (n == "ipc_timeout_s") {
        *value_out = o.ipc_timeout_s;
    } else if (n == "enqueue_ahead_below_us") {
        *value_out = o.enqueue_ahead_below_us;
    } else if (n == "rebalance_after") {
        *value_out = o.rebalance_after;
    } else {
        throw lssvm::Error(LSSVM_ERR_INVALID_ARGUMENT, "unknown option '" + n + "'");
    }
}

/* the options a call runs with: the caller's object, or a snapshot of the process defaults */
lssvm::Options options_of(const lssvm_mi355_options *options) { return options != nullptr ? options->o : lssvm::options_snapshot(); }

struct Handle {
    std::unique_ptr<lssvm::ProblemBase> impl;
};

lssvm::ProblemBase *impl_of(lssvm_mi355_problem *p) {
    LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
    return reinterpret_cast<Handle *>(p)->impl.get();
}

template <typename T>
void solve_one_shot(const lssvm_params *params, const T *X, size_t N, size_t d, const T *y, T eps, uint64_t max_iter, T *alpha_out, T *rho_out, lssvm_cg_info *info,
                    const int *devices, int num_devices, const lssvm_mi355_options *options, const double *weights = nullptr) {
    lssvm::check_params(params);
    LSSVM_REQUIRE(X != nullptr && N > 0, "The data must not be empty!");                                                                  // csvm.cpp:73
    LSSVM_REQUIRE(d > 0, "The data points must contain at least one feature!");                                                           // csvm.cpp:74
    LSSVM_REQUIRE(y != nullptr, "The number of data points in the matrix A and the values in the right hand side vector must be the same!");  // csvm.cpp:76
    LSSVM_REQUIRE(eps > T(0), "The stopping criterion in the CG algorithm must be greater than 0.0, but is " + std::to_string(eps) + "!");  // csvm.cpp:77
    LSSVM_REQUIRE(max_iter > 0, "The number of CG iterations must be greater than 0!");                                                   // csvm.cpp:78
    LSSVM_REQUIRE(alpha_out != nullptr && rho_out != nullptr, "alpha_out / rho_out must not be NULL");
    if (weights != nullptr) lssvm::check_weights<T>(weights, N, params->cost);  // (before any device is touched)
    const lssvm::Options opt = options_of(options);
    lssvm::Solver<T> prob(opt, *params, X, LSSVM_MEM_HOST, N, d, lssvm::resolve_devices(devices, num_devices, N), nullptr);
    if (weights != nullptr) prob.set_weights(weights, N);
    prob.cg_begin(y, static_cast<double>(eps));
    // option rebalance_after (several devices, symmetric variant): the first iterations measure every shard's pace, then the shares follow it (lssvm_mi355_problem_rebalance)
    const uint64_t first = static_cast<uint64_t>(opt.rebalance_after);
    if (first > 0 && first < max_iter) {
        prob.cg_step(first, nullptr);
        (void) prob.rebalance(nullptr, 0);
        prob.cg_step(max_iter - first, nullptr);
    } else {
        prob.cg_step(max_iter, nullptr);
    }
    double rho = 0.0;
    lssvm_cg_info local{};
    prob.cg_finish(alpha_out, &rho, &local);
    local.max_iterations = max_iter;
    *rho_out = static_cast<T>(rho);
    if (info != nullptr) *info = local;
}

/* what the one-shot entry points ask of the data before a device is touched */
void check_data(const void *X, size_t N, size_t d) {
    LSSVM_REQUIRE(X != nullptr && N > 0, "The data must not be empty!");         // csvm.cpp:73
    LSSVM_REQUIRE(d > 0, "The data points must contain at least one feature!");  // csvm.cpp:74
}

/* the problem of a one-shot entry point that runs on device 0 alone (the cost path, PCG, the fixed-size fits); the caller has made every check that needs no device */
template <typename T>
lssvm::Solver<T> device0_solver(const lssvm_mi355_options *options, const lssvm_params &params, const T *X, size_t N, size_t d) {
    static const int device0 = 0;
    return lssvm::Solver<T>(options_of(options), params, X, LSSVM_MEM_HOST, N, d, lssvm::resolve_devices(&device0, 1, N), nullptr);
}

/* lssvm_mi355_solve_cost_path_*: every argument is checked before a device is touched; the problem is created at the first cost (the path ignores it) */
template <typename T>
void cost_path_one_shot(const lssvm_params *params, const T *X, size_t N, size_t d, const T *y, const double *costs, size_t num_costs, double eps, uint64_t max_iter, int verify,
                        T *alphas_out, double *rhos_out, lssvm_path_info *infos_out, uint64_t *passes_out, const lssvm_mi355_options *options) {
    LSSVM_REQUIRE(params != nullptr, "params must not be NULL!");
    lssvm::check_cost_path_arguments(y, costs, num_costs, eps, max_iter, alphas_out, rhos_out, infos_out);
    lssvm_params with_cost = *params;
    with_cost.cost = costs[0];
    lssvm::check_params(&with_cost);
    check_data(X, N, d);
    lssvm::Solver<T> prob = device0_solver<T>(options, with_cost, X, N, d);
    prob.solve_cost_path(y, costs, num_costs, eps, max_iter, verify != 0, alphas_out, rhos_out, infos_out, passes_out);
}

/* lssvm_mi355_solve_pcg_*: every argument that needs no device is checked before one is touched; problem, preconditioner and solves on device 0 */
template <typename T>
void pcg_one_shot(const lssvm_params *params, const T *X, size_t N, size_t d, const T *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, double eps, uint64_t max_iter,
                  T *alphas_out, double *rhos_out, lssvm_pcg_info *infos_out, const lssvm_mi355_options *options) {
    lssvm::check_params(params);
    lssvm::check_pcg_arguments(Y, num_rhs, eps, max_iter, alphas_out, rhos_out, infos_out);
    check_data(X, N, d);
    lssvm::check_precond_rank(rank, N);
    lssvm::Solver<T> prob = device0_solver<T>(options, *params, X, N, d);
    prob.build_preconditioner(rank, landmarks, nullptr);
    prob.solve_pcg(Y, num_rhs, eps, max_iter, alphas_out, rhos_out, infos_out);
}

/* lssvm_mi355_fit_reduced_*: every argument that needs no device is checked before one is touched; problem and fit on device 0 */
template <typename T>
void fit_reduced_one_shot(const lssvm_params *params, const T *X, size_t N, size_t d, const T *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows,
                          double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_info *info, const lssvm_mi355_options *options, bool on_device = false,
                          lssvm_dense_info *dense = nullptr, const double *weights = nullptr) {
    lssvm::check_params(params);
    check_data(X, N, d);
    lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, N);
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    if (landmarks != nullptr) (void) lssvm::resolve_landmarks(landmarks, static_cast<size_t>(rank), N);
    if (weights != nullptr) (void) lssvm::check_reduced_weights(weights, N);
    lssvm::Solver<T> prob = device0_solver<T>(options, *params, X, N, d);
    if (on_device) {
        prob.fit_reduced_dev(Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info, dense, weights);
    } else {
        prob.fit_reduced(Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info, weights);
    }
}

/* lssvm_mi355_fit_reduced_logistic_*: likewise */
template <typename T>
void fit_reduced_logistic_one_shot(const lssvm_params *params, const T *X, size_t N, size_t d, const T *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks,
                                   uint64_t slab_rows, int factor, double tol, uint64_t max_iter, const double *betas0, const double *rhos0, double *betas_out, double *rhos_out,
                                   uint64_t *landmarks_out, lssvm_reduced_logistic_info *infos, const lssvm_mi355_options *options) {
    lssvm::check_params(params);
    check_data(X, N, d);
    lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, N);
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    if (landmarks != nullptr) (void) lssvm::resolve_landmarks(landmarks, static_cast<size_t>(rank), N);
    if (weights != nullptr) (void) lssvm::check_reduced_weights(weights, N);
    lssvm::check_reduced_factor(factor);
    lssvm::check_reduced_logistic_arguments(tol, max_iter, betas0, rhos0, num_rhs, rank);
    lssvm::check_reduced_logistic_labels(Y, std::is_same_v<T, float> ? LSSVM_DTYPE_F32 : LSSVM_DTYPE_F64, num_rhs, N);
    lssvm::Solver<T> prob = device0_solver<T>(options, *params, X, N, d);
    prob.fit_reduced_logistic(Y, num_rhs, weights, rank, landmarks, slab_rows, factor, tol, max_iter, betas0, rhos0, betas_out, rhos_out, landmarks_out, infos);
}

/* lssvm_mi355_fit_reduced_loo_*: likewise */
template <typename T>
void fit_reduced_loo_one_shot(const lssvm_params *params, const T *X, size_t N, size_t d, const T *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows,
                              const double *costs, size_t num_costs, double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out,
                              uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_loo_info *infos, const lssvm_mi355_options *options, bool on_device = false,
                              lssvm_dense_info *dense = nullptr, const double *weights = nullptr) {
    lssvm::check_params(params);
    check_data(X, N, d);
    lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, N);
    lssvm::check_reduced_loo_costs(costs, num_costs);
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    if (landmarks != nullptr) (void) lssvm::resolve_landmarks(landmarks, static_cast<size_t>(rank), N);
    if (weights != nullptr) (void) lssvm::check_reduced_weights(weights, N);
    lssvm::Solver<T> prob = device0_solver<T>(options, *params, X, N, d);
    if (on_device) {
        prob.fit_reduced_loo_dev(Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out, press_out, loo_errors_out, landmarks_out, infos,
                                 dense, weights);
    } else {
        prob.fit_reduced_loo(Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out, press_out, loo_errors_out, landmarks_out, infos,
                             weights);
    }
}

/* lssvm_mi355_fit_reduced_grid_*: likewise; the problem is created with the gamma of `params` (it decides how the data is held, not the fit) */
template <typename T>
void fit_reduced_grid_one_shot(const lssvm_params *params, const T *X, size_t N, size_t d, const T *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks,
                               uint64_t slab_rows, const double *gammas, size_t num_gammas, const double *costs, size_t num_costs, int factor, int product, double *betas_out,
                               double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out,
                               lssvm_reduced_grid_info *infos, lssvm_dense_info *dense, const lssvm_mi355_options *options) {
    lssvm::check_reduced_factor(factor);
    lssvm::check_params(params);
    check_data(X, N, d);
    lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, N);
    lssvm::check_reduced_loo_costs(costs, num_costs);
    lssvm::check_reduced_grid_arguments(gammas, num_gammas, num_costs, product);
    lssvm::check_reduced_grid_kernel(params->kernel_type);
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    if (landmarks != nullptr) (void) lssvm::resolve_landmarks(landmarks, static_cast<size_t>(rank), N);
    if (weights != nullptr) (void) lssvm::check_reduced_weights(weights, N);
    lssvm::Solver<T> prob = device0_solver<T>(options, *params, X, N, d);
    prob.fit_reduced_grid(Y, num_rhs, weights, rank, landmarks, slab_rows, gammas, num_gammas, costs, num_costs, factor, product, betas_out, rhos_out, leverage_out, fitted_out, loo_out,
                          press_out, loo_errors_out, landmarks_out, infos, dense);
}

/* lssvm_mi355_fit_reduced_rank_path_*: likewise */
template <typename T>
void fit_reduced_rank_path_one_shot(const lssvm_params *params, const T *X, size_t N, size_t d, const T *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks,
                                    uint64_t slab_rows, const uint64_t *ranks, size_t num_ranks, const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out,
                                    double *press_out, uint64_t *loo_errors_out, double *leverage_out, double *fitted_out, double *loo_out, uint64_t *landmarks_out,
                                    lssvm_reduced_rank_info *infos, lssvm_dense_info *dense, const lssvm_mi355_options *options) {
    lssvm::check_reduced_factor(factor);
    lssvm::check_params(params);
    check_data(X, N, d);
    lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, N);
    lssvm::check_reduced_loo_costs(costs, num_costs);
    lssvm::check_reduced_rank_list(ranks, num_ranks, rank, num_costs);
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    if (landmarks != nullptr) (void) lssvm::resolve_landmarks(landmarks, static_cast<size_t>(rank), N);
    if (weights != nullptr) (void) lssvm::check_reduced_weights(weights, N);
    lssvm::Solver<T> prob = device0_solver<T>(options, *params, X, N, d);
    prob.fit_reduced_rank_path(Y, num_rhs, weights, rank, landmarks, slab_rows, ranks, num_ranks, costs, num_costs, factor, betas_out, rhos_out, press_out, loo_errors_out, leverage_out,
                               fitted_out, loo_out, landmarks_out, infos, dense);
}

/* lssvm_mi355_select_landmarks_*: likewise */
template <typename T>
void select_landmarks_one_shot(const lssvm_params *params, const T *X, size_t N, size_t d, uint64_t rank, int method, uint64_t pool, uint64_t seed, double tol, uint64_t *landmarks_out,
                               double *trace_out, double *residual_out, lssvm_landmark_select_info *info, const lssvm_mi355_options *options) {
    lssvm::check_params(params);
    check_data(X, N, d);
    (void) lssvm::check_select_arguments(rank, method, pool, tol, landmarks_out, N);
    lssvm::Solver<T> prob = device0_solver<T>(options, *params, X, N, d);
    prob.select_landmarks(rank, method, pool, seed, tol, landmarks_out, trace_out, residual_out, info);
}

template <typename T>
void generate_q_one_shot(const lssvm_params *params, const T *X, size_t N, size_t d, T *q_out, const lssvm_mi355_options *options) {
    lssvm::check_params(params);
    LSSVM_REQUIRE(q_out != nullptr, "q_out must not be NULL");
    lssvm::Solver<T> prob(options_of(options), *params, X, LSSVM_MEM_HOST, N, d, { 0 }, nullptr);
    prob.get_q(q_out, nullptr);
}

/* the arguments of lssvm_mi355_predict_values_multi_* are checked here, before a device is touched */
template <typename T>
void predict_values_multi_checked(const lssvm_params *params, const T *sv, size_t nsv, size_t nfeat, const T *alpha, const T *rho, size_t nvec, T *w_inout, int *w_valid,
                                         const T *points, size_t npoints, T *out, lssvm_predict_info *info, const lssvm_mi355_options *options) {
    LSSVM_REQUIRE(params != nullptr, "params must not be NULL!");
    LSSVM_REQUIRE(nvec > 0, "The number of weight vectors must be greater than 0!");
    LSSVM_REQUIRE(alpha != nullptr, "The number of support vectors and number of weights must be the same!");  // csvm.cpp:192
    LSSVM_REQUIRE(rho != nullptr, "rho must hold one value per weight vector");
    LSSVM_REQUIRE(out != nullptr && w_valid != nullptr, "out / w_valid must not be NULL");
    lssvm::predict_values_multi<T>(options_of(options), *params, sv, nsv, nfeat, alpha, rho, nvec, w_inout, w_valid, points, npoints, out, info);
}

}  // namespace

extern "C" {

static_assert(sizeof(lssvm_cg_info) == 168, "lssvm_cg_info changed: bump PLSSVM_AMD_ABI_VERSION and plssvm_amd/_capi.py (LssvmCgInfo) with it");
int lssvm_mi355_abi_version(void) { return PLSSVM_AMD_ABI_VERSION; }

const char *lssvm_mi355_last_error(void) { return lssvm::last_error_message().c_str(); }

int lssvm_mi355_device_count(void) {
    int count = 0;
    const hipError_t err = hipGetDeviceCount(&count);
    if (err != hipSuccess) {
        (void) hipGetLastError();
        if (err == hipErrorNoDevice) return 0;
        lssvm::last_error_message() = std::string("hipGetDeviceCount failed: ") + hipGetErrorString(err);
        return 0;
    }
    return count;
}

int lssvm_mi355_device_name(int device, char *buf, size_t buf_len) {
    return guarded([&] {
        LSSVM_REQUIRE(buf != nullptr && buf_len > 0, "buf must not be NULL");
        lssvm::select_device_checked(device);
        hipDeviceProp_t prop{};
        LSSVM_HIP_CHECK(hipGetDeviceProperties(&prop, device));
        std::snprintf(buf, buf_len, "%s (%s), %d CUs", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    });
}

int lssvm_mi355_solve_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *y, float eps, uint64_t max_iter,
                          float *alpha_out, float *rho_out, lssvm_cg_info *info, const lssvm_mi355_options *options) {
    static const int device0 = 0;
    return guarded([&] { solve_one_shot<float>(params, X, num_points, num_features, y, eps, max_iter, alpha_out, rho_out, info, &device0, 1, options); });
}
int lssvm_mi355_solve_multi_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *y, float eps, uint64_t max_iter,
                                float *alpha_out, float *rho_out, lssvm_cg_info *info, const int *devices, int num_devices, const lssvm_mi355_options *options) {
    return guarded([&] { solve_one_shot<float>(params, X, num_points, num_features, y, eps, max_iter, alpha_out, rho_out, info, devices, num_devices, options); });
}
int lssvm_mi355_solve_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *y, double eps, uint64_t max_iter,
                          double *alpha_out, double *rho_out, lssvm_cg_info *info, const lssvm_mi355_options *options) {
    static const int device0 = 0;
    return guarded([&] { solve_one_shot<double>(params, X, num_points, num_features, y, eps, max_iter, alpha_out, rho_out, info, &device0, 1, options); });
}
int lssvm_mi355_solve_multi_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *y, double eps, uint64_t max_iter,
                                double *alpha_out, double *rho_out, lssvm_cg_info *info, const int *devices, int num_devices, const lssvm_mi355_options *options) {
    return guarded([&] { solve_one_shot<double>(params, X, num_points, num_features, y, eps, max_iter, alpha_out, rho_out, info, devices, num_devices, options); });
}

int lssvm_mi355_solve_weighted_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *y, const double *weights, float eps,
                                   uint64_t max_iter, float *alpha_out, float *rho_out, lssvm_cg_info *info, const lssvm_mi355_options *options) {
    static const int device0 = 0;
    return guarded([&] {
        LSSVM_REQUIRE(weights != nullptr, "weights must not be NULL (lssvm_mi355_solve_f32 is the unweighted solve)");
        solve_one_shot<float>(params, X, num_points, num_features, y, eps, max_iter, alpha_out, rho_out, info, &device0, 1, options, weights);
    });
}
int lssvm_mi355_solve_weighted_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *y, const double *weights, double eps,
                                   uint64_t max_iter, double *alpha_out, double *rho_out, lssvm_cg_info *info, const lssvm_mi355_options *options) {
    static const int device0 = 0;
    return guarded([&] {
        LSSVM_REQUIRE(weights != nullptr, "weights must not be NULL (lssvm_mi355_solve_f64 is the unweighted solve)");
        solve_one_shot<double>(params, X, num_points, num_features, y, eps, max_iter, alpha_out, rho_out, info, &device0, 1, options, weights);
    });
}

static_assert(sizeof(lssvm_refine_info) == 104, "lssvm_refine_info changed: plssvm_amd/_capi.py (LssvmRefineInfo) changes with it");
int lssvm_mi355_solve_refined_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights, double eps,
                                  uint64_t max_iter, double *alphas_out, double *rhos_out, lssvm_cg_info *infos_out, lssvm_refine_info *refine_out, uint64_t passes_out[2],
                                  const lssvm_mi355_options *options) {
    return guarded([&] {
        // (all before a device is touched)
        lssvm::check_params(params);
        LSSVM_REQUIRE(X != nullptr && num_points > 0, "The data must not be empty!");                                                                  // csvm.cpp:73
        LSSVM_REQUIRE(num_features > 0, "The data points must contain at least one feature!");                                                        // csvm.cpp:74
        LSSVM_REQUIRE(num_rhs > 0, "The number of right hand sides must be greater than 0!");
        LSSVM_REQUIRE(Y != nullptr, "The number of data points in the matrix A and the values in the right hand side vector must be the same!");      // csvm.cpp:76
        LSSVM_REQUIRE(eps > 0.0, "The stopping criterion in the CG algorithm must be greater than 0.0, but is " + std::to_string(eps) + "!");          // csvm.cpp:77
        LSSVM_REQUIRE(max_iter > 0, "The number of CG iterations must be greater than 0!");                                                           // csvm.cpp:78
        LSSVM_REQUIRE(alphas_out != nullptr && rhos_out != nullptr, "alpha_out / rho_out must not be NULL");
        if (weights != nullptr) lssvm::check_weights<double>(weights, num_points, params->cost);
        lssvm::solve_refined_f64(options_of(options), *params, X, num_points, num_features, Y, num_rhs, weights, eps, max_iter, alphas_out, rhos_out, infos_out, refine_out, passes_out);
    });
}

int lssvm_mi355_predict_values_f32(const lssvm_params *params, const float *sv, size_t nsv, size_t nfeat, const float *alpha, float rho, float *w_inout,
                                   int *w_valid, const float *points, size_t npoints, float *out, lssvm_predict_info *info, const lssvm_mi355_options *options) {
    return guarded([&] {
        LSSVM_REQUIRE(params != nullptr, "params must not be NULL!");
        lssvm::predict_values<float>(options_of(options), *params, sv, nsv, nfeat, alpha, rho, w_inout, w_valid, points, npoints, out, info);
    });
}
int lssvm_mi355_predict_values_f64(const lssvm_params *params, const double *sv, size_t nsv, size_t nfeat, const double *alpha, double rho, double *w_inout,
                                   int *w_valid, const double *points, size_t npoints, double *out, lssvm_predict_info *info, const lssvm_mi355_options *options) {
    return guarded([&] {
        LSSVM_REQUIRE(params != nullptr, "params must not be NULL!");
        lssvm::predict_values<double>(options_of(options), *params, sv, nsv, nfeat, alpha, rho, w_inout, w_valid, points, npoints, out, info);
    });
}

static_assert(sizeof(lssvm_predict_info) == 56, "lssvm_predict_info changed: bump PLSSVM_AMD_ABI_VERSION and plssvm_amd/_capi.py (LssvmPredictInfo) with it");
int lssvm_mi355_predict_values_multi_f32(const lssvm_params *params, const float *sv, size_t nsv, size_t nfeat, const float *alpha, const float *rho, size_t nvec, float *w_inout,
                                         int *w_valid, const float *points, size_t npoints, float *out, lssvm_predict_info *info, const lssvm_mi355_options *options) {
    return guarded([&] { predict_values_multi_checked<float>(params, sv, nsv, nfeat, alpha, rho, nvec, w_inout, w_valid, points, npoints, out, info, options); });
}
int lssvm_mi355_predict_values_multi_f64(const lssvm_params *params, const double *sv, size_t nsv, size_t nfeat, const double *alpha, const double *rho, size_t nvec, double *w_inout,
                                         int *w_valid, const double *points, size_t npoints, double *out, lssvm_predict_info *info, const lssvm_mi355_options *options) {
    return guarded([&] { predict_values_multi_checked<double>(params, sv, nsv, nfeat, alpha, rho, nvec, w_inout, w_valid, points, npoints, out, info, options); });
}

struct lssvm_mi355_predictor {
    std::unique_ptr<lssvm::PredictorBase> impl;
};
int lssvm_mi355_predictor_create(lssvm_mi355_predictor **out, const lssvm_params *params, int dtype, const void *support_vectors, size_t num_support_vectors,
                                 size_t num_features, const void *alpha, double rho, const lssvm_mi355_options *options) {
    return guarded([&] {
        LSSVM_REQUIRE(out != nullptr, "out must not be NULL");
        *out = nullptr;
        lssvm::check_params(params);
        LSSVM_REQUIRE(dtype == LSSVM_DTYPE_F32 || dtype == LSSVM_DTYPE_F64, "dtype must be LSSVM_DTYPE_F32 or LSSVM_DTYPE_F64");
        auto h = std::make_unique<lssvm_mi355_predictor>();
        h->impl = lssvm::make_predictor(options_of(options), *params, dtype, support_vectors, num_support_vectors, num_features, alpha, &rho, 1);
        *out = h.release();
    });
}
/* _create_multi, _create_resident and _create_panels: one validation, one set of error texts; `forms`: the resident forms the handle may take (lssvm::FORMS_*) */
static int create_predictor_of_vectors(lssvm_mi355_predictor **out, const lssvm_params *params, int dtype, const void *support_vectors, size_t num_support_vectors, size_t num_features,
                                       const void *alphas, const double *rhos, size_t num_vectors, const lssvm_mi355_options *options, int forms) {
    return guarded([&] {
        LSSVM_REQUIRE(out != nullptr, "out must not be NULL");
        *out = nullptr;
        lssvm::check_params(params);
        LSSVM_REQUIRE(dtype == LSSVM_DTYPE_F32 || dtype == LSSVM_DTYPE_F64, "dtype must be LSSVM_DTYPE_F32 or LSSVM_DTYPE_F64");
        LSSVM_REQUIRE(num_vectors > 0, "The number of weight vectors must be greater than 0!");
        LSSVM_REQUIRE(alphas != nullptr, "The number of support vectors and number of weights must be the same!");  // csvm.cpp:192
        LSSVM_REQUIRE(rhos != nullptr, "rhos must hold one value per weight vector");
        auto h = std::make_unique<lssvm_mi355_predictor>();
        h->impl = lssvm::make_predictor(options_of(options), *params, dtype, support_vectors, num_support_vectors, num_features, alphas, rhos, num_vectors, forms);
        *out = h.release();
    });
}
int lssvm_mi355_predictor_create_multi(lssvm_mi355_predictor **out, const lssvm_params *params, int dtype, const void *support_vectors, size_t num_support_vectors,
                                       size_t num_features, const void *alphas, const double *rhos, size_t num_vectors, const lssvm_mi355_options *options) {
    return create_predictor_of_vectors(out, params, dtype, support_vectors, num_support_vectors, num_features, alphas, rhos, num_vectors, options, lssvm::FORMS_DEFAULT);
}
int lssvm_mi355_predictor_create_resident(lssvm_mi355_predictor **out, const lssvm_params *params, int dtype, const void *support_vectors, size_t num_support_vectors,
                                          size_t num_features, const void *alphas, const double *rhos, size_t num_vectors, const lssvm_mi355_options *options) {
    return create_predictor_of_vectors(out, params, dtype, support_vectors, num_support_vectors, num_features, alphas, rhos, num_vectors, options, lssvm::FORMS_EVERY);
}
int lssvm_mi355_predictor_create_panels(lssvm_mi355_predictor **out, const lssvm_params *params, int dtype, const void *support_vectors, size_t num_support_vectors,
                                        size_t num_features, const void *alphas, const double *rhos, size_t num_vectors, const lssvm_mi355_options *options) {
    return create_predictor_of_vectors(out, params, dtype, support_vectors, num_support_vectors, num_features, alphas, rhos, num_vectors, options, lssvm::FORMS_PANELS);
}
int lssvm_mi355_predictor_predict(lssvm_mi355_predictor *predictor, const void *predict_points, int mem_kind, size_t num_predict_points, void *out, lssvm_predict_info *info) {
    return guarded([&] {
        LSSVM_REQUIRE(predictor != nullptr, "predictor handle must not be NULL");
        LSSVM_REQUIRE(mem_kind == LSSVM_MEM_HOST || mem_kind == LSSVM_MEM_DEVICE, "invalid mem_kind");
        predictor->impl->predict(predict_points, mem_kind, num_predict_points, out, info, false);
    });
}
int lssvm_mi355_predictor_predict_multi(lssvm_mi355_predictor *predictor, const void *predict_points, int mem_kind, size_t num_predict_points, void *out,
                                        lssvm_predict_info *info) {
    return guarded([&] {
        LSSVM_REQUIRE(predictor != nullptr, "predictor handle must not be NULL");
        LSSVM_REQUIRE(mem_kind == LSSVM_MEM_HOST || mem_kind == LSSVM_MEM_DEVICE, "invalid mem_kind");
        predictor->impl->predict(predict_points, mem_kind, num_predict_points, out, info, true);
    });
}
int lssvm_mi355_predictor_destroy(lssvm_mi355_predictor *predictor) {
    return guarded([&] { delete predictor; });
}

/* the reduced stream: create / destroy as the predictor; every argument that needs no device is checked before one is touched */
struct lssvm_mi355_reduced_stream {
    std::unique_ptr<lssvm::ReducedStreamBase> impl;
};
static int create_reduced_stream(lssvm_mi355_reduced_stream **out, const lssvm_params *params, int dtype, const void *landmark_rows, size_t rank, size_t num_features, size_t num_rhs,
                                 int weighted, uint64_t slab_rows, const lssvm_mi355_options *options) {
    return guarded([&] {
        LSSVM_REQUIRE(out != nullptr, "out must not be NULL");
        *out = nullptr;
        (void) options_of(options);  // (no tuning knob bears on a stream; the argument keeps the create calls alike)
        lssvm::check_reduced_stream_arguments(params, landmark_rows, rank, num_features, num_rhs, slab_rows);
        auto h = std::make_unique<lssvm_mi355_reduced_stream>();
        h->impl = lssvm::make_reduced_stream(*params, dtype, landmark_rows, rank, num_features, num_rhs, weighted != 0, slab_rows);
        *out = h.release();
    });
}
int lssvm_mi355_reduced_stream_create_f32(lssvm_mi355_reduced_stream **out, const lssvm_params *params, const float *landmark_rows, size_t rank, size_t num_features, size_t num_rhs,
                                          int weighted, uint64_t slab_rows, const lssvm_mi355_options *options) {
    return create_reduced_stream(out, params, LSSVM_DTYPE_F32, landmark_rows, rank, num_features, num_rhs, weighted, slab_rows, options);
}
int lssvm_mi355_reduced_stream_create_f64(lssvm_mi355_reduced_stream **out, const lssvm_params *params, const double *landmark_rows, size_t rank, size_t num_features, size_t num_rhs,
                                          int weighted, uint64_t slab_rows, const lssvm_mi355_options *options) {
    return create_reduced_stream(out, params, LSSVM_DTYPE_F64, landmark_rows, rank, num_features, num_rhs, weighted, slab_rows, options);
}
int lssvm_mi355_reduced_stream_update(lssvm_mi355_reduced_stream *stream, const void *X, const void *Y, const double *weights, size_t n) {
    return guarded([&] {
        LSSVM_REQUIRE(stream != nullptr, "stream handle must not be NULL");
        stream->impl->update(X, Y, weights, n);
    });
}
int lssvm_mi355_reduced_stream_solve(lssvm_mi355_reduced_stream *stream, const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out,
                                     lssvm_reduced_loo_info *infos) {
    return guarded([&] {
        LSSVM_REQUIRE(stream != nullptr, "stream handle must not be NULL");
        stream->impl->solve(costs, num_costs, factor, betas_out, rhos_out, infos);
    });
}
int lssvm_mi355_reduced_stream_loo(lssvm_mi355_reduced_stream *stream, const void *X, const void *Y, const double *weights, size_t n, double *leverage_out, double *fitted_out,
                                   double *loo_out) {
    return guarded([&] {
        LSSVM_REQUIRE(stream != nullptr, "stream handle must not be NULL");
        stream->impl->loo(X, Y, weights, n, leverage_out, fitted_out, loo_out);
    });
}
int lssvm_mi355_reduced_stream_export_state(lssvm_mi355_reduced_stream *stream, double *gram_out, double *kmm_out, uint64_t *num_points_out, uint64_t *fingerprint_out) {
    return guarded([&] {
        LSSVM_REQUIRE(stream != nullptr, "stream handle must not be NULL");
        stream->impl->export_state(gram_out, kmm_out, num_points_out, fingerprint_out);
    });
}
int lssvm_mi355_reduced_stream_merge_state(lssvm_mi355_reduced_stream *stream, const double *gram, uint64_t num_points, const uint64_t *fingerprint) {
    return guarded([&] {
        LSSVM_REQUIRE(stream != nullptr, "stream handle must not be NULL");
        stream->impl->merge_state(gram, num_points, fingerprint);
    });
}
int lssvm_mi355_reduced_stream_info(lssvm_mi355_reduced_stream *stream, lssvm_reduced_stream_info *info, double *centre_out, double *kmm_out) {
    return guarded([&] {
        LSSVM_REQUIRE(stream != nullptr, "stream handle must not be NULL");
        stream->impl->info(info, centre_out, kmm_out);
    });
}
int lssvm_mi355_reduced_stream_phi(lssvm_mi355_reduced_stream *stream, const void *X, size_t n, double *phi_out) {
    return guarded([&] {
        LSSVM_REQUIRE(stream != nullptr, "stream handle must not be NULL");
        stream->impl->phi(X, n, phi_out);
    });
}
int lssvm_mi355_reduced_stream_time_kernels(lssvm_mi355_reduced_stream *stream, const void *X, size_t n, int repeats, double *cross_ms_out, double *landmark_ms_out) {
    return guarded([&] {
        LSSVM_REQUIRE(stream != nullptr, "stream handle must not be NULL");
        stream->impl->time_kernels(X, n, repeats, cross_ms_out, landmark_ms_out);
    });
}
int lssvm_mi355_reduced_stream_destroy(lssvm_mi355_reduced_stream *stream) {
    return guarded([&] { delete stream; });
}

int lssvm_mi355_generate_q_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, float *q_out, const lssvm_mi355_options *options) {
    return guarded([&] { generate_q_one_shot<float>(params, X, num_points, num_features, q_out, options); });
}
int lssvm_mi355_generate_q_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, double *q_out, const lssvm_mi355_options *options) {
    return guarded([&] { generate_q_one_shot<double>(params, X, num_points, num_features, q_out, options); });
}

int lssvm_mi355_run_device_kernel_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *q, const float *d,
                                      float *ret_inout, float QA_cost, float add, const lssvm_mi355_options *options) {
    return guarded([&] {
        lssvm::check_params(params);
        LSSVM_REQUIRE(q != nullptr, "The q array may not be empty!");  // csvm.cpp:284
        (void) QA_cost;  // q and QA_cost are functions of (X, params); they are recomputed on the device and must agree with the caller's
        lssvm::Solver<float> prob(options_of(options), *params, X, LSSVM_MEM_HOST, num_points, num_features, { 0 }, nullptr);
        prob.matvec(d, ret_inout, static_cast<double>(add));
    });
}
int lssvm_mi355_run_device_kernel_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *q, const double *d,
                                      double *ret_inout, double QA_cost, double add, const lssvm_mi355_options *options) {
    return guarded([&] {
        lssvm::check_params(params);
        LSSVM_REQUIRE(q != nullptr, "The q array may not be empty!");
        (void) QA_cost;
        lssvm::Solver<double> prob(options_of(options), *params, X, LSSVM_MEM_HOST, num_points, num_features, { 0 }, nullptr);
        prob.matvec(d, ret_inout, add);
    });
}

int lssvm_mi355_calculate_w_f32(const float *sv, size_t nsv, size_t nfeat, const float *alpha, float *w_out) {
    return guarded([&] { lssvm::calculate_w<float>(sv, nsv, nfeat, alpha, w_out); });
}
int lssvm_mi355_calculate_w_f64(const double *sv, size_t nsv, size_t nfeat, const double *alpha, double *w_out) {
    return guarded([&] { lssvm::calculate_w<double>(sv, nsv, nfeat, alpha, w_out); });
}

int lssvm_mi355_shard_blocks(size_t num_points, int world, int rank, int symmetric, int64_t *block_begin, int64_t *block_end) {
    return guarded([&] {
        LSSVM_REQUIRE(block_begin != nullptr && block_end != nullptr, "output pointers must not be NULL");
        LSSVM_REQUIRE(num_points >= 2 && num_points < (size_t(1) << 31) - 4 * lssvm::TILE, "invalid number of data points");
        LSSVM_REQUIRE(world >= 1 && rank >= 0 && rank < world, "invalid shard descriptor");
        int b = 0, e = 0;
        const lssvm::Options opt = lssvm::options_snapshot();
        lssvm::shard_blocks(static_cast<int>((num_points - 1 + lssvm::TILE - 1) / lssvm::TILE), world, rank, symmetric != 0, b, e, &opt.shard_weights);
        *block_begin = b;
        *block_end = e;
    });
}

int lssvm_mi355_set_shard_weights(const double *weights, int count) {
    return guarded([&] {
        LSSVM_REQUIRE(count >= 0 && count <= 4096 && (count == 0 || weights != nullptr), "invalid shard weights");
        std::vector<double> w;
        for (int k = 0; k < count; ++k) {
            LSSVM_REQUIRE(std::isfinite(weights[k]) && weights[k] > 0.0, "shard weights must be positive and finite");
            w.push_back(weights[k]);
        }
        const std::lock_guard<std::mutex> lock(lssvm::options_mutex());
        lssvm::options().shard_weights = w;
    });
}

/* ---- communicator ---- */
int lssvm_mi355_comm_get_unique_id(unsigned char id_out[LSSVM_UNIQUE_ID_BYTES]) {
    return guarded([&] {
        LSSVM_REQUIRE(id_out != nullptr, "id_out must not be NULL");
        static_assert(sizeof(ncclUniqueId) == LSSVM_UNIQUE_ID_BYTES, "ncclUniqueId size changed");
        lssvm::comm_load();
        ncclUniqueId id;
        const ncclResult_t rc = lssvm::comm().pGetUniqueId(&id);
        if (rc != ncclSuccess) throw lssvm::Error(LSSVM_ERR_COMM, std::string("ncclGetUniqueId failed: ") + lssvm::comm().pGetErrorString(rc));
        std::memcpy(id_out, &id, sizeof(id));
    });
}
int lssvm_mi355_comm_init(int device, int rank, int world, const unsigned char id_in[LSSVM_UNIQUE_ID_BYTES]) {
    return guarded([&] {
        LSSVM_REQUIRE(id_in != nullptr, "id must not be NULL");
        LSSVM_REQUIRE(world >= 1 && rank >= 0 && rank < world, "invalid rank/world");
        lssvm::Comm &c = lssvm::comm();
        LSSVM_REQUIRE(c.comm == nullptr, "a communicator already exists in this process");
        lssvm::comm_load();
        lssvm::select_device_checked(device);
        ncclUniqueId id;
        std::memcpy(&id, id_in, sizeof(id));
        ncclComm_t nc = nullptr;
        const ncclResult_t rc = c.pCommInitRank(&nc, world, id, rank);
        if (rc != ncclSuccess) throw lssvm::Error(LSSVM_ERR_COMM, std::string("ncclCommInitRank failed: ") + c.pGetErrorString(rc));
        c.comm = nc;
        c.rank = rank;
        c.world = world;
        c.device = device;
    });
}
int lssvm_mi355_comm_library_path(char *buf, size_t buf_len) {
    return guarded([&] {
        LSSVM_REQUIRE(buf != nullptr && buf_len > 0, "buf must not be NULL");
        lssvm::comm_load();
        Dl_info di{};
        const char *path = dladdr(reinterpret_cast<void *>(lssvm::comm().pAllReduce), &di) != 0 && di.dli_fname != nullptr ? di.dli_fname : "";
        std::snprintf(buf, buf_len, "%s", path);
    });
}
int lssvm_mi355_comm_destroy(void) {
    return guarded([&] {
        lssvm::Comm &c = lssvm::comm();
        if (c.comm != nullptr) {
            (void) hipSetDevice(c.device);
            c.pCommDestroy(c.comm);
            c.comm = nullptr;
            c.world = 1;
            c.rank = 0;
        }
    });
}

/* ---- resident problem ---- */
int lssvm_mi355_problem_create(lssvm_mi355_problem **out, const lssvm_params *params, int dtype, const void *X, int mem_kind, size_t num_points,
                               size_t num_features, int device, const lssvm_shard *shard, const lssvm_mi355_options *options) {
    return guarded([&] {
        LSSVM_REQUIRE(out != nullptr, "out must not be NULL");
        *out = nullptr;
        lssvm::check_params(params);
        LSSVM_REQUIRE(dtype == LSSVM_DTYPE_F32 || dtype == LSSVM_DTYPE_F64, "dtype must be LSSVM_DTYPE_F32 or LSSVM_DTYPE_F64");
        auto h = std::make_unique<Handle>();
        lssvm::select_device_checked(device);
        if (dtype == LSSVM_DTYPE_F32) {
            h->impl = std::make_unique<lssvm::Solver<float>>(options_of(options), *params, X, mem_kind, num_points, num_features, std::vector<int>{ device }, shard);
        } else {
            h->impl = std::make_unique<lssvm::Solver<double>>(options_of(options), *params, X, mem_kind, num_points, num_features, std::vector<int>{ device }, shard);
        }
        *out = reinterpret_cast<lssvm_mi355_problem *>(h.release());
    });
}
int lssvm_mi355_problem_create_multi(lssvm_mi355_problem **out, const lssvm_params *params, int dtype, const void *X, int mem_kind, size_t num_points,
                                     size_t num_features, const int *devices, int num_devices, const lssvm_mi355_options *options) {
    return guarded([&] {
        LSSVM_REQUIRE(out != nullptr, "out must not be NULL");
        *out = nullptr;
        lssvm::check_params(params);
        LSSVM_REQUIRE(dtype == LSSVM_DTYPE_F32 || dtype == LSSVM_DTYPE_F64, "dtype must be LSSVM_DTYPE_F32 or LSSVM_DTYPE_F64");
        LSSVM_REQUIRE(num_points >= 2, "The data must contain at least two data points!");
        const std::vector<int> devs = lssvm::resolve_devices(devices, num_devices, num_points);
        auto h = std::make_unique<Handle>();
        if (dtype == LSSVM_DTYPE_F32) {
            h->impl = std::make_unique<lssvm::Solver<float>>(options_of(options), *params, X, mem_kind, num_points, num_features, devs, nullptr);
        } else {
            h->impl = std::make_unique<lssvm::Solver<double>>(options_of(options), *params, X, mem_kind, num_points, num_features, devs, nullptr);
        }
        *out = reinterpret_cast<lssvm_mi355_problem *>(h.release());
    });
}
int lssvm_mi355_problem_ipc_export(lssvm_mi355_problem *p, void *blob_out, size_t blob_bytes) {
    return guarded([&] { impl_of(p)->ipc_export(blob_out, blob_bytes); });
}
int lssvm_mi355_problem_ipc_connect(lssvm_mi355_problem *p, const void *blobs, size_t total_bytes) {
    return guarded([&] { impl_of(p)->ipc_connect(blobs, total_bytes); });
}
int lssvm_mi355_problem_destroy(lssvm_mi355_problem *p) {
    return guarded([&] { delete reinterpret_cast<Handle *>(p); });
}
int lssvm_mi355_problem_get_q(lssvm_mi355_problem *p, void *q_out, double *QA_cost_out) {
    return guarded([&] { impl_of(p)->get_q(q_out, QA_cost_out); });
}
int lssvm_mi355_problem_set_weights(lssvm_mi355_problem *p, const double *weights, size_t num_points) {
    return guarded([&] { impl_of(p)->set_weights(weights, num_points); });
}
int lssvm_mi355_problem_matvec(lssvm_mi355_problem *p, const void *d, void *ret_inout, double add) {
    return guarded([&] { impl_of(p)->matvec(d, ret_inout, add); });
}
int lssvm_mi355_problem_matvec_pair(lssvm_mi355_problem *p, const void *d0, const void *d1, void *ret0_inout, void *ret1_inout, double add, int *two_vector_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        LSSVM_REQUIRE(d0 != nullptr && d1 != nullptr && ret0_inout != nullptr && ret1_inout != nullptr, "The d / ret arrays may not be empty!");  // csvm.cpp:284-286
        LSSVM_REQUIRE(add == 1.0 || add == -1.0, "add must either be -1.0 or 1.0, but is " + std::to_string(add) + "!");                       // svm_kernel.cpp:28
        impl_of(p)->matvec_pair(d0, d1, ret0_inout, ret1_inout, add, two_vector_out);
    });
}
int lssvm_mi355_problem_solve_lockstep(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out, double *rhos_out,
                                       lssvm_cg_info *infos_out, uint64_t passes_out[2]) {
    return guarded([&] {
        // (before any device work; the solver repeats the tests that need the real type)
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        LSSVM_REQUIRE(num_rhs > 0, "The number of right hand sides must be greater than 0!");
        LSSVM_REQUIRE(Y != nullptr, "The number of data points in the matrix A and the values in the right hand side vector must be the same!");  // csvm.cpp:76
        LSSVM_REQUIRE(eps > 0.0, "The stopping criterion in the CG algorithm must be greater than 0.0, but is " + std::to_string(eps) + "!");      // csvm.cpp:77
        LSSVM_REQUIRE(max_iter > 0, "The number of CG iterations must be greater than 0!");                                                      // csvm.cpp:78
        LSSVM_REQUIRE(alphas_out != nullptr && rhos_out != nullptr, "alpha_out / rho_out must not be NULL");
        impl_of(p)->solve_lockstep(Y, num_rhs, eps, max_iter, alphas_out, rhos_out, infos_out, passes_out);
    });
}
static_assert(sizeof(lssvm_path_info) == 48, "lssvm_path_info changed: plssvm_amd/_capi.py (LssvmPathInfo) changes with it");
int lssvm_mi355_problem_solve_cost_path(lssvm_mi355_problem *p, const void *y, const double *costs, size_t num_costs, double eps, uint64_t max_iter, int verify, void *alphas_out,
                                        double *rhos_out, lssvm_path_info *infos_out, uint64_t passes_out[2]) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_cost_path_arguments(y, costs, num_costs, eps, max_iter, alphas_out, rhos_out, infos_out);  // (before any device work)
        impl_of(p)->solve_cost_path(y, costs, num_costs, eps, max_iter, verify != 0, alphas_out, rhos_out, infos_out, passes_out);
    });
}
int lssvm_mi355_solve_cost_path_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *y, const double *costs, size_t num_costs, double eps,
                                    uint64_t max_iter, int verify, float *alphas_out, double *rhos_out, lssvm_path_info *infos_out, uint64_t passes_out[2],
                                    const lssvm_mi355_options *options) {
    return guarded([&] { cost_path_one_shot<float>(params, X, num_points, num_features, y, costs, num_costs, eps, max_iter, verify, alphas_out, rhos_out, infos_out, passes_out, options); });
}
int lssvm_mi355_solve_cost_path_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *y, const double *costs, size_t num_costs, double eps,
                                    uint64_t max_iter, int verify, double *alphas_out, double *rhos_out, lssvm_path_info *infos_out, uint64_t passes_out[2],
                                    const lssvm_mi355_options *options) {
    return guarded([&] { cost_path_one_shot<double>(params, X, num_points, num_features, y, costs, num_costs, eps, max_iter, verify, alphas_out, rhos_out, infos_out, passes_out, options); });
}
static_assert(sizeof(lssvm_precond_info) == 40 && sizeof(lssvm_pcg_info) == 80, "lssvm_precond_info / lssvm_pcg_info changed: plssvm_amd/_capi.py (LssvmPrecondInfo, LssvmPcgInfo) changes with them");
int lssvm_mi355_problem_build_preconditioner(lssvm_mi355_problem *p, uint64_t rank, const uint64_t *landmarks, lssvm_precond_info *info) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        LSSVM_REQUIRE(rank >= 1 && rank <= static_cast<uint64_t>(lssvm::PRECOND_MAX_RANK),
                      "The rank of the preconditioner must lie in [1, " + std::to_string(lssvm::PRECOND_MAX_RANK) + "], but is " + std::to_string(rank) + "!");  // (before any device work; N: the solver)
        impl_of(p)->build_preconditioner(rank, landmarks, info);
    });
}
int lssvm_mi355_problem_precond_landmarks(lssvm_mi355_problem *p, uint64_t *out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        impl_of(p)->precond_landmarks(out);
    });
}
int lssvm_mi355_problem_precond_apply(lssvm_mi355_problem *p, const void *r, void *z_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        impl_of(p)->precond_apply(r, z_out);
    });
}
int lssvm_mi355_problem_solve_pcg(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out, double *rhos_out, lssvm_pcg_info *infos_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_pcg_arguments(Y, num_rhs, eps, max_iter, alphas_out, rhos_out, infos_out);  // (before any device work)
        impl_of(p)->solve_pcg(Y, num_rhs, eps, max_iter, alphas_out, rhos_out, infos_out);
    });
}
int lssvm_mi355_solve_pcg_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks,
                              double eps, uint64_t max_iter, float *alphas_out, double *rhos_out, lssvm_pcg_info *infos_out, const lssvm_mi355_options *options) {
    return guarded([&] { pcg_one_shot<float>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, eps, max_iter, alphas_out, rhos_out, infos_out, options); });
}
int lssvm_mi355_solve_pcg_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks,
                              double eps, uint64_t max_iter, double *alphas_out, double *rhos_out, lssvm_pcg_info *infos_out, const lssvm_mi355_options *options) {
    return guarded([&] { pcg_one_shot<double>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, eps, max_iter, alphas_out, rhos_out, infos_out, options); });
}
static_assert(sizeof(lssvm_reduced_info) == 64, "lssvm_reduced_info changed: plssvm_amd/_capi.py (LssvmReducedInfo) changes with it");
int lssvm_mi355_problem_fit_reduced(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out,
                                    uint64_t *landmarks_out, lssvm_reduced_info *info) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);  // (before any device work; N and the landmarks: the solver, before it touches the device)
        LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
        impl_of(p)->fit_reduced(Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info);
    });
}
int lssvm_mi355_problem_landmark_gram(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *gram_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);
        LSSVM_REQUIRE(gram_out != nullptr, "gram_out must not be NULL");
        impl_of(p)->landmark_gram(Y, num_rhs, rank, landmarks, slab_rows, gram_out);
    });
}
int lssvm_mi355_problem_time_gram_kernels(lssvm_mi355_problem *p, int repeats, double *parent_ms_out, double *mfma_ms_out, double *max_diff_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        impl_of(p)->time_gram_kernels(repeats, parent_ms_out, mfma_ms_out, max_diff_out);
    });
}
int lssvm_mi355_fit_reduced_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks,
                                uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_info *info, const lssvm_mi355_options *options) {
    return guarded([&] { fit_reduced_one_shot<float>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info, options); });
}
int lssvm_mi355_fit_reduced_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks,
                                uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_info *info, const lssvm_mi355_options *options) {
    return guarded([&] { fit_reduced_one_shot<double>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info, options); });
}
static_assert(sizeof(lssvm_reduced_loo_info) == 56, "lssvm_reduced_loo_info changed: plssvm_amd/_capi.py (LssvmReducedLooInfo) changes with it");
static_assert(sizeof(lssvm_landmark_select_info) == 56, "lssvm_landmark_select_info changed: plssvm_amd/_capi.py (LssvmLandmarkSelectInfo) changes with it");
int lssvm_mi355_problem_select_landmarks(lssvm_mi355_problem *p, uint64_t rank, int method, uint64_t pool, uint64_t seed, double tol, uint64_t *landmarks_out, double *trace_out,
                                         double *residual_out, lssvm_landmark_select_info *info) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        (void) lssvm::check_select_arguments(rank, method, pool, tol, landmarks_out, 0);  // (before any device work; N: the solver)
        impl_of(p)->select_landmarks(rank, method, pool, seed, tol, landmarks_out, trace_out, residual_out, info);
    });
}
int lssvm_mi355_select_landmarks_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, uint64_t rank, int method, uint64_t pool, uint64_t seed, double tol,
                                     uint64_t *landmarks_out, double *trace_out, double *residual_out, lssvm_landmark_select_info *info, const lssvm_mi355_options *options) {
    return guarded([&] { select_landmarks_one_shot<float>(params, X, num_points, num_features, rank, method, pool, seed, tol, landmarks_out, trace_out, residual_out, info, options); });
}
int lssvm_mi355_select_landmarks_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, uint64_t rank, int method, uint64_t pool, uint64_t seed, double tol,
                                     uint64_t *landmarks_out, double *trace_out, double *residual_out, lssvm_landmark_select_info *info, const lssvm_mi355_options *options) {
    return guarded([&] { select_landmarks_one_shot<double>(params, X, num_points, num_features, rank, method, pool, seed, tol, landmarks_out, trace_out, residual_out, info, options); });
}

int lssvm_mi355_problem_fit_reduced_loo(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs,
                                        double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out,
                                        uint64_t *landmarks_out, lssvm_reduced_loo_info *infos) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);  // (before any device work; N and the landmarks: the solver, before it touches the device)
        lssvm::check_reduced_loo_costs(costs, num_costs);
        LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
        impl_of(p)->fit_reduced_loo(Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out, press_out, loo_errors_out, landmarks_out, infos);
    });
}
int lssvm_mi355_fit_reduced_loo_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks,
                                    uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out,
                                    double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_loo_info *infos, const lssvm_mi355_options *options) {
    return guarded([&] {
        fit_reduced_loo_one_shot<float>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out,
                                        press_out, loo_errors_out, landmarks_out, infos, options);
    });
}
int lssvm_mi355_fit_reduced_loo_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks,
                                    uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out,
                                    double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_loo_info *infos, const lssvm_mi355_options *options) {
    return guarded([&] {
        fit_reduced_loo_one_shot<double>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out,
                                         press_out, loo_errors_out, landmarks_out, infos, options);
    });
}
/* the same six with the dense steps on the device (lssvm_dense.hip): the checks of the host forms, in their order */
static_assert(sizeof(lssvm_dense_info) == 72, "lssvm_dense_info changed: plssvm_amd/_capi.py (LssvmDenseInfo) changes with it");
int lssvm_mi355_problem_fit_reduced_dev(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out,
                                        uint64_t *landmarks_out, lssvm_reduced_info *info, lssvm_dense_info *dense) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);
        LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
        impl_of(p)->fit_reduced_dev(Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info, dense);
    });
}
int lssvm_mi355_fit_reduced_dev_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks,
                                    uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_info *info, const lssvm_mi355_options *options,
                                    lssvm_dense_info *dense) {
    return guarded([&] { fit_reduced_one_shot<float>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info, options, true, dense); });
}
int lssvm_mi355_fit_reduced_dev_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks,
                                    uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_info *info, const lssvm_mi355_options *options,
                                    lssvm_dense_info *dense) {
    return guarded([&] { fit_reduced_one_shot<double>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info, options, true, dense); });
}
int lssvm_mi355_problem_fit_reduced_loo_dev(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs,
                                            size_t num_costs, double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out,
                                            uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_loo_info *infos, lssvm_dense_info *dense) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);
        lssvm::check_reduced_loo_costs(costs, num_costs);
        LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
        impl_of(p)->fit_reduced_loo_dev(Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out, press_out, loo_errors_out, landmarks_out,
                                        infos, dense);
    });
}
int lssvm_mi355_fit_reduced_loo_dev_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, uint64_t rank,
                                        const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out, double *rhos_out, double *leverage_out,
                                        double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_loo_info *infos,
                                        const lssvm_mi355_options *options, lssvm_dense_info *dense) {
    return guarded([&] {
        fit_reduced_loo_one_shot<float>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out,
                                        press_out, loo_errors_out, landmarks_out, infos, options, true, dense);
    });
}
int lssvm_mi355_fit_reduced_loo_dev_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, uint64_t rank,
                                        const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out, double *rhos_out, double *leverage_out,
                                        double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_loo_info *infos,
                                        const lssvm_mi355_options *options, lssvm_dense_info *dense) {
    return guarded([&] {
        fit_reduced_loo_one_shot<double>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out,
                                         press_out, loo_errors_out, landmarks_out, infos, options, true, dense);
    });
}
/* the weighted forms: the checks of the unweighted forms in their order, then `factor`; the weights need N: the solver checks them before it touches
 * the device.  weights NULL: the unweighted entry point's call */
int lssvm_mi355_problem_fit_reduced_weighted(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows,
                                             int factor, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_info *info, lssvm_dense_info *dense) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);
        LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
        lssvm::check_reduced_factor(factor);
        if (factor == 1) {
            impl_of(p)->fit_reduced_dev(Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info, dense, weights);
        } else {
            impl_of(p)->fit_reduced(Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info, weights);
        }
    });
}
int lssvm_mi355_fit_reduced_weighted_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, const double *weights,
                                         uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, int factor, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                                         lssvm_reduced_info *info, lssvm_dense_info *dense, const lssvm_mi355_options *options) {
    return guarded([&] {
        lssvm::check_reduced_factor(factor);
        fit_reduced_one_shot<float>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info, options, factor == 1, dense, weights);
    });
}
int lssvm_mi355_fit_reduced_weighted_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights,
                                         uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, int factor, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                                         lssvm_reduced_info *info, lssvm_dense_info *dense, const lssvm_mi355_options *options) {
    return guarded([&] {
        lssvm::check_reduced_factor(factor);
        fit_reduced_one_shot<double>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, betas_out, rhos_out, landmarks_out, info, options, factor == 1, dense, weights);
    });
}
/* the fixed-size logistic regression (lssvm_logistic.hip): the checks of the weighted fit in their order, then tol, max_iter and the start values; the
 * weights and the labels need N: the solver checks them before it touches the device */
static_assert(sizeof(lssvm_reduced_logistic_info) == 104, "lssvm_reduced_logistic_info changed: plssvm_amd/_capi.py (LssvmReducedLogisticInfo) changes with it");
int lssvm_mi355_problem_fit_reduced_logistic(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows,
                                             int factor, double tol, uint64_t max_iter, const double *betas0, const double *rhos0, double *betas_out, double *rhos_out,
                                             uint64_t *landmarks_out, lssvm_reduced_logistic_info *infos) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);
        LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
        lssvm::check_reduced_factor(factor);
        lssvm::check_reduced_logistic_arguments(tol, max_iter, betas0, rhos0, num_rhs, rank);
        impl_of(p)->fit_reduced_logistic(Y, num_rhs, weights, rank, landmarks, slab_rows, factor, tol, max_iter, betas0, rhos0, betas_out, rhos_out, landmarks_out, infos);
    });
}
int lssvm_mi355_fit_reduced_logistic_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, const double *weights,
                                         uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, int factor, double tol, uint64_t max_iter, const double *betas0,
                                         const double *rhos0, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_logistic_info *infos,
                                         const lssvm_mi355_options *options) {
    return guarded([&] {
        fit_reduced_logistic_one_shot<float>(params, X, num_points, num_features, Y, num_rhs, weights, rank, landmarks, slab_rows, factor, tol, max_iter, betas0, rhos0, betas_out, rhos_out,
                                             landmarks_out, infos, options);
    });
}
int lssvm_mi355_fit_reduced_logistic_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights,
                                         uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, int factor, double tol, uint64_t max_iter, const double *betas0,
                                         const double *rhos0, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_logistic_info *infos,
                                         const lssvm_mi355_options *options) {
    return guarded([&] {
        fit_reduced_logistic_one_shot<double>(params, X, num_points, num_features, Y, num_rhs, weights, rank, landmarks, slab_rows, factor, tol, max_iter, betas0, rhos0, betas_out, rhos_out,
                                              landmarks_out, infos, options);
    });
}
int lssvm_mi355_problem_reduced_logistic_step(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows,
                                              const double *betas, const double *rhos, double *eta_out, double *q_out, double *z_out, double *loss_out, uint64_t *floored_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);
        impl_of(p)->reduced_logistic_step(Y, num_rhs, weights, rank, landmarks, slab_rows, betas, rhos, eta_out, q_out, z_out, loss_out, floored_out);
    });
}
int lssvm_mi355_problem_fit_reduced_loo_weighted(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows,
                                                 const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out,
                                                 double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_loo_info *infos,
                                                 lssvm_dense_info *dense) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);
        lssvm::check_reduced_loo_costs(costs, num_costs);
        LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
        lssvm::check_reduced_factor(factor);
        if (factor == 1) {
            impl_of(p)->fit_reduced_loo_dev(Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out, press_out, loo_errors_out,
                                            landmarks_out, infos, dense, weights);
        } else {
            impl_of(p)->fit_reduced_loo(Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out, press_out, loo_errors_out,
                                        landmarks_out, infos, weights);
        }
    });
}
int lssvm_mi355_fit_reduced_loo_weighted_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, const double *weights,
                                             uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, int factor, double *betas_out,
                                             double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out,
                                             uint64_t *landmarks_out, lssvm_reduced_loo_info *infos, lssvm_dense_info *dense, const lssvm_mi355_options *options) {
    return guarded([&] {
        lssvm::check_reduced_factor(factor);
        fit_reduced_loo_one_shot<float>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out,
                                        press_out, loo_errors_out, landmarks_out, infos, options, factor == 1, dense, weights);
    });
}
int lssvm_mi355_fit_reduced_loo_weighted_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights,
                                             uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, int factor, double *betas_out,
                                             double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out,
                                             uint64_t *landmarks_out, lssvm_reduced_loo_info *infos, lssvm_dense_info *dense, const lssvm_mi355_options *options) {
    return guarded([&] {
        lssvm::check_reduced_factor(factor);
        fit_reduced_loo_one_shot<double>(params, X, num_points, num_features, Y, num_rhs, rank, landmarks, slab_rows, costs, num_costs, betas_out, rhos_out, leverage_out, fitted_out, loo_out,
                                         press_out, loo_errors_out, landmarks_out, infos, options, factor == 1, dense, weights);
    });
}
/* the (gamma, cost) grid: the checks of the weighted leave-one-out form in their order, then the grid's own */
static_assert(sizeof(lssvm_reduced_grid_info) == 80, "lssvm_reduced_grid_info changed: plssvm_amd/_capi.py (LssvmReducedGridInfo) changes with it");
int lssvm_mi355_problem_fit_reduced_grid(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows,
                                         const double *gammas, size_t num_gammas, const double *costs, size_t num_costs, int factor, int product, double *betas_out, double *rhos_out,
                                         double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out,
                                         lssvm_reduced_grid_info *infos, lssvm_dense_info *dense) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);
        lssvm::check_reduced_loo_costs(costs, num_costs);
        LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
        lssvm::check_reduced_factor(factor);
        lssvm::check_reduced_grid_arguments(gammas, num_gammas, num_costs, product);
        impl_of(p)->fit_reduced_grid(Y, num_rhs, weights, rank, landmarks, slab_rows, gammas, num_gammas, costs, num_costs, factor, product, betas_out, rhos_out, leverage_out, fitted_out,
                                     loo_out, press_out, loo_errors_out, landmarks_out, infos, dense);
    });
}
int lssvm_mi355_fit_reduced_grid_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, const double *weights, uint64_t rank,
                                     const uint64_t *landmarks, uint64_t slab_rows, const double *gammas, size_t num_gammas, const double *costs, size_t num_costs, int factor, int product,
                                     double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out,
                                     uint64_t *landmarks_out, lssvm_reduced_grid_info *infos, lssvm_dense_info *dense, const lssvm_mi355_options *options) {
    return guarded([&] {
        fit_reduced_grid_one_shot<float>(params, X, num_points, num_features, Y, num_rhs, weights, rank, landmarks, slab_rows, gammas, num_gammas, costs, num_costs, factor, product, betas_out,
                                         rhos_out, leverage_out, fitted_out, loo_out, press_out, loo_errors_out, landmarks_out, infos, dense, options);
    });
}
int lssvm_mi355_fit_reduced_grid_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights, uint64_t rank,
                                     const uint64_t *landmarks, uint64_t slab_rows, const double *gammas, size_t num_gammas, const double *costs, size_t num_costs, int factor, int product,
                                     double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out,
                                     uint64_t *landmarks_out, lssvm_reduced_grid_info *infos, lssvm_dense_info *dense, const lssvm_mi355_options *options) {
    return guarded([&] {
        fit_reduced_grid_one_shot<double>(params, X, num_points, num_features, Y, num_rhs, weights, rank, landmarks, slab_rows, gammas, num_gammas, costs, num_costs, factor, product, betas_out,
                                          rhos_out, leverage_out, fitted_out, loo_out, press_out, loo_errors_out, landmarks_out, infos, dense, options);
    });
}
/* every prefix rank of one fit: the checks of the weighted leave-one-out form in their order, then the rank list */
static_assert(sizeof(lssvm_reduced_rank_info) == 72, "lssvm_reduced_rank_info changed: plssvm_amd/_capi.py (LssvmReducedRankInfo) changes with it");
int lssvm_mi355_problem_fit_reduced_rank_path(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows,
                                              const uint64_t *ranks, size_t num_ranks, const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out,
                                              double *press_out, uint64_t *loo_errors_out, double *leverage_out, double *fitted_out, double *loo_out, uint64_t *landmarks_out,
                                              lssvm_reduced_rank_info *infos, lssvm_dense_info *dense) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);
        lssvm::check_reduced_loo_costs(costs, num_costs);
        LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
        lssvm::check_reduced_factor(factor);
        lssvm::check_reduced_rank_list(ranks, num_ranks, rank, num_costs);
        impl_of(p)->fit_reduced_rank_path(Y, num_rhs, weights, rank, landmarks, slab_rows, ranks, num_ranks, costs, num_costs, factor, betas_out, rhos_out, press_out, loo_errors_out,
                                          leverage_out, fitted_out, loo_out, landmarks_out, infos, dense);
    });
}
int lssvm_mi355_fit_reduced_rank_path_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, const double *weights,
                                          uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const uint64_t *ranks, size_t num_ranks, const double *costs, size_t num_costs,
                                          int factor, double *betas_out, double *rhos_out, double *press_out, uint64_t *loo_errors_out, double *leverage_out, double *fitted_out,
                                          double *loo_out, uint64_t *landmarks_out, lssvm_reduced_rank_info *infos, lssvm_dense_info *dense, const lssvm_mi355_options *options) {
    return guarded([&] {
        fit_reduced_rank_path_one_shot<float>(params, X, num_points, num_features, Y, num_rhs, weights, rank, landmarks, slab_rows, ranks, num_ranks, costs, num_costs, factor, betas_out,
                                              rhos_out, press_out, loo_errors_out, leverage_out, fitted_out, loo_out, landmarks_out, infos, dense, options);
    });
}
int lssvm_mi355_fit_reduced_rank_path_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights,
                                          uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const uint64_t *ranks, size_t num_ranks, const double *costs, size_t num_costs,
                                          int factor, double *betas_out, double *rhos_out, double *press_out, uint64_t *loo_errors_out, double *leverage_out, double *fitted_out,
                                          double *loo_out, uint64_t *landmarks_out, lssvm_reduced_rank_info *infos, lssvm_dense_info *dense, const lssvm_mi355_options *options) {
    return guarded([&] {
        fit_reduced_rank_path_one_shot<double>(params, X, num_points, num_features, Y, num_rhs, weights, rank, landmarks, slab_rows, ranks, num_ranks, costs, num_costs, factor, betas_out,
                                               rhos_out, press_out, loo_errors_out, leverage_out, fitted_out, loo_out, landmarks_out, infos, dense, options);
    });
}
int lssvm_mi355_problem_reduced_leverage_prefix(lssvm_mi355_problem *p, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *V, const double *shift, const double *Z,
                                                size_t k, const uint64_t *ranks, size_t num_ranks, double *h_out, double *f_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        LSSVM_REQUIRE(V != nullptr && shift != nullptr && h_out != nullptr, "V / shift / h_out must not be NULL");
        lssvm::check_reduced_arguments(V, 1, rank, slab_rows, 0);
        lssvm::check_reduced_rank_list(ranks, num_ranks, rank, 1);
        impl_of(p)->reduced_leverage_prefix(rank, landmarks, slab_rows, V, shift, Z, k, ranks, num_ranks, h_out, f_out);
    });
}
int lssvm_mi355_problem_time_leverage_prefix_kernel(lssvm_mi355_problem *p, uint64_t rank, uint64_t slab_rows, size_t k, const uint64_t *ranks, size_t num_ranks, int repeats,
                                                    double *prefix_ms_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        impl_of(p)->time_leverage_prefix_kernel(rank, slab_rows, k, ranks, num_ranks, repeats, prefix_ms_out);
    });
}
int lssvm_mi355_problem_landmark_acc(lssvm_mi355_problem *p, const uint64_t *landmarks, uint64_t rank, int product, double *D_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        LSSVM_REQUIRE(D_out != nullptr, "D_out must not be NULL");
        lssvm::check_reduced_arguments(D_out, 1, rank, 0, 0);
        LSSVM_REQUIRE(product == 0 || product == 1, "product must be 0 (ordered) or 1 (matrix), but is " + std::to_string(product) + "!");
        impl_of(p)->landmark_acc(landmarks, rank, product, D_out);
    });
}
int lssvm_mi355_problem_landmark_gram_weighted(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows,
                                               double *gram_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        lssvm::check_reduced_arguments(Y, num_rhs, rank, slab_rows, 0);
        LSSVM_REQUIRE(gram_out != nullptr, "gram_out must not be NULL");
        impl_of(p)->landmark_gram(Y, num_rhs, rank, landmarks, slab_rows, gram_out, weights);
    });
}
/* the dense toolbox alone on host arrays (include/plssvm_amd_testing.h): every refusal before a device is touched */
int lssvm_mi355_dense_cholesky(const double *A, size_t m, double nu, double *L_out, uint64_t *status_out, double *ms_out) {
    return guarded([&] {
        LSSVM_REQUIRE(m >= 1 && m <= static_cast<size_t>(lssvm::DENSE_MAX_RANK), "m must lie in [1, 1024], but is " + std::to_string(m) + "!");
        LSSVM_REQUIRE(A != nullptr && L_out != nullptr && status_out != nullptr, "A / L_out / status_out must not be NULL");
        lssvm::dense_cholesky_aid(A, static_cast<int>(m), nu, L_out, status_out, ms_out);
    });
}
int lssvm_mi355_dense_solve(const double *L, size_t m, const double *B, size_t k, double *X_out, double *ms_out) {
    return guarded([&] {
        LSSVM_REQUIRE(m >= 1 && m <= static_cast<size_t>(lssvm::DENSE_MAX_RANK), "m must lie in [1, 1024], but is " + std::to_string(m) + "!");
        LSSVM_REQUIRE(k >= 1 && k <= 4096, "k must lie in [1, 4096], but is " + std::to_string(k) + "!");
        LSSVM_REQUIRE(L != nullptr && B != nullptr && X_out != nullptr, "L / B / X_out must not be NULL");
        lssvm::dense_solve_aid(L, static_cast<int>(m), B, static_cast<int>(k), X_out, ms_out);
    });
}
int lssvm_mi355_dense_invert_lower(const double *L, size_t m, double *V_out, double *ms_out) {
    return guarded([&] {
        LSSVM_REQUIRE(m >= 1 && m <= static_cast<size_t>(lssvm::DENSE_MAX_RANK), "m must lie in [1, 1024], but is " + std::to_string(m) + "!");
        LSSVM_REQUIRE(L != nullptr && V_out != nullptr, "L / V_out must not be NULL");
        lssvm::dense_invert_lower_aid(L, static_cast<int>(m), V_out, ms_out);
    });
}
int lssvm_mi355_problem_reduced_leverage(lssvm_mi355_problem *p, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *V, const double *shift, const double *B_extra, size_t k,
                                         double *h_out, double *f_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        LSSVM_REQUIRE(V != nullptr && shift != nullptr && h_out != nullptr, "V / shift / h_out must not be NULL");
        lssvm::check_reduced_arguments(V, 1, rank, slab_rows, 0);
        impl_of(p)->reduced_leverage(rank, landmarks, slab_rows, V, shift, B_extra, k, h_out, f_out);
    });
}
int lssvm_mi355_problem_time_leverage_kernel(lssvm_mi355_problem *p, uint64_t rank, uint64_t slab_rows, size_t k, int repeats, double *gram_ms_out, double *leverage_ms_out) {
    return guarded([&] {
        LSSVM_REQUIRE(p != nullptr, "problem handle must not be NULL");
        impl_of(p)->time_leverage_kernel(rank, slab_rows, k, repeats, gram_ms_out, leverage_ms_out);
    });
}
int lssvm_mi355_cg_begin(lssvm_mi355_problem *p, const void *y, double eps) {
    return guarded([&] { impl_of(p)->cg_begin(y, eps); });
}
int lssvm_mi355_cg_step(lssvm_mi355_problem *p, uint64_t iterations, int *done_out) {
    return guarded([&] { impl_of(p)->cg_step(iterations, done_out); });
}
int lssvm_mi355_cg_finish(lssvm_mi355_problem *p, void *alpha_out, double *rho_out, lssvm_cg_info *info) {
    return guarded([&] { impl_of(p)->cg_finish(alpha_out, rho_out, info); });
}
int lssvm_mi355_problem_synchronize(lssvm_mi355_problem *p) {
    return guarded([&] { impl_of(p)->synchronize(); });
}
int lssvm_mi355_problem_rebalance(lssvm_mi355_problem *p, const double *weights, int count, int *changed_out) {
    return guarded([&] {
        LSSVM_REQUIRE(count >= 0 && (weights == nullptr) == (count == 0), "weights and count go together (NULL, 0: measured shares)");
        const int changed = impl_of(p)->rebalance(weights, count);
        if (changed_out != nullptr) *changed_out = changed;
    });
}
int lssvm_mi355_problem_info(lssvm_mi355_problem *p, lssvm_cg_info *info) {
    return guarded([&] {
        LSSVM_REQUIRE(info != nullptr, "info must not be NULL");
        impl_of(p)->fill_info(info);
    });
}

int lssvm_mi355_measure_bf16_mfma_ceiling(int device, int b_from_lds, double settle_ms, double *tflops_out, double *clock_ghz_out, double *nominal_tflops_out) {
    return guarded([&] {
        LSSVM_REQUIRE(settle_ms >= 0.0 && settle_ms <= 60000.0, "settle_ms must lie in [0, 60000]");
        lssvm::measure_bf16_mfma_ceiling(device, b_from_lds, settle_ms, tflops_out, clock_ghz_out, nominal_tflops_out);
    });
}

int lssvm_mi355_set_option(const char *name, int64_t value) {
    return guarded([&] {
        LSSVM_REQUIRE(name != nullptr, "name must not be NULL");
        const std::lock_guard<std::mutex> lock(lssvm::options_mutex());
        set_option_in(lssvm::options(), name, value);
    });
}
int lssvm_mi355_get_option(const char *name, int64_t *value_out) {
    return guarded([&] {
        LSSVM_REQUIRE(name != nullptr && value_out != nullptr, "name / value_out must not be NULL");
        const std::lock_guard<std::mutex> lock(lssvm::options_mutex());
        get_option_from(lssvm::options(), name, value_out);
    });
}

/* ---- options of one caller (ABI 4) ---- */
int lssvm_mi355_options_create(lssvm_mi355_options **out) {
    return guarded([&] {
        LSSVM_REQUIRE(out != nullptr, "out must not be NULL");
        *out = new lssvm_mi355_options{ lssvm::options_snapshot() };
    });
}
int lssvm_mi355_options_set(lssvm_mi355_options *options, const char *name, int64_t value) {
    return guarded([&] {
        LSSVM_REQUIRE(options != nullptr && name != nullptr, "options / name must not be NULL");
        set_option_in(options->o, name, value);
    });
}
int lssvm_mi355_options_get(const lssvm_mi355_options *options, const char *name, int64_t *value_out) {
    return guarded([&] {
        LSSVM_REQUIRE(options != nullptr && name != nullptr && value_out != nullptr, "options / name / value_out must not be NULL");
        get_option_from(options->o, name, value_out);
    });
}
int lssvm_mi355_options_destroy(lssvm_mi355_options *options) {
    return guarded([&] { delete options; });
}

/* The process-wide option defaults can be preset from the environment, LSSVM_MI355_OPTIONS="name=value,name=value" (applied once when the
 * library is loaded; unknown names or bad values are reported on stderr and ignored): lets a whole test suite or an unmodified host
 * program run against another kernel selection. */
namespace {
struct EnvOptions {
    EnvOptions() {
        const char *env = std::getenv("LSSVM_MI355_OPTIONS");
        if (env == nullptr) return;
        std::string all(env);
        size_t pos = 0;
        while (pos < all.size()) {
            const size_t end = std::min(all.find(',', pos), all.size());
            const std::string item = all.substr(pos, end - pos);
            pos = end + 1;
            const size_t eq = item.find('=');
            if (eq == std::string::npos) continue;
            char *stop = nullptr;
            const long long value = std::strtoll(item.c_str() + eq + 1, &stop, 10);
            if (lssvm_mi355_set_option(item.substr(0, eq).c_str(), value) != LSSVM_SUCCESS) {
                std::fprintf(stderr, "libplssvm_amd: LSSVM_MI355_OPTIONS: %s\n", lssvm_mi355_last_error());
            }
        }
    }
};
const EnvOptions g_env_options;
}  // namespace

}  // extern "C"
