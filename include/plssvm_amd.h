/*
 * plssvm_amd.h -- C ABI of the MI355X-native LS-SVM Conjugate-Gradient backend (libplssvm_amd.so).
 *
 * This is the drop-in boundary for ONE path of SC-SGS/PLSSVM: the CG solve behind
 * plssvm::csvm::solve_system_of_linear_equations and the kernels it is built from.  Plain C: pointers + sizes only,
 * no C++ or torch types.  The C++ adaptor with the reference's virtual signatures lives in
 * include/plssvm_amd/csvm.hpp, the Python mirror of the reference's bindings in plssvm_amd/ (both sit ABOVE this ABI).
 *
 * Conventions
 *   - every function returns LSSVM_SUCCESS (0) or a negative lssvm_status; lssvm_mi355_last_error() returns the
 *     thread-local message of the last failure (the C++ adaptor rethrows it as plssvm::mi355::backend_exception,
 *     the counterpart of plssvm::hip::backend_exception, include/plssvm/backends/HIP/exceptions.hpp);
 *   - the caller owns every host pointer; data matrices are dense ROW-MAJOR `num_points x num_features`
 *     (the reference's std::vector<std::vector<T>> flattened, include/plssvm/csvm.hpp:188);
 *   - n = num_points - 1 is the size of the reduced system ("dept" in the reference);
 *   - `_f32` / `_f64` twins mirror the reference's float/double overload pairs (csvm.hpp:188-208);
 *   - kernel arithmetic runs ONLY on the GPU: there is no CPU fallback, a missing device is LSSVM_ERR_NO_DEVICE.
 *
 * All `file:line` citations are relative to the reference tree (SC-SGS/PLSSVM v2.0.0).
 */
#ifndef PLSSVM_AMD_H
#define PLSSVM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLSSVM_AMD_ABI_VERSION 4 /* 2: multi-device entry points (_multi), lssvm_cg_info grew local_devices / exchange; 3: lssvm_cg_info grew matvec_timed /
                                  * matvec_kernel_ms_total / rccl_nranks / rccl_rank / rccl_device / persistent_launches; 4: PER-CALL OPTIONS -- every entry point
                                  * that creates a problem takes a trailing `const lssvm_mi355_options *` (NULL = the process defaults), predict_values reports
                                  * lssvm_predict_info, lssvm_cg_info grew f16_row_rel_error, model / data file writers and the model reader, the shard-weight
                                  * entry points moved to plssvm_amd_testing.h (experimental) */

typedef enum lssvm_status {
    LSSVM_SUCCESS = 0,
    LSSVM_ERR_INVALID_ARGUMENT = -1, /* a violated precondition (the reference's PLSSVM_ASSERTs, csvm.cpp:73-78, svm_kernel.cpp:24-28) */
    LSSVM_ERR_NO_DEVICE = -2,        /* "HIP backend selected but no HIP capable devices were found!" (csvm.hip.cpp:70-72) */
    LSSVM_ERR_HIP = -3,              /* a HIP runtime call failed (PLSSVM_HIP_ERROR_CHECK, utility.hip.cpp:19-23) */
    LSSVM_ERR_COMM = -4,             /* RCCL missing or a collective failed */
    LSSVM_ERR_OUT_OF_MEMORY = -5,
    LSSVM_ERR_INTERNAL = -6
} lssvm_status;

/* plssvm::kernel_function_type (include/plssvm/kernel_function_types.hpp:31-38) */
typedef enum lssvm_kernel_type {
    LSSVM_KERNEL_LINEAR = 0,     /* u . v */
    LSSVM_KERNEL_POLYNOMIAL = 1, /* (gamma * u . v + coef0)^degree */
    LSSVM_KERNEL_RBF = 2         /* exp(-gamma * |u - v|^2) */
} lssvm_kernel_type;

/* plssvm::detail::parameter<T> (include/plssvm/parameter.hpp:156-165) with gamma ALREADY resolved
 * (the 1 / num_features default is applied by the caller exactly as csvm::fit does, csvm.hpp:303-307). */
typedef struct lssvm_params {
    int32_t kernel_type; /* lssvm_kernel_type */
    int32_t degree;      /* polynomial only */
    double gamma;        /* polynomial, rbf: must be > 0 (svm_kernel.cpp:68, :77) */
    double coef0;        /* polynomial only */
    double cost;         /* C; must be != 0 (svm_kernel.cpp:27 checks 1/C) */
} lssvm_params;

/* What the reference logs / tracks for a solve: keys cg/iterations, cg/max_iterations, cg/residuum, cg/target_residuum,
 * cg/avg_iteration_time, cg/epsilon, cg/total_runtime (csvm.cpp:167-176, csvm.hpp:318-320), plus device timings. */
typedef struct lssvm_cg_info {
    uint64_t iterations;     /* min(iter + 1, max_iter) */
    uint64_t max_iterations;
    double residuum;         /* delta = r^T r after the last iteration */
    double initial_residuum; /* delta0 */
    double target_residuum;  /* eps * eps * delta0 */
    double epsilon;
    double avg_iteration_ms; /* host wall clock per CG iteration */
    double total_ms;         /* host wall clock of begin + all steps + finish */
    double setup_ms;         /* host->device transfer of the data matrix, q vector, norms */
    double matvec_kernel_ms; /* average device time of the tile-kernel launches of ONE implicit matvec (HIP events on the solver stream): matvec_kernel_ms_total / matvec_timed */
    uint64_t matvec_launches; /* implicit matvecs enqueued since cg_begin */
    int32_t devices_used;    /* world size of the row-block sharding (1 = single GPU) */
    int32_t converged;       /* 1 if the stop test delta <= eps^2 * delta0 fired */
    int32_t symmetric;       /* 1 if the implicit matvec evaluated only the tiles on/below the diagonal (half the multiply-adds) */
    int32_t gram_mode;       /* fp32: how the Gram tiles ran: 0 = native v_mfma_f32 chains, 1 = "bf16x6" (exact 3-way bf16 split), 2 = "f16x3" (two f16 planes per operand),
                              * 3 = rbf on f16 GRID planes (three planes, six products: option rbf_form) */
    int32_t local_devices;   /* devices driven by THIS process (1 for a single GPU and for one process per GPU) */
    int32_t exchange;        /* how the partial K*v vectors were combined per matvec: 0 none, 1 RCCL (all-reduce / all-gather), 2 peer kernels over xGMI */
    int32_t tile_launches_per_matvec; /* tile-kernel launches per implicit matvec: row-block bands (option colslab_band_mb) x feature panels of a wide linear problem; matvec_kernel_ms is their SUM */
    int32_t rbf_direct;      /* fp32 rbf: 1 if the formula-exact (x_i - x_j)^2 kernel ran instead of the matrix-core norm expansion (option rbf_form) */
    double rbf_exponent_scale; /* fp32 rbf, rbf_form 0: 2 gamma log2(e) max|x - mean|^2, the quantity compared with rbf_direct_above */
    uint64_t matvec_timed;   /* of matvec_launches, the matvecs whose tile-kernel launches were bracketed by HIP events AND have been read back (short matvecs
                              * are sampled: launches 1 ... 4 and then every 8th, never the first after cg_begin) */
    double matvec_kernel_ms_total; /* summed device time of the tile-kernel launches of those matvec_timed matvecs (slowest shard of this process): differences of
                                    * (matvec_kernel_ms_total, matvec_timed) between two lssvm_mi355_problem_info calls give the average over the steps between them */
    int32_t rccl_nranks;     /* exchange == 1: ncclCommCount of the communicator the partial vectors travel over (what RCCL itself says, not what was asked for); else 0 */
    int32_t rccl_rank;       /* exchange == 1: ncclCommUserRank of this process's (first) communicator; else -1 */
    int32_t rccl_device;     /* exchange == 1: ncclCommCuDevice of that communicator; else -1 */
    int32_t persistent_launches; /* of tile_launches_per_matvec, the launches that are PERSISTENT: one workgroup per CU, the work items drawn from per-XCD counters instead of one
                                  * workgroup per item dealt by the hardware (256-row workgroups, launches of more items than CUs) */
    double f16_row_rel_error; /* fp32, gram_mode 2 / 3: what the set-up MEASURED on this data -- the largest relative error (2-norm) of a row represented as two f16 planes;
                               * mode 3 takes "f16x3" up to 2^-22 (rbf: or an absolute bound on the exponent), else "bf16x6".  -1 where the check did not run, NaN for a plane that overflows */
} lssvm_cg_info;

/* What a predict_values call reports (the reference tracks the whole call, gpu_csvm.hpp:656-730). */
typedef struct lssvm_predict_info {
    double total_ms;   /* host wall clock of the call: uploads, data preparation, the product, the read-back */
    double setup_ms;   /* ... of which before the product kernel was enqueued (uploads of both point sets, centring, norms, operand planes) */
    double kernel_ms;  /* device time of the kernel that evaluates the product (HIP events): the rectangular tile kernel, or w.x for the linear kernel;
                        * predict_values_multi: the sum over the product launches of the call */
    double rbf_exponent_scale; /* as lssvm_cg_info */
    double f16_row_rel_error;  /* as lssvm_cg_info, over support vectors and points */
    int32_t gram_mode;         /* as lssvm_cg_info */
    int32_t rbf_direct;        /* as lssvm_cg_info */
    int32_t resident;          /* lssvm_mi355_predictor_predict: 1 if the batch ran against the RESIDENT support vectors, 0 if it took the one-shot path (same result) */
    int32_t vectors_per_launch; /* lssvm_mi355_predict_values_multi_*: the largest number of weight vectors ONE launch of the product kernel evaluated (2 where the
                                 * two-vector kernel ran, 1 on the per-vector paths), lssvm_mi355_predictor_predict_multi alike; the single-vector entry points and lssvm_mi355_predictor_predict write 0 */
} lssvm_predict_info;

/* ------------------------------------------------------------------------------------------------------------------ */
/* library / device queries                                                                                           */
/* ------------------------------------------------------------------------------------------------------------------ */
int lssvm_mi355_abi_version(void);
/* number of visible HIP devices (hip::detail::get_device_count, csvm.hip.cpp:66); 0 if none, <0 on error */
int lssvm_mi355_device_count(void);
/* writes "name (gcnArchName), CUs" of `device` into buf (csvm.hip.cpp:77-81 logs the same properties) */
int lssvm_mi355_device_name(int device, char *buf, size_t buf_len);
const char *lssvm_mi355_last_error(void);

/* ------------------------------------------------------------------------------------------------------------------ */
/* options of ONE caller (ABI 4)                                                                                       */
/* ------------------------------------------------------------------------------------------------------------------ */
/* The tuning knobs listed at the end of this header, held by the caller instead of the process: a plssvm::csvm object is a move-only object whose const
 * virtuals share no state with other objects beyond `verbosity` (include/plssvm/csvm.hpp:50-83) -- two backend objects with different settings must be able to
 * solve at the same time from two threads.  `create` copies the process-wide defaults of that moment (lssvm_mi355_set_option / LSSVM_MI355_OPTIONS); `set` / `get`
 * take the names and ranges of lssvm_mi355_set_option.  Every entry point below that creates a problem takes a trailing `const lssvm_mi355_options *`:
 * NULL = a snapshot of the process defaults (the behaviour of ABI 3); the object is read during the call only and may be changed or destroyed afterwards. */
typedef struct lssvm_mi355_options lssvm_mi355_options; /* opaque */
int lssvm_mi355_options_create(lssvm_mi355_options **out);
int lssvm_mi355_options_set(lssvm_mi355_options *options, const char *name, int64_t value);
int lssvm_mi355_options_get(const lssvm_mi355_options *options, const char *name, int64_t *value_out);
int lssvm_mi355_options_destroy(lssvm_mi355_options *options);

/* ------------------------------------------------------------------------------------------------------------------ */
/* one-shot entry points: exactly what plssvm::csvm's pure virtuals need (include/plssvm/csvm.hpp:188-208)           */
/* ------------------------------------------------------------------------------------------------------------------ */

/* csvm::solve_system_of_linear_equations (csvm.hpp:188, :192; recipe: backends/OpenMP/csvm.cpp:71-183).
 * X: N x d row-major, y: N labels (+-1), alpha_out: N entries (alpha[N-1] = -sum(alpha[0..N-1))), rho_out = -bias.
 * Runs on device 0 of the calling process.  info may be NULL. */
int lssvm_mi355_solve_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *y,
                          float eps, uint64_t max_iter, float *alpha_out, float *rho_out, lssvm_cg_info *info, const lssvm_mi355_options *options);
int lssvm_mi355_solve_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *y,
                          double eps, uint64_t max_iter, double *alpha_out, double *rho_out, lssvm_cg_info *info, const lssvm_mi355_options *options);

/* The same solve on SEVERAL devices of the calling process -- what a plssvm::csvm backend needs, since the reference drives all
 * its devices from one process behind csvm::fit (gpu_csvm.hpp:283-299 device split, :574-593 per-device launches, :449-475
 * device_reduction).  The implicit matrix is row-block sharded over the devices (the data matrix is replicated), one stream per
 * device is driven by the calling thread, and the partial K*v vectors are combined once per matvec with an RCCL all-reduce
 * (ncclCommInitAll) or, option "exchange" = 2, by peer kernels over xGMI.
 *   num_devices == 0: automatic = every visible device, but at least 4096 points per device; devices must then be NULL;
 *   num_devices >= 1: devices[0..num_devices) are HIP device ordinals, or NULL for 0 .. num_devices-1.  The same ordinal may be
 *   listed several times (shards then share that device; the exchange falls back to peer kernels): how the sharded path is
 *   exercised on a single-GPU machine. */
int lssvm_mi355_solve_multi_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *y,
                                float eps, uint64_t max_iter, float *alpha_out, float *rho_out, lssvm_cg_info *info,
                                const int *devices, int num_devices, const lssvm_mi355_options *options);
int lssvm_mi355_solve_multi_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *y,
                                double eps, uint64_t max_iter, double *alpha_out, double *rho_out, lssvm_cg_info *info,
                                const int *devices, int num_devices, const lssvm_mi355_options *options);

/* WEIGHTED LS-SVM (Suykens et al. 2002; no counterpart in the reference, whose Python bindings reject class_weight and sample_weight,
 * bindings/Python/sklearn.cpp:85-86, :148-150): point i carries a weight w_i > 0 and its own regularisation 1 / (C w_i) -- the primal
 * minimises 1/2 |w|^2 + 1/2 C sum_i w_i e_i^2, the dual is [0 1^T; 1 K + diag(1 / (C w))] [b; alpha] = [0; y].  b is eliminated through the
 * last point exactly as in the unweighted solve (csvm.cpp:71-183), which leaves
 *     Abar(w)_ij = k(x_i,x_j) + delta_ij / (C w_i) + QA_cost(w) - q_i - q_j,   QA_cost(w) = k(x_N,x_N) + 1 / (C w_N);
 * q, b = y[0..n) - y[n], x0 = 1, the stop test, the refresh every 50th iteration, bias and alpha[N-1] = -sum are those of the unweighted solve.
 * Every diagonal term is formed as 1 / C is, in the real type: T(1) / (T(C) * T(w_i)).  So w == 1 gives exactly the bits of lssvm_mi355_solve_*
 * (alpha, rho, iteration count), and w == 2 exactly those of the unweighted solve at cost 2C.
 * weights: num_points entries, each finite and > 0 (and 1 / (C w_i) finite in the real type); NULL, a NaN, an inf or a weight <= 0 is
 * LSSVM_ERR_INVALID_ARGUMENT, reported before any device is touched.  Runs on device 0 of the calling process; info may be NULL. */
int lssvm_mi355_solve_weighted_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *y,
                                   const double *weights, float eps, uint64_t max_iter, float *alpha_out, float *rho_out,
                                   lssvm_cg_info *info, const lssvm_mi355_options *options);
int lssvm_mi355_solve_weighted_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *y,
                                   const double *weights, double eps, uint64_t max_iter, double *alpha_out, double *rho_out,
                                   lssvm_cg_info *info, const lssvm_mi355_options *options);

/* MIXED-PRECISION REFINEMENT (no counterpart in the reference): the fp64 system solved to the fp64 stop test, with the CG iterations run in fp32 on the
 * matrix-core kernels.  The fp64 problem supplies only the TRUE residual r = b - A x (one fp64 Gram pass per outer step); every outer step solves
 * A e = r / max|r| by the fp32 CG (x0 = 0) on the data rounded to float, to a tolerance derived from what is still missing, and accepts x + max|r| e only if
 * the true residual fell to at most half.  A step that does not (a system whose ridge lies below fp32's resolution, a non-finite inner result) is discarded,
 * and the plain fp64 CG finishes the solve from the current (x, r).  b, x0 = 1, the stop test r^T r <= eps^2 delta0 -- here on the true residual --, bias,
 * alpha[N-1] and rho are those of lssvm_mi355_solve_f64.  max_iter bounds the fp32 iterations plus the fp64 iterations of a take-over (the outer residual
 * passes do not count, as the refresh passes of the plain solve do not); a solve that exhausts it returns converged = 0 with the current x.
 * Y: num_rhs right-hand sides of N values each (one-vs-all); every one runs the scheme on its own, the outer fp64 passes of two that are due together share
 * one pass of the two-vector kernel where that applies (passes_out = {two-vector, single-vector} fp64 passes of the call), and column c of the result has the
 * bits of the call with that right-hand side alone.  weights: NULL, or num_points weights as for lssvm_mi355_solve_weighted_f64.
 * Where X does not survive the rounding to float (an entry that is not finite afterwards) or an option leaves no fp32 problem, the call IS the plain fp64
 * solve (lssvm_mi355_solve_f64 / _solve_weighted_f64, several right-hand sides: lssvm_mi355_problem_solve_lockstep) and reports refined = 0.
 * Device 0; deterministic (fixed-order reductions).  The gain grows with the iteration count; a solve of a handful of iterations has none. */
typedef struct lssvm_refine_info {
    int32_t  refined;            /* 1: the refinement ran; 0: the plain fp64 solve ran instead (see above) */
    int32_t  took_over_f64;      /* 1: a step was rejected and fp64 CG finished the solve */
    uint64_t outer_steps;        /* accepted + the rejected one */
    uint64_t inner_iterations;   /* fp32 CG iterations, all steps */
    uint64_t f64_cg_iterations;  /* of the take-over */
    uint64_t f64_passes;         /* fp64 Gram passes this right-hand side took part in (1 + outer_steps + the take-over's) */
    uint64_t f32_passes;         /* fp32 Gram passes */
    double   initial_residuum, residuum, target_residuum;  /* true fp64 r^T r */
    double   f64_ms, f32_ms, total_ms;                     /* host wall clock: fp64 passes and take-over | fp32 solves | since the call began */
    int32_t  inner_gram_mode, inner_rbf_direct;            /* what the fp32 problem chose (lssvm_cg_info) */
} lssvm_refine_info;
int lssvm_mi355_solve_refined_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features,
                                  const double *Y /* num_rhs x N */, size_t num_rhs, const double *weights /* N or NULL */,
                                  double eps, uint64_t max_iter, double *alphas_out /* num_rhs x N */, double *rhos_out,
                                  lssvm_cg_info *infos_out /* num_rhs, may be NULL */, lssvm_refine_info *refine_out /* num_rhs, may be NULL */,
                                  uint64_t passes_out[2] /* may be NULL: two-vector / single fp64 passes of the call */,
                                  const lssvm_mi355_options *options);

/* csvm::predict_values (csvm.hpp:204, :208; recipe: backends/OpenMP/csvm.cpp:188-227, HIP/predict_kernel.hip.hpp:34-117).
 * w_inout has num_features entries; *w_valid != 0 on entry means it already holds w (linear kernel only), on exit it is
 * set to 1 when w was computed (calculate_w, csvm.cpp:255-280).  out: num_predict_points decision values.  info (may be NULL): the timings of the call. */
int lssvm_mi355_predict_values_f32(const lssvm_params *params, const float *support_vectors, size_t num_support_vectors,
                                   size_t num_features, const float *alpha, float rho, float *w_inout, int *w_valid,
                                   const float *predict_points, size_t num_predict_points, float *out, lssvm_predict_info *info,
                                   const lssvm_mi355_options *options);
int lssvm_mi355_predict_values_f64(const lssvm_params *params, const double *support_vectors, size_t num_support_vectors,
                                   size_t num_features, const double *alpha, double rho, double *w_inout, int *w_valid,
                                   const double *predict_points, size_t num_predict_points, double *out, lssvm_predict_info *info,
                                   const lssvm_mi355_options *options);

/* predict_values for SEVERAL weight vectors over the same support vectors -- a one-vs-all multi-class model: classifier v is (alpha[v], rho[v]).
 * Layout: alpha is num_vectors x num_support_vectors and out is num_predict_points x num_vectors, both row-major; rho has num_vectors entries; w_inout (linear kernel
 * only) is num_vectors x num_features with ONE flag *w_valid for all of it.  Column v of out holds exactly the values lssvm_mi355_predict_values_* returns for
 * alpha[v], rho[v] (the same operations in the same order, bit for bit); what the call saves is the work that does not depend on the weight vector: both point sets
 * are uploaded and prepared once, and where the call is eligible for the rectangular 256-row kernel -- fp32, rbf / polynomial of degree 2 or 3, at most 128 features,
 * a split Gram mode, at least 64 row blocks (8065 points) to predict, rbf within the folded form's range -- one pass over the Gram tiles feeds TWO weight vectors
 * (ceil(num_vectors / 2) launches; lssvm_predict_info.vectors_per_launch == 2).  Everywhere else every vector has a product launch of its own on the shared
 * preparation (vectors_per_launch == 1).  NULL alpha / rho / out or num_vectors == 0: LSSVM_ERR_INVALID_ARGUMENT, before a device is touched. */
int lssvm_mi355_predict_values_multi_f32(const lssvm_params *params, const float *support_vectors, size_t num_support_vectors, size_t num_features,
                                         const float *alpha, const float *rho, size_t num_vectors, float *w_inout, int *w_valid,
                                         const float *predict_points, size_t num_predict_points, float *out, lssvm_predict_info *info,
                                         const lssvm_mi355_options *options);
int lssvm_mi355_predict_values_multi_f64(const lssvm_params *params, const double *support_vectors, size_t num_support_vectors, size_t num_features,
                                         const double *alpha, const double *rho, size_t num_vectors, double *w_inout, int *w_valid,
                                         const double *predict_points, size_t num_predict_points, double *out, lssvm_predict_info *info,
                                         const lssvm_mi355_options *options);

/* The same prediction with the MODEL RESIDENT in HBM across calls (no counterpart in the reference, whose predict_values uploads the support vectors on every call --
 * gpu_csvm.hpp:656-730 -- which is the whole cost of a small batch): `create` uploads the support vectors and prepares them once (centring, norms, operand planes,
 * packed records; the linear kernel: w), `predict` uploads a batch of points (host memory, num_points x num_features row-major of the predictor's dtype), prepares
 * it alike and writes num_points decision values.  fp32 rbf / polynomial models of at most 128 features run against the resident form; everything else, and any batch
 * the resident form cannot take (it lies further from the support vectors' centre than the norm expansion allows, or two f16 planes do not represent it), goes through
 * the one-shot path (a resident model keeps no host copy: its support vectors come back from HBM the first time that happens) -- the values are the same either way,
 * lssvm_predict_info.resident says which.  `mem_kind` (LSSVM_MEM_HOST / LSSVM_MEM_DEVICE, as lssvm_mi355_problem_create's) says where BOTH `predict_points` and `out`
 * live: with LSSVM_MEM_DEVICE they are memory of device 0 (e.g. torch tensors' data_ptr) and a batch crosses no PCIe at all.  Device 0, like predict_values; calls on
 * one handle are not re-entrant. */
typedef struct lssvm_mi355_predictor lssvm_mi355_predictor; /* opaque */
int lssvm_mi355_predictor_create(lssvm_mi355_predictor **out, const lssvm_params *params, int dtype, const void *support_vectors, size_t num_support_vectors,
                                 size_t num_features, const void *alpha, double rho, const lssvm_mi355_options *options);
int lssvm_mi355_predictor_predict(lssvm_mi355_predictor *predictor, const void *predict_points, int mem_kind, size_t num_predict_points, void *out, lssvm_predict_info *info);
int lssvm_mi355_predictor_destroy(lssvm_mi355_predictor *predictor);

/* The resident predictor of a ONE-VS-ALL model: num_vectors weight vectors over the same support vectors (alphas is num_vectors x num_support_vectors row-major,
 * rhos has num_vectors entries, of type double whatever the dtype).  `create_multi` prepares the support vectors once, keeps the alpha matrix in HBM and packs the
 * column records of every launch group there and then -- pairs (0,1), (2,3), ... and an odd last vector alone; the linear kernel: one w per vector --, so a batch
 * pays for its own upload and preparation (once, whatever num_vectors is) and for the product launches only.  lssvm_mi355_predictor_create is the num_vectors == 1
 * case of the same object; `destroy` is shared.
 * `predict_multi` works on any handle and writes num_predict_points x num_vectors values row-major, as lssvm_mi355_predict_values_multi_* does; column v holds
 * exactly the bits a single-vector predictor of (alphas[v], rhos[v]) with the same options returns.  Per batch the product runs on the rectangular 256-row kernel with
 * two vectors per pass under that kernel's conditions (lssvm_mi355_predict_values_multi_*), otherwise on the 128-row full-square kernels -- two vectors per pass for
 * the polynomial kernel and for rbf within the folded form's range, one per launch for rbf beyond it; lssvm_predict_info.vectors_per_launch reports the largest
 * number of vectors one product launch evaluated (2 or 1; the linear kernel: 1).  Models and batches outside the resident form (see above) go through
 * lssvm_mi355_predict_values_multi_* inside the predictor: resident == 0, the same values as that call.
 * lssvm_mi355_predictor_predict on a handle of more than one vector is LSSVM_ERR_INVALID_ARGUMENT; so are num_vectors == 0 and NULL alphas / rhos, before a
 * device is touched. */
int lssvm_mi355_predictor_create_multi(lssvm_mi355_predictor **out, const lssvm_params *params, int dtype, const void *support_vectors, size_t num_support_vectors,
                                       size_t num_features, const void *alphas, const double *rhos, size_t num_vectors, const lssvm_mi355_options *options);
int lssvm_mi355_predictor_predict_multi(lssvm_mi355_predictor *predictor, const void *predict_points, int mem_kind, size_t num_predict_points, void *out,
                                        lssvm_predict_info *info);

/* The same handle, running against a resident form WHEREVER THE LIBRARY HAS ONE: the fp32 form of `create` / `create_multi` above; in addition an fp64 form for
 * rbf / polynomial models (gamma > 0) of at most 256 padded features with tile_kernel != 1; and the fp32 form for rbf / polynomial models of MORE than 128 features,
 * as far as the one-pass split kernels reach (features padded to 64: polynomial up to 512 on f16 planes, rbf and every model on bf16 planes up to 384).
 * (`create` / `create_multi` keep their documented routing: an fp64 model of these kernels, and an fp32 model beyond 128 features, take the one-shot path there.)
 * Arguments, their validation and the error texts are those of `create_multi`, refused before a device is touched;
 * num_vectors == 1 gives the handle of one vector.  `predict`, `predict_multi` and `destroy` work on the handle as on any other.
 * The fp64 form uploads the support vectors once and prepares them as lssvm_mi355_predict_values_f64 prepares them per call (rbf: centred by their column means and
 * scaled, norms; polynomial: scaled by sqrt(gamma)), keeps the alpha matrix in HBM and packs the records of every launch group: a pair record for (0,1), (2,3), ...,
 * the single-vector record for an odd last vector.  A batch is padded, centred (with the support vectors' means), scaled and chunked as the one-shot call does it and
 * runs one launch of the full-square two-vector fp64 kernel per pair: the kernel value of an element is computed once, each vector's sums are the chains of a
 * single-vector launch.  Every value has the bits of lssvm_mi355_predict_values_f64 for that (alphas[v], rhos[v]) with the same options.  fp64 rbf has no direct
 * form and no plane check, so this form never declines a batch and keeps no host copy of the support vectors.  lssvm_predict_info.resident and .vectors_per_launch
 * report as for fp32: 2 where a pair launch ran, 1 for a `predict_multi` call of one-vector launches, 0 from `predict`.
 * The wide fp32 form prepares the support vectors as the form of `create_multi` does (centre, norms, operand planes, the records of every launch group) and declines
 * what that form declines (gram_mode 0, tile_kernel 1, rbf_form 1 / 3, exponent scales beyond the norm expansion, a batch that fails the f16 check beside f16 planes:
 * the one-shot path, resident == 0, its values).  A batch always runs on the 128-row full-square kernels, its row slabs reduced over the column chunks of the one-shot
 * call: two weight vectors per launch for the polynomial kernel and for rbf within the folded form's range, one for rbf beyond it.  Every column has the bits of a
 * single-vector handle of (alphas[v], rhos[v]); rbf values are those of lssvm_mi355_predict_values_multi_f32, polynomial values differ from it by the rounding of the
 * planes' power-of-two scale (taken from the support vectors alone here, from both sides there).
 * An fp32 model of at most 128 features gives a handle indistinguishable from a `create_multi` handle; outside all forms (fp64 beyond 256 features, fp32 beyond the
 * one-pass split kernels -- the feature-panel kernels --, tile_kernel = 1) the handle does what a `create_multi` handle does, resident == 0. */
int lssvm_mi355_predictor_create_resident(lssvm_mi355_predictor **out, const lssvm_params *params, int dtype, const void *support_vectors, size_t num_support_vectors,
                                          size_t num_features, const void *alphas, const double *rhos, size_t num_vectors, const lssvm_mi355_options *options);

/* The same handle once more, with every form of `create_resident` AND the models beyond the one-pass kernels resident on the kernels that walk feature panels inside
 * a tile: fp32 rbf / polynomial models (non-negative degree) beyond 512 padded features (384 for rbf and on bf16 planes), fp64 rbf / polynomial models (gamma > 0,
 * non-negative degree) beyond 256 -- 784-feature image data, for one.  (`create`, `create_multi` and `create_resident` keep their documented routing: such a model
 * takes the one-shot path there.)  Arguments, their validation and the error texts are those of `create_multi`, refused before a device is touched; `predict`,
 * `predict_multi` and `destroy` work on the handle as on any other.  A model that is not that wide gives a handle indistinguishable from a `create_resident` handle.
 * The fp32 panel form keeps what the wide fp32 form keeps, the planes padded to whole 128-feature panels; a batch runs on the full-square panel kernel, chunked as
 * the one-shot call chunks it.  The polynomial kernel and rbf within the folded form's range take two weight vectors per launch (vectors_per_launch == 2), rbf
 * beyond it (or with option rbf_fold = 0) one.  It declines what the wide fp32 form declines -- and a negative polynomial degree, which the panel kernels do not
 * take --: resident == 0, the one-shot call's values.  The fp64 panel form is prepared as lssvm_mi355_predict_values_f64 prepares it (padding to 64-feature panels,
 * centre, scale), takes two vectors per launch and never declines a batch.
 * Every column has the bits of a single-vector `create_panels` handle of (alphas[v], rhos[v]); fp64 and fp32 rbf values are those of
 * lssvm_mi355_predict_values_multi_*, fp32 polynomial values differ from it by the rounding of the planes' power-of-two scale, as in the wide fp32 form.
 * What the handle saves is the upload and preparation of the support vectors per call and half of the product launches of a model of several vectors; a call of one
 * weight vector on a batch of several times the support vectors' size is mostly the batch's own upload and product and gains little (README, "Wide models"). */
int lssvm_mi355_predictor_create_panels(lssvm_mi355_predictor **out, const lssvm_params *params, int dtype, const void *support_vectors, size_t num_support_vectors,
                                        size_t num_features, const void *alphas, const double *rhos, size_t num_vectors, const lssvm_mi355_options *options);

/* ------------------------------------------------------------------------------------------------------------------ */
/* fine-grained entry points for kernel-level parity tests: the protected members the reference's backend tests re-export  */
/* (tests/backends/HIP/mock_hip_csvm.hpp:22-44): generate_q, run_device_kernel, calculate_w                           */
/* ------------------------------------------------------------------------------------------------------------------ */

/* gpu_csvm::generate_q (gpu_csvm.hpp:349-384) / openmp generate_q (csvm.cpp:232-251): q_out has N-1 entries */
int lssvm_mi355_generate_q_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, float *q_out, const lssvm_mi355_options *options);
int lssvm_mi355_generate_q_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, double *q_out, const lssvm_mi355_options *options);

/* run_device_kernel (gpu_csvm.hpp:431-447 / csvm.cpp:283-306): ret[0..N-1) += add * Abar * d with
 * Abar_ij = k(x_i,x_j) + delta_ij / C + QA_cost - q_i - q_j; add must be +1 or -1 (svm_kernel.cpp:28). */
int lssvm_mi355_run_device_kernel_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features,
                                      const float *q, const float *d, float *ret_inout, float QA_cost, float add, const lssvm_mi355_options *options);
int lssvm_mi355_run_device_kernel_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features,
                                      const double *q, const double *d, double *ret_inout, double QA_cost, double add, const lssvm_mi355_options *options);

/* calculate_w (gpu_csvm.hpp:386-429 / csvm.cpp:255-280): w[f] = sum_i alpha_i * sv[i][f] */
int lssvm_mi355_calculate_w_f32(const float *support_vectors, size_t num_support_vectors, size_t num_features, const float *alpha, float *w_out);
int lssvm_mi355_calculate_w_f64(const double *support_vectors, size_t num_support_vectors, size_t num_features, const double *alpha, double *w_out);

/* ------------------------------------------------------------------------------------------------------------------ */
/* resident-problem API: what the one-shot calls are built from.  The data matrix is uploaded once and stays in HBM;  */
/* the CG recipe is split into begin / step / finish so that a caller (bench.py, a multi-rank launcher) can time the  */
/* iterations alone and can drive row-block sharding across several GPUs (one rank = one process = one GPU).          */
/* Replaces: gpu_csvm::setup_data_on_device (gpu_csvm.hpp:302-346) + the CG loop (gpu_csvm.hpp:477-654).             */
/* ------------------------------------------------------------------------------------------------------------------ */
typedef struct lssvm_mi355_problem lssvm_mi355_problem; /* opaque */

#define LSSVM_DTYPE_F32 0
#define LSSVM_DTYPE_F64 1

#define LSSVM_MEM_HOST 0   /* X points to host memory */
#define LSSVM_MEM_DEVICE 1 /* X points to memory of `device` (e.g. a torch tensor's data_ptr); it is copied into the padded layout */

/* Row-block sharding descriptor.  rank r of `world` owns a contiguous block of output rows of the
 * implicit matrix; the data matrix is replicated.  world == 1: single GPU, no communicator needed.
 * For world > 1 the ranks exchange their partial K*v once per implicit matvec: over RCCL (lssvm_mi355_comm_init on this rank first)
 * or over HIP IPC (lssvm_mi355_problem_ipc_export / _connect after the problem exists); option "exchange" selects. */
typedef struct lssvm_shard {
    int32_t rank;
    int32_t world;
} lssvm_shard;

/* Host only, no device needed: the 128-row blocks [*block_begin, *block_end) of the implicit matrix that shard `rank` of `world`
 * evaluates for a data set of `num_points` points.  symmetric != 0: only tiles on/below the diagonal are evaluated, blocks are
 * dealt by equal AREA (boundary r = round(blocks * sqrt(r / world))); else equal contiguous runs.  The partition every
 * Problem uses (plssvm_amd/sharding.py restates it for the flop accounting of bench.py). */
int lssvm_mi355_shard_blocks(size_t num_points, int world, int rank, int symmetric, int64_t *block_begin, int64_t *block_end);
/* RCCL bootstrap: rank 0 obtains a 128-byte unique id and hands it to the other ranks out of band
 * (bench.py / the Python launcher broadcast it with torch.distributed); every rank then calls comm_init.
 * One communicator per process.  Replaces the reference's host-staged device_reduction (gpu_csvm.hpp:449-475). */
#define LSSVM_UNIQUE_ID_BYTES 128
int lssvm_mi355_comm_get_unique_id(unsigned char id_out[LSSVM_UNIQUE_ID_BYTES]);
int lssvm_mi355_comm_init(int device, int rank, int world, const unsigned char id[LSSVM_UNIQUE_ID_BYTES]);
int lssvm_mi355_comm_destroy(void);

/* One process per GPU WITHOUT RCCL (option "exchange" = 2, or "exchange" = 0 and no communicator in this process): the ranks of one
 * node map each other's partial K*v vectors with HIP IPC and every rank sums (symmetric variant) or gathers (full square) them in
 * rank order with the peer kernel the single-process mode uses -- the same bits on every rank.  The ranks meet at host flags in
 * POSIX shared memory, twice per implicit matvec.  After lssvm_mi355_problem_create(..., shard) on every rank:
 *   1. every rank: lssvm_mi355_problem_ipc_export -> LSSVM_IPC_BLOB_BYTES bytes,
 *   2. the application hands every rank the blobs of ALL ranks, concatenated in rank order (bench.py: torch.distributed all_gather),
 *   3. every rank: lssvm_mi355_problem_ipc_connect.
 * HSA_ENABLE_IPC_MODE_LEGACY=0 must be set where the host driver only supports dmabuf IPC.  A rank that waits longer than option
 * "ipc_timeout_s" for its peers fails with LSSVM_ERR_COMM and makes the others fail too. */
#define LSSVM_IPC_BLOB_BYTES 256
int lssvm_mi355_problem_ipc_export(lssvm_mi355_problem *p, void *blob_out, size_t blob_bytes);
int lssvm_mi355_problem_ipc_connect(lssvm_mi355_problem *p, const void *blobs, size_t total_bytes);

/* upload X (N x d row-major, dtype per `dtype`), compute q, QA_cost and the per-row norms on `device`. */
int lssvm_mi355_problem_create(lssvm_mi355_problem **out, const lssvm_params *params, int dtype, const void *X, int mem_kind,
                               size_t num_points, size_t num_features, int device, const lssvm_shard *shard /* NULL = single GPU */, const lssvm_mi355_options *options);
/* the same on several devices of this process (see lssvm_mi355_solve_multi_*); mem_kind LSSVM_MEM_DEVICE: X may live on any of them.
 * Every lssvm_mi355_problem_* / lssvm_mi355_cg_* call below accepts the handle. */
int lssvm_mi355_problem_create_multi(lssvm_mi355_problem **out, const lssvm_params *params, int dtype, const void *X, int mem_kind,
                                     size_t num_points, size_t num_features, const int *devices, int num_devices, const lssvm_mi355_options *options);
int lssvm_mi355_problem_destroy(lssvm_mi355_problem *p);

/* read back q (N-1 entries, dtype of the problem) and QA_cost (of the weighted system where weights are set) */
int lssvm_mi355_problem_get_q(lssvm_mi355_problem *p, void *q_out, double *QA_cost_out);

/* v: num_points weights, each finite and > 0; NULL = unweighted (today's system).  Takes effect from the next
 * lssvm_mi355_cg_begin / lssvm_mi355_problem_matvec; rejected between cg_begin and cg_finish.
 * The weighted system of lssvm_mi355_solve_weighted_* (the same w == 1 guarantee), on any handle: every shard of a
 * lssvm_mi355_problem_create_multi handle takes the vector, and with one process per GPU (lssvm_shard) every rank must be given the same full vector. */
int lssvm_mi355_problem_set_weights(lssvm_mi355_problem *p, const double *weights, size_t num_points);

/* ret[0..N-1) += add * Abar * d -- Abar(w) where weights are set -- (host vectors of the problem's dtype, N-1 entries EACH: the library reads and writes exactly
 * num_points - 1 elements of both).  With sharding every rank returns the full vector. */
int lssvm_mi355_problem_matvec(lssvm_mi355_problem *p, const void *d, void *ret_inout, double add);

/* lssvm_mi355_problem_matvec for TWO vectors: ret_u[0..N-1) += add * Abar * d_u.  Each result has the bits lssvm_mi355_problem_matvec gives for that vector, whatever its
 * partner is.  *two_vector_out (may be NULL) = 1 if ONE pass over the Gram tiles served both -- fp64, one device, symmetric = 1, at most 256 features on the resident-row-panel
 * kernel; fp32, one device, symmetric = 1, 129 ... 512 features (bf16x6 planes and rbf: ... 384) on the one-pass split kernels, polynomial or rbf with folded records --
 * and 0 where the call ran two single passes (everywhere else).  Rejected between cg_begin and cg_finish. */
int lssvm_mi355_problem_matvec_pair(lssvm_mi355_problem *p, const void *d0, const void *d1, void *ret0_inout, void *ret1_inout, double add, int *two_vector_out);

/* num_rhs right-hand sides (Y: num_rhs x N row-major, the problem's dtype) on one resident problem, in LOCKSTEP: every right-hand side runs the recipe of
 * lssvm_mi355_cg_begin / _cg_step / _cg_finish, all of them advance one iteration per step, and in every step the right-hand sides still active are paired afresh so that
 * one pass over the Gram tiles serves two of them (where lssvm_mi355_problem_matvec_pair's does; an odd one takes a single-vector pass).  One that meets its stop test or
 * reaches max_iter leaves.  Row c of alphas_out (num_rhs x N), rhos_out[c] and iterations / converged / residuum / target_residuum of infos_out[c] (num_rhs entries, may
 * be NULL) are the bits of a fresh one-shot solve of right-hand side c.  Nothing is enqueued ahead of a stop test: matvec_launches of infos_out[c] is exactly
 * 1 + it + it / 50.  The time fields differ from a one-shot solve's: total_ms of infos_out[c] is the wall clock from the start of the CALL until right-hand side c left,
 * avg_iteration_ms that over its iterations, and matvec_kernel_ms the average over the passes it took part in (a two-vector pass counts in full for both).
 * passes_out (may be NULL): [0] two-vector Gram passes, [1] single-vector Gram passes.  Weights set with lssvm_mi355_problem_set_weights are honoured.  Rejected between
 * cg_begin and cg_finish.  Elsewhere -- several devices or ranks, symmetric = 0, tile_kernel = 1, fp64 on more than 256 features, fp32 outside the range
 * lssvm_mi355_problem_matvec_pair names (at most 128 features, gram_mode = 0, unfolded rbf, the panel kernels) -- the right-hand sides are solved one after the other and
 * passes_out[0] is 0. */
int lssvm_mi355_problem_solve_lockstep(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out /* num_rhs x N */,
                                       double *rhos_out, lssvm_cg_info *infos_out /* num_rhs, may be NULL */, uint64_t passes_out[2]);

/* COST PATH (no counterpart in the reference): the solutions of ONE right-hand side for EVERY cost of a grid from one multi-shift CG sequence -- one pass over the
 * Gram tiles per iteration for the whole grid instead of one per cost, as many iterations as the hardest (largest) cost alone needs.  For fixed data and kernel
 * function the cost enters the reduced system only as a shift: Abar(C) = A0 + sigma M with sigma = 1 / C, A0 v = K v + (k_NN S - q.v) 1 - S q (S = sum v) and
 * M = I + 1 1^T.  With P = M^(-1/2) = I - theta 1 1^T, theta = (1 - 1 / sqrt(N)) / (N - 1), the systems (P A0 P + sigma_s I) z_s = P b are shifted systems of one
 * matrix and one right-hand side; they share the Krylov space of the seed sigma_0 = min sigma_s, whose CG iteration (from z = 0) is run, and every other cost follows
 * by scalar recurrences and two vector updates.  x_s = P z_s; alpha_s[N-1] = -sum x_s and rho_s = -(y_N + (k_NN + sigma_s) sum x_s - q.x_s).
 * THE STOP TEST IS NOT THE ONE OF lssvm_mi355_solve_*.  Those start from x0 = 1 and stop at |r|^2 <= eps^2 |b - A 1|^2 in the plain 2-norm.  The path starts from
 * x0 = 0 and stops cost s at |P r_s|^2 <= eps^2 |P b|^2: the residual in the norm of M^-1, relative to the right-hand side in that norm.  DO NOT CARRY AN eps OVER FROM
 * lssvm_mi355_solve_*: the same eps asks the path for an accuracy that can be ORDERS OF MAGNITUDE stricter.  |b - A 1| is large where the Gram matrix has large row
 * sums, so the one-shot test is met early: measured on 50 000 x 128 rbf blobs, one-shot solves at eps 1e-3 ... 1e-6 stopped after a handful of iterations with true
 * residuals of 1e-2 ... 1 in the path's measure (above 1 at C = 0.1), where the path goes on until it reaches eps itself -- and takes a multiple of the time at the
 * same eps.  Choose the path's eps as the relative residual that is wanted; iteration counts of the two are not comparable.
 * The residual of a cost is known through the recurrence only (zeta_s^2 r^T r).  With verify != 0 the call evaluates the TRUE residual b - Abar(sigma_s) x_s of every
 * cost afterwards, one Gram pass per cost -- two costs per pass where lssvm_mi355_problem_matvec_pair has a two-vector pass -- and reports it in the same norm;
 * verified = 1 where true_residuum <= 4 target_residuum (twice the norm).  Nothing is repaired or hidden: in float, a system whose ridge lies below float's
 * resolution (the linear kernel on few features at large costs) drifts, and the caller sees converged = 1, verified = 0 and both numbers.
 * y: N values of the problem's dtype.  costs: num_costs values (1 ... 64), each finite and > 0, in any order, duplicates allowed; row s of alphas_out
 * (num_costs x N, the problem's dtype), rhos_out[s] and infos_out[s] belong to costs[s].  The cost of the problem's lssvm_params is ignored, and the problem is left
 * as it was.  passes_out (may be NULL): [0] Gram passes of the iteration (= the seed's iterations), [1] Gram passes of the verification.  Deterministic: fixed-order
 * reductions, the same bits for the same arguments, and a permuted cost list gives the permuted rows.  max_iter bounds the iterations; costs still active then come
 * back with converged = 0 and their current iterate.
 * LSSVM_ERR_INVALID_ARGUMENT: a problem on several devices or ranks, weights set on the problem, a call between cg_begin and cg_finish; and, before any device
 * work, num_costs == 0 or > 64, a cost that is not finite and > 0, eps <= 0 (or not finite), max_iter == 0, a NULL y / costs / alphas_out / rhos_out / infos_out. */
typedef struct lssvm_path_info {
    uint64_t iterations;                                   /* at which this cost froze (max_iter where it did not) */
    int32_t  converged, verified;
    double   initial_residuum, residuum, target_residuum;  /* squared, as lssvm_cg_info: |P b|^2, zeta_s^2 |r|^2 when it froze, eps^2 |P b|^2 */
    double   true_residuum;                                /* |P (b - Abar(sigma_s) x_s)|^2; -1 without verify */
} lssvm_path_info;
int lssvm_mi355_problem_solve_cost_path(lssvm_mi355_problem *p, const void *y, const double *costs, size_t num_costs, double eps, uint64_t max_iter, int verify,
                                        void *alphas_out /* num_costs x N */, double *rhos_out, lssvm_path_info *infos_out, uint64_t passes_out[2]);
/* one-shot: create the problem on device 0 (as lssvm_mi355_solve_*), solve the path, destroy it; params->cost is ignored */
int lssvm_mi355_solve_cost_path_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *y, const double *costs,
                                    size_t num_costs, double eps, uint64_t max_iter, int verify, float *alphas_out, double *rhos_out,
                                    lssvm_path_info *infos_out, uint64_t passes_out[2], const lssvm_mi355_options *options);
int lssvm_mi355_solve_cost_path_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *y, const double *costs,
                                    size_t num_costs, double eps, uint64_t max_iter, int verify, double *alphas_out, double *rhos_out,
                                    lssvm_path_info *infos_out, uint64_t passes_out[2], const lssvm_mi355_options *options);

/* Nystrom-preconditioned CG on a resident problem (opt-in).  With n = N - 1, sigma = 1 / C, E = [I_n | -1] and H = K + sigma I the reduced
 * matrix of the recipe is the congruence Abar = E H E^T.  From `rank` = m landmark points the library forms K_Nm and K_mm, factors L L^T = K_mm + nu I on the host in
 * double (nu starts at eps64 trace(K_mm) and is raised tenfold, six times at most, while the factorisation fails), B_f = K_Nm L^-T, Bhat = [E B_f | sqrt(sigma) 1]
 * (n x (m + 1), stored once in the problem's dtype) and G = Bhat^T Bhat + sigma I (double; factored and inverted on the host).  The preconditioner is
 * P = E (B_f B_f^T + sigma I) E^T = Bhat Bhat^T + sigma I, symmetric positive definite by construction, applied as z = r - Bhat G^-1 Bhat^T r = sigma P^-1 r (PCG does
 * not see the factor).  It uses the cost of the problem's lssvm_params.  It pays where the kernel matrix has spectral decay and COSTS iterations where it has none and
 * the rank is small (README.md has both kinds of row): nothing selects it automatically.
 * build_preconditioner: 1 <= rank <= min(N - 1, 512).  landmarks: `rank` distinct indices < N (the last point is allowed), or NULL for the library's choice -- the first
 * `rank` entries of a Fisher-Yates shuffle of 0 ... N-1 (for i = 0 ... rank-1: swap entry i with entry i + next() mod (N - i)), next() = splitmix64 from the state
 * 0x243F6A8885A308D3: the same landmarks for the same N.  Building again replaces the preconditioner; lssvm_mi355_problem_destroy frees it.  info may be NULL.
 * precond_landmarks: the `rank` landmarks in use.  precond_apply: host vectors of n = N - 1 entries of the problem's dtype, z = r - Bhat G^-1 Bhat^T r (the operator alone).
 * solve_pcg: the right-hand sides of Y (num_rhs x N) one after the other on the ONE preconditioner, in the frame of lssvm_mi355_solve_*: x0 = 1, r0 = b - Abar 1, stop at
 * |r|^2 <= eps^2 |r0|^2 on the unpreconditioned recurrence residual (so eps means what it means there, and iteration counts compare), the true residual every 50th
 * iteration; alpha_N and rho as lssvm_mi355_cg_finish forms them.  Row c of alphas_out (num_rhs x N), rhos_out[c], infos_out[c] belong to right-hand side c.  One Gram
 * pass per iteration (plus the refreshes); the problem is left as it was.  Deterministic: fixed-order reductions, the same bits for the same arguments.
 * LSSVM_ERR_INVALID_ARGUMENT: a problem on several devices or ranks, weights set on the problem, a call between cg_begin and cg_finish, solve_pcg / precond_apply /
 * precond_landmarks without a preconditioner; a rank outside its range, duplicate or out-of-range landmarks; eps <= 0 (or not finite), max_iter == 0, num_rhs == 0, a NULL
 * Y / alphas_out / rhos_out / infos_out / r / z_out / out.  LSSVM_ERR_INTERNAL: K_mm + nu I could not be factored. */
typedef struct lssvm_precond_info {
    uint64_t rank;
    double   jitter;           /* nu */
    double   build_ms;         /* the whole call */
    double   host_ms;          /* of which the factorisations and inverses on the host */
    uint64_t device_bytes;     /* what the preconditioner keeps in device memory */
} lssvm_precond_info;
typedef struct lssvm_pcg_info {
    uint64_t iterations, gram_passes;
    int32_t  converged, rank;
    double   initial_residuum, residuum, target_residuum;  /* squared, as lssvm_cg_info: |r0|^2, |r|^2, eps^2 |r0|^2 */
    double   jitter;           /* nu of the preconditioner */
    double   build_ms;         /* of the preconditioner in use (paid once, whatever the number of solves) */
    double   apply_ms;         /* device time of applying the preconditioner, average per iteration */
    double   total_ms;         /* this right-hand side */
} lssvm_pcg_info;
int lssvm_mi355_problem_build_preconditioner(lssvm_mi355_problem *p, uint64_t rank, const uint64_t *landmarks /* NULL: the library's choice */, lssvm_precond_info *info);
int lssvm_mi355_problem_precond_landmarks(lssvm_mi355_problem *p, uint64_t *out /* rank */);
int lssvm_mi355_problem_precond_apply(lssvm_mi355_problem *p, const void *r, void *z_out);
int lssvm_mi355_problem_solve_pcg(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out /* num_rhs x N */,
                                  double *rhos_out, lssvm_pcg_info *infos_out);
/* one-shot: create the problem on device 0 (as lssvm_mi355_solve_*), build the preconditioner (landmarks as above), solve every right-hand side, destroy it */
int lssvm_mi355_solve_pcg_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, uint64_t rank,
                              const uint64_t *landmarks, double eps, uint64_t max_iter, float *alphas_out, double *rhos_out, lssvm_pcg_info *infos_out,
                              const lssvm_mi355_options *options);
int lssvm_mi355_solve_pcg_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, uint64_t rank,
                              const uint64_t *landmarks, double eps, uint64_t max_iter, double *alphas_out, double *rhos_out, lssvm_pcg_info *infos_out,
                              const lssvm_mi355_options *options);

/* Fixed-size (reduced, "subset of regressors") LS-SVM on a resident problem (opt-in): the decision function is expanded over `rank` = m landmark
 * points only, f(x) = sum_j beta_j k(x, x_L[j]) + b, and minimises  1/2 beta^T K_mm beta + C/2 sum_i (y_i - Phi_i beta - b)^2  with Phi = K(X, X_L) (N x m, evaluated in
 * double from the problem's resident data exactly as the preconditioner above evaluates K_Nm) and K_mm = Phi[L, :].  No CG: the device forms, slab of `slab_rows` rows by
 * slab, the lower triangle of St = Pt^T Pt for Pt = [Phi | 1 | y_0 ... y_{k-1}] (N x (m + 1 + k)) on v_mfma_f64_16x16x4_f64; the host solves in double, with sigma = 1 / C,
 *   S = St[:m,:m], s = St[m,:m], t_c = St[m+1+c,:m], eta_c = St[m+1+c,m]:   M = S - s s^T / N + sigma K_mm,   (M + nu I) beta_c = t_c - s eta_c / N,
 *   b_c = (eta_c - s^T beta_c) / N,   rho_c = -b_c.
 * nu follows the preconditioner's rule on M (eps64 trace(M), tenfold while the factorisation fails, six times at most) and is reported as `jitter`: the conditioning of
 * M grows with the rank and is the method's limit (README.md).  One St and one factorisation serve all num_rhs right-hand sides; row c of the results has the bits of the
 * call with right-hand side c alone: the order in which an entry of St is summed depends on N and slab_rows only.  The result is an ordinary model of m support vectors
 * (the landmark rows, alpha = beta, rho); it trades accuracy for size, nothing selects it automatically.
 * rank: 1 <= rank <= min(N, 1024).  landmarks: as for the preconditioner (`rank` distinct indices < N, or NULL for the library's rule).  slab_rows: a multiple of 256,
 * 0 = the library's default (65 536); it bounds the work space (about slab_rows x (rank + 1 + num_rhs) doubles).  betas_out is DOUBLE whatever the problem's dtype (a
 * float model rounds it afterwards).  landmarks_out and info may be NULL.  It uses the cost of the problem's lssvm_params.  The problem is left as it was and keeps its
 * preconditioner.  Deterministic: fixed-order sums without atomics, the same bits for the same arguments.
 * LSSVM_ERR_INVALID_ARGUMENT, all before a device is touched: a problem on several devices or ranks, weights set on the problem, a call between cg_begin and cg_finish;
 * rank 0, beyond 1024 or beyond N; duplicate or out-of-range landmarks; slab_rows no multiple of 256; num_rhs == 0; a NULL Y / betas_out / rhos_out.
 * LSSVM_ERR_INTERNAL: M + nu I could not be factored. */
typedef struct lssvm_reduced_info {
    uint64_t rank, slabs;
    double   jitter;           /* nu */
    double   landmark_ms;      /* device time of Phi, the 1 and y columns and K_mm, all slabs */
    double   gram_ms;          /* device time of St, all slabs */
    double   host_ms;          /* the factorisation and the solves on the host */
    double   total_ms;         /* the whole call */
    uint64_t workspace_bytes;  /* device memory held during the call */
} lssvm_reduced_info;
int lssvm_mi355_problem_fit_reduced(lssvm_mi355_problem *p, const void *Y /* num_rhs x N, the problem's dtype */, size_t num_rhs, uint64_t rank,
                                    const uint64_t *landmarks /* NULL: the preconditioner's rule */, uint64_t slab_rows, double *betas_out /* num_rhs x rank */,
                                    double *rhos_out, uint64_t *landmarks_out /* rank */, lssvm_reduced_info *info);
/* one-shot: create the problem on device 0 (as lssvm_mi355_solve_*), fit, destroy it */
int lssvm_mi355_fit_reduced_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, uint64_t rank,
                                const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_info *info,
                                const lssvm_mi355_options *options);
int lssvm_mi355_fit_reduced_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, uint64_t rank,
                                const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_info *info,
                                const lssvm_mi355_options *options);

/* Exact leave-one-out scores of the fixed-size model over a grid of costs (opt-in) -- leave-one-out with the landmark set held fixed.  The fit
 * above is a linear smoother with an unpenalised intercept: with Phic = Phi - 1 s^T / N (column-centred) and M_s + nu I = L L^T, the matrix fit_reduced factors at the
 * cost C_s,
 *   h_ii = 1 / N + |L^-1 (phi_i - s / N)|^2,   f_c(x_i) = (phi_i - s / N) beta_c + eta_c / N,   f_c^(-i)(x_i) = y_ic - (y_ic - f_c(x_i)) / (1 - h_ii)
 * where f_c^(-i) is the model refitted without point i on the SAME landmarks: an identity, not an approximation.  h does not depend on y, so one leverage vector serves
 * all right-hand sides.  Pass 1 is the pass of lssvm_mi355_problem_fit_reduced; per cost the host forms M_s (the jitter rule per cost), L_s, V_s = L_s^-1 and beta, rho
 * exactly as fit_reduced does: betas and rhos of cost s have the bits of fit_reduced on a problem created with that cost.  Pass 2 evaluates the Phi slabs again (the same
 * kernels, the same bits) and per slab and cost forms the N x m x m product Phic V_s^T on v_mfma_f64_16x16x4_f64 without storing it: only its rows' squared norms, the
 * fitted values and the leave-one-out values leave the device.  No atomics; the order of every sum depends on the rank only, so h is the same to the bit for any num_rhs,
 * column c of a call has the bits of the call with that right-hand side alone, and a cost has the bits of the call with that cost alone.
 * costs: 1 <= num_costs <= 64, each finite and > 0; the cost of the problem's lssvm_params is IGNORED.  Every output is double.  betas_out: num_costs x num_rhs x rank;
 * rhos_out, press_out (sum_i (y_ic - loo_ic)^2, summed in row order on the host) and loo_errors_out (the number of i with sign(loo_ic) != sign(y_ic), sign(0) = 0):
 * num_costs x num_rhs; leverage_out: num_costs x N; fitted_out and loo_out: num_costs x num_rhs x N.  leverage_out, fitted_out, loo_out, press_out, loo_errors_out,
 * landmarks_out and infos may be NULL.  The problem is left as it was and keeps its preconditioner.  Refusals: those of lssvm_mi355_problem_fit_reduced and a bad cost
 * grid, all LSSVM_ERR_INVALID_ARGUMENT before a device is touched. */
typedef struct lssvm_reduced_loo_info {
    double cost;
    double jitter;        /* nu of this cost */
    double max_leverage;  /* the largest h_ii */
    double landmark_ms;   /* device time of Phi, the 1 and y columns and K_mm: both passes, all slabs (the same figure for every cost) */
    double gram_ms;       /* device time of St, all slabs (the same figure for every cost) */
    double leverage_ms;   /* device time of this cost's leverage kernel, all slabs */
    double host_ms;       /* this cost's factorisation, inverse and solves on the host */
} lssvm_reduced_loo_info;
int lssvm_mi355_problem_fit_reduced_loo(lssvm_mi355_problem *p, const void *Y /* num_rhs x N, the problem's dtype */, size_t num_rhs, uint64_t rank, const uint64_t *landmarks,
                                        uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out,
                                        double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_loo_info *infos /* num_costs */);
/* one-shot: create the problem on device 0 (as lssvm_mi355_solve_*), fit, destroy it */
int lssvm_mi355_fit_reduced_loo_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, uint64_t rank,
                                    const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out, double *rhos_out, double *leverage_out,
                                    double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_loo_info *infos,
                                    const lssvm_mi355_options *options);
int lssvm_mi355_fit_reduced_loo_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, uint64_t rank,
                                    const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out, double *rhos_out, double *leverage_out,
                                    double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_loo_info *infos,
                                    const lssvm_mi355_options *options);

/* The two fits above with their dense steps on the device (opt-in).  The entry points mirror the six above argument for argument and add one trailing
 * `dense` (may be NULL; the leave-one-out forms: num_costs records).  Where the host forms download St and K_mm and run scalar loops on one host thread, these keep both
 * on the device: per cost and jitter attempt one kernel assembles the lower triangle of M + nu I = S - s s^T / N + sigma K_mm + nu I and the right-hand sides
 * t_c - s eta_c / N, a blocked left-looking Cholesky factorisation (block width `block`; per block column an update on v_mfma_f64_16x16x4_f64, the diagonal block factored
 * in LDS, a panel solve against it) gives L, one workgroup per right-hand side solves L z = rhs, L^T beta = z and forms rho, and -- leave-one-out only -- V = L^-1 is formed
 * row block by row block with triangular solves against the diagonal blocks (no inverted block is multiplied in) straight into the leverage kernel's operand.  Only the
 * betas, the rhos and one status word per attempt come back.  A pivot that is not positive and finite ends the attempt: every later kernel of it returns at once, the host
 * reads the word and retries with the tenfold nu, seven attempts as above, the same refusal after the last.  nu's start value is eps64 trace(M) taken on the host in the
 * host path's order: where no retry happens `jitter` has the host path's bits.  Deterministic: no atomics, every sum in a fixed order, the same bits for the same arguments;
 * row c of a call has the bits of the call with that right-hand side alone, a cost the bits of the call with that cost alone, betas and rhos of a leave-one-out cost the
 * bits of lssvm_mi355_problem_fit_reduced_dev at that cost.  The results are NOT the host path's bits (another order of the sums), and on a numerically singular M the
 * number of jitter retries may differ from the host path's.  `host_ms` of the info records then holds what is left on the host (the trace, the waits, the copies of
 * betas and rhos).  Refusals: those of the host forms, all before a device is touched.  Nothing selects these automatically. */
typedef struct lssvm_dense_info {
    uint64_t rank, block;  /* m and the block width of the factorisation */
    uint64_t attempts;     /* factorisations tried: 1 + the jitter retries */
    uint64_t launches;     /* kernels launched by the last attempt */
    double   jitter;       /* nu of the last attempt */
    double   assemble_ms, factor_ms, solve_ms, invert_ms; /* device time between events, last attempt (invert_ms: 0 without leave-one-out) */
} lssvm_dense_info;
int lssvm_mi355_problem_fit_reduced_dev(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *betas_out,
                                        double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_info *info, lssvm_dense_info *dense);
int lssvm_mi355_fit_reduced_dev_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, uint64_t rank,
                                    const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_info *info,
                                    const lssvm_mi355_options *options, lssvm_dense_info *dense);
int lssvm_mi355_fit_reduced_dev_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, uint64_t rank,
                                    const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_info *info,
                                    const lssvm_mi355_options *options, lssvm_dense_info *dense);
int lssvm_mi355_problem_fit_reduced_loo_dev(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows,
                                            const double *costs, size_t num_costs, double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out,
                                            double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_loo_info *infos,
                                            lssvm_dense_info *dense /* num_costs */);
int lssvm_mi355_fit_reduced_loo_dev_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, uint64_t rank,
                                        const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out, double *rhos_out,
                                        double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out,
                                        lssvm_reduced_loo_info *infos, const lssvm_mi355_options *options, lssvm_dense_info *dense);
int lssvm_mi355_fit_reduced_loo_dev_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, uint64_t rank,
                                        const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out, double *rhos_out,
                                        double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out,
                                        lssvm_reduced_loo_info *infos, const lssvm_mi355_options *options, lssvm_dense_info *dense);

/* The two fits above with per-point weights w_i >= 0 (opt-in): the model minimises  1/2 beta^T K_mm beta + C/2 sum_i w_i (y_i - Phi_i beta - b)^2.
 * With W = sum_i w_i these are the normal equations above with St = Pt^T diag(w) Pt and W wherever N stands (K_mm is not weighted):
 *   M = S - s s^T / W + sigma K_mm,   (M + nu I) beta_c = t_c - s eta_c / W,   b_c = (eta_c - s^T beta_c) / W,
 * and the weighted fit is still a linear smoother, so the leave-one-out values stay exact:
 *   h_ii = w_i (1 / W + |L^-1 (phi_i - s / W)|^2),   f_c^(-i)(x_i) = y_ic - (y_ic - f_c(x_i)) / (1 - h_ii).
 * A point of weight 0 takes no part in the fit: its h is 0 and its leave-one-out value IS the fitted value f_c(x_i) (written as such, not through the expression) -- the
 * prediction of a model that never saw it, so one call scores a validation mask.  A landmark of weight 0 is a basis centre like any other.
 * The device multiplies both operands of the Gram pass by q_i = sqrt(w_i) as it stages them (q is formed on the host with sqrt() and uploaded once per call; the slab itself
 * stays unscaled, no pass over it is added); the leverage kernel multiplies by w_i.  W is the host's sum of the weights in index order, in double.
 * weights: N doubles on the HOST whatever the problem's dtype, each finite and >= 0, W finite and > 0.  NULL: the unweighted model, the call then has the bits of the
 * unweighted entry point of the same `factor`.  They are the only source of weights: a problem with weights set (lssvm_mi355_problem_set_weights) is refused as above.
 * factor: 0 = the dense steps on the host (lssvm_mi355_problem_fit_reduced / _loo), 1 = on the device (_dev); `dense` may be NULL and is ignored for factor 0.
 * press_out is sum_i w_i (y_ic - loo_ic)^2, loo_errors_out counts the sign mismatches over the points with w_i > 0, max_leverage is taken over all points.
 * The guarantees of the unweighted forms carry over: fixed-order sums without atomics and the same bits for the same arguments; row c of a call with k right-hand sides
 * has the bits of the call with that right-hand side alone; a cost has the bits of the call with that cost alone; betas and rhos of a leave-one-out cost have the bits of
 * lssvm_mi355_problem_fit_reduced_weighted at that cost with the same `factor`.  With every weight 1.0 each output has the bits of the unweighted entry point (q = 1,
 * W = N, every product exact).  The landmark rules ignore the weights.
 * LSSVM_ERR_INVALID_ARGUMENT, all before a device is touched: the refusals of the unweighted forms; a weight that is negative, NaN or infinite; W == 0 or not finite; a
 * factor other than 0 or 1. */
int lssvm_mi355_problem_fit_reduced_weighted(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights /* N, or NULL */, uint64_t rank,
                                             const uint64_t *landmarks, uint64_t slab_rows, int factor, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                                             lssvm_reduced_info *info, lssvm_dense_info *dense);
int lssvm_mi355_fit_reduced_weighted_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, const double *weights,
                                         uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, int factor, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                                         lssvm_reduced_info *info, lssvm_dense_info *dense, const lssvm_mi355_options *options);
int lssvm_mi355_fit_reduced_weighted_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights,
                                         uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, int factor, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                                         lssvm_reduced_info *info, lssvm_dense_info *dense, const lssvm_mi355_options *options);
int lssvm_mi355_problem_fit_reduced_loo_weighted(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights /* N, or NULL */, uint64_t rank,
                                                 const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, int factor, double *betas_out,
                                                 double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out,
                                                 uint64_t *landmarks_out, lssvm_reduced_loo_info *infos, lssvm_dense_info *dense /* num_costs */);
int lssvm_mi355_fit_reduced_loo_weighted_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, const double *weights,
                                             uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, int factor, double *betas_out,
                                             double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out,
                                             uint64_t *landmarks_out, lssvm_reduced_loo_info *infos, lssvm_dense_info *dense, const lssvm_mi355_options *options);
int lssvm_mi355_fit_reduced_loo_weighted_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights,
                                             uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, int factor, double *betas_out,
                                             double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out,
                                             uint64_t *landmarks_out, lssvm_reduced_loo_info *infos, lssvm_dense_info *dense, const lssvm_mi355_options *options);

/* The leave-one-out scores above over a grid of kernel widths AND costs in one call on one resident problem (opt-in), for rbf and polynomial
 * problems.  Cell (g, s) is lssvm_mi355_problem_fit_reduced_loo_weighted at the cost C_s on the SAME held data with the kernel's gamma replaced by gamma_g.  What the
 * kernel value of a (point, landmark) pair is made from -- D = sum_f (a_f - b_f)^2 (rbf) or sum_f a_f b_f (polynomial) over the held features -- does not depend on gamma:
 * per slab and pass D is formed ONCE into a work space of slab_rows x rank doubles, and per gamma one elementwise kernel writes Phi = k(gamma'_g, D) from it, with
 * gamma'_g = (gamma_g rounded to the problem's dtype) / x_scale^2, the rule every landmark block follows.  The Gram pass then adds into that gamma's own St, and the dense
 * steps and the leverage kernel per (gamma, cost) are those of the calls above (`factor`: 0 host, 1 device).
 * product: 0 ("ordered") forms D with the loop of the calls above -- with one gamma equal to the problem's own, every output has the BITS of
 * lssvm_mi355_problem_fit_reduced_loo_weighted with the same `factor`.  1 ("matrix") forms the dot products x_i . x_l on v_mfma_f64_16x16x4_f64 (both operands staged
 * through LDS and converted to double on the way; the contraction runs over the held features in steps of 16) and, for rbf, D = n_i + n_l - 2 x_i . x_l with the rows'
 * squared norms n (double, summed ascending, once per call), clamped at 0 and exactly 0 where i is the landmark itself (K_mm's diagonal is exactly 1).  Not the ordered
 * path's bits: |dD| <= (ldx + 4) eps64 (n_i + n_l + 2 sum_f |a_f b_f|) for rbf -- the expansion cancels where a point is close to a landmark relative to their norms;
 * centred data (what an rbf problem off the direct form holds) keeps the norms small -- and (ldx + 2) eps64 sum_f |a_f b_f| for the dot products.
 * The cost AND the gamma of the problem's lssvm_params are ignored by the fit, but its gamma still decides how the problem holds its data (x_scale, the direct form;
 * DESIGN.md section 12): create the problem with a gamma from the grid.  Landmarks are the caller's, or the library's fixed rule; none of them depends on gamma.
 * gammas: each finite and > 0.  num_gammas x num_costs <= 64: the operands of all cells stay on the device during pass 2 (0.5 GB at rank 1 024, the bound of the cost
 * grid above), and beside them the St tiles and K_mm of every gamma from pass 1 until that gamma's cells are factored (about 14 MB per gamma at rank 1 024: up to 0.9 GB
 * more at 64 gammas).  Every output of the leave-one-out call gains a
 * leading gamma dimension: betas_out num_gammas x num_costs x num_rhs x rank; rhos_out, press_out, loo_errors_out num_gammas x num_costs x num_rhs; leverage_out
 * num_gammas x num_costs x N; fitted_out, loo_out num_gammas x num_costs x num_rhs x N; infos and dense (may be NULL; ignored for factor 0) num_gammas x num_costs.
 * weights may be NULL.  Deterministic, no atomics: the same bits for the same arguments; a gamma of a grid has the bits of the call with that gamma alone, a cost the bits
 * of the call with that cost alone, column c the bits of the call with that right-hand side alone.  The problem is left as it was and keeps its preconditioner.
 * LSSVM_ERR_INVALID_ARGUMENT, all before a device is touched: the refusals of lssvm_mi355_problem_fit_reduced_loo_weighted; num_gammas == 0 or a NULL gammas; a gamma that
 * is not finite and > 0; num_gammas x num_costs > 64; a product other than 0 or 1; a problem with the linear kernel (it has no gamma to vary). */
typedef struct lssvm_reduced_grid_info {
    double cost;
    double jitter;         /* nu of this cell */
    double max_leverage;   /* the largest h_ii of this cell */
    double landmark_ms;    /* accumulate_ms + values_ms: the device time of this gamma's Phi, both passes */
    double gram_ms;        /* device time of this gamma's K_mm and St, all slabs (the same figure for every cost) */
    double leverage_ms;    /* device time of this cell's leverage kernel, all slabs */
    double host_ms;        /* this cell's dense steps on the host (factor 1: what is left on the host) */
    double gamma;
    double accumulate_ms;  /* device time of D, both passes, all slabs (and of the norms): the same figure in every record */
    double values_ms;      /* device time of the kernel values of this gamma, both passes, all slabs (the same figure for every cost) */
} lssvm_reduced_grid_info;
int lssvm_mi355_problem_fit_reduced_grid(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights /* N, or NULL */, uint64_t rank, const uint64_t *landmarks,
                                         uint64_t slab_rows, const double *gammas, size_t num_gammas, const double *costs, size_t num_costs, int factor, int product,
                                         double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out,
                                         uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_grid_info *infos, lssvm_dense_info *dense);
/* one-shot: create the problem on device 0 from `params` (as lssvm_mi355_solve_*), fit, destroy it */
int lssvm_mi355_fit_reduced_grid_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, const double *weights,
                                     uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *gammas, size_t num_gammas, const double *costs, size_t num_costs,
                                     int factor, int product, double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out,
                                     uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_grid_info *infos, lssvm_dense_info *dense,
                                     const lssvm_mi355_options *options);
int lssvm_mi355_fit_reduced_grid_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights,
                                     uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *gammas, size_t num_gammas, const double *costs, size_t num_costs,
                                     int factor, int product, double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out,
                                     uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_grid_info *infos, lssvm_dense_info *dense,
                                     const lssvm_mi355_options *options);

/* The leave-one-out scores above for EVERY PREFIX RANK of one fit, over a grid of costs, in one call (opt-in).  The landmark list is ordered (both
 * selection rules deliver their pivots in a meaningful order); for a prefix length r, 1 <= r <= rank = m, the model on the first r landmarks needs nothing the rank-m fit
 * has not formed: S, s, K_mm, t_c and therefore M = S - s s^T / W + sigma K_mm restricted to the first r landmarks are the leading r x r blocks of the rank-m quantities,
 * the Cholesky factor of a leading block is the leading block of the factor (L_r = L[:r, :r]; likewise V = L^-1 and z_c = L^-1 (t_c - s eta_c / W): z_c^(r) = z_c[:r]),
 * and with u_i = V (phi_i - s / W)
 *   h_ii^(r) = w_i (1 / W + sum_{j<r} u_ij^2),   f_c^(r)(x_i) = sum_{j<r} u_ij z_cj + eta_c / W,   beta_c^(r) = L_r^-T z_c[:r],   b_c^(r) = (eta_c - s[:r]^T beta_c^(r)) / W,
 * and the leave-one-out identity y - (y - f) / (1 - h) stays exact for every prefix model (each is the same linear smoother on fewer columns).  One Gram pass, one
 * factorisation per cost and one leverage pass per cost score the whole (cost, rank) grid: the leverage kernel takes the running sums of u^2 and u z_c out of its
 * accumulators at the checkpoints `ranks`.
 * THE JITTER differs from separate fits on landmarks[:r]: every prefix model of a cost uses the nu of the FULL rank at that cost -- eps64 trace(M) over all m landmarks,
 * tenfold per failed factorisation as above (also where the failing pivot lies beyond the largest checkpoint) -- which is no smaller than the prefix's own; it is reported.
 * ranks: 1 <= num_ranks <= 16 checkpoints r_0 < r_1 < ..., each in [1, rank]; num_ranks x num_costs <= 64 (the operands of all costs stay on the device during pass 2,
 * the bound of the grid call).  factor: 0 = the dense steps on the host -- the very code of lssvm_mi355_problem_fit_reduced_loo per cost, then per checkpoint the back
 * substitution L_r^T beta = z[:r] on the leading block: at r_q == rank betas and rhos have the bits of lssvm_mi355_problem_fit_reduced_loo_weighted at that cost with
 * factor 0; 1 = on the device: L, V and z stay there, one workgroup per (checkpoint, right-hand side) forms beta^(r) = V[:r, :r]^T z[:r] and rho with sums in a fixed
 * order, and only betas, rhos, the cond_hints and the status word come back.
 * Outputs, all double: betas_out num_costs x num_ranks x num_rhs x rank, the entries from r_q on are 0; rhos_out, press_out, loo_errors_out num_costs x num_ranks x
 * num_rhs (formed as the leave-one-out call forms them: weighted, summed in row order on the host); leverage_out num_costs x num_ranks x N; fitted_out, loo_out
 * num_costs x num_ranks x num_rhs x N; infos num_costs x num_ranks; dense (ignored for factor 0) num_costs.  press_out, loo_errors_out, leverage_out, fitted_out, loo_out,
 * landmarks_out, infos and dense may be NULL.  weights may be NULL.
 * Deterministic, no atomics; the order of every sum depends on rank and on that checkpoint's r_q only: the same bits for the same arguments; a checkpoint of a list has
 * the bits of the call with that checkpoint alone (at the same rank and landmarks); a cost has the bits of the call with that cost alone; column c has the bits of the
 * call with that right-hand side alone.  The problem is left as it was and keeps its preconditioner.
 * LSSVM_ERR_INVALID_ARGUMENT, all before a device is touched: the refusals of lssvm_mi355_problem_fit_reduced_loo_weighted; a NULL or empty rank list, more than 16
 * checkpoints, one that is 0 or above rank, a list that is not strictly ascending; num_ranks x num_costs > 64. */
typedef struct lssvm_reduced_rank_info {
    double   cost;
    uint64_t rank;          /* r_q */
    double   jitter;        /* nu of this cost: the FULL rank's */
    double   max_leverage;  /* the largest h_ii of this (cost, checkpoint) */
    double   landmark_ms;   /* as lssvm_reduced_loo_info (the same figure in every record) */
    double   gram_ms;       /* as lssvm_reduced_loo_info (the same figure in every record) */
    double   leverage_ms;   /* device time of this cost's prefix leverage kernel, all slabs and all checkpoints (the same figure for every checkpoint of a cost) */
    double   host_ms;       /* this cost's dense steps on the host (factor 1: what is left on the host) */
    double   cond_hint;     /* max_j L_jj^2 / min_j L_jj^2 over j < r_q, read off the factor: a cheap LOWER BOUND of cond(M_r + nu I), not the condition number */
} lssvm_reduced_rank_info;
int lssvm_mi355_problem_fit_reduced_rank_path(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights /* N, or NULL */, uint64_t rank,
                                              const uint64_t *landmarks, uint64_t slab_rows, const uint64_t *ranks, size_t num_ranks, const double *costs, size_t num_costs,
                                              int factor, double *betas_out, double *rhos_out, double *press_out, uint64_t *loo_errors_out, double *leverage_out,
                                              double *fitted_out, double *loo_out, uint64_t *landmarks_out, lssvm_reduced_rank_info *infos, lssvm_dense_info *dense);
/* one-shot: create the problem on device 0 from `params` (as lssvm_mi355_solve_*), fit, destroy it */
int lssvm_mi355_fit_reduced_rank_path_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs,
                                          const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const uint64_t *ranks, size_t num_ranks,
                                          const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out, double *press_out, uint64_t *loo_errors_out,
                                          double *leverage_out, double *fitted_out, double *loo_out, uint64_t *landmarks_out, lssvm_reduced_rank_info *infos,
                                          lssvm_dense_info *dense, const lssvm_mi355_options *options);
int lssvm_mi355_fit_reduced_rank_path_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs,
                                          const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const uint64_t *ranks, size_t num_ranks,
                                          const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out, double *press_out, uint64_t *loo_errors_out,
                                          double *leverage_out, double *fitted_out, double *loo_out, uint64_t *landmarks_out, lssvm_reduced_rank_info *infos,
                                          lssvm_dense_info *dense, const lssvm_mi355_options *options);

/* The fixed-size model from a STREAM of chunks (opt-in): what the fits above keep of the data is S~ = [Phi | 1 | Y]^T diag(w) [Phi | 1 | Y],
 * (rank + 1 + num_rhs)^2 doubles and additive over rows, so the N points need never be held at once and no resident problem is needed.  A reduced stream is an opaque
 * handle on device 0 (one HIP stream; upload and compute follow each other, nothing overlaps) that owns
 *   the m = rank landmark ROWS X_L (m x num_features, row major, the stream's dtype), features zero-padded to a multiple of 16;
 *   the centre (rbf only; else 0): c_f = (sum_l X_L[l][f], l ascending, in double) / m -- every operand is staged as (double) x_f - c_f: rbf is translation invariant, so
 *     the function is unchanged and the norm expansion below keeps its digits;
 *   K_mm (m x m, double): evaluated at creation by the kernel below on the landmarks themselves, the rbf distance forced to 0 on the diagonal (K_mm[l][l] == 1.0) and the
 *     lower triangle mirrored (symmetric to the bit);
 *   the running St and one PENDING slab of slab_rows rows x (m + 1 + k) columns (with its sqrt(w) column on a weighted stream), a fill count, and N.
 * Phi of a chunk: the dot products (x_i - c) . (x_l - c) on v_mfma_f64_16x16x4_f64 (128 landmarks x 128 rows per workgroup, both operands through LDS in steps of 16
 * features), rbf: D = max(n_i + n_l - 2 x_i . x_l, 0) with the squared norms of the centred rows; a streamed row carries no index, so a row that IS a landmark gets the
 * expansion's rounding and not an exact 0 (K_mm alone has the exact diagonal).  The kernel values, the Gram sums, the dense steps and the leverage kernel are the ones of
 * the fits above.
 * _create_f32 / _f64: params' cost is ignored.  1 <= rank <= 1024; slab_rows: a multiple of 256, 0 = the library's default (65 536); weighted != 0: chunks may carry weights.
 *   slab_rows bounds the work space: the pending slab, a scratch of its shape for the feature sums and, once _loo or _phi has run, a scratch slab -- about
 *   3 x slab_rows x (rank + 1 + num_rhs) doubles (lssvm_reduced_stream_info.workspace_bytes reports what is held).
 * _update: n >= 1 rows X (n x num_features), Y (num_rhs x n, the stream's dtype), w (n doubles >= 0, or NULL = 1.0; a weighted stream only) go behind the pending rows;
 *   whenever the slab is full it is summed into St exactly as the fits above sum one, and the fill restarts at 0.  The caller's buffers are free when the call returns.
 *   After any sequence of updates the state is the one a single update of the concatenated rows leaves: every entry of St is summed over the 2048-row ranges of slabs of
 *   slab_rows rows in row order, so NO result depends on how the stream was cut into chunks.
 * _solve (non-destructive): the pending rows, zero-padded to a multiple of 256, are summed into a COPY of St; then per cost the dense steps of the fits above, factor 0:
 *   on the host, 1: on the device (section 15), the jitter rule per cost.  W = S~[m][m], the Gram kernel's own sum of the weights (== N exactly on an unweighted stream),
 *   stands wherever those take N or W.  betas_out: num_costs x num_rhs x rank, rhos_out: num_costs x num_rhs, infos (may be NULL): num_costs records (cost, jitter,
 *   gram_ms: the pending rows' sum and the download, host_ms).  update -> solve -> update -> solve leaves, for the second solve, the bits of update -> update -> solve.
 *   The per-cost leverage operands are kept until the next update, solve or merge.
 * _loo: after a solve and before the next update; evaluates the chunk's Phi again in scratch slabs of its own and runs the leverage kernel of section 13 per cost:
 *   leverage_out num_costs x n, fitted_out and loo_out num_costs x num_rhs x n, all double.  The rows must be rows that were streamed in (the caller's contract, not
 *   checked); a row of weight 0 is a held-out point as in section 16.  Sums over the points (PRESS, error counts) are the caller's.
 * _export_state: S~ (cols x cols row major, both triangles, the pending rows included as in _solve), K_mm, N and the fingerprint: kernel_type, degree, gamma, coef0, m,
 *   num_features, num_rhs, dtype and a hash (FNV-1a) of the landmark rows' bytes, LSSVM_REDUCED_STREAM_FINGERPRINT_WORDS words.
 * _merge_state: adds a foreign exported S~ entrywise into the handle's FLUSHED St (one rounding per entry and merge) and its N to N; the handle's pending rows stay
 *   pending and are summed behind the merged part; the result depends on the order of the merge calls only.  The multi-process form: every rank streams its shard, one
 *   of them merges the others' states.
 * _info: the counts (info may be NULL), the centre (num_features doubles, may be NULL) and K_mm (rank x rank, may be NULL).
 * LSSVM_ERR_INVALID_ARGUMENT, all before a device is touched: NULL handles / pointers; n == 0; num_rhs == 0; rank 0 or beyond 1024; slab_rows no multiple of 256; for rbf and
 * polynomial kernels a gamma that is not finite or not above 0; weights on an unweighted stream; a weight that is negative or not finite; a bad cost grid (as for
 * lssvm_mi355_problem_fit_reduced_loo); factor outside {0, 1}; _solve with N == 0; _loo without a preceding solve or after a later update; a fingerprint that differs. */
typedef struct lssvm_mi355_reduced_stream lssvm_mi355_reduced_stream;
#define LSSVM_REDUCED_STREAM_FINGERPRINT_WORDS 9
typedef struct lssvm_reduced_stream_info {
    uint64_t num_points;       /* N: rows streamed in and merged in */
    uint64_t pending;          /* rows in the pending slab */
    uint64_t rank, num_features, num_rhs, slab_rows;
    int32_t  weighted, dtype;
    uint64_t workspace_bytes;  /* device memory the handle holds */
} lssvm_reduced_stream_info;
int lssvm_mi355_reduced_stream_create_f32(lssvm_mi355_reduced_stream **out, const lssvm_params *params, const float *landmark_rows, size_t rank, size_t num_features,
                                          size_t num_rhs, int weighted, uint64_t slab_rows, const lssvm_mi355_options *options);
int lssvm_mi355_reduced_stream_create_f64(lssvm_mi355_reduced_stream **out, const lssvm_params *params, const double *landmark_rows, size_t rank, size_t num_features,
                                          size_t num_rhs, int weighted, uint64_t slab_rows, const lssvm_mi355_options *options);
int lssvm_mi355_reduced_stream_update(lssvm_mi355_reduced_stream *stream, const void *X, const void *Y, const double *weights /* n, or NULL */, size_t n);
int lssvm_mi355_reduced_stream_solve(lssvm_mi355_reduced_stream *stream, const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out,
                                     lssvm_reduced_loo_info *infos /* num_costs */);
int lssvm_mi355_reduced_stream_loo(lssvm_mi355_reduced_stream *stream, const void *X, const void *Y, const double *weights /* n, or NULL */, size_t n, double *leverage_out,
                                   double *fitted_out, double *loo_out);
int lssvm_mi355_reduced_stream_export_state(lssvm_mi355_reduced_stream *stream, double *gram_out, double *kmm_out, uint64_t *num_points_out, uint64_t *fingerprint_out);
int lssvm_mi355_reduced_stream_merge_state(lssvm_mi355_reduced_stream *stream, const double *gram, uint64_t num_points, const uint64_t *fingerprint);
int lssvm_mi355_reduced_stream_info(lssvm_mi355_reduced_stream *stream, lssvm_reduced_stream_info *info, double *centre_out, double *kmm_out);
int lssvm_mi355_reduced_stream_destroy(lssvm_mi355_reduced_stream *stream);

/* Fixed-size kernel logistic regression by iteratively reweighted least squares (opt-in): with labels y_i in {-1, +1}, prior weights a_i >= 0
 * (NULL: 1) and the problem's cost C the model minimises
 *   J(beta, b) = 1/2 beta^T K_mm beta + C sum_i a_i log(1 + exp(-y_i eta_i)),   eta_i = Phi_i beta + b,
 * so that P(y = +1 | x) = 1 / (1 + exp(-eta(x))) and the decision values of the returned model (betas, rho = -b) are log-odds.  One Newton step from (beta, b) is the
 * weighted fit above at the same C with v_i = a_i max(mu_i, delta), z_i = eta_i + g_i / max(mu_i, delta), mu_i = p_i (1 - p_i), g_i = (y_i + 1) / 2 - p_i, delta = 2^-32,
 * and W = sum_i v_i as the Gram pass sums it.  With s = y_i eta_i and e = exp(-|s|) the device evaluates mu = e / ((1 + e)(1 + e)), the loss max(-s, 0) + log1p(e),
 * g = y_i (s >= 0 ? e / (1 + e) : 1 / (1 + e)) and q = sqrt(a_i max(mu, delta)): no p (1 - p) is formed from p.
 * A pass walks the slabs once: Phi, k_reduced_logistic_step (eta, q, z and the loss sums of up to four classes from one read of the slab), and per class the weighted Gram
 * pass on [Phi | 1 | z_c] with q_c.  Pass t >= 1 compares J_t with the objective J' of the last accepted iterate: J' - J_t < -tol J' rejects the iterate (it becomes the
 * midpoint of itself and the last accepted one and the pass is repeated: a halving); |J' - J_t| <= tol J' ends the class with the iterate of the smaller J (the newer
 * one unless J_t - J' > 2 (N + 16) eps64 J': closer than that the two sums differ by their own rounding only, and the newer iterate is the more accurate) and converged = 1; otherwise the iterate is accepted and the next one solved from this pass's sums.  max_iter counts passes, rejected ones included: when it runs out the
 * class returns the iterate solved last with the objective of the one before it (after a rejected last pass: the last accepted iterate and its objective) and
 * converged = 0.  30 halvings in a row end the class with the last accepted iterate and converged = 0.  The classes of a call run in lockstep and share each evaluation
 * of a Phi slab; a finished class launches nothing more; column c of a call has the bits of the call with that class alone.  One host wait per pass with factor 0; factor 1 adds the wait of
 * every class's dense step (one per jitter attempt), the classes one after the other.  Work space: that of lssvm_mi355_problem_fit_reduced at rank + 2 columns, the packed
 * St tiles per class, and 3 num_rhs slab_rows doubles.
 * Y: num_rhs x N in the problem's dtype, every entry exactly -1 or +1.  weights: as for lssvm_mi355_problem_fit_reduced_weighted.  factor: 0 or 1, as there.
 * tol: finite and > 0 (1e-8 is a good default); max_iter >= 1.  betas0 (num_rhs x rank) and rhos0 (num_rhs): the start values, all finite, or both NULL for zeros.
 * Every output is double; landmarks_out and infos may be NULL.  The problem is left as it was.  LSSVM_ERR_INVALID_ARGUMENT, all before a device is touched: the
 * refusals of lssvm_mi355_problem_fit_reduced_weighted; a label other than -1 or +1; a bad tol; max_iter == 0; start values that are not finite or only half given. */
typedef struct lssvm_reduced_logistic_info {
    uint64_t passes;        /* evaluations of this class, rejected ones included */
    uint64_t halvings;      /* rejected passes */
    uint64_t floored;       /* rows with mu < delta in the class's last pass */
    int32_t  converged;
    int32_t  reserved;
    double   objective;     /* J of the returned iterate where it was evaluated, else of the iterate before it (see above) */
    double   last_decrease; /* J' - J_t of the last pass that was tested */
    double   jitter;        /* nu of the class's last solve (0 only where the class never solved) */
    double   max_abs_eta;   /* max_i |eta_i| in the class's last pass */
    double   landmark_ms, step_ms, gram_ms; /* device time of Phi, of the step kernel and of the Gram passes over the passes this class took part in (shared launches count whole) */
    double   host_ms;       /* this class's dense steps and bookkeeping */
    double   total_ms;      /* the call */
} lssvm_reduced_logistic_info;
int lssvm_mi355_problem_fit_reduced_logistic(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights /* N, or NULL */, uint64_t rank,
                                             const uint64_t *landmarks, uint64_t slab_rows, int factor, double tol, uint64_t max_iter,
                                             const double *betas0 /* num_rhs x rank, or NULL */, const double *rhos0 /* num_rhs, or NULL */, double *betas_out,
                                             double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_logistic_info *infos /* num_rhs */);
int lssvm_mi355_fit_reduced_logistic_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, const float *Y, size_t num_rhs, const double *weights,
                                         uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, int factor, double tol, uint64_t max_iter, const double *betas0,
                                         const double *rhos0, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_logistic_info *infos,
                                         const lssvm_mi355_options *options);
int lssvm_mi355_fit_reduced_logistic_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights,
                                         uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, int factor, double tol, uint64_t max_iter, const double *betas0,
                                         const double *rhos0, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_logistic_info *infos,
                                         const lssvm_mi355_options *options);

/* Landmark selection on a resident problem (opt-in): the pivots of a partial Cholesky factorisation of the kernel matrix, chosen greedily or
 * at random in proportion to the residual diagonal (randomly pivoted Cholesky).  The result is a list of point indices for the `landmarks` argument of the entry points
 * above; nothing else changes, and nothing selects it automatically.  Neither rule dominates the other or the fixed shuffle (README.md has the rows of all three kinds).
 * Candidates cand[0 ... n): pool == 0: all N points in order; else the first `pool` entries of the library's fixed shuffle (as for the preconditioner above), in that
 * order -- pool bounds the work space, rank x ld(n) doubles with ld(n) = n rounded up to 256.  Everything is double whatever the problem's dtype; k is evaluated from
 * the problem's resident data exactly as the preconditioner evaluates K_Nm.
 *   d_i = k(x_i, x_i), d0 = max d_i; S = the sum of the sums of d over blocks of 256 candidates, blocks ascending.
 *   for j = 0 ... rank-1:  choose the pivot p
 *       GREEDY:      the largest d_i, among equal values the smallest candidate position;
 *       RPCHOLESKY:  u = (next() >> 11) 2^-53 with next() = splitmix64 from the state 0x243F6A8885A308D3 ^ seed, t = u S; the first block whose inclusive prefix of the
 *                    block sums exceeds t, inside it the first position whose running sum (ascending) exceeds the remainder; the greedy pivot if rounding leaves none
 *                    or the hit has d = 0;
 *     stop with rank_found = j if d_p <= max(tol, 64 eps64) d0 (the rank is exhausted: a linear kernel on 5 features after 5 pivots);
 *     c_i = k(x_i, x_p) - sum_{t<j} F[t][i] F[t][p] (t ascending), F[j][i] = c_i / sqrt(d_p), d_i <- max(d_i - F[j][i]^2, 0), d_p <- 0.
 * landmarks_out: the pivots as point indices in the order they were chosen, UINT64_MAX from rank_found on.  trace_out (rank doubles or NULL): S after step j (the
 * trace of the Nystrom residual K - K[:, P] K[P, P]^-1 K[P, :] over the candidates); from rank_found on the value at the stop.  residual_out (N doubles or NULL): the
 * final d of every candidate, NaN for points that were not candidates.  1 <= rank <= min(candidates, 1024).  One launch pair per step on the problem's stream, no
 * host round trip between steps; fixed-order reductions without atomics: the same bits for the same arguments.  The problem is left as it was and keeps its
 * preconditioner.
 * LSSVM_ERR_INVALID_ARGUMENT, all before a device is touched: a problem on several devices or ranks, weights set on the problem, a call between cg_begin and cg_finish;
 * rank 0 or beyond its bound; 0 < pool < rank or pool > N; an unknown method; a negative or non-finite tol; a NULL landmarks_out. */
#define LSSVM_LANDMARKS_GREEDY 1
#define LSSVM_LANDMARKS_RPCHOLESKY 2
typedef struct lssvm_landmark_select_info {
    uint64_t rank_found, candidates;
    double   trace0;        /* S before the first step */
    double   trace;         /* S after the last step taken */
    double   max_residual;  /* the largest d_i left */
    double   select_ms;     /* the whole call */
    double   device_bytes;  /* work space held during the call */
} lssvm_landmark_select_info;
int lssvm_mi355_problem_select_landmarks(lssvm_mi355_problem *p, uint64_t rank, int method, uint64_t pool, uint64_t seed, double tol, uint64_t *landmarks_out /* rank */,
                                         double *trace_out /* rank or NULL */, double *residual_out /* N or NULL */, lssvm_landmark_select_info *info);
/* one-shot: create the problem on device 0 (as lssvm_mi355_solve_*), select, destroy it */
int lssvm_mi355_select_landmarks_f32(const lssvm_params *params, const float *X, size_t num_points, size_t num_features, uint64_t rank, int method, uint64_t pool,
                                     uint64_t seed, double tol, uint64_t *landmarks_out, double *trace_out, double *residual_out, lssvm_landmark_select_info *info,
                                     const lssvm_mi355_options *options);
int lssvm_mi355_select_landmarks_f64(const lssvm_params *params, const double *X, size_t num_points, size_t num_features, uint64_t rank, int method, uint64_t pool,
                                     uint64_t seed, double tol, uint64_t *landmarks_out, double *trace_out, double *residual_out, lssvm_landmark_select_info *info,
                                     const lssvm_mi355_options *options);

/* CG, csvm.cpp:89-111: b = y[0..n) - y[n], x = 1, r = b - A x, delta0, d = r */
int lssvm_mi355_cg_begin(lssvm_mi355_problem *p, const void *y, double eps);
/* run at most `iterations` further CG iterations (csvm.cpp:125-166); stops early when delta <= eps^2 delta0.
 * *done_out (may be NULL) is set to 1 when the stop test fired. */
int lssvm_mi355_cg_step(lssvm_mi355_problem *p, uint64_t iterations, int *done_out);
/* csvm.cpp:179-182: bias, alpha[N-1] = -sum, rho = -bias; alpha_out has N entries of the problem's dtype */
int lssvm_mi355_cg_finish(lssvm_mi355_problem *p, void *alpha_out, double *rho_out, lssvm_cg_info *info);
/* block until all work queued on the problem's stream has finished (gpu_csvm::device_synchronize, gpu_csvm.hpp:208) */
int lssvm_mi355_problem_synchronize(lssvm_mi355_problem *p);
/* timing / counters accumulated since cg_begin (same struct as cg_finish fills); does not synchronize */
int lssvm_mi355_problem_info(lssvm_mi355_problem *p, lssvm_cg_info *info);

/* ---- LIBSVM data files (the input format of plssvm-train, include/plssvm/detail/io/libsvm_parsing.hpp:47-229) ----
 * Multi-threaded fast path for WELL-FORMED files: `open` reads and validates the file (labels on every line or on none; one-based,
 * strictly increasing indices; every token converts) and reports its shape, `fill` writes the dense row-major matrix (missing
 * features = 0; ldx >= num_features, in elements) and the labels (always double; may be NULL; ignored for unlabelled files).  Any irregularity
 * -> LSSVM_ERR_INVALID_ARGUMENT without a diagnosis: callers re-parse with their reference-exact parser for the error message
 * (plssvm_amd/io_libsvm.py does).  Host code only, no device needed. */
typedef struct lssvm_mi355_libsvm_file lssvm_mi355_libsvm_file;
int lssvm_mi355_libsvm_open(const char *path, uint64_t skipped_lines, lssvm_mi355_libsvm_file **file_out, uint64_t *num_points, uint64_t *num_features,
                            int *has_label);
int lssvm_mi355_libsvm_fill_f32(lssvm_mi355_libsvm_file *file, float *X, uint64_t ldx, double *labels);
int lssvm_mi355_libsvm_fill_f64(lssvm_mi355_libsvm_file *file, double *X, uint64_t ldx, double *labels);
int lssvm_mi355_libsvm_close(lssvm_mi355_libsvm_file *file);

/* ---- LIBSVM data files: writer (include/plssvm/detail/io/libsvm_parsing.hpp:244-296) ----
 * `header` (may be NULL) is written verbatim first -- the reference's two comment lines "# This data set has been created at ..." and "# NxD" are the caller's
 * to word.  Then one line per point: "label idx:val idx:val ... " -- every number as {:.10e}, zero features left out, one-based indices, a blank after every
 * token, like the reference.  The label column: int_labels (whole numbers, written as integers), OR label_text + label_offsets (point i's label is the
 * bytes [label_offsets[i], label_offsets[i + 1]) of label_text: string labels, or numbers the caller has already formatted), or neither: no labels.  The
 * points are written in their order by all host threads (chunks of rows formatted concurrently, flushed in order): the file does not depend on the thread
 * count (the reference's order is unspecified, :251).  Host code only, no device needed. */
int lssvm_mi355_libsvm_write_f32(const char *path, const char *header, const float *X, uint64_t num_points, uint64_t num_features, uint64_t ldx,
                                 const int64_t *int_labels, const char *label_text, const uint64_t *label_offsets);
int lssvm_mi355_libsvm_write_f64(const char *path, const char *header, const double *X, uint64_t num_points, uint64_t num_features, uint64_t ldx,
                                 const int64_t *int_labels, const char *label_text, const uint64_t *label_offsets);

/* ---- LIBSVM model files: what plssvm-train writes and plssvm-predict reads (include/plssvm/detail/io/libsvm_model_parsing.hpp) ----
 * Writer (:371-499): `header` -- the lines from the "#" time stamp to "SV" (:296-342; a dozen short lines, worded by the caller: plssvm_amd/model.py) -- is
 * written verbatim, then `count` lines "alpha idx:val idx:val ... " ({:.10e}, zeros left out, a blank after every token) for the support vectors
 * order[0 .. count) -- the caller lists them grouped by class in the order of the header's "label" line (:416-499); order == NULL: all of them as they lie
 * (count must equal num_support_vectors).  Multi-threaded like the data writer, the same bytes for any thread count. */
int lssvm_mi355_model_write_f32(const char *path, const char *header, const float *support_vectors, uint64_t num_support_vectors, uint64_t num_features,
                                uint64_t ldx, const float *alpha, const uint64_t *order, uint64_t count);
int lssvm_mi355_model_write_f64(const char *path, const char *header, const double *support_vectors, uint64_t num_support_vectors, uint64_t num_features,
                                uint64_t ldx, const double *alpha, const uint64_t *order, uint64_t count);
/* Reader (:64-262), the same contract as the data readers: a multi-threaded fast path for WELL-FORMED files -- every header key at most once and spelled
 * out ("svm_type c_svc", "kernel_type linear|polynomial|rbf", "degree", "gamma", "coef0", "nr_class", "total_sv", "rho", "label", "nr_sv", then "SV"; any
 * order and case), only the parameters its kernel uses, counts that add up, then exactly total_sv lines "alpha idx:val ..." that follow the data-file
 * rules.  `open` maps and validates the file and reports the header; `labels` hands out the "label" line's entries (separated by single blanks, NUL
 * terminated, lssvm_model_info.label_text_bytes bytes; the caller converts them to its label type and checks them for duplicates AFTER that conversion,
 * as the reference does) and the nr_sv counts (nr_class entries); `fill` writes the support vectors (dense row-major, missing features = 0) and their
 * weights.  Any irregularity -> LSSVM_ERR_INVALID_ARGUMENT without a diagnosis: callers re-parse with their reference-exact parser for the error message
 * (plssvm_amd/model.py does). */
typedef struct lssvm_model_info {
    int32_t kernel_type; /* lssvm_kernel_type */
    int32_t has_degree;  /* which of the kernel parameters the header states (an rbf / polynomial header may leave gamma to the 1 / num_features default) */
    int32_t has_gamma;
    int32_t has_coef0;
    int64_t degree;
    double gamma;
    double coef0;
    double rho;
    uint64_t nr_class;
    uint64_t total_sv;         /* = number of support-vector lines */
    uint64_t num_features;     /* largest feature index of the body */
    uint64_t label_text_bytes; /* bytes lssvm_mi355_model_labels writes into label_text_out, the terminating NUL included */
} lssvm_model_info;
typedef struct lssvm_mi355_model_file lssvm_mi355_model_file;
int lssvm_mi355_model_open(const char *path, lssvm_mi355_model_file **file_out, lssvm_model_info *info);
int lssvm_mi355_model_labels(lssvm_mi355_model_file *file, char *label_text_out, uint64_t label_text_bytes, uint64_t *nr_sv_out);
int lssvm_mi355_model_fill_f32(lssvm_mi355_model_file *file, float *support_vectors, uint64_t ldx, float *alpha);
int lssvm_mi355_model_fill_f64(lssvm_mi355_model_file *file, double *support_vectors, uint64_t ldx, double *alpha);
int lssvm_mi355_model_close(lssvm_mi355_model_file *file);

/* ---- ARFF data files (the second format of plssvm::data_set, include/plssvm/detail/io/arff_parsing.hpp:57-372) ----
 * The same contract as the LIBSVM reader above: a multi-threaded fast path for WELL-FORMED files -- "@RELATION name", "@ATTRIBUTE name NUMERIC" per feature, at
 * most one "@ATTRIBUTE class {l1,l2,...}" with numeric labels, "@DATA", then dense rows (one value per attribute) or sparse rows ("{index value,...}", zero-based
 * attribute indices) whose labels are among the header's.  int_labels != 0: the caller's label type is an integer, the labels must be written as plain integers.
 * `fill` writes the dense row-major matrix and the labels (always double; may be NULL).  Any irregularity -> LSSVM_ERR_INVALID_ARGUMENT without a diagnosis:
 * callers re-parse with their reference-exact parser for the error message (plssvm_amd/io_arff.py does).  Host code only, no device needed. */
typedef struct lssvm_mi355_arff_file lssvm_mi355_arff_file;
int lssvm_mi355_arff_open(const char *path, int int_labels, lssvm_mi355_arff_file **file_out, uint64_t *num_points, uint64_t *num_features, int *has_label);
int lssvm_mi355_arff_fill_f32(lssvm_mi355_arff_file *file, float *X, uint64_t ldx, double *labels);
int lssvm_mi355_arff_fill_f64(lssvm_mi355_arff_file *file, double *X, uint64_t ldx, double *labels);
int lssvm_mi355_arff_close(lssvm_mi355_arff_file *file);

/* tuning knobs, by name (all have defaults; unknown names -> LSSVM_ERR_INVALID_ARGUMENT).  set_option changes the process-wide DEFAULTS (thread safe);
 * every problem / solve that is not handed a lssvm_mi355_options of its own takes a snapshot of them when it is created, so later changes never affect a live problem.  The defaults can
 * be preset from the environment: LSSVM_MI355_OPTIONS="name=value,name=value" (read once when the library is loaded).  Thirteen options here, two
 * testing aids and one experimental option in plssvm_amd_testing.h -- who sets each besides the tests: DESIGN.md section 4.5 (round 4 retired xcd_map, lds_extra_kb, item_order,
 * linear_panel_features, check_shards, rbf_direct_above and mfma_shape = 1: measured, decided, constants now):
 *   "rbf_form"      fp32 rbf: 0 = automatic (default): the norm expansion c_i + c_j + x_i'.x_j' on the matrix cores, unless
 *                   R2 = 2 gamma log2(e) max|x - mean|^2 exceeds 32 -- the expansion's exponent carries an absolute error of
 *                   ~2^-24 R2 whatever the distance of the pair, which nearby pairs (K ~ 1) see as a relative error of K
 *                   ([-1,1]-scaled data with gamma = 1 / num_features has R2 <= 3); then, up to R2 = 4096 (times sqrt(128 / num_features) beyond 128 features), the matrix
 *                   cores on GRID planes (since round 5: x = h + s1 + s2 with h on a grid, the accumulators started from the exact grid norms and
 *                   fed the h.h products first, so that the large terms cancel exactly -- the direct form's accuracy at 1.6x the f16x3 time); beyond
 *                   that, and with 1 = always, the formula-exact (x_i - x_j)^2 kernel on the vector ALU (10x slower than the grid planes at
 *                   50 000 x 128); 2 = always the norm expansion; 3 = the grid planes wherever they exist (R2 within that limit)
 *   "rbf_fold"      fp32 rbf on the split kernels: 1 (default) = the column records carry (2^c_j d_j | 2^c_j) and the accumulators start
 *                   from c_i as the C operand of their first MFMA (256-row workgroups: from 0, the row's term folded too) -- no start-value
 *                   instructions, K_ij = 2^acc 2^c_j (one more rounding than 2^(acc + c_j); used while the exponent scale R2 <= 200 keeps both factors
 *                   far inside the fp32 range); 0 = start values c_i + c_j
 *   "j_chunk_tiles" number of 128-column tiles per work item; 0 = automatic (default: about 4096 work items per device, 2 ... 16 tiles each,
 *                   up to 64 for the split kernels; 256-row workgroups: the length whose replayed dispatch over the CUs finishes first)
 *   "j_chunk_head"  256-row workgroups (see "mfma_shape"): the FIRST `count` column chunks of every pair of row blocks have `tiles` tiles instead of j_chunk_tiles, value =
 *                   1024 count + tiles; their short work items are dispatched last and fill the final dispatch round of a launch that is only a few rounds long.
 *                   1 (default) = the replayed dispatch chooses a head together with the chunk length (j_chunk_tiles = 0; 3-5 % at 20 000-50 000 points since the
 *                   launches are persistent and draw their items from per-XCD counters); 0 = none
 *   "symmetric"     1 = evaluate only the kernel-matrix tiles on/below the diagonal and mirror them (default; any num_features -- beyond 512 (fp32) /
 *                   256 (fp64) features over feature panels -- except fp32 with gram_mode = 0 beyond 512 features and a negative polynomial
 *                   degree, which run the full square),
 *                   0 = full square (row-owned sums, results independent of the GPU count)
 *   "tile_kernel"   0 = automatic: the "resident row panel" kernels for num_features <= 512 (fp32) / 256 (fp64) and their feature-panel forms beyond
 *                   (default), 1 = always the generic kernel
 *   "gram_mode"     fp32 Gram tiles on the 16-bit matrix cores with fp32 accumulation, at fp32-equivalent accuracy:
 *                   3 (default) = "f16x3" where the data allows, else "bf16x6"; 2 = "f16x3": every operand as TWO f16 planes (hi + mid; rbf: shifted by
 *                   2^-6 / 2^6, others pre-scaled by a power of two), three plane products on v_mfma_f32_16x16x32_f16; num_features <= 512 (rbf 384)
 *                   in one pass, beyond that over feature panels of 128 (linear: one launch per panel; rbf / polynomial: inside a tile, symmetric variant)
 *                   -- without the check whether two f16 planes represent THIS data as well as fp32 does, which mode 3 makes at set-up (linear kernel, round 6: where ONE
 *                   power-of-two scale for the matrix fails that check -- points that differ by orders of magnitude -- mode 3 gives every ROW its own scale and stays f16x3);
 *                   1 = "bf16x6": exact split into THREE bf16 planes, six plane products on v_mfma_f32_16x16x32_bf16, num_features <= 384 in one
 *                   pass (rbf / polynomial beyond that: feature panels inside a tile);
 *                   0 = Gram tiles on v_mfma_f32_32x32x2_f32 (exact fmaf chains)
 *   "mfma_shape"    split kernels, symmetric variant, at most 128 features per pass: 3 (default) = 256-row workgroups -- eight waves on a pair of row
 *                   blocks share one column stream per CU -- from 64 row blocks (8 192 points) on; 2 = 128-row workgroups (four waves) throughout
 *   "colslab_band_mb" the symmetric variant leaves one record of 128 column sums per evaluated off-diagonal tile (256-row workgroups: per pair of row
 *                   blocks and column tile); the device's row blocks are
 *                   cut into bands of equal area whose records fit this many MiB (default 2048), the tile kernel runs band by band into one
 *                   slab and every band is folded into K*v before the next (1M points in fp32: 15.6 GB of records -> 8 bands, 2 GiB)
 *   "colslab_limit_mb" upper bound of the band slab (default 98304); 0 switches the symmetric variant off (full square)
 *   "exchange"      several devices in one process (the _multi entry points): 0 = automatic (RCCL when the listed devices are distinct, peer
 *                   kernels otherwise; default), 1 = RCCL all-reduce / all-gather, 2 = peer kernels: every device adds the partial vectors of all
 *                   devices through its xGMI peer mappings in rank order (bit-equal on all devices, deterministic).
 *                   One process per GPU (lssvm_shard): 0 = RCCL when lssvm_mi355_comm_init was called in this process, else HIP IPC;
 *                   1 = RCCL; 2 = HIP IPC + the peer kernel (lssvm_mi355_problem_ipc_export / _connect)
 *   "ipc_timeout_s" one process per GPU over HIP IPC: seconds a rank waits for its peers at an exchange before it fails (default 600)
 *   "enqueue_ahead_below_us" CG loop: while an implicit matvec is expected to take less than this many microseconds (default 5000; the expectation is a rule
 *                   on the shape, the real type and the kernel path -- never a measurement, every rank of a sharded solve must agree), the direction update and
 *                   the NEXT matvec are enqueued before the host reads the stop test of the current iteration, so the device never waits for
 *                   the host; they touch d and K*d only, so a converged solve ends exactly where the reference's does, one matvec is discarded.
 *                   0 = the host reads every stop test before it enqueues anything further
 */
int lssvm_mi355_set_option(const char *name, int64_t value);
int lssvm_mi355_get_option(const char *name, int64_t *value_out);

#ifdef __cplusplus
}
#endif
#endif /* PLSSVM_AMD_H */
