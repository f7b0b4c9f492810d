/*
 * plssvm_amd_testing.h -- entry points and option names of libplssvm_amd.so that are NOT part of the boundary a PLSSVM maintainer binds
 * (include/plssvm_amd.h): measurement and test aids used by bench.py, tests/ and tests/tools/ only.  They are exported by the same
 * library so that what is measured is the shipped code; nothing in include/plssvm_amd/csvm.hpp or plssvm_amd/csvm.py calls them.
 */
#ifndef PLSSVM_AMD_TESTING_H
#define PLSSVM_AMD_TESTING_H

#include "plssvm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Measurement utility, not on the solve path and without a counterpart in the reference: what a BARE loop of v_mfma_f32_16x16x32_bf16
 * (the instruction of the fp32 "bf16x6" Gram kernel; 64 x 64 wave tiles, two waves per SIMD, normal(0,1) operands, nothing else in the
 * loop) sustains on `device` after `settle_ms` of back-to-back launches.  b_from_lds bit 0: the B fragments are re-read from LDS every
 * pass, as the Gram kernel does; bit 1: v_mfma_f32_16x16x32_f16 on f16 operands (the instruction of the "f16x3" kernels) instead of the bf16 form.  Returns TFLOP/s, the in-kernel clock (s_memtime / s_memrealtime, median over workgroups) and the
 * nominal peak (4096 FLOP/clk/CU x CUs x nominal clock).  The chip lowers its clock under matrix-core load, so this -- not the
 * nominal peak -- is what a kernel on this device is up against; bench.py prints it beside roofline.frac. */
int lssvm_mi355_measure_bf16_mfma_ceiling(int device, int b_from_lds, double settle_ms, double *tflops_out, double *clock_ghz_out, double *nominal_tflops_out);

/* The file the library's RCCL entry points were resolved from (dladdr of ncclAllReduce after the lazy dlopen of "librccl.so.1"): a bench line or a
 * test can then say WHICH library carried the exchange -- the process's RCCL (PyTorch's or /opt/rocm's), or a stand-in with that SONAME which a test
 * harness loaded into the process first (tests/tools/; the library itself never looks for one). */
int lssvm_mi355_comm_library_path(char *buf, size_t buf_len);

/* ---- EXPERIMENTAL: shares by weight for devices of unequal pace ----
 * Not part of the boundary: built in round 5 for hardware nobody has measured yet (two DIFFERENT devices behind one solve), exercised for self-consistency on one
 * time-shared GPU only, where "pace" is the scheduler's and not a device's.  Frozen until a multi-GPU node exists; the names may change. */
/* Devices of unequal pace (the MI355X boxes of one pool run the same kernel in 252 ... 277 ms): rank r of a sharded SYMMETRIC problem gets weights[r] / sum of the triangle's area
 * instead of 1 / world -- a process-wide default like the options below, snapshotted when a problem is created, applied when `count` equals the problem's world (any other
 * length, or count = 0: equal shares).  EVERY rank of a sharded solve must set the same weights (the partition is computed locally by every rank); the data is replicated on
 * every device, so a new partition costs a new problem, no data exchange.  bench.py --balance-shares measures the ranks' pace and sets them.  No counterpart in the reference
 * (its multi-device split is by features, gpu_csvm.hpp:283-299). */
int lssvm_mi355_set_shard_weights(const double *weights, int count);
/* The same for a LIVE problem, between two lssvm_mi355_cg_step calls: the shards' row blocks, work items and slabs are rebuilt for new shares; the data, the vectors and the
 * CG state stay (the implicit matrix does not change, only who evaluates which tiles).  weights == NULL, count == 0: shares by MEASURED pace -- every shard's tile-kernel time
 * per matvec so far against the area of its share; one process driving all devices knows them, one process per GPU gathers them over the library's RCCL communicator (every rank
 * must make the call; not over HIP IPC: explicit weights there, the same on every rank).  *changed_out = 0 where the times lie within 2 % of each other or the problem is not
 * sharded / not symmetric.  A solve that wants it: cg_begin, a few cg_step, problem_rebalance, the remaining cg_step. */
int lssvm_mi355_problem_rebalance(lssvm_mi355_problem *p, const double *weights, int count, int *changed_out);
/* option (lssvm_mi355_set_option / lssvm_mi355_options_set), experimental with the two entry points above:
 *   "rebalance_after" lssvm_mi355_solve_multi_*: after this many CG iterations the shards get new shares of the triangle by their measured pace
 *                   (lssvm_mi355_problem_rebalance with weights = NULL); 0 (default) = never -- devices are taken to run at one pace
 */

/* The file readers and writers (lssvm_mi355_libsvm_*, _arff_*, _model_*) use at most this many host threads; 0 (default) = as many as the hardware has,
 * at most 32.  For the tests that a written file does not depend on the thread count. */
int lssvm_mi355_set_io_threads(int threads);

/* The operator of the fixed-size model alone (lssvm_mi355_problem_fit_reduced): St = Pt^T Pt for Pt = [Phi | 1 | y_0 ... y_{k-1}], as the device sums
 * it, (rank + 1 + num_rhs)^2 doubles row-major with BOTH triangles (the upper one is the host's copy of the lower).  Arguments and refusals as there. */
int lssvm_mi355_problem_landmark_gram(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *gram_out);
/* ... and of the weighted model (lssvm_mi355_problem_fit_reduced_weighted): St = Pt^T diag(w) Pt alone, both operands scaled by sqrt(w_i) as they
 * are staged.  weights NULL: the call above.  Arguments and refusals as there. */
int lssvm_mi355_problem_landmark_gram_weighted(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks,
                                               uint64_t slab_rows, double *gram_out);

/* The operator of the leave-one-out pass alone (lssvm_mi355_problem_fit_reduced_loo) on the caller's operands, apart from any conditioning: for every
 * point i, with phic_i = phi_i - shift (phi_i: row i of Phi = K(X, X_L) as the problem evaluates it),
 *   h_out[i] = |V phic_i|^2   (the 1 / N of the leverage left out),     f_out[c * N + i] = phic_i . B_extra[:, c]   (the mean of y left out)
 * V: rank x rank row major, only its LOWER triangle counts -- whatever stands above the diagonal is never used: column blocks above the diagonal of V^T are not read, the
 * blocks on it are masked.  B_extra: rank x k row major (NULL with k = 0; then f_out may be NULL).  Arguments and refusals as for lssvm_mi355_problem_landmark_gram. */
int lssvm_mi355_problem_reduced_leverage(lssvm_mi355_problem *p, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *V, const double *shift,
                                         const double *B_extra, size_t k, double *h_out, double *f_out);

/* The operator of the rank path alone (lssvm_mi355_problem_fit_reduced_rank_path) on the caller's operands, apart from any conditioning; it mirrors
 * lssvm_mi355_problem_reduced_leverage: for every point i and checkpoint q, with phic_i = phi_i - shift,
 *   h_out[q * N + i] = sum_{j < r_q} (V phic_i)_j^2,     f_out[(q * k + c) * N + i] = sum_{j < r_q} (V phic_i)_j Z[c][j]
 * V: rank x rank row major, only its LOWER triangle counts, as there.  Z: k x rank row major (NULL with k = 0; then f_out may be NULL).  ranks: 1 <= num_ranks <= 16
 * checkpoints, strictly ascending, each in [1, rank].  Arguments and refusals as for lssvm_mi355_problem_reduced_leverage, and a bad rank list. */
int lssvm_mi355_problem_reduced_leverage_prefix(lssvm_mi355_problem *p, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *V, const double *shift,
                                                const double *Z, size_t k, const uint64_t *ranks, size_t num_ranks, double *h_out, double *f_out);
/* Measurement aid of tests/tools/reduced_rank_path_timing.py, beside lssvm_mi355_problem_time_leverage_kernel and on the same slab and operands (an identity V, k rows of
 * ones for Z): the prefix leverage kernel with the checkpoints `ranks` and its leave-one-out outputs, prefix_ms_out[r]: device time of repeat r after one untimed run. */
int lssvm_mi355_problem_time_leverage_prefix_kernel(lssvm_mi355_problem *p, uint64_t rank, uint64_t slab_rows, size_t k, const uint64_t *ranks, size_t num_ranks, int repeats,
                                                    double *prefix_ms_out);

/* The operator of the (gamma, cost) grid alone (lssvm_mi355_problem_fit_reduced_grid), apart from any fit: D_out[l * N + i] = what the kernel value
 * of (point i, landmark l) is made from on the data as the problem holds it -- sum_f (a_f - b_f)^2 (rbf) or sum_f a_f b_f (polynomial, linear) -- for all N points, rank x N
 * doubles, in slabs of the library's default size.  product: 0 = the ordered loop of the landmark block, 1 = the dot products on the matrix cores (and the norm expansion
 * for rbf).  landmarks: `rank` distinct indices < N, or NULL for the library's rule.  Refusals as for lssvm_mi355_problem_landmark_gram, and a product other than 0 or 1. */
int lssvm_mi355_problem_landmark_acc(lssvm_mi355_problem *p, const uint64_t *landmarks, uint64_t rank, int product, double *D_out);

/* The operator of a reduced stream alone (lssvm_mi355_reduced_stream_*), apart from any fit: phi_out[i * rank + l] = k(x_i, x_L[l]) for the n rows
 * of the chunk X (n x num_features, the stream's dtype) as the stream evaluates them -- the centred dot products on the matrix cores, the norm expansion for rbf, the
 * kernel values -- n x rank doubles.  The state is left untouched (the rows go through the stream's scratch slab).  NULL handle / X / phi_out or n == 0:
 * LSSVM_ERR_INVALID_ARGUMENT before a device is touched. */
int lssvm_mi355_reduced_stream_phi(lssvm_mi355_reduced_stream *stream, const void *X, size_t n, double *phi_out);
/* Measurement aid of tests/tools/reduced_stream_timing.py: on the chunk X (1 <= n <= slab_rows rows) the stream's k_cross_product (cross_ms_out[r]) and, at the same
 * shape -- the chunk's rows and the landmark rows as one resident set, the landmarks by index -- k_landmark_product (landmark_ms_out[r]), device time of repeat r each
 * after one untimed run.  The state is left untouched. */
int lssvm_mi355_reduced_stream_time_kernels(lssvm_mi355_reduced_stream *stream, const void *X, size_t n, int repeats, double *cross_ms_out, double *landmark_ms_out);

/* The step operator of the fixed-size logistic regression alone (lssvm_mi355_problem_fit_reduced_logistic), apart from any fit: one launch sequence
 * of k_reduced_logistic_step over the slabs at the caller's coefficients.  betas: num_rhs x rank, rhos: num_rhs (b = -rho), Y: num_rhs x N labels of exactly -1 or +1 in
 * the problem's dtype, weights: N doubles or NULL.  eta_out, q_out, z_out: num_rhs x N doubles each (eta_i = Phi_i beta + b, q_i = sqrt(a_i max(mu_i, delta)),
 * z_i = eta_i + g_i / max(mu_i, delta)); loss_out: num_rhs sums of a_i l_i, the kernel's partial sums of 64 rows added in ascending row order on the host; floored_out
 * (may be NULL): num_rhs counts of the rows with mu_i < delta.  Arguments and refusals as for the fit. */
int lssvm_mi355_problem_reduced_logistic_step(lssvm_mi355_problem *p, const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks,
                                              uint64_t slab_rows, const double *betas, const double *rhos, double *eta_out, double *q_out, double *z_out, double *loss_out,
                                              uint64_t *floored_out);

/* Measurement aid of tests/tools/reduced_loo_timing.py: on ONE slab of this problem (its first min(N, slab_rows) points, `rank` landmarks by the library's rule, an
 * identity V, k columns of ones) the Gram kernels of the fixed-size fit (gram_ms_out[r]: partial tiles and their sum over rank + 1 + k columns) and the leverage kernel
 * (leverage_ms_out[r]), device time of repeat r each after one untimed run of both. */
int lssvm_mi355_problem_time_leverage_kernel(lssvm_mi355_problem *p, uint64_t rank, uint64_t slab_rows, size_t k, int repeats, double *gram_ms_out, double *leverage_ms_out);

/* Measurement aid of tests/tools/reduced_timing.py: G = Bhat^T Bhat of the fp64 problem's preconditioner (its own Bhat buffer, rank + 1 columns) `repeats` times by
 * the preconditioner's scalar kernel (parent_ms_out[r]) and by the fixed-size model's matrix-core kernels (mfma_ms_out[r]: partial tiles and their sum), device time of
 * repeat r each, after one untimed run of both.  *max_diff_out (may be NULL): the largest |difference| of the two results over the lower triangle, relative to the largest
 * |entry|.  Refused without a preconditioner and on an fp32 problem. */
int lssvm_mi355_problem_time_gram_kernels(lssvm_mi355_problem *p, int repeats, double *parent_ms_out, double *mfma_ms_out, double *max_diff_out);

/* The dense SPD toolbox of the device-factored fixed-size fits alone (lssvm_mi355_problem_fit_reduced_dev), on the caller's HOST arrays: upload, the
 * toolbox's kernels on device 0, download; everything row major float64, 1 <= m <= 1024, ms_out (may be NULL): device time of the kernels between two events.
 *   _cholesky      L L^T = A + nu I from the LOWER triangle of A (m x m; what stands above the diagonal is never read).  L_out: m x m, exact zeros above the diagonal.
 *                  *status_out: 0, or 1 + the column whose pivot was not positive and finite (L_out is then all zeros); the call returns LSSVM_SUCCESS either way.
 *   _solve         L z = b_c, L^T x_c = z for the k rows b_c of B (k x m; 1 <= k <= 4096) and the lower triangle of L: X_out k x m.  Row c does not depend on k.
 *   _invert_lower  V = L^-1 by block rows, triangular solves against the diagonal blocks: V_out m x m, exact zeros above the diagonal.
 * LSSVM_ERR_INVALID_ARGUMENT before a device is touched: m outside 1 ... 1024, k outside 1 ... 4096, a NULL A / L / B / L_out / X_out / V_out / status_out. */
int lssvm_mi355_dense_cholesky(const double *A, size_t m, double nu, double *L_out, uint64_t *status_out, double *ms_out);
int lssvm_mi355_dense_solve(const double *L, size_t m, const double *B, size_t k, double *X_out, double *ms_out);
int lssvm_mi355_dense_invert_lower(const double *L, size_t m, double *V_out, double *ms_out);

/* option names understood by lssvm_mi355_set_option / _get_option besides the fourteen documented in plssvm_amd.h:
 *   "force_collective" 1 = run the per-matvec RCCL collective even with a world of 1 (testing aid; default 0)
 *   "skip_collective"  1 = problems created with world > 1 need no communicator and do NOT exchange their partial K*v (testing aid:
 *                      lets one GPU evaluate every rank's share in turn; default 0)
 *   ("rebalance_after": above)
 * and, accepted with the value 0 everywhere but effective in development builds only:
 *   "debug_ablate"  timing-only ablation bits of the fp32 tile kernels (-DLSSVM_ENABLE_ABLATION; results are wrong when != 0)
 *   "pair_lag"      256-row workgroups: plane-chunk steps waves 4-7 run behind waves 0-3 (make DEV=1: 0, 1, 3; the shipped library instantiates 0, lock step)
 */

#ifdef __cplusplus
}
#endif
#endif /* PLSSVM_AMD_TESTING_H */
