/*
 * lssvm_reduced.hip -- the fixed-size (reduced, "subset of regressors") LS-SVM of a resident problem (lssvm_mi355_problem_fit_reduced, _landmark_gram,
 * lssvm_mi355_fit_reduced_*).
 *
 * With m landmarks L, sigma = 1 / C, Phi = K(X, X_L) (N x m, double, from the resident data exactly as the preconditioner evaluates K_Nm: k_landmark_block) and
 * K_mm = Phi[L, :] the model minimises 1/2 beta^T K_mm beta + C/2 sum_i (y_i - Phi_i beta - b)^2.  The device forms the lower triangle of St = Pt^T Pt for
 * Pt = [Phi | 1 | y_0 ... y_{k-1}], the host solves (include/plssvm_amd.h has the formulas).  No CG and no n x n pass.
 *
 * Pt is produced in row slabs of `slab_rows` rows, COLUMN by column (a column is contiguous over the rows), so the contraction index of Pt^T Pt is contiguous in both
 * operands.  k_reduced_gram: one workgroup owns (a 128 x 128 tile on or below the diagonal, RG_RANGE rows of the slab) and leaves its partial tile; the four waves hold
 * 64 x 64 each as sixteen accumulators of v_mfma_f64_16x16x4_f64.  k_reduced_sum adds the partial tiles to the running St in ascending row order.  RG_RANGE is a
 * constant: the order in which an entry is summed depends on N and slab_rows only, never on the number of columns -- so row c of a call with k right-hand sides has the
 * bits of the call with that right-hand side alone.  No atomics, no scratch.  Compiled for gfx950 only.
 *
 * Exact leave-one-out scores over a cost grid (lssvm_mi355_problem_fit_reduced_loo, _reduced_leverage, lssvm_mi355_fit_reduced_loo_*), leave-one-out
 * with the landmark set held fixed: the fit is a linear smoother, so with M + nu I = L L^T, V = L^-1 and Phic = Phi - 1 s^T / N the leverage is h_ii = 1 / N + |V phic_i|^2
 * and the model refitted without point i predicts y_i - (y_i - f(x_i)) / (1 - h_ii) at x_i.  Pass 1 is reduced_gram; per cost the host factors (factor_reduced,
 * solve_reduced: the code of fit_reduced) and inverts L; pass 2 evaluates the slabs again and k_reduced_leverage forms Phic [V^T | beta] on the matrix cores per slab and
 * cost, keeping only the rows' squared norms, the fitted and the leave-one-out values.
 *
 * Per-point weights w_i >= 0 (lssvm_mi355_problem_fit_reduced_weighted, _fit_reduced_loo_weighted, _landmark_gram_weighted): St = Pt^T diag(w) Pt and
 * W = sum w_i wherever N stands.  k_reduced_gram<true> multiplies both staged operands by sqrt(w_i) (formed on the host, uploaded once per call; the slab stays unscaled),
 * k_reduced_leverage multiplies by w_i; everything between them takes W as the double it took N as.  Without weights every call launches what it launched before.
 *
 * The leave-one-out scores over a (gamma, cost) grid on one problem (lssvm_mi355_problem_fit_reduced_grid, _landmark_acc, lssvm_mi355_fit_reduced_grid_*; DESIGN.md
 * section 17): what a kernel value is made from, D = sum_f (a_f - b_f)^2 or sum_f a_f b_f, does not depend on gamma.  GridSlabs forms it once per slab and pass --
 * k_landmark_acc (the loop of k_landmark_block) or k_landmark_product (the dot products on v_mfma_f64_16x16x4_f64, the norm expansion for rbf) -- and k_kernel_values
 * writes the Phi columns of a gamma from it; the Gram pass, the dense steps and the leverage kernel per (gamma, cost) are the ones above.
 *
 * The leave-one-out scores of every prefix rank from one fit (lssvm_mi355_problem_fit_reduced_rank_path, _reduced_leverage_prefix, lssvm_mi355_fit_reduced_rank_path_*;
 * DESIGN.md section 18): the landmark list is ordered, and M, L, V = L^-1 and z = L^-1 rhs of the first r landmarks are the leading blocks of the rank-m ones.  Pass 1 and
 * the dense steps per cost are the ones above (the host's solve split into its forward and backward half: z is kept, the back substitution runs on every leading block);
 * in pass 2 k_reduced_leverage_prefix forms Phic V^T as k_reduced_leverage does and takes the running sums of u^2 and u z_c out of its accumulators at the checkpoints.
 * Every prefix model of a cost takes the nu of the full rank.
 *
 * The same model from a STREAM of chunks (lssvm_mi355_reduced_stream_*; the end of this file): St is additive over rows, so a handle that owns the
 * landmark ROWS, K_mm, the running St and one pending slab takes the points piece by piece, without a resident problem.  k_cross_product -- the sibling of
 * k_landmark_product for rows that are in no problem, both operands centred as they are staged -- evaluates a chunk's D at the slab's fill position; k_kernel_values,
 * enqueue_gram, the dense steps per cost and k_reduced_leverage are the ones above, unchanged.  The state after any sequence of updates is the state one update of the
 * concatenated rows leaves: no result depends on the cuts.
 */
#include "lssvm_dense.hip.hpp"
#include "lssvm_landmark.hip.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <optional>

namespace lssvm {

namespace {

/* (RG_TW, RG_KC, RG_LS, RG_RANGE, RG_TILE: lssvm_dense.hip.hpp, with what lssvm_logistic.hip shares of this file) */

/* the 1 column and the y columns of Pt beside Phi, in double: column c of `out` (ld doubles apart) is 1 (c = 0) or right-hand side c - 1; exact zeros from row N on */
template <typename T>
__global__ __launch_bounds__(256) void k_reduced_aux(const T *__restrict__ Y, size_t N, size_t row0, double *__restrict__ out, size_t ld) {
    const size_t local = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    const size_t i = row0 + local;
    const int c = blockIdx.y;
    double v = 0.0;
    if (i < N) v = c == 0 ? 1.0 : static_cast<double>(Y[static_cast<size_t>(c - 1) * N + i]);
    out[static_cast<size_t>(c) * ld + local] = v;
}

/* part[tile][chunk] = A^T B over the rows [chunk RG_RANGE, min((chunk + 1) RG_RANGE, rows)) of the slab, A = the columns 128 bj ... and B = the columns 128 bk ... of the
 * column-major `slab` (ld doubles between two columns; columns from `cols` on count as zeros and are never read; `rows` is a multiple of RG_KC), for tile = (bj, bk),
 * bk <= bj.  Both operands go through LDS: eight threads load the 16 rows of a column of a step as one 128-byte line, the fragments are read as in tile_matvec_f64
 * (lane 16 q + r: column r of the block, row q of the k-step).  A diagonal tile stages and reads ONE operand.  The result of a lane: column r of B, rows q + 4 i of A.
 * Two waves per SIMD (at most 256 registers): the other workgroup of the CU computes while this one waits at its barriers.
 * WEIGHTED: the result is A^T diag(w) B.  `q` holds sqrt(w) for the slab's rows (indexed like them, zeros from row N on) and BOTH operands are
 * multiplied by it between stage_load and stage_store -- one f64x2 of q per step and thread, one product per staged pair; the slab stays as it is.  sqrt(w) on both sides
 * and not w on one: a diagonal tile keeps its single operand, and every partial tile is a Gram matrix (its diagonal a sum of squares), which the Cholesky factorisation
 * behind it rests on.  The `false` instantiation is the kernel as it was: q is not read. */
template <bool WEIGHTED>
__global__ __launch_bounds__(256, 2) void k_reduced_gram(const double *__restrict__ slab, size_t ld, int cols, int rows, int max_chunks, double *__restrict__ part,
                                                         const double *__restrict__ q) {
    __shared__ __attribute__((aligned(16))) double As[RG_TW * RG_LS];
    __shared__ __attribute__((aligned(16))) double Bs_own[RG_TW * RG_LS];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int r = lane & 15, qd = lane >> 4;

    const int tile = blockIdx.x, chunk = blockIdx.y;
    int bj = 0;
    while ((bj + 1) * (bj + 2) / 2 <= tile) ++bj;
    const int bk = tile - bj * (bj + 1) / 2;
    const bool diag = bj == bk;
    const double *Bs = diag ? As : Bs_own;

    const int row_begin = chunk * RG_RANGE;
    const int row_end = min(row_begin + RG_RANGE, rows);
    const int nsteps = (row_end - row_begin) / RG_KC;

    // staging: thread -> (column srow [+ 32 p] of the tile, rows 2 sseg, 2 sseg + 1 of the step)
    const int srow = tid >> 3, sseg = tid & 7;
    const double *Ag[4], *Bg[4];
    bool a_in[4], b_in[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int ca = bj * RG_TW + srow + 32 * p, cb = bk * RG_TW + srow + 32 * p;
        a_in[p] = ca < cols;
        b_in[p] = !diag && cb < cols;
        Ag[p] = slab + static_cast<size_t>(a_in[p] ? ca : 0) * ld + row_begin + 2 * sseg;
        Bg[p] = slab + static_cast<size_t>(b_in[p] ? cb : 0) * ld + row_begin + 2 * sseg;
    }
    const int lds_w = srow * RG_LS + 2 * sseg;
    f64x2 sa[4], sb[4];
    f64x2 sq = { 0.0, 0.0 };  // WEIGHTED: sqrt(w) of the step's rows 2 sseg, 2 sseg + 1
    const f64x2 zero2 = { 0.0, 0.0 };
    const double *qg = WEIGHTED ? q + row_begin + 2 * sseg : nullptr;
    auto stage_load = [&](int s) {
        if constexpr (WEIGHTED) sq = *reinterpret_cast<const f64x2 *>(qg + s * RG_KC);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            sa[p] = a_in[p] ? *reinterpret_cast<const f64x2 *>(Ag[p] + s * RG_KC) : zero2;
            sb[p] = b_in[p] ? *reinterpret_cast<const f64x2 *>(Bg[p] + s * RG_KC) : zero2;
        }
    };
    auto stage_store = [&]() {
        if constexpr (WEIGHTED) {  // (here and not behind the loads: the step's MFMAs stand between a load and its first use)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                sa[p] *= sq;
                if (!diag) sb[p] *= sq;
            }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *reinterpret_cast<f64x2 *>(As + lds_w + p * 32 * RG_LS) = sa[p];
            if (!diag) *reinterpret_cast<f64x2 *>(Bs_own + lds_w + p * 32 * RG_LS) = sb[p];
        }
    };

    f64x4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            acc[mt][nt] = f64x4{ 0.0, 0.0, 0.0, 0.0 };
            // the start values live in the accumulators' OWN registers (C == D for every MFMA of a chain): lssvm_tile_f64_wide.hip.hpp has the hazard this keeps away
            asm volatile("" : "+v"(acc[mt][nt]));
        }

    if (nsteps > 0) {
        stage_load(0);
        stage_store();
    }
    __syncthreads();
    const double *Ab = As + (wr * 64 + r) * RG_LS + qd;
    const double *Bb = Bs + (wc * 64 + r) * RG_LS + qd;
    for (int s = 0; s < nsteps; ++s) {
        const bool has_next = s + 1 < nsteps;
        if (has_next) stage_load(s + 1);
#pragma unroll
        for (int ks = 0; ks < RG_KC / 4; ++ks) {
            double av[4], bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                av[t] = Ab[t * 16 * RG_LS + ks * 4];
                bv[t] = Bb[t * 16 * RG_LS + ks * 4];
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
        }
        __syncthreads();  // (every wave has read this step)
        if (has_next) {
            stage_store();
            __syncthreads();
        }
    }

    double *out = part + (static_cast<size_t>(tile) * max_chunks + chunk) * RG_TILE;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) out[(wr * 64 + mt * 16 + qd + 4 * i) * RG_TW + wc * 64 + nt * 16 + r] = acc[mt][nt][i];
}

/* St[tile] += part[tile][0] + part[tile][1] + ... : the chunks in ascending row order behind what the earlier slabs left, one thread per entry */
__global__ __launch_bounds__(256) void k_reduced_sum(const double *__restrict__ part, int chunks, int max_chunks, double *__restrict__ St) {
    const size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    const size_t tile = blockIdx.y;
    double acc = St[tile * RG_TILE + e];
    for (int c = 0; c < chunks; ++c) acc += part[(tile * max_chunks + c) * RG_TILE + e];
    St[tile * RG_TILE + e] = acc;
}

}  // namespace

int tiles_of(int cols) { return (cols + RG_TW - 1) / RG_TW; }

/* St of one slab into the running sum: `rows` (a multiple of 256) rows of the column-major slab; `q`: sqrt(w) of these rows (`rows` doubles) for the weighted sum, or NULL */
void enqueue_gram(const double *slab, size_t ld, int cols, int rows, int max_chunks, double *part, double *St, hipStream_t st, const double *q) {
    const int nt = tiles_of(cols), ntri = nt * (nt + 1) / 2, chunks = (rows + RG_RANGE - 1) / RG_RANGE;
    if (q != nullptr) {
        hipLaunchKernelGGL(k_reduced_gram<true>, dim3(ntri, chunks), dim3(256), 0, st, slab, ld, cols, rows, max_chunks, part, q);
    } else {
        hipLaunchKernelGGL(k_reduced_gram<false>, dim3(ntri, chunks), dim3(256), 0, st, slab, ld, cols, rows, max_chunks, part, q);
    }
    hipLaunchKernelGGL(k_reduced_sum, dim3(RG_TILE / 256, ntri), dim3(256), 0, st, part, chunks, max_chunks, St);
    LSSVM_HIP_CHECK(hipGetLastError());
}

/* the tiles of St on the host -> cols x cols row major, the upper triangle the copy of the lower */
void unpack_tiles(const std::vector<double> &tiles, int cols, std::vector<double> &G) {
    const int nt = tiles_of(cols);
    G.assign(static_cast<size_t>(cols) * cols, 0.0);
    for (int bj = 0; bj < nt; ++bj) {
        for (int bk = 0; bk <= bj; ++bk) {
            const double *t = &tiles[static_cast<size_t>(bj * (bj + 1) / 2 + bk) * RG_TILE];
            for (int a = 0; a < RG_TW && bj * RG_TW + a < cols; ++a) {
                const int j = bj * RG_TW + a;
                for (int b = 0; b < RG_TW && bk * RG_TW + b <= j; ++b) {
                    const int k = bk * RG_TW + b;
                    G[static_cast<size_t>(j) * cols + k] = G[static_cast<size_t>(k) * cols + j] = t[a * RG_TW + b];
                }
            }
        }
    }
}

/* (SlabPlan: lssvm_dense.hip.hpp) */
namespace {

/* the k right-hand sides (k x N, the problem's type) on the device, or none of them for Y = NULL */
template <typename T>
struct RhsOnDevice {
    DevBuf<T> Y;
    int k = 0;
    RhsOnDevice(const void *Y_host, int num_rhs, size_t N, hipStream_t st) {
        if (Y_host == nullptr) return;
        k = num_rhs;
        Y.alloc_zero(static_cast<size_t>(k) * N, st);
        LSSVM_HIP_CHECK(hipMemcpyAsync(Y.p, Y_host, static_cast<size_t>(k) * N * sizeof(T), hipMemcpyHostToDevice, st));
    }
};

/* slab s of Pt into `slab`: the m columns of Phi and, where there are right-hand sides, the [1 | Y] columns behind them */
template <typename T>
void enqueue_slab(const LandmarkBlock<T> &block, int m, const SlabPlan &plan, int s, const RhsOnDevice<T> &rhs, double *slab, hipStream_t st) {
    block.enqueue(plan.row0(s), plan.rows256(s), slab, plan.ld);
    if (rhs.Y.p != nullptr)
        hipLaunchKernelGGL(k_reduced_aux<T>, dim3(plan.rows256(s) / 256, 1 + rhs.k), dim3(256), 0, st, rhs.Y.p, plan.N, plan.row0(s), slab + static_cast<size_t>(m) * plan.ld, plan.ld);
}

/* the timing aids: one untimed run of `launch`, then `repeats` runs between two events; `before` is enqueued ahead of each, outside the timed span */
template <typename Before, typename Launch>
void timed_repeats(hipStream_t st, int repeats, double *out_ms, Before before, Launch launch) {
    Event ev[2];
    for (Event &e : ev) e.create(true);
    for (int rep = -1; rep < repeats; ++rep) {  // (-1: the untimed run)
        before();
        LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
        launch();
        LSSVM_HIP_CHECK(hipGetLastError());
        LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
        LSSVM_HIP_CHECK(hipEventSynchronize(ev[1].e));
        if (rep >= 0) out_ms[rep] = elapsed_ms(ev[0], ev[1]);
    }
}

/* ---- the host's part of a fit, in double, shared by fit_reduced and fit_reduced_loo: M = S - s s^T / N + sigma K_mm (lower triangle), (M + nu I) = L L^T,
 * (M + nu I) beta_c = t_c - s eta_c / N, b_c = (eta_c - s^T beta_c) / N ---- */
}  // namespace

double factor_reduced(const std::vector<double> &St, const std::vector<double> &Kmm, int m, int cols, double Nd, double sigma, std::vector<double> &L) {
    const double *s = &St[static_cast<size_t>(m) * cols];
    std::vector<double> M(static_cast<size_t>(m) * m, 0.0);
    for (int j = 0; j < m; ++j)
        for (int l = 0; l <= j; ++l) M[static_cast<size_t>(j) * m + l] = St[static_cast<size_t>(j) * cols + l] - s[j] * s[l] / Nd + sigma * Kmm[static_cast<size_t>(j) * m + l];
    return cholesky_with_jitter(M, m, "the matrix of the reduced model", L);
}

namespace {

/* the two halves of a solve, for right-hand side c and the leading r x r block of the m x m factor L (solve_reduced: r = m; the rank path, DESIGN.md section 18: every
 * checkpoint r <= m -- the factor of a leading block is the leading block of the factor, and z of the block is z[:r]) */
void forward_reduced(const std::vector<double> &St, const std::vector<double> &L, int m, int c, int cols, double Nd, double *z) {
    const double *s = &St[static_cast<size_t>(m) * cols];
    const double *t = &St[static_cast<size_t>(m + 1 + c) * cols];
    const double eta = t[m];
    for (int j = 0; j < m; ++j) {  // L z = t_c - s eta_c / N
        double v = t[j] - s[j] * eta / Nd;
        for (int l = 0; l < j; ++l) v -= L[static_cast<size_t>(j) * m + l] * z[l];
        z[j] = v / L[static_cast<size_t>(j) * m + j];
    }
}

double backward_reduced(const std::vector<double> &St, const std::vector<double> &L, int m, int r, int c, int cols, double Nd, const double *z, double *beta) {
    const double *s = &St[static_cast<size_t>(m) * cols];
    const double eta = St[static_cast<size_t>(m + 1 + c) * cols + m];
    for (int j = r - 1; j >= 0; --j) {  // L_r^T beta = z[:r]
        double v = z[j];
        for (int l = j + 1; l < r; ++l) v -= L[static_cast<size_t>(l) * m + j] * beta[l];
        beta[j] = v / L[static_cast<size_t>(j) * m + j];
    }
    double sb = 0.0;
    for (int j = 0; j < r; ++j) sb += s[j] * beta[j];
    return -((eta - sb) / Nd);
}

}  // namespace

void solve_reduced(const std::vector<double> &St, const std::vector<double> &L, int m, int k, int cols, double Nd, double *betas_out, double *rhos_out) {
    std::vector<double> z(static_cast<size_t>(m));
    for (int c = 0; c < k; ++c) {
        forward_reduced(St, L, m, c, cols, Nd, z.data());
        rhos_out[c] = backward_reduced(St, L, m, m, c, cols, Nd, z.data(), betas_out + static_cast<size_t>(c) * m);
    }
}

namespace {

/* row n of `out` (ldb doubles apart, zeros beyond the diagonal) = row n of V = L^-1 by forward substitution, row by row: V[n][:] = (e_n - sum_{l < n} L[n][l] V[l][:]) / L[n][n],
 * the l ascending for every entry.
 * NOT to be merged with invert_lower_by_reciprocal (lssvm_precond.hip), which multiplies by 1 / L[n][n]: either change moves the bits of every leverage or of every
 * preconditioned solve. */
void invert_lower_rows(const std::vector<double> &L, int m, double *out, size_t ldb) {
    for (int n = 0; n < m; ++n) {
        double *vn = out + static_cast<size_t>(n) * ldb;
        std::fill(vn, vn + ldb, 0.0);
        vn[n] = 1.0;
        for (int l = 0; l < n; ++l) {
            const double f = L[static_cast<size_t>(n) * m + l];
            const double *vl = out + static_cast<size_t>(l) * ldb;
            for (int j = 0; j <= l; ++j) vn[j] -= f * vl[j];
        }
        const double d = L[static_cast<size_t>(n) * m + n];
        for (int j = 0; j <= n; ++j) vn[j] /= d;
    }
}

/* One cost of a leave-one-out grid on the host, in double: M, L, beta and rho as fit_reduced forms them, V = L^-1; fills the cost's betas (k x m), rhos (k), ybar (k) and
 * the leverage kernel's operand Bt (m rows of V, then the betas; ldb doubles apart); returns nu.  Shared by fit_reduced_loo and fit_reduced_grid. */
double host_operand(const std::vector<double> &St, const std::vector<double> &Kmm, int m, int k, int cols, double Nd, double cost, int ldb, double *betas, double *rhos,
                    std::vector<double> &L, std::vector<double> &Bt, double *ybar) {
    const double nu = factor_reduced(St, Kmm, m, cols, Nd, 1.0 / cost, L);
    solve_reduced(St, L, m, k, cols, Nd, betas, rhos);
    invert_lower_rows(L, m, Bt.data(), static_cast<size_t>(ldb));
    for (int c = 0; c < k; ++c) {
        double *row = &Bt[static_cast<size_t>(m + c) * ldb];
        std::fill(row, row + ldb, 0.0);
        std::copy(betas + static_cast<size_t>(c) * m, betas + static_cast<size_t>(c + 1) * m, row);
        ybar[c] = St[static_cast<size_t>(m + 1 + c) * cols + m] / Nd;
    }
    return nu;
}

/* ---- the same steps on the device (lssvm_dense.hip) ---- */
}  // namespace

/* trace(M) from the host copies, with factor_reduced's expression and cholesky_with_jitter's order: where no attempt fails, nu has the host path's bits */
double reduced_trace(const std::vector<double> &St, const std::vector<double> &Kmm, int m, int cols, double Nd, double sigma) {
    const double *s = &St[static_cast<size_t>(m) * cols];
    std::vector<double> diag(static_cast<size_t>(m));
    for (int j = 0; j < m; ++j) diag[j] = St[static_cast<size_t>(j) * cols + j] - s[j] * s[j] / Nd + sigma * Kmm[static_cast<size_t>(j) * m + j];
    double trace = 0.0;
    for (int k = 0; k < m; ++k) trace += diag[k];
    return trace;
}

/* what one cost needs on the device besides St and K_mm, held over the costs of a grid (the struct: lssvm_dense.hip.hpp) */
DenseFit::DenseFit(int rank, int num_rhs, hipStream_t stream) :
    dense(rank, num_rhs, stream), watch(stream), betas_host(static_cast<size_t>(num_rhs) * rank), rhos_host(static_cast<size_t>(num_rhs)), m(rank), k(num_rhs), st(stream) {
    betas.alloc_zero(static_cast<size_t>(k) * m, st);
    rhos.alloc_zero(static_cast<size_t>(k), st);
}

double DenseFit::run(const ReducedOnDevice &dev, const std::vector<double> &St, const std::vector<double> &Kmm, int cols, double Nd, double sigma, double *Bt_op, int ldb,
                     double *betas_out, double *rhos_out, lssvm_dense_info *d, double *device_ms_out, double *Z_op) {
    {
        const double trace = reduced_trace(St, Kmm, m, cols, Nd, sigma);
        LSSVM_REQUIRE(std::isfinite(trace) && trace > 0.0, "the matrix of the reduced model has no positive finite trace");
        double nu = DBL_EPSILON * trace;
        for (int attempt = 0; attempt < 7; ++attempt, nu *= 10.0) {
            dense.begin_attempt();
            watch.mark(0);
            dense.enqueue_assemble(dev.St.p, dev.Kmm.p, k, Nd, sigma, nu);
            watch.mark(1);
            dense.enqueue_factor();
            watch.mark(2);
            dense.enqueue_solve(k, betas.p, static_cast<size_t>(m), Bt_op != nullptr ? Bt_op + static_cast<size_t>(m) * ldb : nullptr, static_cast<size_t>(ldb), true, Nd, rhos.p);
            watch.mark(3);
            if (Bt_op != nullptr) {
                dense.enqueue_invert(Bt_op, ldb);
                watch.mark(4);
            }
            if (Z_op != nullptr) dense.enqueue_forward(k, Z_op, static_cast<size_t>(ldb));  // (the rank path: z_c beside V, ldb doubles apart)
            LSSVM_HIP_CHECK(hipMemcpyAsync(betas_host.data(), betas.p, betas.count * sizeof(double), hipMemcpyDeviceToHost, st));
            LSSVM_HIP_CHECK(hipMemcpyAsync(rhos_host.data(), rhos.p, rhos.count * sizeof(double), hipMemcpyDeviceToHost, st));
            if (dense.status() != 0) continue;  // (the wait; a failed attempt's kernels have all returned at once and written nothing)
            // the caller's arrays are written only now: where every attempt fails they stay as they were, as on the host path
            std::copy(betas_host.begin(), betas_host.end(), betas_out);
            std::copy(rhos_host.begin(), rhos_host.end(), rhos_out);
            DenseTimes t;
            watch.read(Bt_op != nullptr, t);
            if (device_ms_out != nullptr) *device_ms_out = t.assemble_ms + t.factor_ms + t.solve_ms + t.invert_ms;
            if (d != nullptr) {
                *d = lssvm_dense_info{};
                d->rank = static_cast<uint64_t>(m);
                d->block = DENSE_BLOCK;
                d->attempts = static_cast<uint64_t>(attempt + 1);
                d->launches = dense.launches();
                d->jitter = nu;
                d->assemble_ms = t.assemble_ms;
                d->factor_ms = t.factor_ms;
                d->solve_ms = t.solve_ms;
                d->invert_ms = t.invert_ms;
            }
            return nu;
        }
        throw Error(LSSVM_ERR_INTERNAL, "the matrix of the reduced model could not be factored (jitter up to " + std::to_string(nu / 10.0) + ")");
    }
}

namespace {

/* ---- the leave-one-out pass ---- */
constexpr int LV_LSA = RG_TW + 16;  // doubles between two columns of Phi in LDS: the four k-rows of an MFMA's A fragments start 32 banks apart

/* One workgroup: 128 rows of the column-major `slab` (as k_reduced_gram takes it: ld doubles between columns, rows padded to 256 with zeros) times ALL columns of the operand
 * Bt -- row n of Bt (ldb doubles apart, ldb >= m rounded up to 16) is column n of the m x (m + k) matrix B of the header: row n of V = L^-1 for n < m, beta_{n-m} from m on.
 * T = (Phi - 1 shift^T) B is accumulated in 128 x 128 tiles (four waves of 64 x 64, sixteen accumulators of v_mfma_f64_16x16x4_f64 each, as k_reduced_gram) over the
 * column blocks of B in ascending order and never stored: the squares of the columns below m are added to the row's running sum, the columns from m on are the fitted
 * values.  Phi goes through LDS with `shift` SUBTRACTED ON THE WAY (centring after the product would cancel for nearly constant kernels), a step is 16 columns of Phi;
 * Bt through LDS as k_reduced_gram's operands.  A column block wholly inside V^T contracts over j < 128 (bk + 1) only (V is lower triangular: the blocks above the diagonal
 * are never read), any other over j < m rounded up to 16; an entry V[n][j] with j > n is replaced by 0 as it is staged, whatever the buffer holds.  Columns of Phi from m
 * on and rows of Bt from m + k on count as zeros and are never read.
 * A row's sum of squares: per column block a lane's four column tiles in ascending order, then the sixteen lanes that share the row (xor 1, 2, 4, 8), the blocks one
 * behind the other in LDS (the sums are not held in registers across a block), at the end the two column waves -- an order that depends on m only. A row's values depend on that row, Bt, shift and ybar only.  No atomics, no scratch.
 * h_out[i] = inv_n + sum; f_out[c ldo + i] = T[i][m + c] + ybar[c] (ybar NULL: 0); loo_out[c ldo + i] = y - (y - f) / (1 - h) with y = ycols[c ld + i] (loo_out NULL:
 * not formed).  Rows from `rows` on write nothing.
 * `w` (NULL: the unweighted model, the expressions above): the rows' weights, indexed like the slab's rows; then h_out[i] = w[i] (inv_n + sum) with
 * inv_n = 1 / sum of the weights, and a row of weight 0 -- h = 0, it took no part in the fit -- gets loo = f itself (y - (y - f) / 1 rounds twice). */
__global__ __launch_bounds__(256, 2) void k_reduced_leverage(const double *__restrict__ slab, size_t ld, int rows, int m, int k, const double *__restrict__ Bt, int ldb,
                                                             const double *__restrict__ shift, const double *__restrict__ ybar, double inv_n, const double *__restrict__ ycols,
                                                             double *__restrict__ h_out, double *f_out, double *__restrict__ loo_out, size_t ldo, const double *__restrict__ w) {
    __shared__ __attribute__((aligned(16))) double As[RG_KC * LV_LSA];
    __shared__ __attribute__((aligned(16))) double Bs[RG_TW * RG_LS];
    __shared__ double hs[3 * RG_TW];  // the rows' sums of squares of the two column waves, then h

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int r = lane & 15, qd = lane >> 4;
    const int row0 = blockIdx.x * RG_TW;
    const int nblocks = (m + k + RG_TW - 1) / RG_TW;
    const int m16 = (m + RG_KC - 1) / RG_KC * RG_KC;

    // staging of Phi: thread -> (column akk of the step, rows 2 aseg + 32 p, 2 aseg + 32 p + 1 of the workgroup's 128)
    const int akk = tid >> 4, aseg = tid & 15;
    const double *Ag = slab + static_cast<size_t>(akk) * ld + row0 + 2 * aseg;
    const int a_lds = akk * LV_LSA + 2 * aseg;
    // staging of Bt: thread -> (row srow + 32 p of the column block, columns 2 sseg, 2 sseg + 1 of the step), as k_reduced_gram
    const int srow = tid >> 3, sseg = tid & 7;
    const int b_lds = srow * RG_LS + 2 * sseg;
    const f64x2 zero2 = { 0.0, 0.0 };
    f64x2 sa[4], sb[4];

    // lane 16 qd of a wave owns the sums of the wave's rows qd + 4 i + 16 mt: nobody else touches them before the barrier behind the last block
    double *hrow = hs + wc * RG_TW + wr * 64 + qd;
    if (r == 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) hrow[4 * e] = 0.0;
    }

    const double *Ab = As + qd * LV_LSA + wr * 64 + r;
    const double *Bb = Bs + (wc * 64 + r) * RG_LS + qd;

    for (int bk = 0; bk < nblocks; ++bk) {
        const int nsteps = ((bk + 1) * RG_TW <= m ? (bk + 1) * RG_TW : m16) / RG_KC;
        const int n0 = bk * RG_TW + srow;  // this thread's rows of Bt: n0 + 32 p
        auto stage_load = [&](int s) {
            const int j = s * RG_KC + akk;
            const bool a_in = j < m;
            const double sh = a_in ? shift[j] : 0.0;
            const double *a = Ag + static_cast<size_t>(s) * RG_KC * ld;
            const int jb = s * RG_KC + 2 * sseg;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                f64x2 v = a_in ? *reinterpret_cast<const f64x2 *>(a + 32 * p) : zero2;
                if (a_in) {
                    v[0] -= sh;
                    v[1] -= sh;
                }
                sa[p] = v;
                const int n = n0 + 32 * p;
                const int last = n < m ? n : m16;  // the last column of Bt's row that counts: the diagonal for a row of V, all of them for a beta
                f64x2 w = n < m + k ? *reinterpret_cast<const f64x2 *>(Bt + static_cast<size_t>(n) * ldb + jb) : zero2;
                if (jb > last) w[0] = 0.0;
                if (jb + 1 > last) w[1] = 0.0;
                sb[p] = w;
            }
        };
        auto stage_store = [&]() {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                *reinterpret_cast<f64x2 *>(As + a_lds + 32 * p) = sa[p];
                *reinterpret_cast<f64x2 *>(Bs + b_lds + p * 32 * RG_LS) = sb[p];
            }
        };

        f64x4 acc[4][4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                acc[mt][nt] = f64x4{ 0.0, 0.0, 0.0, 0.0 };
                // the start values live in the accumulators' OWN registers (C == D for every MFMA of a chain), as in k_reduced_gram
                asm volatile("" : "+v"(acc[mt][nt]));
            }

        stage_load(0);  // (the barrier that ended the block before lets every wave write: all of them have read its last step)
        stage_store();
        __syncthreads();
        for (int s = 0; s < nsteps; ++s) {
            const bool has_next = s + 1 < nsteps;
            if (has_next) stage_load(s + 1);
#pragma unroll
            for (int ks = 0; ks < RG_KC / 4; ++ks) {
                double av[4], bv[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    av[t] = Ab[ks * 4 * LV_LSA + t * 16];
                    bv[t] = Bb[t * 16 * RG_LS + ks * 4];
                }
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
            }
            __syncthreads();  // (every wave has read this step)
            if (has_next) {
                stage_store();
                __syncthreads();
            }
        }

        // a lane holds rows qd + 4 i of its four row tiles and column r of its four column tiles
        const int nw = bk * RG_TW + wc * 64 + r;  // its columns: nw + 16 nt
        if (bk * RG_TW < m) {
            // the squares of the columns of V^T: the lane's four columns in ascending order, the sixteen lanes of a row (xor 1, 2, 4, 8), then behind the blocks before
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    double v = 0.0;
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) v += nw + 16 * nt < m ? acc[mt][nt][i] * acc[mt][nt][i] : 0.0;
                    v += __shfl_xor(v, 1);
                    v += __shfl_xor(v, 2);
                    v += __shfl_xor(v, 4);
                    v += __shfl_xor(v, 8);
                    if (r == 0) hrow[4 * i + 16 * mt] += v;
                }
        }
        if ((bk + 1) * RG_TW > m) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int c = nw + 16 * nt - m;
                if (c >= 0 && c < k) {
                    const double yb = ybar != nullptr ? ybar[c] : 0.0;
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int row = row0 + wr * 64 + mt * 16 + qd + 4 * i;
                            if (row < rows) f_out[static_cast<size_t>(c) * ldo + row] = acc[mt][nt][i] + yb;
                        }
                }
            }
        }
    }

    __syncthreads();  // (and this workgroup's f_out is visible to all of it)
    const int lrow = tid & (RG_TW - 1);
    if (tid < RG_TW) {
        const double h = w != nullptr ? w[row0 + tid] * (inv_n + (hs[tid] + hs[RG_TW + tid])) : inv_n + (hs[tid] + hs[RG_TW + tid]);
        hs[2 * RG_TW + tid] = h;
        if (row0 + tid < rows) h_out[row0 + tid] = h;
    }
    __syncthreads();
    if (loo_out != nullptr && row0 + lrow < rows) {
        const double h = hs[2 * RG_TW + lrow];
        const bool left_out = w != nullptr && w[row0 + lrow] == 0.0;
        for (int c = tid >> 7; c < k; c += 2) {
            const double y = ycols[static_cast<size_t>(c) * ld + row0 + lrow];
            const double f = f_out[static_cast<size_t>(c) * ldo + row0 + lrow];
            loo_out[static_cast<size_t>(c) * ldo + row0 + lrow] = left_out ? f : y - (y - f) / (1.0 - h);
        }
    }
}

/* ---- the leave-one-out pass over every prefix rank ---- */
constexpr int PFX_KMAX = 4;        // right-hand sides per launch: 1 + PFX_KMAX running sums per row and column wave in LDS (the host launches once per group of four)
constexpr int PFX_SUMS = (1 + PFX_KMAX) * 2 * RG_TW;  // doubles: [sum][column wave][row of the workgroup]

/* The sibling of k_reduced_leverage for the rank path: the same slab layout, LDS staging (centring subtracted on the way in), masked staging of the triangular operand
 * and 128 x 128 tiles of v_mfma_f64_16x16x4_f64, four waves of 64 x 64.  The operand is V ALONE: row n of Vt (ldb doubles apart) is row n of V = L^-1, n < m; rows from m
 * on count as zeros and are never read, an entry V[n][j] with j > n is replaced by 0 as it is staged.  Z: row c (ldb doubles apart) is z_c, k <= PFX_KMAX rows, read below m
 * only.  ranks: num_ranks ascending checkpoints 1 <= r_q <= m.  Only the column blocks up to the one of the last checkpoint are formed.
 * After each 128-column block the tile U = (Phi - 1 shift^T) V^T stands in the accumulators.  A lane forms, for each of its sixteen rows and a column limit `lim`, the
 * 1 + k sums of u^2 and u z_c over its four columns below lim in ascending order (one fma each), then the sixteen lanes of the row add up (xor 1, 2, 4, 8): row_sums.
 *   a checkpoint r_q inside the block (128 bk < r_q <= 128 (bk + 1)): row_sums with lim = r_q, BEHIND the running sums of the blocks before, per column wave; the two
 *   column waves meet in LDS (cps) and one thread per row forms  h[q ldo + i] = inv_n + sum  (w given: w_i (inv_n + sum)),  f[(q k + c) ldo + i] = sum_c + ybar[c],
 *   loo[(q k + c) ldo + i] = y - (y - f) / (1 - h)  (a row of weight 0: f itself; loo_out NULL: not formed), as k_reduced_leverage's end does;
 *   then, where a block follows, row_sums with lim = m goes behind the running sums (`run`, LDS: the sums are not held in registers across a block).
 * So checkpoint q is (blocks before, ascending) + (its own masked block), then wave 0 + wave 1: an order that depends on m and r_q only -- not on the other checkpoints,
 * not on k (every sum is its own chain), not on N.  No atomics, no scratch.  Rows from `rows` on write nothing. */
__global__ __launch_bounds__(256, 2) void k_reduced_leverage_prefix(const double *__restrict__ slab, size_t ld, int rows, int m, int k, const double *__restrict__ Vt, int ldb,
                                                                    const double *__restrict__ Z, const int *__restrict__ ranks, int num_ranks, const double *__restrict__ shift,
                                                                    const double *__restrict__ ybar, double inv_n, const double *__restrict__ ycols, double *__restrict__ h_out,
                                                                    double *__restrict__ f_out, double *__restrict__ loo_out, size_t ldo, const double *__restrict__ w) {
    __shared__ __attribute__((aligned(16))) double As[RG_KC * LV_LSA];
    __shared__ __attribute__((aligned(16))) double Bs[RG_TW * RG_LS];
    __shared__ double run[PFX_SUMS];  // the running sums of the blocks before
    __shared__ double cps[PFX_SUMS];  // a checkpoint's sums, where the two column waves meet

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int r = lane & 15, qd = lane >> 4;
    const int row0 = blockIdx.x * RG_TW;
    const int nblocks = (ranks[num_ranks - 1] + RG_TW - 1) / RG_TW;
    const int m16 = (m + RG_KC - 1) / RG_KC * RG_KC;

    // staging of Phi and of Vt: as k_reduced_leverage
    const int akk = tid >> 4, aseg = tid & 15;
    const double *Ag = slab + static_cast<size_t>(akk) * ld + row0 + 2 * aseg;
    const int a_lds = akk * LV_LSA + 2 * aseg;
    const int srow = tid >> 3, sseg = tid & 7;
    const int b_lds = srow * RG_LS + 2 * sseg;
    const f64x2 zero2 = { 0.0, 0.0 };
    f64x2 sa[4], sb[4];

    // lane 16 qd of a wave owns the sums of the wave's rows qd + 4 i + 16 mt in `run`: nobody else touches them
    const int own = wc * RG_TW + wr * 64 + qd;  // + 4 i + 16 mt, + 2 RG_TW per sum
    if (r == 0) {
#pragma unroll
        for (int s = 0; s <= PFX_KMAX; ++s)
#pragma unroll
            for (int e = 0; e < 16; ++e) run[s * 2 * RG_TW + own + 4 * e] = 0.0;
    }

    const double *Ab = As + qd * LV_LSA + wr * 64 + r;
    const double *Bb = Bs + (wc * 64 + r) * RG_LS + qd;

    for (int bk = 0; bk < nblocks; ++bk) {
        const int nsteps = ((bk + 1) * RG_TW <= m ? (bk + 1) * RG_TW : m16) / RG_KC;
        const int n0 = bk * RG_TW + srow;  // this thread's rows of Vt: n0 + 32 p
        auto stage_load = [&](int s) {
            const int j = s * RG_KC + akk;
            const bool a_in = j < m;
            const double sh = a_in ? shift[j] : 0.0;
            const double *a = Ag + static_cast<size_t>(s) * RG_KC * ld;
            const int jb = s * RG_KC + 2 * sseg;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                f64x2 v = a_in ? *reinterpret_cast<const f64x2 *>(a + 32 * p) : zero2;
                if (a_in) {
                    v[0] -= sh;
                    v[1] -= sh;
                }
                sa[p] = v;
                const int n = n0 + 32 * p;  // the last column of the row that counts: the diagonal
                f64x2 vv = n < m ? *reinterpret_cast<const f64x2 *>(Vt + static_cast<size_t>(n) * ldb + jb) : zero2;
                if (jb > n) vv[0] = 0.0;
                if (jb + 1 > n) vv[1] = 0.0;
                sb[p] = vv;
            }
        };
        auto stage_store = [&]() {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                *reinterpret_cast<f64x2 *>(As + a_lds + 32 * p) = sa[p];
                *reinterpret_cast<f64x2 *>(Bs + b_lds + p * 32 * RG_LS) = sb[p];
            }
        };

        f64x4 acc[4][4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                acc[mt][nt] = f64x4{ 0.0, 0.0, 0.0, 0.0 };
                // the start values live in the accumulators' OWN registers (C == D for every MFMA of a chain), as in k_reduced_gram
                asm volatile("" : "+v"(acc[mt][nt]));
            }

        stage_load(0);  // (the barrier that ended the block before lets every wave write: all of them have read its last step)
        stage_store();
        __syncthreads();
        for (int s = 0; s < nsteps; ++s) {
            const bool has_next = s + 1 < nsteps;
            if (has_next) stage_load(s + 1);
#pragma unroll
            for (int ks = 0; ks < RG_KC / 4; ++ks) {
                double av[4], bv[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    av[t] = Ab[ks * 4 * LV_LSA + t * 16];
                    bv[t] = Bb[t * 16 * RG_LS + ks * 4];
                }
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
            }
            __syncthreads();  // (every wave has read this step)
            if (has_next) {
                stage_store();
                __syncthreads();
            }
        }

        // a lane holds rows qd + 4 i of its four row tiles and column r of its four column tiles: nw + 16 nt; z of these columns
        const int nw = bk * RG_TW + wc * 64 + r;
        double zr[PFX_KMAX][4];
#pragma unroll
        for (int c = 0; c < PFX_KMAX; ++c)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) zr[c][nt] = c < k && nw + 16 * nt < m ? Z[static_cast<size_t>(c) * ldb + nw + 16 * nt] : 0.0;
        // v[0]: the squares, v[1 + c]: the products with z_c, of row (mt, i) over the lane's columns below lim, then over the sixteen lanes of the row
        auto row_sums = [&](int lim, int mt, int i, double(&v)[1 + PFX_KMAX]) {
#pragma unroll
            for (int s = 0; s <= PFX_KMAX; ++s) v[s] = 0.0;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const double a = nw + 16 * nt < lim ? acc[mt][nt][i] : 0.0;
                v[0] = fma(a, a, v[0]);
#pragma unroll
                for (int c = 0; c < PFX_KMAX; ++c)
                    if (c < k) v[1 + c] = fma(a, zr[c][nt], v[1 + c]);
            }
#pragma unroll
            for (int s = 0; s <= PFX_KMAX; ++s) {
                if (s <= k) {
                    v[s] += __shfl_xor(v[s], 1);
                    v[s] += __shfl_xor(v[s], 2);
                    v[s] += __shfl_xor(v[s], 4);
                    v[s] += __shfl_xor(v[s], 8);
                }
            }
        };

        for (int q = 0; q < num_ranks; ++q) {
            const int rq = ranks[q];
            if ((rq - 1) / RG_TW != bk) continue;  // (the same for the whole workgroup)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    double v[1 + PFX_KMAX];
                    row_sums(rq, mt, i, v);
                    if (r == 0) {
                        const int at = own + 4 * i + 16 * mt;
#pragma unroll
                        for (int s = 0; s <= PFX_KMAX; ++s)
                            if (s <= k) cps[s * 2 * RG_TW + at] = run[s * 2 * RG_TW + at] + v[s];
                    }
                }
            __syncthreads();
            {
                const int lrow = tid & (RG_TW - 1), row = row0 + lrow;
                const double sum = cps[lrow] + cps[RG_TW + lrow];
                const double h = w != nullptr ? w[row] * (inv_n + sum) : inv_n + sum;
                if (row < rows) {
                    if (tid < RG_TW) h_out[static_cast<size_t>(q) * ldo + row] = h;
                    const bool left_out = w != nullptr && w[row] == 0.0;
                    for (int c = tid >> 7; c < k; c += 2) {
                        const double f = (cps[(1 + c) * 2 * RG_TW + lrow] + cps[(1 + c) * 2 * RG_TW + RG_TW + lrow]) + (ybar != nullptr ? ybar[c] : 0.0);
                        const size_t at = (static_cast<size_t>(q) * k + c) * ldo + row;
                        f_out[at] = f;
                        if (loo_out != nullptr) {
                            const double y = ycols[static_cast<size_t>(c) * ld + row];
                            loo_out[at] = left_out ? f : y - (y - f) / (1.0 - h);
                        }
                    }
                }
            }
            __syncthreads();  // (cps is free for the next checkpoint)
        }

        if (bk + 1 < nblocks) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    double v[1 + PFX_KMAX];
                    row_sums(m, mt, i, v);
                    if (r == 0) {
                        const int at = own + 4 * i + 16 * mt;
#pragma unroll
                        for (int s = 0; s <= PFX_KMAX; ++s)
                            if (s <= k) run[s * 2 * RG_TW + at] += v[s];
                    }
                }
        }
    }
}

/* ---- what every gamma of a (gamma, cost) grid shares ---- */
template <typename T>
struct PairOf;
template <>
struct PairOf<float> {
    using type = float __attribute__((ext_vector_type(2)));
};
template <>
struct PairOf<double> {
    using type = f64x2;
};

/* n[i] = the sum over the ldx held features (ascending) of x_if^2, in double: the squared norms k_landmark_product expands the rbf distance with */
template <typename T>
__global__ __launch_bounds__(256) void k_row_norms(const T *__restrict__ X, int ldx, size_t N, double *__restrict__ n) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= N) return;
    const T *xi = X + i * ldx;
    double acc = 0.0;
    for (int f = 0; f < ldx; ++f) {
        const double a = static_cast<double>(xi[f]);
        acc += a * a;
    }
    n[i] = acc;
}

/* D[l][i - row0] of k_landmark_acc with the dot products x_i . x_lm[l] on v_mfma_f64_16x16x4_f64: one workgroup owns 128 landmarks (blockIdx.y) x 128 rows of the slab
 * (blockIdx.x), the four waves hold 64 x 64 each as sixteen accumulators, exactly as k_reduced_gram.  The contraction runs over the ldx held features in steps of RG_KC = 16
 * (ldx is a multiple of 16); both operands go through LDS in k_reduced_gram's layout (RG_LS doubles between two points), converted to double as they are staged: eight
 * threads load the 16 features of a point as one 64-byte (fp32) or 128-byte (fp64) line.  The A operand are the landmarks' rows, gathered through lm[], the B operand the
 * slab's rows: a lane holds landmarks qd + 4 i of its four landmark tiles and row r of its four row tiles, so sixteen lanes write 128 contiguous bytes of a column of D.
 * Landmarks from m on and rows from N on count as zeros and are never read; landmarks from m on are not written, rows from N on are written as zeros.
 * rbf: D = n_i + n_l - 2 x_i . x_l with `norms` of k_row_norms, clamped at 0, and EXACTLY 0 where i == lm[l] (the expansion leaves a rounding there; K_mm's diagonal is
 * exactly 1, as on the ordered path).  Any other kernel type: the dot product.  No atomics, no scratch; the order of every sum depends on ldx only. */
template <typename T>
__global__ __launch_bounds__(256, 2) void k_landmark_product(const T *__restrict__ X, int ldx, int N, int row0, const int *__restrict__ lm, int m, int kernel_type,
                                                             const double *__restrict__ norms, double *__restrict__ D, size_t ldN) {
    using pair = typename PairOf<T>::type;
    __shared__ __attribute__((aligned(16))) double As[RG_TW * RG_LS];
    __shared__ __attribute__((aligned(16))) double Bs[RG_TW * RG_LS];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int r = lane & 15, qd = lane >> 4;
    const int l0 = blockIdx.y * RG_TW;             // the workgroup's first landmark
    const int local0 = blockIdx.x * RG_TW;         // ... and first row of the slab
    const int nsteps = ldx / RG_KC;

    // staging: thread -> (point srow [+ 32 p] of the tile, features 2 sseg, 2 sseg + 1 of the step), as k_reduced_gram
    const int srow = tid >> 3, sseg = tid & 7;
    const T *Ag[4], *Bg[4];
    bool a_in[4], b_in[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int la = l0 + srow + 32 * p, ib = row0 + local0 + srow + 32 * p;
        a_in[p] = la < m;
        b_in[p] = ib < N;
        Ag[p] = X + static_cast<size_t>(a_in[p] ? lm[la] : 0) * ldx + 2 * sseg;
        Bg[p] = X + static_cast<size_t>(b_in[p] ? ib : 0) * ldx + 2 * sseg;
    }
    const int lds_w = srow * RG_LS + 2 * sseg;
    f64x2 sa[4], sb[4];
    const f64x2 zero2 = { 0.0, 0.0 };
    auto stage_load = [&](int s) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            sa[p] = zero2;
            sb[p] = zero2;
            if (a_in[p]) {
                const pair v = *reinterpret_cast<const pair *>(Ag[p] + s * RG_KC);
                sa[p] = f64x2{ static_cast<double>(v[0]), static_cast<double>(v[1]) };
            }
            if (b_in[p]) {
                const pair v = *reinterpret_cast<const pair *>(Bg[p] + s * RG_KC);
                sb[p] = f64x2{ static_cast<double>(v[0]), static_cast<double>(v[1]) };
            }
        }
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *reinterpret_cast<f64x2 *>(As + lds_w + p * 32 * RG_LS) = sa[p];
            *reinterpret_cast<f64x2 *>(Bs + lds_w + p * 32 * RG_LS) = sb[p];
        }
    };

    f64x4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            acc[mt][nt] = f64x4{ 0.0, 0.0, 0.0, 0.0 };
            // the start values live in the accumulators' OWN registers (C == D for every MFMA of a chain), as in k_reduced_gram
            asm volatile("" : "+v"(acc[mt][nt]));
        }

    if (nsteps > 0) {
        stage_load(0);
        stage_store();
    }
    __syncthreads();
    const double *Ab = As + (wr * 64 + r) * RG_LS + qd;
    const double *Bb = Bs + (wc * 64 + r) * RG_LS + qd;
    for (int s = 0; s < nsteps; ++s) {
        const bool has_next = s + 1 < nsteps;
        if (has_next) stage_load(s + 1);
#pragma unroll
        for (int ks = 0; ks < RG_KC / 4; ++ks) {
            double av[4], bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                av[t] = Ab[t * 16 * RG_LS + ks * 4];
                bv[t] = Bb[t * 16 * RG_LS + ks * 4];
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
        }
        __syncthreads();  // (every wave has read this step)
        if (has_next) {
            stage_store();
            __syncthreads();
        }
    }

    // a lane holds landmarks l0 + wr 64 + mt 16 + qd + 4 i and rows local0 + wc 64 + nt 16 + r
    const bool rbf = kernel_type == LSSVM_KERNEL_RBF;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int local = local0 + wc * 64 + nt * 16 + r;
        const int row = row0 + local;
        const bool row_in = row < N;
        const double ni = rbf && row_in ? norms[row] : 0.0;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int l = l0 + wr * 64 + mt * 16 + qd + 4 * i;
                if (l >= m) continue;
                double d = acc[mt][nt][i];
                if (rbf) {
                    const int at = lm[l];
                    d = fmax((ni + norms[at]) - 2.0 * d, 0.0);
                    if (at == row) d = 0.0;
                }
                D[static_cast<size_t>(l) * ldN + local] = row_in ? d : 0.0;
            }
    }
}

/* Phi[l][i] = k from D[l][i] (landmark_kernel_value: the epilogue of k_landmark_block) for the rows row0 + i < N of a slab, EXACT zeros from N on (exp(0) is 1, not 0);
 * `gamma`: the kernel function's for the data as X_ holds it (LandmarkBlock::kernel_scalars).  One thread per entry; the grid's x extent times 256 rows, m columns. */
__global__ __launch_bounds__(256) void k_kernel_values(const double *__restrict__ D, size_t ld, int N, int row0, int kernel_type, int degree, double gamma, double coef0,
                                                       double *__restrict__ Phi) {
    const int local = blockIdx.x * 256 + threadIdx.x;
    const size_t at = static_cast<size_t>(blockIdx.y) * ld + local;
    Phi[at] = row0 + local < N ? landmark_kernel_value(kernel_type, degree, gamma, coef0, D[at]) : 0.0;
}

}  // namespace

/* what a leave-one-out pass works on: `num_ops` operands on the device (Bt of k_reduced_leverage, op_stride doubles apart; ybar: num_ops x k or none), and where its results go */
struct LeverageArgs {
    const int m, k, ldb;
    const size_t num_ops, op_stride;
    DevBuf<double> Bt, shift, ybar;
    double inv_n = 0.0;
    const void *Y = nullptr;                                             // the host's right-hand sides (k x N, the problem's type), or NULL: no leave-one-out values
    const double *w = nullptr;                                           // the host's N weights (inv_n is then 1 / their sum), or NULL: the unweighted model
    double *h_out = nullptr, *f_out = nullptr, *loo_out = nullptr;       // num_ops x N, num_ops x k x N, num_ops x k x N; each may be NULL
    double *press = nullptr;                                             // num_ops x k, or NULL
    uint64_t *errors = nullptr;                                          // num_ops x k, or NULL
    std::vector<double> max_leverage, leverage_ms;                       // per operand
    double landmark_ms = 0.0;

    /* the operands as zeros on the device; `shifts`: how many shift vectors of m doubles the pass takes (one per gamma of a grid: the operands are shared out evenly
     * among them, in order) */
    LeverageArgs(int rank, int num_cols, size_t operands, bool with_ybar, hipStream_t stream, size_t shifts = 1) :
        m(rank), k(num_cols), ldb(round_up(rank, RG_KC)), num_ops(operands), op_stride(static_cast<size_t>(rank + num_cols) * ldb), st(stream) {
        Bt.alloc_zero(num_ops * op_stride, st);
        shift.alloc_zero(shifts * static_cast<size_t>(m), st);
        if (with_ybar) ybar.alloc_zero(num_ops * k, st);
    }
    /* operand o <- the host's m + k rows of ldb doubles; asynchronous: the rows stay as they are until the stream has been synchronised */
    void upload_operand(size_t o, const double *Bt_host) {
        LSSVM_HIP_CHECK(hipMemcpyAsync(Bt.p + o * op_stride, Bt_host, op_stride * sizeof(double), hipMemcpyHostToDevice, st));
    }
    /* shift (m per shift vector) and, where the pass takes one, ybar (num_ops x k); returns when these and the operands are on the device */
    void upload_shift(const double *shift_host, const double *ybar_host) {
        LSSVM_HIP_CHECK(hipMemcpyAsync(shift.p, shift_host, shift.count * sizeof(double), hipMemcpyHostToDevice, st));
        if (ybar_host != nullptr) LSSVM_HIP_CHECK(hipMemcpyAsync(ybar.p, ybar_host, ybar.count * sizeof(double), hipMemcpyHostToDevice, st));
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    }
    /* k_reduced_leverage for operand o on `rows` rows of a slab (ld doubles between its columns; its [1 | Y] columns stand behind Phi where `loo` is given) */
    void enqueue(size_t o, const double *slab, size_t ld, int rows, double *h, double *f, double *loo, const double *w_dev = nullptr, size_t shift_at = 0) const {
        hipLaunchKernelGGL(k_reduced_leverage, dim3(round_up(rows, 256) / RG_TW), dim3(256), 0, st, slab, ld, rows, m, k, Bt.p + o * op_stride, ldb, shift.p + shift_at * m, ybar.p != nullptr ? ybar.p + o * k : nullptr,
                           inv_n, loo != nullptr ? slab + static_cast<size_t>(m + 1) * ld : nullptr, h, f, loo, ld, w_dev);
        LSSVM_HIP_CHECK(hipGetLastError());
    }
    hipStream_t st;
};

/* what a pass over every prefix rank works on: per operand (a cost) the m rows of V and, behind them, the k rows of z, ldb doubles apart -- the
 * layout of LeverageArgs' operands with z where the betas stand, so that DenseFit::run fills it as it is; the checkpoints; and where the results go, every output with
 * the checkpoint dimension behind the operand's */
struct PrefixArgs {
    const int m, k, ldb, R;
    const size_t num_ops, op_stride;
    DevBuf<double> ops, shift, ybar;
    DevBuf<int> ranks_dev;
    std::vector<int> ranks;
    double inv_n = 0.0;
    const void *Y = nullptr;                                        // the host's right-hand sides (k x N, the problem's type), or NULL: no leave-one-out values
    const double *w = nullptr;                                      // the host's N weights, or NULL
    double *h_out = nullptr, *f_out = nullptr, *loo_out = nullptr;  // num_ops x R x N, num_ops x R x k x N, num_ops x R x k x N; each may be NULL
    double *press = nullptr;                                        // num_ops x R x k, or NULL
    uint64_t *errors = nullptr;                                     // num_ops x R x k, or NULL
    std::vector<double> max_leverage, leverage_ms;                  // num_ops x R; per operand
    double landmark_ms = 0.0;
    hipStream_t st;

    PrefixArgs(int rank, int num_cols, const uint64_t *ranks_in, size_t num_ranks, size_t operands, bool with_ybar, hipStream_t stream) :
        m(rank), k(num_cols), ldb(round_up(rank, RG_KC)), R(static_cast<int>(num_ranks)), num_ops(operands), op_stride(static_cast<size_t>(rank + num_cols) * ldb),
        ranks(ranks_in, ranks_in + num_ranks), st(stream) {
        ops.alloc_zero(num_ops * op_stride, st);
        shift.alloc_zero(static_cast<size_t>(m), st);
        if (with_ybar) ybar.alloc_zero(num_ops * std::max(k, 1), st);
        ranks_dev.alloc_zero(static_cast<size_t>(R), st);
        LSSVM_HIP_CHECK(hipMemcpyAsync(ranks_dev.p, ranks.data(), static_cast<size_t>(R) * sizeof(int), hipMemcpyHostToDevice, st));
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    }
    double *V_of(size_t o) const { return ops.p + o * op_stride; }
    double *Z_of(size_t o) const { return ops.p + o * op_stride + static_cast<size_t>(m) * ldb; }
    /* operand o <- the host's m + k rows of ldb doubles; returns when they are on the device */
    void upload_operand(size_t o, const double *host) {
        LSSVM_HIP_CHECK(hipMemcpyAsync(V_of(o), host, op_stride * sizeof(double), hipMemcpyHostToDevice, st));
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    }
    void upload_shift(const double *shift_host, const double *ybar_host) {
        LSSVM_HIP_CHECK(hipMemcpyAsync(shift.p, shift_host, shift.count * sizeof(double), hipMemcpyHostToDevice, st));
        if (ybar_host != nullptr) LSSVM_HIP_CHECK(hipMemcpyAsync(ybar.p, ybar_host, num_ops * k * sizeof(double), hipMemcpyHostToDevice, st));
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    }
    /* k_reduced_leverage_prefix for operand o and its right-hand sides c0 ... c0 + kc - 1 (kc <= PFX_KMAX) on `rows` rows of a slab; h: R x ld, f and loo: R x kc x ld */
    void enqueue(size_t o, int c0, int kc, const double *slab, size_t ld, int rows, double *h, double *f, double *loo, const double *w_dev) const {
        hipLaunchKernelGGL(k_reduced_leverage_prefix, dim3(round_up(rows, 256) / RG_TW), dim3(256), 0, st, slab, ld, rows, m, kc, V_of(o), ldb, Z_of(o) + static_cast<size_t>(c0) * ldb,
                           ranks_dev.p, R, shift.p, ybar.p != nullptr ? ybar.p + o * k + c0 : nullptr, inv_n, loo != nullptr ? slab + static_cast<size_t>(m + 1 + c0) * ld : nullptr, h, f, loo,
                           ld, w_dev);
        LSSVM_HIP_CHECK(hipGetLastError());
    }
};

void check_reduced_rank_list(const uint64_t *ranks, size_t num_ranks, uint64_t rank, size_t num_costs) {
    LSSVM_REQUIRE(ranks != nullptr, "ranks must not be NULL");
    LSSVM_REQUIRE(num_ranks >= 1 && num_ranks <= REDUCED_RANK_PATH_MAX_RANKS,
                  "The rank path takes between 1 and " + std::to_string(REDUCED_RANK_PATH_MAX_RANKS) + " checkpoints, but got " + std::to_string(num_ranks) + "!");
    LSSVM_REQUIRE(num_ranks * num_costs <= REDUCED_GRID_MAX_CELLS,
                  "The rank path takes at most " + std::to_string(REDUCED_GRID_MAX_CELLS) + " (cost, checkpoint) cells, but got " + std::to_string(num_costs) + " x " + std::to_string(num_ranks) + "!");
    for (size_t q = 0; q < num_ranks; ++q) {
        LSSVM_REQUIRE(ranks[q] >= 1 && ranks[q] <= rank, "Every checkpoint must lie in [1, " + std::to_string(rank) + "], but checkpoint " + std::to_string(q) + " is " + std::to_string(ranks[q]) + "!");
        LSSVM_REQUIRE(q == 0 || ranks[q] > ranks[q - 1], "The checkpoints must be strictly ascending, but checkpoint " + std::to_string(q) + " is " + std::to_string(ranks[q]) + " behind " +
                                                             std::to_string(ranks[q - 1]) + "!");
    }
}

void check_reduced_arguments(const void *Y, size_t num_rhs, uint64_t rank, uint64_t slab_rows, size_t num_points) {
    LSSVM_REQUIRE(Y != nullptr, "The right hand side vector must not be empty!");
    LSSVM_REQUIRE(num_rhs > 0, "The number of right hand sides must be greater than 0!");
    const uint64_t most = num_points > 0 ? std::min<uint64_t>(num_points, REDUCED_MAX_RANK) : REDUCED_MAX_RANK;
    LSSVM_REQUIRE(rank >= 1 && rank <= most, "The rank of the reduced model must lie in [1, " + std::to_string(most) + "], but is " + std::to_string(rank) + "!");
    LSSVM_REQUIRE(slab_rows % 256 == 0, "slab_rows must be a multiple of 256 (0: the library's default), but is " + std::to_string(slab_rows) + "!");
}

double check_reduced_weights(const double *weights, size_t num_points) {
    double total = 0.0;
    for (size_t i = 0; i < num_points; ++i) {
        LSSVM_REQUIRE(std::isfinite(weights[i]) && weights[i] >= 0.0,
                      "Every weight of the reduced model must be finite and not less than 0.0, but weight " + std::to_string(i) + " is " + std::to_string(weights[i]) + "!");
        total += weights[i];
    }
    LSSVM_REQUIRE(std::isfinite(total) && total > 0.0, "The weights of the reduced model must have a finite sum greater than 0.0, but it is " + std::to_string(total) + "!");
    return total;
}

void check_reduced_factor(int factor) { LSSVM_REQUIRE(factor == 0 || factor == 1, "factor must be 0 (the host) or 1 (the device), but is " + std::to_string(factor) + "!"); }

namespace {

/* `values` (N doubles, or their square roots: std::sqrt on the host, correctly rounded, so that the device takes none) on the device behind each other as the slabs' rows
 * are, zeros from row N on */
void upload_per_row(const double *values, bool take_sqrt, const SlabPlan &plan, DevBuf<double> &out, hipStream_t st) {
    std::vector<double> host(static_cast<size_t>(plan.slabs) * plan.ld, 0.0);
    for (size_t i = 0; i < plan.N; ++i) host[i] = take_sqrt ? std::sqrt(values[i]) : values[i];
    out.alloc_zero(host.size(), st);
    LSSVM_HIP_CHECK(hipMemcpyAsync(out.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, st));
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (`host` goes)
}

}  // namespace

void check_reduced_grid_arguments(const double *gammas, size_t num_gammas, size_t num_costs, int product) {
    LSSVM_REQUIRE(gammas != nullptr, "gammas must not be NULL");
    LSSVM_REQUIRE(num_gammas >= 1, "The grid takes at least 1 gamma, but got 0!");
    LSSVM_REQUIRE(num_gammas <= REDUCED_GRID_MAX_CELLS && num_gammas * num_costs <= REDUCED_GRID_MAX_CELLS,
                  "The grid takes at most " + std::to_string(REDUCED_GRID_MAX_CELLS) + " (gamma, cost) cells, but got " + std::to_string(num_gammas) + " x " + std::to_string(num_costs) + "!");
    for (size_t g = 0; g < num_gammas; ++g)  // (behind the cap: at most 64 entries are read)
        LSSVM_REQUIRE(std::isfinite(gammas[g]) && gammas[g] > 0.0, "Every gamma must be finite and greater than 0, but gamma " + std::to_string(g) + " is " + std::to_string(gammas[g]) + "!");
    LSSVM_REQUIRE(product == 0 || product == 1, "product must be 0 (ordered) or 1 (matrix), but is " + std::to_string(product) + "!");
}

void check_reduced_grid_kernel(int kernel_type) {
    LSSVM_REQUIRE(kernel_type != LSSVM_KERNEL_LINEAR, "The linear kernel has no gamma to vary: the (gamma, cost) grid takes an rbf or a polynomial problem!");
}

/* What the slabs of a (gamma, cost) grid are made from: per slab, D -- the feature sums behind every kernel value, k_landmark_acc (product 0) or
 * k_landmark_product (1) -- is formed once into a work space of its own, and per gamma k_kernel_values writes the Phi columns of the slab from it.  Both passes of a fit
 * go through the same object: the same kernels with the same arguments, hence the same bits.  The landmarks, the right-hand sides and (rbf, product 1) the rows' squared
 * norms go to the device once.  `gammas_in`: the kernel function's, as the caller gives them; held here for the data as X_ holds it (LandmarkBlock::kernel_scalars). */
template <typename T>
struct GridSlabs {
    const Problem<T> &p;
    const SlabPlan plan;
    const int m, product;
    hipStream_t st;
    const LandmarkBlock<T> block;
    const RhsOnDevice<T> rhs;
    DevBuf<double> D, norms;
    std::vector<double> gammas, values_ms;
    double coef0 = 0.0, accumulate_ms = 0.0;
    Event ev[2];

    GridSlabs(const Problem<T> &problem, const std::vector<uint64_t> &lm, const void *Y, int k, uint64_t slab_rows, const double *gammas_in, size_t num_gammas, int product_in,
              hipStream_t stream) :
        p(problem), plan(problem.N_, slab_rows), m(static_cast<int>(lm.size())), product(product_in), st(stream), block(problem, lm, stream), rhs(Y, k, problem.N_, stream),
        gammas(num_gammas), values_ms(num_gammas, 0.0) {
        for (size_t g = 0; g < num_gammas; ++g) LandmarkBlock<T>::kernel_scalars(p, gammas_in[g], gammas[g], coef0);
        for (Event &e : ev) e.create(true);
        D.alloc_zero(static_cast<size_t>(m) * plan.ld, st);
        if (product == 1 && p.params_.kernel_type == LSSVM_KERNEL_RBF) {
            norms.alloc_zero(p.N_, st);
            LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
            hipLaunchKernelGGL(k_row_norms<T>, dim3(static_cast<unsigned>((p.N_ + 255) / 256)), dim3(256), 0, st, p.X_.data.p, p.X_.ldx, p.N_, norms.p);
            LSSVM_HIP_CHECK(hipGetLastError());
            LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
            LSSVM_HIP_CHECK(hipEventSynchronize(ev[1].e));
            accumulate_ms += elapsed_ms(ev[0], ev[1]);
        }
    }
    size_t device_bytes() const { return (D.count + norms.count) * sizeof(double) + rhs.Y.count * sizeof(T) + block.device_bytes(); }

    /* D of slab s */
    void enqueue_acc(int s) const {
        const int rows256 = plan.rows256(s), N = static_cast<int>(p.N_), row0 = static_cast<int>(plan.row0(s));
        if (product == 1) {
            hipLaunchKernelGGL(k_landmark_product<T>, dim3(rows256 / RG_TW, (m + RG_TW - 1) / RG_TW), dim3(256), 0, st, p.X_.data.p, p.X_.ldx, N, row0, block.landmarks_dev(), m,
                               p.params_.kernel_type, norms.p, D.p, plan.ld);
        } else {
            hipLaunchKernelGGL(k_landmark_acc<T>, dim3(rows256 / 256, (m + 15) / 16), dim3(256), 0, st, p.X_.data.p, p.X_.ldx, N, row0, block.landmarks_dev(), m, p.params_.kernel_type, D.p,
                               plan.ld);
        }
        LSSVM_HIP_CHECK(hipGetLastError());
    }
    /* what the gammas share of slab s: D (timed), and the [1 | Y] columns of `slab` behind the m columns of Phi where there are right-hand sides */
    void enqueue_shared(int s, double *slab) {
        LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
        enqueue_acc(s);
        LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
        if (rhs.Y.p != nullptr)
            hipLaunchKernelGGL(k_reduced_aux<T>, dim3(plan.rows256(s) / 256, 1 + rhs.k), dim3(256), 0, st, rhs.Y.p, plan.N, plan.row0(s), slab + static_cast<size_t>(m) * plan.ld, plan.ld);
        LSSVM_HIP_CHECK(hipGetLastError());
        LSSVM_HIP_CHECK(hipEventSynchronize(ev[1].e));
        accumulate_ms += elapsed_ms(ev[0], ev[1]);
    }
    /* the m columns of Phi of slab s at gamma g, from the D enqueue_shared left (timed; returns when they are written) */
    void enqueue_values(size_t g, int s, double *slab) {
        LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
        hipLaunchKernelGGL(k_kernel_values, dim3(plan.rows256(s) / 256, m), dim3(256), 0, st, D.p, plan.ld, static_cast<int>(p.N_), static_cast<int>(plan.row0(s)), p.params_.kernel_type,
                           p.params_.degree, gammas[g], coef0, slab);
        LSSVM_HIP_CHECK(hipGetLastError());
        LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
        LSSVM_HIP_CHECK(hipEventSynchronize(ev[1].e));
        values_ms[g] += elapsed_ms(ev[0], ev[1]);
    }
};

template <typename T>
Problem<T> &Solver<T>::reduced_problem(const char *what, bool unweighted_only) {
    LSSVM_REQUIRE(shards_.size() == 1 && world_ == 1 && exchange_ == Exchange::none, std::string("the reduced model (") + what + ") is fitted on a problem of one device and one rank");
    Problem<T> &p = *shards_[0];
    LSSVM_REQUIRE(!unweighted_only || !p.weighted_,
                  std::string("the reduced model (") + what + ") is fitted to the unweighted objective: the problem has weights set (lssvm_mi355_problem_set_weights(p, NULL, 0) removes them)");
    LSSVM_REQUIRE(!in_cg_, std::string(what) + " cannot run between cg_begin and cg_finish");
    return p;
}

template <typename T>
void Solver<T>::reduced_gram(const char *what, const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, std::vector<uint64_t> &lm,
                             std::vector<double> &gram, std::vector<double> &Kmm, lssvm_reduced_info &info, ReducedOnDevice *keep, const double *weights, double *total_out) {
    // ---- everything that needs no device ----
    Problem<T> &p = reduced_problem(what, true);
    const size_t N = p.N_;
    check_reduced_arguments(Y, num_rhs, rank, slab_rows, N);
    LSSVM_REQUIRE(num_rhs <= 4096, "at most 4096 right hand sides per call");
    const int m = static_cast<int>(rank), k = static_cast<int>(num_rhs), cols = m + 1 + k;
    lm = resolve_landmarks(landmarks, static_cast<size_t>(m), N);
    // what stands for N in the host's formulas: the sum of the weights in index order, N itself without weights
    const double total = weights != nullptr ? check_reduced_weights(weights, N) : static_cast<double>(N);
    if (total_out != nullptr) *total_out = total;

    const double t0 = now_ms();
    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    const SlabPlan plan(N, slab_rows);
    const size_t ld = plan.ld;
    const int nt = tiles_of(cols), ntri = nt * (nt + 1) / 2;
    const int max_chunks = static_cast<int>((ld + RG_RANGE - 1) / RG_RANGE);

    const LandmarkBlock<T> block(p, lm, st);
    const RhsOnDevice<T> rhs(Y, k, N, st);
    DevBuf<double> slab, part, St_dev, Kmm_dev, q_dev;
    slab.alloc_zero(static_cast<size_t>(cols) * ld, st);
    part.alloc_zero(static_cast<size_t>(ntri) * max_chunks * RG_TILE, st);
    St_dev.alloc_zero(static_cast<size_t>(ntri) * RG_TILE, st);
    Kmm_dev.alloc_zero(static_cast<size_t>(m) * m, st);
    if (weights != nullptr) upload_per_row(weights, true, plan, q_dev, st);

    Event ev[3];
    for (Event &e : ev) e.create(true);
    double landmark_ms = 0.0, gram_ms = 0.0;
    for (int s = 0; s < plan.slabs; ++s) {
        LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
        enqueue_slab(block, m, plan, s, rhs, slab.p, st);
        block.enqueue_gather_kmm(slab.p, ld, plan.row0(s), plan.rows(s), Kmm_dev.p);
        LSSVM_HIP_CHECK(hipGetLastError());
        LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
        enqueue_gram(slab.p, ld, cols, plan.rows256(s), max_chunks, part.p, St_dev.p, st, q_dev.p != nullptr ? q_dev.p + plan.row0(s) : nullptr);
        LSSVM_HIP_CHECK(hipEventRecord(ev[2].e, st));
        LSSVM_HIP_CHECK(hipEventSynchronize(ev[2].e));
        landmark_ms += elapsed_ms(ev[0], ev[1]);
        gram_ms += elapsed_ms(ev[1], ev[2]);
    }
    std::vector<double> tiles(static_cast<size_t>(ntri) * RG_TILE);
    Kmm.resize(static_cast<size_t>(m) * m);
    LSSVM_HIP_CHECK(hipMemcpyAsync(tiles.data(), St_dev.p, tiles.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    LSSVM_HIP_CHECK(hipMemcpyAsync(Kmm.data(), Kmm_dev.p, Kmm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    unpack_tiles(tiles, cols, gram);

    info = lssvm_reduced_info{};
    info.rank = static_cast<uint64_t>(m);
    info.slabs = static_cast<uint64_t>(plan.slabs);
    info.landmark_ms = landmark_ms;
    info.gram_ms = gram_ms;
    info.total_ms = now_ms() - t0;
    info.workspace_bytes = (slab.count + part.count + St_dev.count + Kmm_dev.count + q_dev.count) * sizeof(double) + rhs.Y.count * sizeof(T) + block.device_bytes();
    if (keep != nullptr) {  // the device-factored fits go on with both where they lie
        std::swap(keep->St.p, St_dev.p);
        std::swap(keep->St.count, St_dev.count);
        std::swap(keep->Kmm.p, Kmm_dev.p);
        std::swap(keep->Kmm.count, Kmm_dev.count);
    }
}

template <typename T>
void Solver<T>::landmark_gram(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *gram_out, const double *weights) {
    LSSVM_REQUIRE(gram_out != nullptr, "gram_out must not be NULL");
    std::vector<uint64_t> lm;
    std::vector<double> gram, Kmm;
    lssvm_reduced_info info{};
    reduced_gram("landmark_gram", Y, num_rhs, rank, landmarks, slab_rows, lm, gram, Kmm, info, nullptr, weights);
    std::copy(gram.begin(), gram.end(), gram_out);
}

template <typename T>
void Solver<T>::fit_reduced(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                            lssvm_reduced_info *info_out, const double *weights) {
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    const double t0 = now_ms();
    std::vector<uint64_t> lm;
    std::vector<double> St, Kmm;
    lssvm_reduced_info info{};
    double Nd = 0.0;  // N, or the sum of the weights
    reduced_gram("fit_reduced", Y, num_rhs, rank, landmarks, slab_rows, lm, St, Kmm, info, nullptr, weights, &Nd);

    // ---- the host's part, in double (factor_reduced, solve_reduced: shared with fit_reduced_loo) ----
    const double t_host = now_ms();
    const int m = static_cast<int>(rank), k = static_cast<int>(num_rhs), cols = m + 1 + k;
    const double sigma = 1.0 / shards_[0]->params_.cost;  // (in double, whatever the real type: the host's part is the formulation's)
    std::vector<double> L;
    const double nu = factor_reduced(St, Kmm, m, cols, Nd, sigma, L);
    solve_reduced(St, L, m, k, cols, Nd, betas_out, rhos_out);
    if (landmarks_out != nullptr) std::copy(lm.begin(), lm.end(), landmarks_out);
    if (info_out != nullptr) {
        info.jitter = nu;
        info.host_ms = now_ms() - t_host;
        info.total_ms = now_ms() - t0;
        *info_out = info;
    }
}

/* fit_reduced with the host's part on the device: St and K_mm stay where reduced_gram summed them */
template <typename T>
void Solver<T>::fit_reduced_dev(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                                lssvm_reduced_info *info_out, lssvm_dense_info *dense_out, const double *weights) {
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    const double t0 = now_ms();
    std::vector<uint64_t> lm;
    std::vector<double> St, Kmm;
    lssvm_reduced_info info{};
    ReducedOnDevice dev;
    double Nd = 0.0;  // N, or the sum of the weights
    reduced_gram("fit_reduced", Y, num_rhs, rank, landmarks, slab_rows, lm, St, Kmm, info, &dev, weights, &Nd);

    const double t_dense = now_ms();
    const int m = static_cast<int>(rank), k = static_cast<int>(num_rhs), cols = m + 1 + k;
    Problem<T> &p = *shards_[0];
    const double sigma = 1.0 / p.params_.cost;
    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    DenseFit fit(m, k, p.stream());
    double device_ms = 0.0;
    const double nu = fit.run(dev, St, Kmm, cols, Nd, sigma, nullptr, 0, betas_out, rhos_out, dense_out, &device_ms);
    if (landmarks_out != nullptr) std::copy(lm.begin(), lm.end(), landmarks_out);
    if (info_out != nullptr) {
        info.jitter = nu;
        info.host_ms = std::max(0.0, now_ms() - t_dense - device_ms);
        info.total_ms = now_ms() - t0;
        info.workspace_bytes += fit.device_bytes();
        *info_out = info;
    }
}

void check_reduced_loo_costs(const double *costs, size_t num_costs) {
    LSSVM_REQUIRE(costs != nullptr, "costs must not be NULL");
    LSSVM_REQUIRE(num_costs >= 1 && num_costs <= REDUCED_LOO_MAX_COSTS,
                  "The leave-one-out scores take between 1 and " + std::to_string(REDUCED_LOO_MAX_COSTS) + " costs, but got " + std::to_string(num_costs) + "!");
    for (size_t s = 0; s < num_costs; ++s)
        LSSVM_REQUIRE(std::isfinite(costs[s]) && costs[s] > 0.0, "Every cost must be finite and greater than 0, but cost " + std::to_string(s) + " is " + std::to_string(costs[s]) + "!");
}

/* The Phi slabs once more (the kernels and arguments of reduced_gram: the same bits) and, per slab, k_reduced_leverage once per operand; h, f and loo of the slab go to the
 * caller's arrays, the sums over the points are formed here in row order.  The caller has made the checks that need no device. */
template <typename T>
void Solver<T>::leverage_pass(const std::vector<uint64_t> &lm, uint64_t slab_rows, LeverageArgs &a, GridSlabs<T> *grid) {
    Problem<T> &p = *shards_[0];
    const size_t N = p.N_;
    const int m = a.m, k = a.k;
    const bool with_y = a.Y != nullptr;
    const int cols = with_y ? m + 1 + k : m;
    hipStream_t st = p.stream();
    const SlabPlan plan(N, slab_rows);
    const size_t ld = plan.ld;
    // a grid brings its own landmarks and right-hand sides on the device and fills the slab once per gamma; the operands are shared out evenly among the gammas, in order
    const size_t groups = grid != nullptr ? grid->gammas.size() : 1, per_group = a.num_ops / groups;

    std::optional<LandmarkBlock<T>> block;
    if (grid == nullptr) block.emplace(p, lm, st);
    const RhsOnDevice<T> rhs(grid == nullptr ? a.Y : nullptr, k, N, st);
    DevBuf<double> slab, h_dev, f_dev, loo_dev, w_dev;
    if (a.w != nullptr) upload_per_row(a.w, false, plan, w_dev, st);
    if (with_y) loo_dev.alloc_zero(static_cast<size_t>(k) * ld, st);
    slab.alloc_zero(static_cast<size_t>(cols) * ld, st);
    h_dev.alloc_zero(ld, st);
    f_dev.alloc_zero(static_cast<size_t>(std::max(k, 1)) * ld, st);
    std::vector<double> h_host(ld), f_host(static_cast<size_t>(k) * ld), loo_host(with_y ? static_cast<size_t>(k) * ld : 0);

    Event ev[2];
    for (Event &e : ev) e.create(true);
    a.max_leverage.assign(a.num_ops, 0.0);
    a.leverage_ms.assign(a.num_ops, 0.0);
    a.landmark_ms = 0.0;
    if (a.press != nullptr) std::fill(a.press, a.press + a.num_ops * k, 0.0);
    if (a.errors != nullptr) std::fill(a.errors, a.errors + a.num_ops * k, uint64_t{ 0 });
    const T *Yh = static_cast<const T *>(a.Y);
    for (int s = 0; s < plan.slabs; ++s) {
        const size_t row0 = plan.row0(s);
        const int rows = plan.rows(s);
        if (grid != nullptr) {
            grid->enqueue_shared(s, slab.p);
        } else {
            LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
            enqueue_slab(*block, m, plan, s, rhs, slab.p, st);
            LSSVM_HIP_CHECK(hipGetLastError());
            LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
            LSSVM_HIP_CHECK(hipEventSynchronize(ev[1].e));
            a.landmark_ms += elapsed_ms(ev[0], ev[1]);
        }
        for (size_t o = 0; o < a.num_ops; ++o) {
            const size_t g = o / per_group;
            if (grid != nullptr && o % per_group == 0) grid->enqueue_values(g, s, slab.p);  // (every operand of the gamma before has been waited for)
            LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
            a.enqueue(o, slab.p, ld, rows, h_dev.p, f_dev.p, loo_dev.p, w_dev.p != nullptr ? w_dev.p + row0 : nullptr, g);
            LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
            LSSVM_HIP_CHECK(hipMemcpyAsync(h_host.data(), h_dev.p, static_cast<size_t>(rows) * sizeof(double), hipMemcpyDeviceToHost, st));
            for (int c = 0; c < k; ++c) {
                LSSVM_HIP_CHECK(hipMemcpyAsync(&f_host[static_cast<size_t>(c) * ld], f_dev.p + static_cast<size_t>(c) * ld, static_cast<size_t>(rows) * sizeof(double), hipMemcpyDeviceToHost, st));
                if (with_y)
                    LSSVM_HIP_CHECK(hipMemcpyAsync(&loo_host[static_cast<size_t>(c) * ld], loo_dev.p + static_cast<size_t>(c) * ld, static_cast<size_t>(rows) * sizeof(double), hipMemcpyDeviceToHost, st));
            }
            LSSVM_HIP_CHECK(hipStreamSynchronize(st));
            a.leverage_ms[o] += elapsed_ms(ev[0], ev[1]);
            for (int i = 0; i < rows; ++i) a.max_leverage[o] = std::max(a.max_leverage[o], h_host[i]);
            if (a.h_out != nullptr) std::copy(h_host.begin(), h_host.begin() + rows, a.h_out + o * N + row0);
            for (int c = 0; c < k; ++c) {
                const size_t oc = o * k + c;
                if (a.f_out != nullptr) std::copy(&f_host[static_cast<size_t>(c) * ld], &f_host[static_cast<size_t>(c) * ld] + rows, a.f_out + oc * N + row0);
                if (!with_y) continue;
                const double *loo = &loo_host[static_cast<size_t>(c) * ld];
                if (a.loo_out != nullptr) std::copy(loo, loo + rows, a.loo_out + oc * N + row0);
                double press = a.press != nullptr ? a.press[oc] : 0.0;
                uint64_t errors = 0;
                for (int i = 0; i < rows; ++i) {
                    const double y = static_cast<double>(Yh[static_cast<size_t>(c) * N + row0 + i]), d = y - loo[i];
                    const bool wrong = ((loo[i] > 0.0) - (loo[i] < 0.0)) != ((y > 0.0) - (y < 0.0));
                    if (a.w != nullptr) {  // sum_i w_i d_i^2; the errors over the points that took part in the fit
                        press += a.w[row0 + i] * (d * d);
                        errors += wrong && a.w[row0 + i] > 0.0 ? 1 : 0;
                    } else {
                        press += d * d;
                        errors += wrong ? 1 : 0;
                    }
                }
                if (a.press != nullptr) a.press[oc] = press;
                if (a.errors != nullptr) a.errors[oc] += errors;
            }
        }
    }
}

template <typename T>
void Solver<T>::fit_reduced_loo(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out,
                                double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out,
                                lssvm_reduced_loo_info *infos, const double *weights) {
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    check_reduced_loo_costs(costs, num_costs);
    std::vector<uint64_t> lm;
    std::vector<double> St, Kmm;
    lssvm_reduced_info info{};
    double Nd = 0.0;  // N, or the sum of the weights
    reduced_gram("fit_reduced_loo", Y, num_rhs, rank, landmarks, slab_rows, lm, St, Kmm, info, nullptr, weights, &Nd);  // pass 1, and every other check that needs no device

    const int m = static_cast<int>(rank), k = static_cast<int>(num_rhs), cols = m + 1 + k;
    Problem<T> &p = *shards_[0];
    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    LeverageArgs a(m, k, num_costs, true, st);

    // ---- per cost, on the host in double: M_s, L_s, beta and rho as fit_reduced forms them, V_s = L_s^-1; the operand of the cost goes to the device once ----
    const double *s_row = &St[static_cast<size_t>(m) * cols];
    std::vector<double> shift(static_cast<size_t>(m)), ybar(a.num_ops * k), Bt(a.op_stride), L, nus(num_costs), host_ms(num_costs);
    for (int j = 0; j < m; ++j) shift[j] = s_row[j] / Nd;
    for (size_t s = 0; s < num_costs; ++s) {
        const double t_host = now_ms();
        nus[s] = host_operand(St, Kmm, m, k, cols, Nd, costs[s], a.ldb, betas_out + s * k * m, rhos_out + s * k, L, Bt, &ybar[s * k]);
        host_ms[s] = now_ms() - t_host;
        a.upload_operand(s, Bt.data());
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (Bt is filled again for the next cost)
    }
    a.upload_shift(shift.data(), ybar.data());

    a.inv_n = 1.0 / Nd;
    a.Y = Y;
    a.w = weights;
    a.h_out = leverage_out;
    a.f_out = fitted_out;
    a.loo_out = loo_out;
    a.press = press_out;
    a.errors = loo_errors_out;
    leverage_pass(lm, slab_rows, a);

    if (landmarks_out != nullptr) std::copy(lm.begin(), lm.end(), landmarks_out);
    if (infos != nullptr) {
        for (size_t s = 0; s < num_costs; ++s) {
            infos[s] = lssvm_reduced_loo_info{};
            infos[s].cost = costs[s];
            infos[s].jitter = nus[s];
            infos[s].max_leverage = a.max_leverage[s];
            infos[s].landmark_ms = info.landmark_ms + a.landmark_ms;
            infos[s].gram_ms = info.gram_ms;
            infos[s].leverage_ms = a.leverage_ms[s];
            infos[s].host_ms = host_ms[s];
        }
    }
}

/* fit_reduced_loo with the per-cost steps on the device: nothing of size m^2 crosses the bus per cost, the operand of the leverage kernel is written where it is read */
template <typename T>
void Solver<T>::fit_reduced_loo_dev(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out,
                                    double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out,
                                    lssvm_reduced_loo_info *infos, lssvm_dense_info *dense_out, const double *weights) {
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    check_reduced_loo_costs(costs, num_costs);
    std::vector<uint64_t> lm;
    std::vector<double> St, Kmm;
    lssvm_reduced_info info{};
    ReducedOnDevice dev;
    double Nd = 0.0;  // N, or the sum of the weights
    reduced_gram("fit_reduced_loo", Y, num_rhs, rank, landmarks, slab_rows, lm, St, Kmm, info, &dev, weights, &Nd);  // pass 1, and every other check that needs no device

    const int m = static_cast<int>(rank), k = static_cast<int>(num_rhs), cols = m + 1 + k;
    Problem<T> &p = *shards_[0];
    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    LeverageArgs a(m, k, num_costs, true, st);
    DenseFit fit(m, k, st);

    const double *s_row = &St[static_cast<size_t>(m) * cols];
    std::vector<double> shift(static_cast<size_t>(m)), ybar(a.num_ops * k), nus(num_costs), host_ms(num_costs);
    for (int j = 0; j < m; ++j) shift[j] = s_row[j] / Nd;
    for (size_t s = 0; s < num_costs; ++s) {
        const double t_cost = now_ms();
        double device_ms = 0.0;
        nus[s] = fit.run(dev, St, Kmm, cols, Nd, 1.0 / costs[s], a.Bt.p + s * a.op_stride, a.ldb, betas_out + s * k * m, rhos_out + s * k, dense_out != nullptr ? dense_out + s : nullptr,
                         &device_ms);
        for (int c = 0; c < k; ++c) ybar[s * k + c] = St[static_cast<size_t>(m + 1 + c) * cols + m] / Nd;
        host_ms[s] = std::max(0.0, now_ms() - t_cost - device_ms);
    }
    a.upload_shift(shift.data(), ybar.data());

    a.inv_n = 1.0 / Nd;
    a.Y = Y;
    a.w = weights;
    a.h_out = leverage_out;
    a.f_out = fitted_out;
    a.loo_out = loo_out;
    a.press = press_out;
    a.errors = loo_errors_out;
    leverage_pass(lm, slab_rows, a);

    if (landmarks_out != nullptr) std::copy(lm.begin(), lm.end(), landmarks_out);
    if (infos != nullptr) {
        for (size_t s = 0; s < num_costs; ++s) {
            infos[s] = lssvm_reduced_loo_info{};
            infos[s].cost = costs[s];
            infos[s].jitter = nus[s];
            infos[s].max_leverage = a.max_leverage[s];
            infos[s].landmark_ms = info.landmark_ms + a.landmark_ms;
            infos[s].gram_ms = info.gram_ms;
            infos[s].leverage_ms = a.leverage_ms[s];
            infos[s].host_ms = host_ms[s];
        }
    }
}

/* fit_reduced_loo / _dev at every gamma of a grid on this one problem: the two passes of the leave-one-out fit, with the slabs made by GridSlabs --
 * per slab D once, per gamma the Phi columns from it, K_mm and that gamma's own running St; per (gamma, cost) the dense steps of `factor` and, in pass 2, the leverage
 * kernel.  Cell (g, s) of every output stands at g num_costs + s. */
template <typename T>
void Solver<T>::fit_reduced_grid(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *gammas,
                                 size_t num_gammas, const double *costs, size_t num_costs, int factor, int product, double *betas_out, double *rhos_out, double *leverage_out,
                                 double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_grid_info *infos,
                                 lssvm_dense_info *dense_out) {
    // ---- everything that needs no device ----
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    check_reduced_loo_costs(costs, num_costs);
    check_reduced_grid_arguments(gammas, num_gammas, num_costs, product);
    check_reduced_factor(factor);
    Problem<T> &p = reduced_problem("fit_reduced_grid", true);
    check_reduced_grid_kernel(p.params_.kernel_type);
    const size_t N = p.N_;
    check_reduced_arguments(Y, num_rhs, rank, slab_rows, N);
    LSSVM_REQUIRE(num_rhs <= 4096, "at most 4096 right hand sides per call");
    const int m = static_cast<int>(rank), k = static_cast<int>(num_rhs), cols = m + 1 + k;
    const std::vector<uint64_t> lm = resolve_landmarks(landmarks, static_cast<size_t>(m), N);
    const double Nd = weights != nullptr ? check_reduced_weights(weights, N) : static_cast<double>(N);  // N, or the sum of the weights in index order
    const size_t G = num_gammas, S = num_costs;

    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    GridSlabs<T> grid(p, lm, Y, k, slab_rows, gammas, G, product, st);
    const SlabPlan &plan = grid.plan;
    const size_t ld = plan.ld;
    const int nt = tiles_of(cols), ntri = nt * (nt + 1) / 2;
    const int max_chunks = static_cast<int>((ld + RG_RANGE - 1) / RG_RANGE);

    // ---- pass 1: per slab D once; per gamma Phi from it, K_mm, and St into the gamma's own running sum ----
    std::vector<ReducedOnDevice> dev(G);
    std::vector<double> gram_ms(G, 0.0);
    {
        DevBuf<double> slab, part, q_dev;
        slab.alloc_zero(static_cast<size_t>(cols) * ld, st);
        part.alloc_zero(static_cast<size_t>(ntri) * max_chunks * RG_TILE, st);
        for (ReducedOnDevice &d : dev) {
            d.St.alloc_zero(static_cast<size_t>(ntri) * RG_TILE, st);
            d.Kmm.alloc_zero(static_cast<size_t>(m) * m, st);
        }
        if (weights != nullptr) upload_per_row(weights, true, plan, q_dev, st);
        Event ev[2];
        for (Event &e : ev) e.create(true);
        for (int s = 0; s < plan.slabs; ++s) {
            grid.enqueue_shared(s, slab.p);
            for (size_t g = 0; g < G; ++g) {
                grid.enqueue_values(g, s, slab.p);
                LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
                grid.block.enqueue_gather_kmm(slab.p, ld, plan.row0(s), plan.rows(s), dev[g].Kmm.p);
                LSSVM_HIP_CHECK(hipGetLastError());
                enqueue_gram(slab.p, ld, cols, plan.rows256(s), max_chunks, part.p, dev[g].St.p, st, q_dev.p != nullptr ? q_dev.p + plan.row0(s) : nullptr);
                LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
                LSSVM_HIP_CHECK(hipEventSynchronize(ev[1].e));
                gram_ms[g] += elapsed_ms(ev[0], ev[1]);
            }
        }
    }

    // ---- per (gamma, cost): the dense steps of fit_reduced_loo (factor 0) or fit_reduced_loo_dev (1); the operand of the cell goes to, or is written on, the device ----
    LeverageArgs a(m, k, G * S, true, st, G);
    std::unique_ptr<DenseFit> fit;
    if (factor == 1) fit = std::make_unique<DenseFit>(m, k, st);
    std::vector<double> tiles(static_cast<size_t>(ntri) * RG_TILE), St, Kmm(static_cast<size_t>(m) * m), shift(G * m), ybar(a.num_ops * k), Bt(a.op_stride), L, nus(G * S), host_ms(G * S);
    for (size_t g = 0; g < G; ++g) {
        LSSVM_HIP_CHECK(hipMemcpyAsync(tiles.data(), dev[g].St.p, tiles.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        LSSVM_HIP_CHECK(hipMemcpyAsync(Kmm.data(), dev[g].Kmm.p, Kmm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));
        unpack_tiles(tiles, cols, St);
        const double *s_row = &St[static_cast<size_t>(m) * cols];
        for (int j = 0; j < m; ++j) shift[g * m + j] = s_row[j] / Nd;
        for (size_t s = 0; s < S; ++s) {
            const size_t o = g * S + s;
            const double t_cell = now_ms();
            if (factor == 1) {
                double device_ms = 0.0;
                nus[o] = fit->run(dev[g], St, Kmm, cols, Nd, 1.0 / costs[s], a.Bt.p + o * a.op_stride, a.ldb, betas_out + o * k * m, rhos_out + o * k, dense_out != nullptr ? dense_out + o : nullptr,
                                  &device_ms);
                for (int c = 0; c < k; ++c) ybar[o * k + c] = St[static_cast<size_t>(m + 1 + c) * cols + m] / Nd;
                host_ms[o] = std::max(0.0, now_ms() - t_cell - device_ms);
            } else {
                nus[o] = host_operand(St, Kmm, m, k, cols, Nd, costs[s], a.ldb, betas_out + o * k * m, rhos_out + o * k, L, Bt, &ybar[o * k]);
                host_ms[o] = now_ms() - t_cell;
                a.upload_operand(o, Bt.data());
                LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (Bt is filled again for the next cell)
            }
        }
        dev[g].St.release();  // (the cells of this gamma are done with both)
        dev[g].Kmm.release();
    }
    a.upload_shift(shift.data(), ybar.data());

    // ---- pass 2: the slabs again, the leverage kernel per (gamma, cost) ----
    a.inv_n = 1.0 / Nd;
    a.Y = Y;
    a.w = weights;
    a.h_out = leverage_out;
    a.f_out = fitted_out;
    a.loo_out = loo_out;
    a.press = press_out;
    a.errors = loo_errors_out;
    leverage_pass(lm, slab_rows, a, &grid);

    if (landmarks_out != nullptr) std::copy(lm.begin(), lm.end(), landmarks_out);
    if (infos != nullptr) {
        for (size_t o = 0; o < G * S; ++o) {
            const size_t g = o / S;
            infos[o] = lssvm_reduced_grid_info{};
            infos[o].cost = costs[o % S];
            infos[o].jitter = nus[o];
            infos[o].max_leverage = a.max_leverage[o];
            infos[o].landmark_ms = grid.accumulate_ms + grid.values_ms[g];
            infos[o].gram_ms = gram_ms[g];
            infos[o].leverage_ms = a.leverage_ms[o];
            infos[o].host_ms = host_ms[o];
            infos[o].gamma = gammas[g];
            infos[o].accumulate_ms = grid.accumulate_ms;
            infos[o].values_ms = grid.values_ms[g];
        }
    }
}

/* D alone for all N points (a test aid): the slabs of GridSlabs in the library's default size, each downloaded column by column */
template <typename T>
void Solver<T>::landmark_acc(const uint64_t *landmarks, uint64_t rank, int product, double *D_out) {
    LSSVM_REQUIRE(D_out != nullptr, "D_out must not be NULL");
    LSSVM_REQUIRE(product == 0 || product == 1, "product must be 0 (ordered) or 1 (matrix), but is " + std::to_string(product) + "!");
    Problem<T> &p = reduced_problem("landmark_acc", true);
    const size_t N = p.N_;
    check_reduced_arguments(D_out, 1, rank, 0, N);
    const int m = static_cast<int>(rank);
    const std::vector<uint64_t> lm = resolve_landmarks(landmarks, static_cast<size_t>(m), N);

    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    GridSlabs<T> grid(p, lm, nullptr, 0, 0, nullptr, 0, product, st);
    for (int s = 0; s < grid.plan.slabs; ++s) {
        grid.enqueue_acc(s);
        LSSVM_HIP_CHECK(hipMemcpy2DAsync(D_out + grid.plan.row0(s), N * sizeof(double), grid.D.p, grid.plan.ld * sizeof(double), static_cast<size_t>(grid.plan.rows(s)) * sizeof(double),
                                         static_cast<size_t>(m), hipMemcpyDeviceToHost, st));
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    }
}

template <typename T>
void Solver<T>::reduced_leverage(uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *V, const double *shift, const double *B_extra, size_t num_extra, double *h_out,
                                 double *f_out) {
    // ---- everything that needs no device (as reduced_gram) ----
    Problem<T> &p = reduced_problem("reduced_leverage", true);
    check_reduced_arguments(V, 1, rank, slab_rows, p.N_);
    LSSVM_REQUIRE(V != nullptr && shift != nullptr && h_out != nullptr, "V / shift / h_out must not be NULL");
    LSSVM_REQUIRE(num_extra <= 4096 && (num_extra == 0 || (B_extra != nullptr && f_out != nullptr)), "at most 4096 extra columns; B_extra / f_out must not be NULL where there are some");
    const int m = static_cast<int>(rank), k = static_cast<int>(num_extra);
    const std::vector<uint64_t> lm = resolve_landmarks(landmarks, static_cast<size_t>(m), p.N_);

    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    LeverageArgs a(m, k, 1, false, p.stream());
    std::vector<double> Bt(a.op_stride, 0.0);
    for (int n = 0; n < m; ++n) std::copy(V + static_cast<size_t>(n) * m, V + static_cast<size_t>(n + 1) * m, &Bt[static_cast<size_t>(n) * a.ldb]);  // (as given, what stands above the diagonal too: the kernel masks it)
    for (int c = 0; c < k; ++c)
        for (int j = 0; j < m; ++j) Bt[static_cast<size_t>(m + c) * a.ldb + j] = B_extra[static_cast<size_t>(j) * k + c];
    a.upload_operand(0, Bt.data());
    a.upload_shift(shift, nullptr);
    a.h_out = h_out;
    a.f_out = f_out;
    leverage_pass(lm, slab_rows, a);
}

/* ---- every prefix rank of one fit ---- */
/* The Phi slabs once more (as leverage_pass) and, per slab and operand, k_reduced_leverage_prefix once per group of PFX_KMAX right-hand sides; h, f and loo of the slab
 * and every checkpoint go to the caller's arrays, the sums over the points are formed here in row order as leverage_pass forms them. */
template <typename T>
void Solver<T>::prefix_pass(const std::vector<uint64_t> &lm, uint64_t slab_rows, PrefixArgs &a) {
    Problem<T> &p = *shards_[0];
    const size_t N = p.N_;
    const int m = a.m, k = a.k, R = a.R;
    const bool with_y = a.Y != nullptr;
    const int cols = with_y ? m + 1 + k : m;
    hipStream_t st = p.stream();
    const SlabPlan plan(N, slab_rows);
    const size_t ld = plan.ld;

    const LandmarkBlock<T> block(p, lm, st);
    const RhsOnDevice<T> rhs(a.Y, k, N, st);
    DevBuf<double> slab, h_dev, f_dev, loo_dev, w_dev;
    if (a.w != nullptr) upload_per_row(a.w, false, plan, w_dev, st);
    const size_t group = static_cast<size_t>(R) * PFX_KMAX * ld;  // what one launch writes of f and of loo
    slab.alloc_zero(static_cast<size_t>(cols) * ld, st);
    h_dev.alloc_zero(static_cast<size_t>(R) * ld, st);
    f_dev.alloc_zero(group, st);
    if (with_y) loo_dev.alloc_zero(group, st);
    std::vector<double> h_host(static_cast<size_t>(R) * ld), f_host(group), loo_host(with_y ? group : 0);

    Event ev[2];
    for (Event &e : ev) e.create(true);
    a.max_leverage.assign(a.num_ops * R, 0.0);
    a.leverage_ms.assign(a.num_ops, 0.0);
    a.landmark_ms = 0.0;
    if (a.press != nullptr) std::fill(a.press, a.press + a.num_ops * R * k, 0.0);
    if (a.errors != nullptr) std::fill(a.errors, a.errors + a.num_ops * R * k, uint64_t{ 0 });
    const T *Yh = static_cast<const T *>(a.Y);
    for (int s = 0; s < plan.slabs; ++s) {
        const size_t row0 = plan.row0(s);
        const int rows = plan.rows(s);
        LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
        enqueue_slab(block, m, plan, s, rhs, slab.p, st);
        LSSVM_HIP_CHECK(hipGetLastError());
        LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
        LSSVM_HIP_CHECK(hipEventSynchronize(ev[1].e));
        a.landmark_ms += elapsed_ms(ev[0], ev[1]);
        for (size_t o = 0; o < a.num_ops; ++o) {
            for (int c0 = 0; c0 == 0 || c0 < k; c0 += PFX_KMAX) {  // (k == 0: one launch for h alone)
                const int kc = std::min(PFX_KMAX, k - c0);
                const size_t out_bytes = static_cast<size_t>(R) * std::max(kc, 1) * ld * sizeof(double);
                LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
                a.enqueue(o, c0, kc, slab.p, ld, rows, h_dev.p, f_dev.p, loo_dev.p, w_dev.p != nullptr ? w_dev.p + row0 : nullptr);
                LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
                if (c0 == 0) LSSVM_HIP_CHECK(hipMemcpyAsync(h_host.data(), h_dev.p, h_host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
                if (kc > 0) LSSVM_HIP_CHECK(hipMemcpyAsync(f_host.data(), f_dev.p, out_bytes, hipMemcpyDeviceToHost, st));
                if (kc > 0 && with_y) LSSVM_HIP_CHECK(hipMemcpyAsync(loo_host.data(), loo_dev.p, out_bytes, hipMemcpyDeviceToHost, st));
                LSSVM_HIP_CHECK(hipStreamSynchronize(st));
                a.leverage_ms[o] += elapsed_ms(ev[0], ev[1]);
                for (int q = 0; q < R; ++q) {
                    const size_t oq = o * R + q;
                    if (c0 == 0) {
                        const double *h = &h_host[static_cast<size_t>(q) * ld];
                        for (int i = 0; i < rows; ++i) a.max_leverage[oq] = std::max(a.max_leverage[oq], h[i]);
                        if (a.h_out != nullptr) std::copy(h, h + rows, a.h_out + oq * N + row0);
                    }
                    for (int c = 0; c < kc; ++c) {
                        const size_t oc = oq * k + c0 + c, at = (static_cast<size_t>(q) * kc + c) * ld;
                        if (a.f_out != nullptr) std::copy(&f_host[at], &f_host[at] + rows, a.f_out + oc * N + row0);
                        if (!with_y) continue;
                        const double *loo = &loo_host[at];
                        if (a.loo_out != nullptr) std::copy(loo, loo + rows, a.loo_out + oc * N + row0);
                        double press = a.press != nullptr ? a.press[oc] : 0.0;
                        uint64_t errors = 0;
                        for (int i = 0; i < rows; ++i) {
                            const double y = static_cast<double>(Yh[static_cast<size_t>(c0 + c) * N + row0 + i]), d = y - loo[i];
                            const bool wrong = ((loo[i] > 0.0) - (loo[i] < 0.0)) != ((y > 0.0) - (y < 0.0));
                            if (a.w != nullptr) {  // sum_i w_i d_i^2; the errors over the points that took part in the fit
                                press += a.w[row0 + i] * (d * d);
                                errors += wrong && a.w[row0 + i] > 0.0 ? 1 : 0;
                            } else {
                                press += d * d;
                                errors += wrong ? 1 : 0;
                            }
                        }
                        if (a.press != nullptr) a.press[oc] = press;
                        if (a.errors != nullptr) a.errors[oc] += errors;
                    }
                }
            }
        }
    }
}

template <typename T>
void Solver<T>::fit_reduced_rank_path(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const uint64_t *ranks,
                                      size_t num_ranks, const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out, double *press_out,
                                      uint64_t *loo_errors_out, double *leverage_out, double *fitted_out, double *loo_out, uint64_t *landmarks_out, lssvm_reduced_rank_info *infos,
                                      lssvm_dense_info *dense_out) {
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    check_reduced_loo_costs(costs, num_costs);
    check_reduced_factor(factor);
    check_reduced_rank_list(ranks, num_ranks, rank, num_costs);
    std::vector<uint64_t> lm;
    std::vector<double> St, Kmm;
    lssvm_reduced_info info{};
    ReducedOnDevice dev;
    double Nd = 0.0;  // N, or the sum of the weights
    reduced_gram("fit_reduced_rank_path", Y, num_rhs, rank, landmarks, slab_rows, lm, St, Kmm, info, factor == 1 ? &dev : nullptr, weights, &Nd);  // pass 1, and every other check that needs no device

    const int m = static_cast<int>(rank), k = static_cast<int>(num_rhs), cols = m + 1 + k, R = static_cast<int>(num_ranks);
    Problem<T> &p = *shards_[0];
    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    PrefixArgs a(m, k, ranks, num_ranks, num_costs, true, st);
    const size_t cell = static_cast<size_t>(k) * m;  // the betas of a (cost, checkpoint)

    // ---- per cost: L, V and z as the leave-one-out call of `factor` forms them, then the betas and rhos of every checkpoint off the leading blocks ----
    const double *s_row = &St[static_cast<size_t>(m) * cols];
    std::vector<double> shift(static_cast<size_t>(m)), ybar(num_costs * k), nus(num_costs), host_ms(num_costs), cond(num_costs * R);
    for (int j = 0; j < m; ++j) shift[j] = s_row[j] / Nd;
    for (size_t s = 0; s < num_costs; ++s)
        for (int c = 0; c < k; ++c) ybar[s * k + c] = St[static_cast<size_t>(m + 1 + c) * cols + m] / Nd;
    if (factor == 1) {
        DenseFit fit(m, k, st);
        DevBuf<double> betas_dev, rhos_dev, cond_dev;
        betas_dev.alloc_zero(static_cast<size_t>(R) * cell, st);
        rhos_dev.alloc_zero(static_cast<size_t>(R) * k, st);
        cond_dev.alloc_zero(static_cast<size_t>(R), st);
        std::vector<double> full_betas(cell), full_rhos(static_cast<size_t>(k));  // the full rank's by the back substitution: not returned (the checkpoints' are V^T z)
        for (size_t s = 0; s < num_costs; ++s) {
            const double t_cost = now_ms();
            double device_ms = 0.0;
            nus[s] = fit.run(dev, St, Kmm, cols, Nd, 1.0 / costs[s], a.V_of(s), a.ldb, full_betas.data(), full_rhos.data(), dense_out != nullptr ? dense_out + s : nullptr, &device_ms, a.Z_of(s));
            fit.dense.enqueue_prefix_betas(a.V_of(s), a.ldb, a.Z_of(s), static_cast<size_t>(a.ldb), k, a.ranks_dev.p, R, Nd, betas_dev.p, rhos_dev.p, cond_dev.p);
            LSSVM_HIP_CHECK(hipMemcpyAsync(betas_out + s * R * cell, betas_dev.p, betas_dev.count * sizeof(double), hipMemcpyDeviceToHost, st));
            LSSVM_HIP_CHECK(hipMemcpyAsync(rhos_out + s * R * k, rhos_dev.p, rhos_dev.count * sizeof(double), hipMemcpyDeviceToHost, st));
            LSSVM_HIP_CHECK(hipMemcpyAsync(&cond[s * R], cond_dev.p, cond_dev.count * sizeof(double), hipMemcpyDeviceToHost, st));
            LSSVM_HIP_CHECK(hipStreamSynchronize(st));
            host_ms[s] = std::max(0.0, now_ms() - t_cost - device_ms);
        }
    } else {
        std::vector<double> L, op(a.op_stride);
        for (size_t s = 0; s < num_costs; ++s) {
            const double t_host = now_ms();
            nus[s] = factor_reduced(St, Kmm, m, cols, Nd, 1.0 / costs[s], L);
            std::fill(op.begin(), op.end(), 0.0);
            for (int c = 0; c < k; ++c) {
                double *z = &op[static_cast<size_t>(m + c) * a.ldb];
                forward_reduced(St, L, m, c, cols, Nd, z);
                for (int q = 0; q < R; ++q) {
                    double *beta = betas_out + (s * R + q) * cell + static_cast<size_t>(c) * m;
                    std::fill(beta, beta + m, 0.0);
                    rhos_out[(s * R + q) * k + c] = backward_reduced(St, L, m, a.ranks[q], c, cols, Nd, z, beta);
                }
            }
            invert_lower_rows(L, m, op.data(), static_cast<size_t>(a.ldb));
            for (int q = 0; q < R; ++q) {
                double hi = 0.0, lo = DBL_MAX;
                for (int j = 0; j < a.ranks[q]; ++j) {
                    const double d = L[static_cast<size_t>(j) * m + j];
                    hi = std::max(hi, d * d);
                    lo = std::min(lo, d * d);
                }
                cond[s * R + q] = hi / lo;
            }
            host_ms[s] = now_ms() - t_host;
            a.upload_operand(s, op.data());
        }
    }
    a.upload_shift(shift.data(), ybar.data());

    // ---- pass 2: the slabs again, the prefix leverage kernel per cost ----
    a.inv_n = 1.0 / Nd;
    a.Y = Y;
    a.w = weights;
    a.h_out = leverage_out;
    a.f_out = fitted_out;
    a.loo_out = loo_out;
    a.press = press_out;
    a.errors = loo_errors_out;
    prefix_pass(lm, slab_rows, a);

    if (landmarks_out != nullptr) std::copy(lm.begin(), lm.end(), landmarks_out);
    if (infos != nullptr) {
        for (size_t o = 0; o < num_costs * R; ++o) {
            const size_t s = o / R;
            infos[o] = lssvm_reduced_rank_info{};
            infos[o].cost = costs[s];
            infos[o].rank = ranks[o % R];
            infos[o].jitter = nus[s];
            infos[o].max_leverage = a.max_leverage[o];
            infos[o].landmark_ms = info.landmark_ms + a.landmark_ms;
            infos[o].gram_ms = info.gram_ms;
            infos[o].leverage_ms = a.leverage_ms[s];
            infos[o].host_ms = host_ms[s];
            infos[o].cond_hint = cond[o];
        }
    }
}

template <typename T>
void Solver<T>::reduced_leverage_prefix(uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *V, const double *shift, const double *Z, size_t num_cols,
                                        const uint64_t *ranks, size_t num_ranks, double *h_out, double *f_out) {
    // ---- everything that needs no device (as reduced_leverage) ----
    Problem<T> &p = reduced_problem("reduced_leverage_prefix", true);
    check_reduced_arguments(V, 1, rank, slab_rows, p.N_);
    LSSVM_REQUIRE(V != nullptr && shift != nullptr && h_out != nullptr, "V / shift / h_out must not be NULL");
    LSSVM_REQUIRE(num_cols <= 4096 && (num_cols == 0 || (Z != nullptr && f_out != nullptr)), "at most 4096 rows of Z; Z / f_out must not be NULL where there are some");
    check_reduced_rank_list(ranks, num_ranks, rank, 1);
    const int m = static_cast<int>(rank), k = static_cast<int>(num_cols);
    const std::vector<uint64_t> lm = resolve_landmarks(landmarks, static_cast<size_t>(m), p.N_);

    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    PrefixArgs a(m, k, ranks, num_ranks, 1, false, p.stream());
    std::vector<double> op(a.op_stride, 0.0);
    for (int n = 0; n < m; ++n) std::copy(V + static_cast<size_t>(n) * m, V + static_cast<size_t>(n + 1) * m, &op[static_cast<size_t>(n) * a.ldb]);  // (as given, what stands above the diagonal too: the kernel masks it)
    for (int c = 0; c < k; ++c) std::copy(Z + static_cast<size_t>(c) * m, Z + static_cast<size_t>(c + 1) * m, &op[static_cast<size_t>(m + c) * a.ldb]);
    a.upload_operand(0, op.data());
    a.upload_shift(shift, nullptr);
    a.h_out = h_out;
    a.f_out = f_out;
    prefix_pass(lm, slab_rows, a);
}

template <typename T>
void Solver<T>::time_leverage_prefix_kernel(uint64_t rank, uint64_t slab_rows, size_t num_cols, const uint64_t *ranks, size_t num_ranks, int repeats, double *prefix_ms_out) {
    Problem<T> &p = reduced_problem("time_leverage_prefix_kernel", false);  // (the aid times a kernel on the data: the weights do not enter)
    LSSVM_REQUIRE(repeats >= 1 && repeats <= 1000 && prefix_ms_out != nullptr, "repeats must lie in [1, 1000]; prefix_ms_out must not be NULL");
    LSSVM_REQUIRE(num_cols >= 1 && num_cols <= static_cast<size_t>(PFX_KMAX), "between 1 and 4 right-hand sides (one launch of the kernel)");
    const size_t N = p.N_;
    check_reduced_arguments(prefix_ms_out, 1, rank, slab_rows, N);
    check_reduced_rank_list(ranks, num_ranks, rank, 1);
    const int m = static_cast<int>(rank), k = static_cast<int>(num_cols), cols = m + 1 + k, R = static_cast<int>(num_ranks);
    const std::vector<uint64_t> lm = resolve_landmarks(nullptr, static_cast<size_t>(m), N);

    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    const SlabPlan plan(N, slab_rows);  // (the first slab alone, as time_leverage_kernel)
    const size_t ld = plan.ld;
    const std::vector<T> Yh(static_cast<size_t>(k) * N, T(1));
    const LandmarkBlock<T> block(p, lm, st);
    const RhsOnDevice<T> rhs(Yh.data(), k, N, st);
    DevBuf<double> slab, h_dev, f_dev, loo_dev;
    slab.alloc_zero(static_cast<size_t>(cols) * ld, st);
    PrefixArgs a(m, k, ranks, num_ranks, 1, false, st);  // V = I, every z of ones, shift = 0
    std::vector<double> op(a.op_stride, 0.0);
    for (int n = 0; n < m + k; ++n)
        for (int j = 0; j < m; ++j) op[static_cast<size_t>(n) * a.ldb + j] = n >= m || n == j ? 1.0 : 0.0;
    a.upload_operand(0, op.data());
    a.inv_n = 1.0 / static_cast<double>(N);
    h_dev.alloc_zero(static_cast<size_t>(R) * ld, st);
    f_dev.alloc_zero(static_cast<size_t>(R) * k * ld, st);
    loo_dev.alloc_zero(static_cast<size_t>(R) * k * ld, st);
    enqueue_slab(block, m, plan, 0, rhs, slab.p, st);
    LSSVM_HIP_CHECK(hipGetLastError());
    timed_repeats(st, repeats, prefix_ms_out, [] {}, [&] { a.enqueue(0, 0, k, slab.p, ld, plan.rows(0), h_dev.p, f_dev.p, loo_dev.p, nullptr); });
}

template <typename T>
void Solver<T>::time_leverage_kernel(uint64_t rank, uint64_t slab_rows, size_t num_extra, int repeats, double *gram_ms_out, double *leverage_ms_out) {
    Problem<T> &p = reduced_problem("time_leverage_kernel", false);  // (the aid times kernels on the data: the weights do not enter)
    LSSVM_REQUIRE(repeats >= 1 && repeats <= 1000 && gram_ms_out != nullptr && leverage_ms_out != nullptr, "repeats must lie in [1, 1000]; gram_ms_out / leverage_ms_out must not be NULL");
    LSSVM_REQUIRE(num_extra >= 1 && num_extra <= 64, "between 1 and 64 extra columns");
    const size_t N = p.N_;
    check_reduced_arguments(gram_ms_out, 1, rank, slab_rows, N);
    const int m = static_cast<int>(rank), k = static_cast<int>(num_extra), cols = m + 1 + k;
    const std::vector<uint64_t> lm = resolve_landmarks(nullptr, static_cast<size_t>(m), N);

    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    const SlabPlan plan(N, slab_rows);  // (the first slab alone)
    const size_t ld = plan.ld;
    const int nt = tiles_of(cols), ntri = nt * (nt + 1) / 2, max_chunks = static_cast<int>((ld + RG_RANGE - 1) / RG_RANGE);
    const std::vector<T> Yh(static_cast<size_t>(k) * N, T(1));
    const LandmarkBlock<T> block(p, lm, st);
    const RhsOnDevice<T> rhs(Yh.data(), k, N, st);
    DevBuf<double> slab, part, St_dev, h_dev, f_dev, loo_dev;
    slab.alloc_zero(static_cast<size_t>(cols) * ld, st);
    part.alloc_zero(static_cast<size_t>(ntri) * max_chunks * RG_TILE, st);
    St_dev.alloc_zero(static_cast<size_t>(ntri) * RG_TILE, st);
    LeverageArgs a(m, k, 1, false, st);  // V = I, every extra column of ones, shift = 0
    std::vector<double> Bt(a.op_stride, 0.0);
    for (int n = 0; n < m + k; ++n)
        for (int j = 0; j < m; ++j) Bt[static_cast<size_t>(n) * a.ldb + j] = n >= m || n == j ? 1.0 : 0.0;
    a.upload_operand(0, Bt.data());
    a.inv_n = 1.0 / static_cast<double>(N);
    h_dev.alloc_zero(ld, st);
    f_dev.alloc_zero(static_cast<size_t>(k) * ld, st);
    loo_dev.alloc_zero(static_cast<size_t>(k) * ld, st);
    enqueue_slab(block, m, plan, 0, rhs, slab.p, st);
    LSSVM_HIP_CHECK(hipGetLastError());
    timed_repeats(st, repeats, gram_ms_out, [&] { LSSVM_HIP_CHECK(hipMemsetAsync(St_dev.p, 0, St_dev.count * sizeof(double), st)); },
                  [&] { enqueue_gram(slab.p, ld, cols, plan.rows256(0), max_chunks, part.p, St_dev.p, st); });
    timed_repeats(st, repeats, leverage_ms_out, [] {}, [&] { a.enqueue(0, slab.p, ld, plan.rows(0), h_dev.p, f_dev.p, loo_dev.p); });
}

template <typename T>
void Solver<T>::time_gram_kernels(int repeats, double *parent_ms_out, double *mfma_ms_out, double *max_diff_out) {
    LSSVM_REQUIRE(repeats >= 1 && repeats <= 1000 && parent_ms_out != nullptr && mfma_ms_out != nullptr, "repeats must lie in [1, 1000]; parent_ms_out / mfma_ms_out must not be NULL");
    if constexpr (!std::is_same_v<T, double>) {
        LSSVM_REQUIRE(false, "time_gram_kernels compares the two kernels on an fp64 problem's preconditioner");
    } else {
        Problem<T> &p = precond_problem("time_gram_kernels");
        LSSVM_REQUIRE(precond_ != nullptr, "the problem has no preconditioner (lssvm_mi355_problem_build_preconditioner builds one)");
        const SetOnExit<bool> busy = hold_busy();
        p.activate();
        hipStream_t st = p.stream();
        const Precond<T> &pc = *precond_;
        const int cols = pc.cols, rows = static_cast<int>(pc.ldn);
        const int tiles16 = (cols + 15) / 16, ldg = tiles16 * 16;
        const int nt = tiles_of(cols), ntri = nt * (nt + 1) / 2, max_chunks = (rows + RG_RANGE - 1) / RG_RANGE;
        DevBuf<double> G_dev, part, St_dev;
        G_dev.alloc_zero(static_cast<size_t>(ldg) * ldg, st);
        part.alloc_zero(static_cast<size_t>(ntri) * max_chunks * RG_TILE, st);
        St_dev.alloc_zero(static_cast<size_t>(ntri) * RG_TILE, st);
        timed_repeats(st, repeats, parent_ms_out, [] {}, [&] { hipLaunchKernelGGL(k_precond_gram<T>, dim3(tiles16, tiles16), dim3(256), 0, st, pc.Bhat.p, pc.ldn, cols, G_dev.p, ldg); });
        timed_repeats(st, repeats, mfma_ms_out, [&] { LSSVM_HIP_CHECK(hipMemsetAsync(St_dev.p, 0, St_dev.count * sizeof(double), st)); },
                      [&] { enqueue_gram(pc.Bhat.p, pc.ldn, cols, rows, max_chunks, part.p, St_dev.p, st); });
        if (max_diff_out != nullptr) {
            std::vector<double> Gpad(static_cast<size_t>(ldg) * ldg), tiles(static_cast<size_t>(ntri) * RG_TILE), G;
            LSSVM_HIP_CHECK(hipMemcpyAsync(Gpad.data(), G_dev.p, Gpad.size() * sizeof(double), hipMemcpyDeviceToHost, st));
            LSSVM_HIP_CHECK(hipMemcpyAsync(tiles.data(), St_dev.p, tiles.size() * sizeof(double), hipMemcpyDeviceToHost, st));
            LSSVM_HIP_CHECK(hipStreamSynchronize(st));
            unpack_tiles(tiles, cols, G);
            double diff = 0.0, largest = 0.0;
            for (int j = 0; j < cols; ++j) {
                for (int l = 0; l <= j; ++l) {
                    diff = std::max(diff, std::fabs(G[static_cast<size_t>(j) * cols + l] - Gpad[static_cast<size_t>(j) * ldg + l]));
                    largest = std::max(largest, std::fabs(Gpad[static_cast<size_t>(j) * ldg + l]));
                }
            }
            *max_diff_out = largest > 0.0 ? diff / largest : diff;
        }
    }
}

template void Solver<float>::landmark_gram(const void *, size_t, uint64_t, const uint64_t *, uint64_t, double *, const double *);
template void Solver<double>::landmark_gram(const void *, size_t, uint64_t, const uint64_t *, uint64_t, double *, const double *);
template void Solver<float>::fit_reduced(const void *, size_t, uint64_t, const uint64_t *, uint64_t, double *, double *, uint64_t *, lssvm_reduced_info *, const double *);
template void Solver<double>::fit_reduced(const void *, size_t, uint64_t, const uint64_t *, uint64_t, double *, double *, uint64_t *, lssvm_reduced_info *, const double *);
template void Solver<float>::fit_reduced_loo(const void *, size_t, uint64_t, const uint64_t *, uint64_t, const double *, size_t, double *, double *, double *, double *, double *, double *, uint64_t *,
                                             uint64_t *, lssvm_reduced_loo_info *, const double *);
template void Solver<double>::fit_reduced_loo(const void *, size_t, uint64_t, const uint64_t *, uint64_t, const double *, size_t, double *, double *, double *, double *, double *, double *, uint64_t *,
                                              uint64_t *, lssvm_reduced_loo_info *, const double *);
template void Solver<float>::fit_reduced_dev(const void *, size_t, uint64_t, const uint64_t *, uint64_t, double *, double *, uint64_t *, lssvm_reduced_info *, lssvm_dense_info *, const double *);
template void Solver<double>::fit_reduced_dev(const void *, size_t, uint64_t, const uint64_t *, uint64_t, double *, double *, uint64_t *, lssvm_reduced_info *, lssvm_dense_info *, const double *);
template void Solver<float>::fit_reduced_loo_dev(const void *, size_t, uint64_t, const uint64_t *, uint64_t, const double *, size_t, double *, double *, double *, double *, double *, double *, uint64_t *,
                                                 uint64_t *, lssvm_reduced_loo_info *, lssvm_dense_info *, const double *);
template void Solver<double>::fit_reduced_loo_dev(const void *, size_t, uint64_t, const uint64_t *, uint64_t, const double *, size_t, double *, double *, double *, double *, double *, double *, uint64_t *,
                                                  uint64_t *, lssvm_reduced_loo_info *, lssvm_dense_info *, const double *);
template void Solver<float>::fit_reduced_grid(const void *, size_t, const double *, uint64_t, const uint64_t *, uint64_t, const double *, size_t, const double *, size_t, int, int, double *, double *,
                                              double *, double *, double *, double *, uint64_t *, uint64_t *, lssvm_reduced_grid_info *, lssvm_dense_info *);
template void Solver<double>::fit_reduced_grid(const void *, size_t, const double *, uint64_t, const uint64_t *, uint64_t, const double *, size_t, const double *, size_t, int, int, double *, double *,
                                               double *, double *, double *, double *, uint64_t *, uint64_t *, lssvm_reduced_grid_info *, lssvm_dense_info *);
template void Solver<float>::landmark_acc(const uint64_t *, uint64_t, int, double *);
template void Solver<double>::landmark_acc(const uint64_t *, uint64_t, int, double *);
template void Solver<float>::reduced_leverage(uint64_t, const uint64_t *, uint64_t, const double *, const double *, const double *, size_t, double *, double *);
template void Solver<double>::reduced_leverage(uint64_t, const uint64_t *, uint64_t, const double *, const double *, const double *, size_t, double *, double *);
template void Solver<float>::fit_reduced_rank_path(const void *, size_t, const double *, uint64_t, const uint64_t *, uint64_t, const uint64_t *, size_t, const double *, size_t, int, double *,
                                                   double *, double *, uint64_t *, double *, double *, double *, uint64_t *, lssvm_reduced_rank_info *, lssvm_dense_info *);
template void Solver<double>::fit_reduced_rank_path(const void *, size_t, const double *, uint64_t, const uint64_t *, uint64_t, const uint64_t *, size_t, const double *, size_t, int, double *,
                                                    double *, double *, uint64_t *, double *, double *, double *, uint64_t *, lssvm_reduced_rank_info *, lssvm_dense_info *);
template void Solver<float>::reduced_leverage_prefix(uint64_t, const uint64_t *, uint64_t, const double *, const double *, const double *, size_t, const uint64_t *, size_t, double *, double *);
template void Solver<double>::reduced_leverage_prefix(uint64_t, const uint64_t *, uint64_t, const double *, const double *, const double *, size_t, const uint64_t *, size_t, double *, double *);
template void Solver<float>::time_leverage_prefix_kernel(uint64_t, uint64_t, size_t, const uint64_t *, size_t, int, double *);
template void Solver<double>::time_leverage_prefix_kernel(uint64_t, uint64_t, size_t, const uint64_t *, size_t, int, double *);
template void Solver<float>::time_leverage_kernel(uint64_t, uint64_t, size_t, int, double *, double *);
template void Solver<double>::time_leverage_kernel(uint64_t, uint64_t, size_t, int, double *, double *);
template void Solver<float>::time_gram_kernels(int, double *, double *, double *);
template void Solver<double>::time_gram_kernels(int, double *, double *, double *);

/* ---- the fixed-size model from a stream of chunks (lssvm_mi355_reduced_stream_*) ---- */
namespace {

/* n[i] = the sum over the ldx held features (ascending) of (x_if - c_f)^2, in double, as k_row_norms forms it: the squared norms k_cross_product expands the rbf distance
 * with, of the rows AS THEY ARE STAGED there (centre: ldx doubles, zeros from the last feature on, so a padded feature adds an exact 0) */
template <typename T>
__global__ __launch_bounds__(256) void k_centred_norms(const T *__restrict__ X, int ldx, size_t N, const double *__restrict__ centre, double *__restrict__ n) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= N) return;
    const T *xi = X + i * ldx;
    double acc = 0.0;
    for (int f = 0; f < ldx; ++f) {
        const double a = static_cast<double>(xi[f]) - centre[f];
        acc += a * a;
    }
    n[i] = acc;
}

/* The sibling of k_landmark_product for rows that are NOT in a resident problem: D[l][i] of the n rows of `Xc` (a chunk, held padded to ldx features) against the m
 * landmark ROWS `XL`, held on their own.  Tiling, LDS layout, fragments and the pinned accumulators are k_landmark_product's: 128 landmarks (blockIdx.y) x 128 rows
 * (blockIdx.x) per workgroup, four waves of 64 x 64, sixteen accumulators of v_mfma_f64_16x16x4_f64 each, both operands through LDS in steps of RG_KC = 16 features.
 * What differs: the A operand is read from XL and the B operand from Xc, two base pointers and no index list; `centre` (ldx doubles, zeros for a kernel that is not
 * translation invariant and from the last feature on) is SUBTRACTED from both operands as they are staged -- one f64x2 of it per step and thread, every operand is
 * (double) x_f - c_f; and D may start at any row of a slab (the host adds the fill position to the pointer), so its stores are 8-byte aligned only.
 * rbf: D = max(n_i + n_l - 2 x_i . x_l, 0) with norms_c / norms_l of k_centred_norms.  A streamed row carries no index, so there is no "the landmark itself" test: only
 * `diag` (the K_mm launch: Xc == XL) sets D[l][l] to exactly 0.  Any other kernel type: the dot product.
 * Landmarks from m on and rows from n on count as zeros and are never read; landmarks from m on are not written, rows from n on up to the end of the workgroup's 128 are
 * written as zeros -- a slab keeps that much slack behind its last row.  No atomics, no scratch; the order of every sum depends on ldx only. */
template <typename T>
__global__ __launch_bounds__(256, 2) void k_cross_product(const T *__restrict__ XL, const T *__restrict__ Xc, int ldx, int n, int m, const double *__restrict__ centre, int kernel_type,
                                                          const double *__restrict__ norms_l, const double *__restrict__ norms_c, int diag, double *__restrict__ D, size_t ld) {
    using pair = typename PairOf<T>::type;
    __shared__ __attribute__((aligned(16))) double As[RG_TW * RG_LS];
    __shared__ __attribute__((aligned(16))) double Bs[RG_TW * RG_LS];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int r = lane & 15, qd = lane >> 4;
    const int l0 = blockIdx.y * RG_TW;      // the workgroup's first landmark
    const int local0 = blockIdx.x * RG_TW;  // ... and first row of the chunk
    const int nsteps = ldx / RG_KC;

    // staging: thread -> (point srow [+ 32 p] of the tile, features 2 sseg, 2 sseg + 1 of the step), as k_landmark_product
    const int srow = tid >> 3, sseg = tid & 7;
    const T *Ag[4], *Bg[4];
    bool a_in[4], b_in[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int la = l0 + srow + 32 * p, ib = local0 + srow + 32 * p;
        a_in[p] = la < m;
        b_in[p] = ib < n;
        Ag[p] = XL + static_cast<size_t>(a_in[p] ? la : 0) * ldx + 2 * sseg;
        Bg[p] = Xc + static_cast<size_t>(b_in[p] ? ib : 0) * ldx + 2 * sseg;
    }
    const double *cg = centre + 2 * sseg;
    const int lds_w = srow * RG_LS + 2 * sseg;
    f64x2 sa[4], sb[4];
    const f64x2 zero2 = { 0.0, 0.0 };
    auto stage_load = [&](int s) {
        const f64x2 c2 = *reinterpret_cast<const f64x2 *>(cg + s * RG_KC);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            sa[p] = zero2;
            sb[p] = zero2;
            if (a_in[p]) {
                const pair v = *reinterpret_cast<const pair *>(Ag[p] + s * RG_KC);
                sa[p] = f64x2{ static_cast<double>(v[0]) - c2[0], static_cast<double>(v[1]) - c2[1] };
            }
            if (b_in[p]) {
                const pair v = *reinterpret_cast<const pair *>(Bg[p] + s * RG_KC);
                sb[p] = f64x2{ static_cast<double>(v[0]) - c2[0], static_cast<double>(v[1]) - c2[1] };
            }
        }
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *reinterpret_cast<f64x2 *>(As + lds_w + p * 32 * RG_LS) = sa[p];
            *reinterpret_cast<f64x2 *>(Bs + lds_w + p * 32 * RG_LS) = sb[p];
        }
    };

    f64x4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            acc[mt][nt] = f64x4{ 0.0, 0.0, 0.0, 0.0 };
            // the start values live in the accumulators' OWN registers (C == D for every MFMA of a chain), as in k_reduced_gram
            asm volatile("" : "+v"(acc[mt][nt]));
        }

    if (nsteps > 0) {
        stage_load(0);
        stage_store();
    }
    __syncthreads();
    const double *Ab = As + (wr * 64 + r) * RG_LS + qd;
    const double *Bb = Bs + (wc * 64 + r) * RG_LS + qd;
    for (int s = 0; s < nsteps; ++s) {
        const bool has_next = s + 1 < nsteps;
        if (has_next) stage_load(s + 1);
#pragma unroll
        for (int ks = 0; ks < RG_KC / 4; ++ks) {
            double av[4], bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                av[t] = Ab[t * 16 * RG_LS + ks * 4];
                bv[t] = Bb[t * 16 * RG_LS + ks * 4];
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
        }
        __syncthreads();  // (every wave has read this step)
        if (has_next) {
            stage_store();
            __syncthreads();
        }
    }

    // a lane holds landmarks l0 + wr 64 + mt 16 + qd + 4 i and rows local0 + wc 64 + nt 16 + r
    const bool rbf = kernel_type == LSSVM_KERNEL_RBF;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int local = local0 + wc * 64 + nt * 16 + r;
        const bool row_in = local < n;
        const double ni = rbf && row_in ? norms_c[local] : 0.0;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int l = l0 + wr * 64 + mt * 16 + qd + 4 * i;
                if (l >= m) continue;
                double d = acc[mt][nt][i];
                if (rbf) {
                    d = fmax((ni + norms_l[l]) - 2.0 * d, 0.0);
                    if (diag != 0 && l == local) d = 0.0;
                }
                D[static_cast<size_t>(l) * ld + local] = row_in ? d : 0.0;
            }
    }
}

/* the sibling of k_reduced_aux for a chunk: column c of `out` (ld doubles apart; the host has added the fill position) is 1 (c = 0) or right-hand side c - 1 of the
 * chunk-local Y (ldy reals between two right-hand sides), exact zeros from row n on up to the end of the grid's 256-row blocks */
template <typename T>
__global__ __launch_bounds__(256) void k_stream_aux(const T *__restrict__ Y, size_t ldy, int n, double *__restrict__ out, size_t ld) {
    const int local = blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    double v = 0.0;
    if (local < n) v = c == 0 ? 1.0 : static_cast<double>(Y[static_cast<size_t>(c - 1) * ldy + local]);
    out[static_cast<size_t>(c) * ld + local] = v;
}

/* Kmm[a][b] = Kmm[b][a] = Phi[b][a] for b <= a: K_mm out of the landmarks' own Phi (column l: landmark l), the lower triangle mirrored -- symmetric to the bit; a copy */
__global__ __launch_bounds__(256) void k_stream_kmm(const double *__restrict__ Phi, size_t ld, int m, double *__restrict__ Kmm) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m * m) return;
    const int a = e / m, b = e % m;
    Kmm[e] = Phi[static_cast<size_t>(min(a, b)) * ld + max(a, b)];
}

uint64_t fnv1a(const void *bytes, size_t count) {
    const unsigned char *p = static_cast<const unsigned char *>(bytes);
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < count; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

uint64_t bits_of(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

constexpr uint64_t STREAM_MAX_SLAB_ROWS = uint64_t{ 1 } << 24;  // (row counts are ints in the kernels)

/* The handle's state (include/plssvm_amd.h has the contract).  Everything runs on ONE stream of device 0, upload and compute one behind the other; every public call
 * returns with the stream idle, so the caller's buffers are free. */
template <typename T>
class ReducedStream final : public ReducedStreamBase {
  public:
    ReducedStream(const lssvm_params &params, const void *XL, size_t m, size_t d, size_t k, bool weighted, uint64_t slab_rows) :
        params_(params), m_(static_cast<int>(m)), d_(static_cast<int>(d)), k_(static_cast<int>(k)), cols_(m_ + 1 + k_), ldx_(round_up(static_cast<long>(d), RG_KC)), weighted_(weighted),
        slab_rows_(static_cast<size_t>(slab_rows == 0 ? REDUCED_DEFAULT_SLAB_ROWS : slab_rows)), ld_(slab_rows_ + 256), ntri_(tiles_of(cols_) * (tiles_of(cols_) + 1) / 2),
        max_chunks_(static_cast<int>((slab_rows_ + RG_RANGE - 1) / RG_RANGE)), hash_(fnv1a(XL, m * d * sizeof(T))) {
        // the kernel function's scalars as LandmarkBlock::kernel_scalars holds them, for data that is held as it is given
        gamma_ = params.kernel_type == LSSVM_KERNEL_LINEAR ? 1.0 : static_cast<double>(static_cast<T>(params.gamma));
        coef0_ = static_cast<double>(static_cast<T>(params.coef0));
        // the centre (rbf only): the landmarks' mean, every feature summed in ascending l, in double
        centre_host_.assign(static_cast<size_t>(ldx_), 0.0);
        if (params.kernel_type == LSSVM_KERNEL_RBF) {
            const T *xl = static_cast<const T *>(XL);
            for (int f = 0; f < d_; ++f) {
                double sum = 0.0;
                for (int l = 0; l < m_; ++l) sum += static_cast<double>(xl[static_cast<size_t>(l) * d_ + f]);
                centre_host_[f] = sum / static_cast<double>(m_);
            }
        }

        select_device_checked(0);
        stream_.create();
        hipStream_t st = stream_.s;
        const size_t m256 = static_cast<size_t>(round_up(m_, 256));
        XL_.alloc_zero(m256 * ldx_, st);
        Xc_.alloc_zero(slab_rows_ * ldx_, st);
        Yc_.alloc_zero(static_cast<size_t>(k_) * slab_rows_, st);
        centre_.alloc_zero(static_cast<size_t>(ldx_), st);
        norms_l_.alloc_zero(m256, st);
        norms_c_.alloc_zero(slab_rows_, st);
        dev_.Kmm.alloc_zero(static_cast<size_t>(m_) * m_, st);
        dev_.St.alloc_zero(static_cast<size_t>(ntri_) * RG_TILE, st);
        St_.alloc_zero(static_cast<size_t>(ntri_) * RG_TILE, st);
        part_.alloc_zero(static_cast<size_t>(ntri_) * max_chunks_ * RG_TILE, st);
        D_.alloc_zero(static_cast<size_t>(m_) * std::max(ld_, m256), st);
        slab_.alloc_zero(static_cast<size_t>(cols_) * ld_, st);
        if (weighted_) q_.alloc_zero(ld_, st);
        LSSVM_HIP_CHECK(hipMemcpy2DAsync(XL_.p, static_cast<size_t>(ldx_) * sizeof(T), XL, d * sizeof(T), d * sizeof(T), m, hipMemcpyHostToDevice, st));
        LSSVM_HIP_CHECK(hipMemcpyAsync(centre_.p, centre_host_.data(), centre_host_.size() * sizeof(double), hipMemcpyHostToDevice, st));
        const bool rbf = params_.kernel_type == LSSVM_KERNEL_RBF;
        if (rbf) hipLaunchKernelGGL(k_centred_norms<T>, dim3(static_cast<unsigned>(m256 / 256)), dim3(256), 0, st, XL_.p, ldx_, static_cast<size_t>(m_), centre_.p, norms_l_.p);
        // K_mm: the new kernel on the landmarks themselves, the diagonal's distance forced to 0; their Phi takes a buffer of its own for the length of this call
        DevBuf<double> phi_mm;
        phi_mm.alloc_zero(static_cast<size_t>(m_) * m256, st);
        hipLaunchKernelGGL(k_cross_product<T>, dim3(static_cast<unsigned>(m256 / RG_TW), (m_ + RG_TW - 1) / RG_TW), dim3(256), 0, st, XL_.p, XL_.p, ldx_, m_, m_, centre_.p, params_.kernel_type,
                           norms_l_.p, norms_l_.p, 1, D_.p, m256);
        hipLaunchKernelGGL(k_kernel_values, dim3(static_cast<unsigned>(m256 / 256), m_), dim3(256), 0, st, D_.p, m256, m_, 0, params_.kernel_type, params_.degree, gamma_, coef0_, phi_mm.p);
        hipLaunchKernelGGL(k_stream_kmm, dim3((m_ * m_ + 255) / 256), dim3(256), 0, st, phi_mm.p, m256, m_, dev_.Kmm.p);
        LSSVM_HIP_CHECK(hipGetLastError());
        Kmm_host_.resize(static_cast<size_t>(m_) * m_);
        LSSVM_HIP_CHECK(hipMemcpyAsync(Kmm_host_.data(), dev_.Kmm.p, Kmm_host_.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    }

    void update(const void *X, const void *Y, const double *w, size_t n) override {
        check_rows(X, Y, w, n);
        activate();
        hipStream_t st = stream_.s;
        std::vector<double> sq;  // sqrt(w): std::sqrt on the host, correctly rounded, as upload_per_row forms it
        if (weighted_) {
            sq.assign(n, 1.0);
            if (w != nullptr)
                for (size_t i = 0; i < n; ++i) sq[i] = std::sqrt(w[i]);
        }
        lev_.reset();  // (a solve's operands stand for the rows it saw)
        for (size_t off = 0; off < n;) {
            const int np = static_cast<int>(std::min(n - off, slab_rows_ - fill_));
            enqueue_rows(X, Y, n, off, np, D_.p + fill_, slab_.p + fill_);
            if (weighted_) LSSVM_HIP_CHECK(hipMemcpyAsync(q_.p + fill_, sq.data() + off, static_cast<size_t>(np) * sizeof(double), hipMemcpyHostToDevice, st));
            fill_ += static_cast<size_t>(np);
            N_ += static_cast<uint64_t>(np);
            off += static_cast<size_t>(np);
            if (fill_ == slab_rows_) {  // a full slab: into the running St exactly as reduced_gram sums one
                enqueue_gram(slab_.p, ld_, cols_, static_cast<int>(slab_rows_), max_chunks_, part_.p, St_.p, st, q_.p);
                fill_ = 0;
            }
        }
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (the caller's buffers and `sq` are free)
    }

    void solve(const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out, lssvm_reduced_loo_info *infos) override {
        LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
        check_reduced_loo_costs(costs, num_costs);
        check_reduced_factor(factor);
        LSSVM_REQUIRE(N_ > 0, "The stream holds no rows yet: solve needs at least one update!");
        activate();
        hipStream_t st = stream_.s;
        lev_.reset();
        std::vector<double> St;
        double gram_ms = 0.0;
        current_gram(St, &gram_ms);
        const int m = m_, k = k_, cols = cols_;
        const double W = St[static_cast<size_t>(m) * cols + m];  // the Gram kernel's own sum of the weights: N itself on an unweighted stream
        LSSVM_REQUIRE(std::isfinite(W) && W > 0.0, "The weights of the streamed rows must have a finite sum greater than 0.0, but it is " + std::to_string(W) + "!");

        auto a = std::make_unique<LeverageArgs>(m, k, num_costs, true, st);
        const double *s_row = &St[static_cast<size_t>(m) * cols];
        std::vector<double> shift(static_cast<size_t>(m)), ybar(num_costs * k), nus(num_costs), host_ms(num_costs);
        for (int j = 0; j < m; ++j) shift[j] = s_row[j] / W;
        if (factor == 0) {
            std::vector<double> Bt(a->op_stride), L;
            for (size_t s = 0; s < num_costs; ++s) {
                const double t_host = now_ms();
                nus[s] = host_operand(St, Kmm_host_, m, k, cols, W, costs[s], a->ldb, betas_out + s * k * m, rhos_out + s * k, L, Bt, &ybar[s * k]);
                host_ms[s] = now_ms() - t_host;
                a->upload_operand(s, Bt.data());
                LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (Bt is filled again for the next cost)
            }
        } else {
            DenseFit fit(m, k, st);
            for (size_t s = 0; s < num_costs; ++s) {
                const double t_cost = now_ms();
                double device_ms = 0.0;
                nus[s] = fit.run(dev_, St, Kmm_host_, cols, W, 1.0 / costs[s], a->Bt.p + s * a->op_stride, a->ldb, betas_out + s * k * m, rhos_out + s * k, nullptr, &device_ms);
                for (int c = 0; c < k; ++c) ybar[s * k + c] = St[static_cast<size_t>(m + 1 + c) * cols + m] / W;
                host_ms[s] = std::max(0.0, now_ms() - t_cost - device_ms);
            }
        }
        a->upload_shift(shift.data(), ybar.data());
        a->inv_n = 1.0 / W;
        lev_ = std::move(a);
        if (infos != nullptr) {
            for (size_t s = 0; s < num_costs; ++s) {
                infos[s] = lssvm_reduced_loo_info{};
                infos[s].cost = costs[s];
                infos[s].jitter = nus[s];
                infos[s].gram_ms = gram_ms;
                infos[s].host_ms = host_ms[s];
            }
        }
    }

    void loo(const void *X, const void *Y, const double *w, size_t n, double *h_out, double *f_out, double *loo_out) override {
        check_rows(X, Y, w, n);
        LSSVM_REQUIRE(h_out != nullptr && f_out != nullptr && loo_out != nullptr, "leverage_out / fitted_out / loo_out must not be NULL");
        LSSVM_REQUIRE(lev_ != nullptr, "loo needs a solve of the rows streamed so far: none has run, or an update followed it!");
        activate();
        hipStream_t st = stream_.s;
        alloc_scratch();
        const LeverageArgs &a = *lev_;
        const size_t S = a.num_ops;
        std::vector<double> wpad;
        for (size_t off = 0; off < n;) {
            const int np = static_cast<int>(std::min(n - off, slab_rows_));
            const size_t np256 = static_cast<size_t>(round_up(np, 256));
            enqueue_rows(X, Y, n, off, np, D_.p, scratch_.p);
            if (weighted_) {  // the rows' weights, indexed like the slab's rows, zeros behind them
                wpad.assign(np256, 0.0);
                for (int i = 0; i < np; ++i) wpad[i] = w != nullptr ? w[off + i] : 1.0;
                LSSVM_HIP_CHECK(hipMemcpyAsync(w_.p, wpad.data(), np256 * sizeof(double), hipMemcpyHostToDevice, st));
            }
            for (size_t o = 0; o < S; ++o) {
                a.enqueue(o, scratch_.p, ld_, np, h_.p, f_.p, loo_.p, weighted_ ? w_.p : nullptr);
                LSSVM_HIP_CHECK(hipMemcpyAsync(h_out + o * n + off, h_.p, static_cast<size_t>(np) * sizeof(double), hipMemcpyDeviceToHost, st));
                for (int c = 0; c < k_; ++c) {
                    LSSVM_HIP_CHECK(hipMemcpyAsync(f_out + (o * k_ + c) * n + off, f_.p + static_cast<size_t>(c) * ld_, static_cast<size_t>(np) * sizeof(double), hipMemcpyDeviceToHost, st));
                    LSSVM_HIP_CHECK(hipMemcpyAsync(loo_out + (o * k_ + c) * n + off, loo_.p + static_cast<size_t>(c) * ld_, static_cast<size_t>(np) * sizeof(double), hipMemcpyDeviceToHost, st));
                }
            }
            LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (`wpad` is filled again)
            off += static_cast<size_t>(np);
        }
    }

    void phi(const void *X, size_t n, double *phi_out) override {
        LSSVM_REQUIRE(X != nullptr && phi_out != nullptr, "X / phi_out must not be NULL");
        LSSVM_REQUIRE(n >= 1, "A chunk holds at least 1 row!");
        activate();
        hipStream_t st = stream_.s;
        alloc_scratch();
        std::vector<double> colmajor;
        for (size_t off = 0; off < n;) {
            const int np = static_cast<int>(std::min(n - off, slab_rows_));
            enqueue_rows(X, nullptr, n, off, np, D_.p, scratch_.p);
            colmajor.resize(static_cast<size_t>(m_) * np);
            LSSVM_HIP_CHECK(hipMemcpy2DAsync(colmajor.data(), static_cast<size_t>(np) * sizeof(double), scratch_.p, ld_ * sizeof(double), static_cast<size_t>(np) * sizeof(double), m_,
                                             hipMemcpyDeviceToHost, st));
            LSSVM_HIP_CHECK(hipStreamSynchronize(st));
            for (int l = 0; l < m_; ++l)
                for (int i = 0; i < np; ++i) phi_out[(off + i) * m_ + l] = colmajor[static_cast<size_t>(l) * np + i];
            off += static_cast<size_t>(np);
        }
    }

    void export_state(double *gram_out, double *kmm_out, uint64_t *num_points_out, uint64_t *fingerprint_out) override {
        LSSVM_REQUIRE(gram_out != nullptr && kmm_out != nullptr && num_points_out != nullptr && fingerprint_out != nullptr,
                      "gram_out / kmm_out / num_points_out / fingerprint_out must not be NULL");
        activate();
        std::vector<double> St;
        current_gram(St, nullptr);
        std::copy(St.begin(), St.end(), gram_out);
        std::copy(Kmm_host_.begin(), Kmm_host_.end(), kmm_out);
        *num_points_out = N_;
        fingerprint(fingerprint_out);
    }

    void merge_state(const double *gram, uint64_t num_points, const uint64_t *fp) override {
        LSSVM_REQUIRE(gram != nullptr && fp != nullptr, "gram / fingerprint must not be NULL");
        uint64_t own[LSSVM_REDUCED_STREAM_FINGERPRINT_WORDS];
        fingerprint(own);
        LSSVM_REQUIRE(std::equal(own, own + LSSVM_REDUCED_STREAM_FINGERPRINT_WORDS, fp),
                      "The state was exported by a stream of other kernel parameters, landmarks, shapes or dtype: its fingerprint differs!");
        activate();
        hipStream_t st = stream_.s;
        lev_.reset();
        // entrywise into the FLUSHED St, one rounding per entry; the pending rows stay pending and are summed behind the merged part
        std::vector<double> tiles(static_cast<size_t>(ntri_) * RG_TILE);
        LSSVM_HIP_CHECK(hipMemcpyAsync(tiles.data(), St_.p, tiles.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));
        const int nt = tiles_of(cols_);
        for (int bj = 0; bj < nt; ++bj)
            for (int bk = 0; bk <= bj; ++bk) {
                double *t = &tiles[static_cast<size_t>(bj * (bj + 1) / 2 + bk) * RG_TILE];
                for (int a = 0; a < RG_TW && bj * RG_TW + a < cols_; ++a)
                    for (int b = 0; b < RG_TW && bk * RG_TW + b < cols_; ++b) t[a * RG_TW + b] += gram[static_cast<size_t>(bj * RG_TW + a) * cols_ + bk * RG_TW + b];
            }
        LSSVM_HIP_CHECK(hipMemcpyAsync(St_.p, tiles.data(), tiles.size() * sizeof(double), hipMemcpyHostToDevice, st));
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));
        N_ += num_points;
    }

    void info(lssvm_reduced_stream_info *out, double *centre_out, double *kmm_out) const override {
        if (out != nullptr) {
            *out = lssvm_reduced_stream_info{};
            out->num_points = N_;
            out->pending = static_cast<uint64_t>(fill_);
            out->rank = static_cast<uint64_t>(m_);
            out->num_features = static_cast<uint64_t>(d_);
            out->num_rhs = static_cast<uint64_t>(k_);
            out->slab_rows = static_cast<uint64_t>(slab_rows_);
            out->weighted = weighted_ ? 1 : 0;
            out->dtype = std::is_same_v<T, float> ? LSSVM_DTYPE_F32 : LSSVM_DTYPE_F64;
            out->workspace_bytes = (centre_.count + norms_l_.count + norms_c_.count + dev_.Kmm.count + dev_.St.count + St_.count + part_.count + D_.count + slab_.count + q_.count + scratch_.count +
                                    w_.count + h_.count + f_.count + loo_.count) * sizeof(double) + (XL_.count + Xc_.count + Yc_.count) * sizeof(T);
        }
        if (centre_out != nullptr) std::copy(centre_host_.begin(), centre_host_.begin() + d_, centre_out);
        if (kmm_out != nullptr) std::copy(Kmm_host_.begin(), Kmm_host_.end(), kmm_out);
    }

    void time_kernels(const void *X, size_t n, int repeats, double *cross_ms_out, double *landmark_ms_out) override {
        LSSVM_REQUIRE(X != nullptr && cross_ms_out != nullptr && landmark_ms_out != nullptr, "X / cross_ms_out / landmark_ms_out must not be NULL");
        LSSVM_REQUIRE(n >= 1 && n <= slab_rows_ && repeats >= 1, "The timed chunk holds between 1 and slab_rows rows, and repeats is at least 1!");
        activate();
        hipStream_t st = stream_.s;
        const int np = static_cast<int>(n), rows128 = round_up(np, RG_TW);
        const bool rbf = params_.kernel_type == LSSVM_KERNEL_RBF;
        const dim3 grid(static_cast<unsigned>(rows128 / RG_TW), (m_ + RG_TW - 1) / RG_TW);
        LSSVM_HIP_CHECK(hipMemcpy2DAsync(Xc_.p, static_cast<size_t>(ldx_) * sizeof(T), X, static_cast<size_t>(d_) * sizeof(T), static_cast<size_t>(d_) * sizeof(T), n, hipMemcpyHostToDevice, st));
        if (rbf) hipLaunchKernelGGL(k_centred_norms<T>, dim3(static_cast<unsigned>(round_up(np, 256) / 256)), dim3(256), 0, st, Xc_.p, ldx_, n, centre_.p, norms_c_.p);
        timed_repeats(st, repeats, cross_ms_out, [] {}, [&] {
            hipLaunchKernelGGL(k_cross_product<T>, grid, dim3(256), 0, st, XL_.p, Xc_.p, ldx_, np, m_, centre_.p, params_.kernel_type, norms_l_.p, norms_c_.p, 0, D_.p, ld_);
        });
        // the sibling at the same shape: the chunk's rows and, behind them, the landmark rows as ONE resident set, the landmarks by index
        DevBuf<T> both;
        DevBuf<double> norms;
        DevBuf<int> lm;
        const size_t total = n + static_cast<size_t>(m_);
        both.alloc_zero(total * ldx_, st);
        norms.alloc_zero(total, st);
        lm.alloc_zero(static_cast<size_t>(m_), st);
        std::vector<int> lm_host(static_cast<size_t>(m_));
        for (int l = 0; l < m_; ++l) lm_host[l] = np + l;
        LSSVM_HIP_CHECK(hipMemcpyAsync(both.p, Xc_.p, n * ldx_ * sizeof(T), hipMemcpyDeviceToDevice, st));
        LSSVM_HIP_CHECK(hipMemcpyAsync(both.p + n * ldx_, XL_.p, static_cast<size_t>(m_) * ldx_ * sizeof(T), hipMemcpyDeviceToDevice, st));
        LSSVM_HIP_CHECK(hipMemcpyAsync(lm.p, lm_host.data(), lm_host.size() * sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_row_norms<T>, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st, both.p, ldx_, total, norms.p);
        timed_repeats(st, repeats, landmark_ms_out, [] {}, [&] {
            hipLaunchKernelGGL(k_landmark_product<T>, grid, dim3(256), 0, st, both.p, ldx_, np, 0, lm.p, m_, params_.kernel_type, norms.p, D_.p, ld_);
        });
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    }

  private:
    void activate() const { LSSVM_HIP_CHECK(hipSetDevice(0)); }

    /* what update and loo refuse before a device is touched */
    void check_rows(const void *X, const void *Y, const double *w, size_t n) const {
        LSSVM_REQUIRE(X != nullptr, "X must not be NULL");
        LSSVM_REQUIRE(Y != nullptr, "The right hand side vector must not be empty!");
        LSSVM_REQUIRE(n >= 1, "A chunk holds at least 1 row!");
        LSSVM_REQUIRE(w == nullptr || weighted_, "The stream was created without weights: a chunk of it takes none!");
        if (w != nullptr)
            for (size_t i = 0; i < n; ++i)
                LSSVM_REQUIRE(std::isfinite(w[i]) && w[i] >= 0.0,
                              "Every weight of the reduced model must be finite and not less than 0.0, but weight " + std::to_string(i) + " is " + std::to_string(w[i]) + "!");
    }

    void fingerprint(uint64_t *out) const {
        out[0] = static_cast<uint64_t>(params_.kernel_type);
        out[1] = static_cast<uint64_t>(static_cast<int64_t>(params_.degree));
        out[2] = bits_of(params_.gamma);
        out[3] = bits_of(params_.coef0);
        out[4] = static_cast<uint64_t>(m_);
        out[5] = static_cast<uint64_t>(d_);
        out[6] = static_cast<uint64_t>(k_);
        out[7] = std::is_same_v<T, float> ? LSSVM_DTYPE_F32 : LSSVM_DTYPE_F64;
        out[8] = hash_;
    }

    void alloc_scratch() {
        if (scratch_.p != nullptr) return;
        hipStream_t st = stream_.s;
        scratch_.alloc_zero(static_cast<size_t>(cols_) * ld_, st);
        h_.alloc_zero(ld_, st);
        f_.alloc_zero(static_cast<size_t>(k_) * ld_, st);
        loo_.alloc_zero(static_cast<size_t>(k_) * ld_, st);
        if (weighted_) w_.alloc_zero(ld_, st);
    }

    /* the rows off ... off + np - 1 of a chunk of n rows (np <= slab_rows): upload, pad, and [Phi | 1 | Y] of them from `rows_at` on (a slab's first column plus a row
     * offset; ld_ doubles between two columns), D through `D_at` at the same offset.  Y NULL: Phi alone.  Zeros are written behind the rows up to the next multiple of 256
     * (the slack every slab keeps). */
    void enqueue_rows(const void *X, const void *Y, size_t n, size_t off, int np, double *D_at, double *rows_at) {
        hipStream_t st = stream_.s;
        const T *Xh = static_cast<const T *>(X) + off * d_;
        const unsigned b256 = static_cast<unsigned>(round_up(np, 256) / 256);
        LSSVM_HIP_CHECK(hipMemcpy2DAsync(Xc_.p, static_cast<size_t>(ldx_) * sizeof(T), Xh, static_cast<size_t>(d_) * sizeof(T), static_cast<size_t>(d_) * sizeof(T), static_cast<size_t>(np),
                                         hipMemcpyHostToDevice, st));
        if (params_.kernel_type == LSSVM_KERNEL_RBF) hipLaunchKernelGGL(k_centred_norms<T>, dim3(b256), dim3(256), 0, st, Xc_.p, ldx_, static_cast<size_t>(np), centre_.p, norms_c_.p);
        hipLaunchKernelGGL(k_cross_product<T>, dim3(static_cast<unsigned>(round_up(np, RG_TW) / RG_TW), (m_ + RG_TW - 1) / RG_TW), dim3(256), 0, st, XL_.p, Xc_.p, ldx_, np, m_, centre_.p,
                           params_.kernel_type, norms_l_.p, norms_c_.p, 0, D_at, ld_);
        hipLaunchKernelGGL(k_kernel_values, dim3(b256, m_), dim3(256), 0, st, D_at, ld_, np, 0, params_.kernel_type, params_.degree, gamma_, coef0_, rows_at);
        if (Y != nullptr) {
            const T *Yh = static_cast<const T *>(Y) + off;
            LSSVM_HIP_CHECK(hipMemcpy2DAsync(Yc_.p, slab_rows_ * sizeof(T), Yh, n * sizeof(T), static_cast<size_t>(np) * sizeof(T), static_cast<size_t>(k_), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_stream_aux<T>, dim3(b256, 1 + k_), dim3(256), 0, st, Yc_.p, slab_rows_, np, rows_at + static_cast<size_t>(m_) * ld_, ld_);
        }
        LSSVM_HIP_CHECK(hipGetLastError());
    }

    /* S~ of every row streamed so far, cols x cols row major with both triangles: the pending rows, zero-padded to a multiple of 256, summed into a COPY of St */
    void current_gram(std::vector<double> &gram, double *gram_ms) {
        hipStream_t st = stream_.s;
        LSSVM_HIP_CHECK(hipMemcpyAsync(dev_.St.p, St_.p, St_.count * sizeof(double), hipMemcpyDeviceToDevice, st));
        const double t0 = now_ms();
        if (fill_ > 0) {
            const size_t r256 = static_cast<size_t>(round_up(static_cast<long>(fill_), 256));
            if (r256 > fill_) {  // what an earlier slab left behind the pending rows
                LSSVM_HIP_CHECK(hipMemset2DAsync(slab_.p + fill_, ld_ * sizeof(double), 0, (r256 - fill_) * sizeof(double), static_cast<size_t>(cols_), st));
                if (weighted_) LSSVM_HIP_CHECK(hipMemsetAsync(q_.p + fill_, 0, (r256 - fill_) * sizeof(double), st));
            }
            enqueue_gram(slab_.p, ld_, cols_, static_cast<int>(r256), max_chunks_, part_.p, dev_.St.p, st, q_.p);
        }
        std::vector<double> tiles(static_cast<size_t>(ntri_) * RG_TILE);
        LSSVM_HIP_CHECK(hipMemcpyAsync(tiles.data(), dev_.St.p, tiles.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));
        if (gram_ms != nullptr) *gram_ms = now_ms() - t0;
        unpack_tiles(tiles, cols_, gram);
    }

    const lssvm_params params_;
    const int m_, d_, k_, cols_, ldx_;
    const bool weighted_;
    const size_t slab_rows_, ld_;  // ld_: doubles between two columns of a slab, slab_rows_ and the slack of the kernels' row tiles
    const int ntri_, max_chunks_;
    const uint64_t hash_;
    double gamma_ = 0.0, coef0_ = 0.0;
    std::vector<double> centre_host_, Kmm_host_;
    Stream stream_;
    DevBuf<T> XL_, Xc_, Yc_;
    DevBuf<double> centre_, norms_l_, norms_c_, St_, part_, D_, slab_, q_, scratch_, w_, h_, f_, loo_;
    ReducedOnDevice dev_;  // K_mm, and the copy of St a solve works on
    size_t fill_ = 0;
    uint64_t N_ = 0;
    std::unique_ptr<LeverageArgs> lev_;  // the operands of the last solve, until the next update, solve or merge
};

}  // namespace

void check_reduced_stream_arguments(const lssvm_params *params, const void *landmark_rows, size_t rank, size_t num_features, size_t num_rhs, uint64_t slab_rows) {
    LSSVM_REQUIRE(params != nullptr, "params must not be NULL!");
    LSSVM_REQUIRE(params->kernel_type == LSSVM_KERNEL_LINEAR || params->kernel_type == LSSVM_KERNEL_POLYNOMIAL || params->kernel_type == LSSVM_KERNEL_RBF,
                  "Invalid kernel function " + std::to_string(params->kernel_type) + " given!");
    if (params->kernel_type != LSSVM_KERNEL_LINEAR)
        LSSVM_REQUIRE(std::isfinite(params->gamma) && params->gamma > 0.0, "gamma must be finite and greater than 0, but is " + std::to_string(params->gamma) + "!");
    LSSVM_REQUIRE(landmark_rows != nullptr, "The landmark rows must not be NULL!");
    LSSVM_REQUIRE(num_features >= 1, "The landmark rows must have at least one feature!");
    LSSVM_REQUIRE(num_rhs > 0, "The number of right hand sides must be greater than 0!");
    LSSVM_REQUIRE(num_rhs <= 4096, "at most 4096 right hand sides per stream");
    LSSVM_REQUIRE(rank >= 1 && rank <= static_cast<size_t>(REDUCED_MAX_RANK), "The rank of the reduced model must lie in [1, " + std::to_string(REDUCED_MAX_RANK) + "], but is " + std::to_string(rank) + "!");
    LSSVM_REQUIRE(slab_rows % 256 == 0 && slab_rows <= STREAM_MAX_SLAB_ROWS,
                  "slab_rows must be a multiple of 256 up to " + std::to_string(STREAM_MAX_SLAB_ROWS) + " (0: the library's default), but is " + std::to_string(slab_rows) + "!");
}

std::unique_ptr<ReducedStreamBase> make_reduced_stream(const lssvm_params &params, int dtype, const void *landmark_rows, size_t rank, size_t num_features, size_t num_rhs, bool weighted,
                                                       uint64_t slab_rows) {
    if (dtype == LSSVM_DTYPE_F32) return std::make_unique<ReducedStream<float>>(params, landmark_rows, rank, num_features, num_rhs, weighted, slab_rows);
    return std::make_unique<ReducedStream<double>>(params, landmark_rows, rank, num_features, num_rhs, weighted, slab_rows);
}

}  // namespace lssvm
