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
 */
#include "lssvm_landmark.hip.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace lssvm {

namespace {

constexpr int RG_TW = 128;                 // columns of Pt per operand of a tile
constexpr int RG_KC = 16;                  // rows of Pt per step
constexpr int RG_LS = RG_KC + 2;           // doubles between two columns in LDS: 144 bytes, conflict-free ds_read_b64 (as the fp64 tile kernels)
constexpr int RG_RANGE = 2048;             // rows of a slab per workgroup: a CONSTANT (see above)
constexpr int RG_TILE = RG_TW * RG_TW;     // entries of a tile

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

/* Kmm[k][l] = Phi[lm[k]][l] for the landmarks that lie in this slab's rows */
__global__ void k_reduced_gather_kmm(const double *__restrict__ slab, size_t ld, int row0, int rows, const int *__restrict__ lm, int m, double *__restrict__ Kmm) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * m) return;
    const int r = lm[e / m] - row0;
    if (r >= 0 && r < rows) Kmm[e] = slab[static_cast<size_t>(e % m) * ld + r];
}

/* part[tile][chunk] = A^T B over the rows [chunk RG_RANGE, min((chunk + 1) RG_RANGE, rows)) of the slab, A = the columns 128 bj ... and B = the columns 128 bk ... of the
 * column-major `slab` (ld doubles between two columns; columns from `cols` on count as zeros and are never read; `rows` is a multiple of RG_KC), for tile = (bj, bk),
 * bk <= bj.  Both operands go through LDS: eight threads load the 16 rows of a column of a step as one 128-byte line, the fragments are read as in tile_matvec_f64
 * (lane 16 q + r: column r of the block, row q of the k-step).  A diagonal tile stages and reads ONE operand.  The result of a lane: column r of B, rows q + 4 i of A.
 * Two waves per SIMD (at most 256 registers): the other workgroup of the CU computes while this one waits at its barriers. */
__global__ __launch_bounds__(256, 2) void k_reduced_gram(const double *__restrict__ slab, size_t ld, int cols, int rows, int max_chunks, double *__restrict__ part) {
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
    const f64x2 zero2 = { 0.0, 0.0 };
    auto stage_load = [&](int s) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            sa[p] = a_in[p] ? *reinterpret_cast<const f64x2 *>(Ag[p] + s * RG_KC) : zero2;
            sb[p] = b_in[p] ? *reinterpret_cast<const f64x2 *>(Bg[p] + s * RG_KC) : zero2;
        }
    };
    auto stage_store = [&]() {
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

int tiles_of(int cols) { return (cols + RG_TW - 1) / RG_TW; }

/* St of one slab into the running sum: `rows` (a multiple of 256) rows of the column-major slab */
void enqueue_gram(const double *slab, size_t ld, int cols, int rows, int max_chunks, double *part, double *St, hipStream_t st) {
    const int nt = tiles_of(cols), ntri = nt * (nt + 1) / 2, chunks = (rows + RG_RANGE - 1) / RG_RANGE;
    hipLaunchKernelGGL(k_reduced_gram, dim3(ntri, chunks), dim3(256), 0, st, slab, ld, cols, rows, max_chunks, part);
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

float elapsed_ms(const Event &a, const Event &b) {
    float ms = 0.0f;
    LSSVM_HIP_CHECK(hipEventElapsedTime(&ms, a.e, b.e));
    return ms;
}

}  // namespace

void check_reduced_arguments(const void *Y, size_t num_rhs, uint64_t rank, uint64_t slab_rows, size_t num_points) {
    LSSVM_REQUIRE(Y != nullptr, "The right hand side vector must not be empty!");
    LSSVM_REQUIRE(num_rhs > 0, "The number of right hand sides must be greater than 0!");
    const uint64_t most = num_points > 0 ? std::min<uint64_t>(num_points, REDUCED_MAX_RANK) : REDUCED_MAX_RANK;
    LSSVM_REQUIRE(rank >= 1 && rank <= most, "The rank of the reduced model must lie in [1, " + std::to_string(most) + "], but is " + std::to_string(rank) + "!");
    LSSVM_REQUIRE(slab_rows % 256 == 0, "slab_rows must be a multiple of 256 (0: the library's default), but is " + std::to_string(slab_rows) + "!");
}

template <typename T>
void Solver<T>::reduced_gram(const char *what, const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, std::vector<uint64_t> &lm,
                             std::vector<double> &gram, std::vector<double> &Kmm, lssvm_reduced_info &info) {
    // ---- everything that needs no device ----
    LSSVM_REQUIRE(shards_.size() == 1 && world_ == 1 && exchange_ == Exchange::none, std::string("the reduced model (") + what + ") is fitted on a problem of one device and one rank");
    Problem<T> &p = *shards_[0];
    LSSVM_REQUIRE(!p.weighted_, std::string("the reduced model (") + what + ") is fitted to the unweighted objective: the problem has weights set (lssvm_mi355_problem_set_weights(p, NULL, 0) removes them)");
    LSSVM_REQUIRE(!in_cg_, std::string(what) + " cannot run between cg_begin and cg_finish");
    const size_t N = p.N_;
    check_reduced_arguments(Y, num_rhs, rank, slab_rows, N);
    LSSVM_REQUIRE(num_rhs <= 4096, "at most 4096 right hand sides per call");
    const int m = static_cast<int>(rank), k = static_cast<int>(num_rhs), cols = m + 1 + k;
    lm = resolve_landmarks(landmarks, static_cast<size_t>(m), N);

    const double t0 = now_ms();
    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    const size_t N256 = static_cast<size_t>(round_up(static_cast<long>(N), 256));
    const size_t ld = std::min<size_t>(slab_rows == 0 ? REDUCED_DEFAULT_SLAB_ROWS : slab_rows, N256);  // rows of a slab = doubles between two columns
    const int slabs = static_cast<int>((N + ld - 1) / ld);
    const int nt = tiles_of(cols), ntri = nt * (nt + 1) / 2;
    const int max_chunks = static_cast<int>((ld + RG_RANGE - 1) / RG_RANGE);

    std::vector<int> lm_host(lm.begin(), lm.end());
    DevBuf<int> lm_dev;
    DevBuf<T> Y_dev;
    DevBuf<double> slab, part, St_dev, Kmm_dev;
    lm_dev.alloc_zero(static_cast<size_t>(m), st);
    LSSVM_HIP_CHECK(hipMemcpyAsync(lm_dev.p, lm_host.data(), static_cast<size_t>(m) * sizeof(int), hipMemcpyHostToDevice, st));
    Y_dev.alloc_zero(static_cast<size_t>(k) * N, st);
    LSSVM_HIP_CHECK(hipMemcpyAsync(Y_dev.p, Y, static_cast<size_t>(k) * N * sizeof(T), hipMemcpyHostToDevice, st));
    slab.alloc_zero(static_cast<size_t>(cols) * ld, st);
    part.alloc_zero(static_cast<size_t>(ntri) * max_chunks * RG_TILE, st);
    St_dev.alloc_zero(static_cast<size_t>(ntri) * RG_TILE, st);
    Kmm_dev.alloc_zero(static_cast<size_t>(m) * m, st);

    // the kernel function on the data as X_ holds it (build_preconditioner): x' = x_scale (x - mean) leaves rbf distances and inner products scaled by x_scale^2
    const lssvm_params &prm = p.params_;
    const double scale2 = p.x_scale_ * p.x_scale_;
    const double gamma = prm.kernel_type == LSSVM_KERNEL_LINEAR ? 1.0 / scale2 : static_cast<double>(static_cast<T>(prm.gamma)) / scale2;
    Event ev[3];
    for (Event &e : ev) e.create(true);
    double landmark_ms = 0.0, gram_ms = 0.0;
    for (int s = 0; s < slabs; ++s) {
        const size_t row0 = static_cast<size_t>(s) * ld;
        const int rows = static_cast<int>(std::min(ld, N - row0)), rows256 = round_up(rows, 256);  // (rows256 <= ld: ld is a multiple of 256)
        LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
        hipLaunchKernelGGL(k_landmark_block<T>, dim3(rows256 / 256, (m + 15) / 16), dim3(256), 0, st, p.X_.data.p, p.X_.ldx, static_cast<int>(N), static_cast<int>(row0), lm_dev.p, m,
                           prm.kernel_type, prm.degree, gamma, static_cast<double>(static_cast<T>(prm.coef0)), slab.p, ld);
        hipLaunchKernelGGL(k_reduced_aux<T>, dim3(rows256 / 256, 1 + k), dim3(256), 0, st, Y_dev.p, N, row0, slab.p + static_cast<size_t>(m) * ld, ld);
        hipLaunchKernelGGL(k_reduced_gather_kmm, dim3((m * m + 255) / 256), dim3(256), 0, st, slab.p, ld, static_cast<int>(row0), rows, lm_dev.p, m, Kmm_dev.p);
        LSSVM_HIP_CHECK(hipGetLastError());
        LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
        enqueue_gram(slab.p, ld, cols, rows256, max_chunks, part.p, St_dev.p, st);
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
    info.slabs = static_cast<uint64_t>(slabs);
    info.landmark_ms = landmark_ms;
    info.gram_ms = gram_ms;
    info.total_ms = now_ms() - t0;
    info.workspace_bytes = (slab.count + part.count + St_dev.count + Kmm_dev.count) * sizeof(double) + Y_dev.count * sizeof(T) + lm_dev.count * sizeof(int);
}

template <typename T>
void Solver<T>::landmark_gram(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *gram_out) {
    LSSVM_REQUIRE(gram_out != nullptr, "gram_out must not be NULL");
    std::vector<uint64_t> lm;
    std::vector<double> gram, Kmm;
    lssvm_reduced_info info{};
    reduced_gram("landmark_gram", Y, num_rhs, rank, landmarks, slab_rows, lm, gram, Kmm, info);
    std::copy(gram.begin(), gram.end(), gram_out);
}

template <typename T>
void Solver<T>::fit_reduced(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                            lssvm_reduced_info *info_out) {
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    const double t0 = now_ms();
    std::vector<uint64_t> lm;
    std::vector<double> St, Kmm;
    lssvm_reduced_info info{};
    reduced_gram("fit_reduced", Y, num_rhs, rank, landmarks, slab_rows, lm, St, Kmm, info);

    // ---- the host's part, in double: M = S - s s^T / N + sigma K_mm (lower triangle), (M + nu I) beta_c = t_c - s eta_c / N, b_c = (eta_c - s^T beta_c) / N ----
    const double t_host = now_ms();
    const int m = static_cast<int>(rank), k = static_cast<int>(num_rhs), cols = m + 1 + k;
    const double Nd = static_cast<double>(shards_[0]->N_), sigma = 1.0 / shards_[0]->params_.cost;  // (in double, whatever the real type: the host's part is the formulation's)
    const double *s = &St[static_cast<size_t>(m) * cols];
    std::vector<double> M(static_cast<size_t>(m) * m, 0.0);
    double trace = 0.0;
    for (int j = 0; j < m; ++j) {
        for (int l = 0; l <= j; ++l) M[static_cast<size_t>(j) * m + l] = St[static_cast<size_t>(j) * cols + l] - s[j] * s[l] / Nd + sigma * Kmm[static_cast<size_t>(j) * m + l];
        trace += M[static_cast<size_t>(j) * m + j];
    }
    LSSVM_REQUIRE(std::isfinite(trace) && trace > 0.0, "the matrix of the reduced model has no positive finite trace");
    double nu = DBL_EPSILON * trace;
    std::vector<double> L;
    bool factored = false;
    for (int attempt = 0; attempt < 7 && !factored; ++attempt, nu *= factored ? 1.0 : 10.0) {
        L = M;
        for (int j = 0; j < m; ++j) L[static_cast<size_t>(j) * m + j] += nu;
        factored = cholesky_lower(L, m);
    }
    if (!factored) throw Error(LSSVM_ERR_INTERNAL, "the matrix of the reduced model could not be factored (jitter up to " + std::to_string(nu / 10.0) + ")");
    std::vector<double> z(static_cast<size_t>(m));
    for (int c = 0; c < k; ++c) {
        const double *t = &St[static_cast<size_t>(m + 1 + c) * cols];
        const double eta = t[m];
        for (int j = 0; j < m; ++j) {  // L z = t_c - s eta_c / N
            double v = t[j] - s[j] * eta / Nd;
            for (int l = 0; l < j; ++l) v -= L[static_cast<size_t>(j) * m + l] * z[l];
            z[j] = v / L[static_cast<size_t>(j) * m + j];
        }
        double *beta = betas_out + static_cast<size_t>(c) * m;
        for (int j = m - 1; j >= 0; --j) {  // L^T beta = z
            double v = z[j];
            for (int l = j + 1; l < m; ++l) v -= L[static_cast<size_t>(l) * m + j] * beta[l];
            beta[j] = v / L[static_cast<size_t>(j) * m + j];
        }
        double sb = 0.0;
        for (int j = 0; j < m; ++j) sb += s[j] * beta[j];
        rhos_out[c] = -((eta - sb) / Nd);
    }
    if (landmarks_out != nullptr) std::copy(lm.begin(), lm.end(), landmarks_out);
    if (info_out != nullptr) {
        info.jitter = nu;
        info.host_ms = now_ms() - t_host;
        info.total_ms = now_ms() - t0;
        *info_out = info;
    }
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
        Event ev[2];
        for (Event &e : ev) e.create(true);
        for (int rep = -1; rep < repeats; ++rep) {  // (-1: the untimed run)
            LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
            hipLaunchKernelGGL(k_precond_gram<T>, dim3(tiles16, tiles16), dim3(256), 0, st, pc.Bhat.p, pc.ldn, cols, G_dev.p, ldg);
            LSSVM_HIP_CHECK(hipGetLastError());
            LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
            LSSVM_HIP_CHECK(hipEventSynchronize(ev[1].e));
            if (rep >= 0) parent_ms_out[rep] = elapsed_ms(ev[0], ev[1]);
        }
        for (int rep = -1; rep < repeats; ++rep) {
            LSSVM_HIP_CHECK(hipMemsetAsync(St_dev.p, 0, St_dev.count * sizeof(double), st));
            LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
            enqueue_gram(pc.Bhat.p, pc.ldn, cols, rows, max_chunks, part.p, St_dev.p, st);
            LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
            LSSVM_HIP_CHECK(hipEventSynchronize(ev[1].e));
            if (rep >= 0) mfma_ms_out[rep] = elapsed_ms(ev[0], ev[1]);
        }
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

template void Solver<float>::reduced_gram(const char *, const void *, size_t, uint64_t, const uint64_t *, uint64_t, std::vector<uint64_t> &, std::vector<double> &, std::vector<double> &,
                                          lssvm_reduced_info &);
template void Solver<double>::reduced_gram(const char *, const void *, size_t, uint64_t, const uint64_t *, uint64_t, std::vector<uint64_t> &, std::vector<double> &, std::vector<double> &,
                                           lssvm_reduced_info &);
template void Solver<float>::landmark_gram(const void *, size_t, uint64_t, const uint64_t *, uint64_t, double *);
template void Solver<double>::landmark_gram(const void *, size_t, uint64_t, const uint64_t *, uint64_t, double *);
template void Solver<float>::fit_reduced(const void *, size_t, uint64_t, const uint64_t *, uint64_t, double *, double *, uint64_t *, lssvm_reduced_info *);
template void Solver<double>::fit_reduced(const void *, size_t, uint64_t, const uint64_t *, uint64_t, double *, double *, uint64_t *, lssvm_reduced_info *);
template void Solver<float>::time_gram_kernels(int, double *, double *, double *);
template void Solver<double>::time_gram_kernels(int, double *, double *, double *);

}  // namespace lssvm
