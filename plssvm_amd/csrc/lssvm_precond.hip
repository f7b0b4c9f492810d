/*
 * lssvm_precond.hip -- the Nystrom preconditioner of a resident problem and the reference recipe's CG preconditioned with it (lssvm_mi355_problem_build_preconditioner,
 * _precond_landmarks, _precond_apply, _solve_pcg, lssvm_mi355_solve_pcg_*).
 *
 * With n = N - 1, sigma = 1 / C, E = [I_n | -1] and H = K + sigma I the reduced matrix is Abar = E H E^T.  From m landmarks: L L^T = K_mm + nu I (host, double),
 * B_f = K_Nm L^-T, Bhat = [E B_f | sqrt(sigma) 1] (n x (m + 1), in the problem's real type) and P = E (B_f B_f^T + sigma I) E^T = Bhat Bhat^T + sigma I, because
 * sigma E E^T = sigma (I + 1 1^T).  With G = Bhat^T Bhat + sigma I (double, inverted on the host) P^-1 r = (r - Bhat G^-1 Bhat^T r) / sigma; the factor is dropped.
 *
 * The build reads the problem's resident X_ (rescaled in place by the constructor: Problem::x_scale_) -- the data is not uploaded again.  The apply is three kernels:
 * (a) Bhat^T r as RED_BLOCKS x (m + 1) double partial sums, (b) their sums and s = G^-1 t (as one share per 32 columns), (c) z = r - Bhat s with the partial sums of r.z.  Bhat is stored column by
 * column, so (a) and (c) each read it exactly once, 16 bytes per lane along a column.  Every reduction has a fixed order: the same bits for the same arguments.
 *
 * PCG keeps the frame of cg_begin / cg_step: x0 = 1, r0 = b - Abar 1, the stop test |r|^2 <= eps^2 |r0|^2 on the unpreconditioned recurrence residual, the true residual
 * every 50th iteration.  Ad, alpha, x and r are the recipe's own steps (CgSteps::advance and ::residual, which launch the recipe's kernels: alpha's numerator r.z stands in the
 * scalar set advance is handed); only the direction update is launched here.  The Gram pass (Problem::enqueue_apply_K_local) is launched, not changed.  Compiled for gfx950 only.
 */
#include "lssvm_landmark.hip.hpp"

#include "lssvm_kernels.hip.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <numeric>

namespace lssvm {

namespace {

constexpr int PC_THREADS = 1024;                              // the apply kernels: sixteen waves, wave w takes the columns w, w + 16, ...
constexpr int PC_WAVES = PC_THREADS / 64;
constexpr int PC_MAX_COLS = PRECOND_MAX_RANK + 1;
constexpr int PC_COLS_PER_WAVE = (PC_MAX_COLS + PC_WAVES - 1) / PC_WAVES;  // 33 accumulators at most
constexpr int PC_COLS_PER_ROUND = (PC_COLS_PER_WAVE + 1) / 2;              // (a) takes them in two rounds of 17
constexpr int PC_SOLVE_COLS = 32;                             // columns of Bhat per block of k_precond_solve

/* ---------------------------------------------------------------- the build ---------------------------------------------------------------- */

/* (K_Nm itself and K_mm out of it: LandmarkBlock, lssvm_landmark.hip.hpp) */

/* Bf[k][i] = sum over l <= k of Kd[l][i] Linv[k][l]: column k of K_Nm L^-T (Linv = L^-1, lower triangular, row major), l ascending */
__global__ __launch_bounds__(256) void k_nystrom_factor(const double *__restrict__ Kd, size_t ldN, const double *__restrict__ Linv, int m, double *__restrict__ Bf) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    const int k = blockIdx.y;
    double acc = 0.0;
    for (int l = 0; l <= k; ++l) acc += Kd[static_cast<size_t>(l) * ldN + i] * Linv[static_cast<size_t>(k) * m + l];
    Bf[static_cast<size_t>(k) * ldN + i] = acc;
}

/* Bhat[k][i] = Bf[k][i] - Bf[k][n] for the landmark columns, sqrt(sigma) for column m; exact zeros from row n on */
template <typename T>
__global__ __launch_bounds__(256) void k_make_bhat(const double *__restrict__ Bf, size_t ldN, int n, int m, double sqrt_sigma, T *__restrict__ Bhat, size_t ldn) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    const int k = blockIdx.y;
    double v = 0.0;
    if (i < static_cast<size_t>(n)) v = k < m ? Bf[static_cast<size_t>(k) * ldN + i] - Bf[static_cast<size_t>(k) * ldN + n] : sqrt_sigma;
    Bhat[static_cast<size_t>(k) * ldn + i] = static_cast<T>(v);
}

/* (G = Bhat^T Bhat: k_precond_gram, lssvm_landmark.hip.hpp) */

/* ---------------------------------------------------------------- the apply ---------------------------------------------------------------- */

/* (a) tpart[block][j] = this block's share of sum_i Bhat[j][i] r_i.  A block walks row chunks of 64 lanes x 16 bytes; wave w owns the columns w, w + 16, ...: a lane
 * keeps its 16 bytes of r in registers and adds 16 bytes of every owned column into that column's double accumulator (r, n reals, is read once per round). */
template <typename T>
__global__ __launch_bounds__(PC_THREADS) void k_precond_Btr(const T *__restrict__ Bhat, size_t ldn, int cols, const T *__restrict__ r, double *__restrict__ tpart) {
    using Vec = typename PcVec<T>::type;
    constexpr int V = PcVec<T>::n, R = 64 * V;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nchunks = static_cast<int>(ldn / R);
    // (two rounds of at most 17 owned columns: all 33 accumulators beside their loads in flight do not fit the 128 registers of a sixteen-wave block)
#pragma unroll 1
    for (int k0 = 0; k0 < PC_COLS_PER_WAVE; k0 += PC_COLS_PER_ROUND) {
        if (wave + PC_WAVES * k0 >= cols) break;  // (the same for every lane of the wave)
        double acc[PC_COLS_PER_ROUND];
#pragma unroll
        for (int k = 0; k < PC_COLS_PER_ROUND; ++k) acc[k] = 0.0;
        for (int chunk = blockIdx.x; chunk < nchunks; chunk += RED_BLOCKS) {
            const size_t row0 = static_cast<size_t>(chunk) * R + lane * V;
            const Vec rv = *reinterpret_cast<const Vec *>(r + row0);
#pragma unroll
            for (int k = 0; k < PC_COLS_PER_ROUND; ++k) {
                const int j = wave + PC_WAVES * (k0 + k);
                if (j < cols) {
                    const Vec b = *reinterpret_cast<const Vec *>(Bhat + static_cast<size_t>(j) * ldn + row0);
#pragma unroll
                    for (int u = 0; u < V; ++u) acc[k] += static_cast<double>(b[u]) * static_cast<double>(rv[u]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < PC_COLS_PER_ROUND; ++k) {
            const int j = wave + PC_WAVES * (k0 + k);
            if (j < cols) {
                double v = acc[k];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
                if (lane == 0) tpart[static_cast<size_t>(blockIdx.x) * cols + j] = v;
            }
        }
    }
}

/* (b) One block per 32 columns of Bhat: t_j of its columns from the RED_BLOCKS partial sums (eight groups of 32 blocks, each added in ascending order with its 32 loads in
 * flight, the groups then as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7))), and the columns' share of s = G^-1 t, spart[block][i] = sum over the block's j of Ginv[j][i] t_j
 * (Ginv is symmetric to the bit: row j serves as column j, read along i).  No block reads another's partial sums twice; (c) adds the blocks' shares in block order. */
__global__ __launch_bounds__(RED_THREADS) void k_precond_solve(const double *__restrict__ tpart, const double *__restrict__ Ginv, int cols, double *__restrict__ spart) {
    static_assert(RED_BLOCKS == 8 * PC_SOLVE_COLS && RED_THREADS == 8 * PC_SOLVE_COLS, "eight groups of 32 partial sums for each of 32 columns");
    __shared__ double share[8][PC_SOLVE_COLS];
    __shared__ double t[PC_SOLVE_COLS];
    const int j0 = blockIdx.x * PC_SOLVE_COLS;
    const int jj = threadIdx.x % PC_SOLVE_COLS, group = threadIdx.x / PC_SOLVE_COLS;
    double v = 0.0;
    if (j0 + jj < cols) {
        const double *col = tpart + static_cast<size_t>(group) * PC_SOLVE_COLS * cols + j0 + jj;
#pragma unroll
        for (int b = 0; b < PC_SOLVE_COLS; ++b) v += col[static_cast<size_t>(b) * cols];
    }
    share[group][jj] = v;
    __syncthreads();
    if (threadIdx.x < PC_SOLVE_COLS) {
        t[jj] = ((share[0][jj] + share[1][jj]) + (share[2][jj] + share[3][jj])) + ((share[4][jj] + share[5][jj]) + (share[6][jj] + share[7][jj]));  // (0 beyond the last column)
    }
    __syncthreads();
    const int jend = min(PC_SOLVE_COLS, cols - j0);
    for (int i = threadIdx.x; i < cols; i += RED_THREADS) {
        double acc = 0.0;
#pragma unroll 8
        for (int k = 0; k < jend; ++k) acc += Ginv[static_cast<size_t>(j0 + k) * cols + i] * t[k];
        spart[static_cast<size_t>(blockIdx.x) * cols + i] = acc;
    }
}

/* (c) s = the sum of (b)'s shares ; z = r - Bhat s ; part = (r.z, 0).  The waves split the columns as in (a); their sixteen shares of a row meet in LDS and are added in wave order. */
template <typename T>
__global__ __launch_bounds__(PC_THREADS) void k_precond_z(const T *__restrict__ Bhat, size_t ldn, int cols, const double *__restrict__ spart, const T *__restrict__ r, T *__restrict__ z,
                                                          double *__restrict__ part) {
    using Vec = typename PcVec<T>::type;
    constexpr int V = PcVec<T>::n, R = 64 * V;
    __shared__ double sl[PC_MAX_COLS + 7];
    __shared__ double share[PC_WAVES][R];
    __shared__ double red[PC_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nshares = (cols + PC_SOLVE_COLS - 1) / PC_SOLVE_COLS;
    for (int j = threadIdx.x; j < cols; j += PC_THREADS) {  // s_j: the shares of k_precond_solve's blocks, in block order
        double v = 0.0;
        for (int b = 0; b < nshares; ++b) v += spart[static_cast<size_t>(b) * cols + j];
        sl[j] = v;
    }
    double rz = 0.0;
    const int nchunks = static_cast<int>(ldn / R);
    for (int chunk = blockIdx.x; chunk < nchunks; chunk += RED_BLOCKS) {
        __syncthreads();  // (sl is written; the previous chunk's shares have been read)
        const size_t row0 = static_cast<size_t>(chunk) * R + lane * V;
        double acc[V];
#pragma unroll
        for (int u = 0; u < V; ++u) acc[u] = 0.0;
#pragma unroll
        for (int k = 0; k < PC_COLS_PER_WAVE; ++k) {
            const int j = wave + PC_WAVES * k;
            if (j < cols) {
                const Vec b = *reinterpret_cast<const Vec *>(Bhat + static_cast<size_t>(j) * ldn + row0);
                const double sj = sl[j];
#pragma unroll
                for (int u = 0; u < V; ++u) acc[u] += static_cast<double>(b[u]) * sj;
            }
        }
#pragma unroll
        for (int u = 0; u < V; ++u) share[wave][lane * V + u] = acc[u];
        __syncthreads();
        if (threadIdx.x < R) {
            double sum = 0.0;
#pragma unroll
            for (int w = 0; w < PC_WAVES; ++w) sum += share[w][threadIdx.x];
            const size_t i = static_cast<size_t>(chunk) * R + threadIdx.x;
            const T ri = r[i];
            const T zi = static_cast<T>(static_cast<double>(ri) - sum);
            z[i] = zi;  // (rows from n on: Bhat and r are exact zeros there, so is z)
            rz += static_cast<double>(ri) * static_cast<double>(zi);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rz += __shfl_down(rz, off);
    __syncthreads();
    if (lane == 0) red[wave] = rz;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (int w = 0; w < PC_WAVES; ++w) v += red[w];
        part[blockIdx.x * 2 + 0] = v;
        part[blockIdx.x * 2 + 1] = 0.0;
    }
}

/* ---------------------------------------------------------------- the PCG step that is new ---------------------------------------------------------------- */

/* r.z from k_precond_z's partials; beta = r.z / (r.z of the previous iteration) ; d = z + beta d (initial: d = z) ; part = (sum d, q.d) for k_Ad_and_dAd.  The new r.z
 * goes to the scalar set of the NEXT iteration (`sc_next`: k_update_x_r reads it as alpha's numerator), every block reads the old one from `sc` -- two sets, so that no
 * block reads what another has overwritten.  beta is rounded to T first, as k_update_d rounds it. */
template <typename T>
__global__ __launch_bounds__(RED_THREADS) void k_pcg_update_d(T *__restrict__ d, const T *__restrict__ z, const T *__restrict__ q, const double *__restrict__ part_rz,
                                                              const double *__restrict__ sc, double *__restrict__ sc_next, int n, int initial, double *__restrict__ part) {
    __shared__ double lds[8];
    __shared__ double tot[2];
    double rz, unused;
    finish2_in_block(part_rz, lds, tot, rz, unused);
    const double beta_d = initial ? 0.0 : rz / sc[SC_DELTA];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sc_next[SC_DELTA_OLD] = initial ? 0.0 : sc[SC_DELTA];
        sc_next[SC_DELTA] = rz;
        sc_next[SC_BETA] = beta_d;
    }
    const T beta = static_cast<T>(beta_d);
    double acc[2] = { 0.0, 0.0 };
    for (int i = blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += RED_BLOCKS * RED_THREADS) {
        const T di = initial ? z[i] : z[i] + beta * d[i];
        d[i] = di;
        acc[0] += static_cast<double>(di);
        acc[1] += static_cast<double>(di) * static_cast<double>(q[i]);
    }
    __syncthreads();  // (lds is reused)
    block_reduce<2>(acc, lds);
    if (threadIdx.x == 0) {
        part[blockIdx.x * 2 + 0] = acc[0];
        part[blockIdx.x * 2 + 1] = acc[1];
    }
}

/* ---------------------------------------------------------------- host: dense factorisations in double (<= 513 x 513, row major) ---------------------------------------------------------------- */

/* L^-1 (lower triangular) of the lower triangle of L, row by row: row i = (e_i - sum over k < i of L[i][k] row k) * (1 / L[i][i]).
 * NOT to be merged with invert_lower_rows (lssvm_reduced.hip), which DIVIDES by L[i][i]: either change moves the bits of every preconditioned solve or of every leverage. */
std::vector<double> invert_lower_by_reciprocal(const std::vector<double> &L, int m) {
    std::vector<double> inv(static_cast<size_t>(m) * m, 0.0);
    for (int i = 0; i < m; ++i) {
        double *ri = &inv[static_cast<size_t>(i) * m];
        for (int k = 0; k < i; ++k) {
            const double lik = L[static_cast<size_t>(i) * m + k];
            const double *rk = &inv[static_cast<size_t>(k) * m];
            for (int j = 0; j <= k; ++j) ri[j] -= lik * rk[j];
        }
        const double d = 1.0 / L[static_cast<size_t>(i) * m + i];
        for (int j = 0; j < i; ++j) ri[j] *= d;
        ri[i] = d;
    }
    return inv;
}

/* (L L^T)^-1 = L^-T L^-1 from L^-1: the lower triangle is summed (k ascending), the upper one is its copy -- symmetric to the bit */
std::vector<double> inverse_from_lower_inverse(const std::vector<double> &inv, int m) {
    std::vector<double> out(static_cast<size_t>(m) * m, 0.0);
    for (int k = 0; k < m; ++k) {
        const double *rk = &inv[static_cast<size_t>(k) * m];
        for (int i = 0; i <= k; ++i) {
            const double a = rk[i];
            double *oi = &out[static_cast<size_t>(i) * m];
            for (int j = 0; j <= i; ++j) oi[j] += a * rk[j];
        }
    }
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < i; ++j) out[static_cast<size_t>(j) * m + i] = out[static_cast<size_t>(i) * m + j];
    }
    return out;
}

}  // namespace

/* A = L L^T in place (lower triangle; the upper one is left alone); false at a pivot that is not positive and finite */
bool cholesky_lower(std::vector<double> &A, int m) {
    for (int i = 0; i < m; ++i) {
        double *ai = &A[static_cast<size_t>(i) * m];
        for (int j = 0; j <= i; ++j) {
            const double *aj = &A[static_cast<size_t>(j) * m];
            double s = ai[j];
            for (int k = 0; k < j; ++k) s -= ai[k] * aj[k];
            if (j < i) {
                ai[j] = s / aj[j];
            } else {
                if (!(s > 0.0) || !std::isfinite(s)) return false;
                ai[i] = std::sqrt(s);
            }
        }
    }
    return true;
}

double cholesky_with_jitter(const std::vector<double> &M, int m, const char *subject, std::vector<double> &L) {
    double trace = 0.0;
    for (int k = 0; k < m; ++k) trace += M[static_cast<size_t>(k) * m + k];
    LSSVM_REQUIRE(std::isfinite(trace) && trace > 0.0, std::string(subject) + " has no positive finite trace");
    double nu = DBL_EPSILON * trace;
    bool factored = false;
    for (int attempt = 0; attempt < 7 && !factored; ++attempt, nu *= factored ? 1.0 : 10.0) {
        L = M;
        for (int k = 0; k < m; ++k) L[static_cast<size_t>(k) * m + k] += nu;
        factored = cholesky_lower(L, m);
    }
    if (!factored) throw Error(LSSVM_ERR_INTERNAL, std::string(subject) + " could not be factored (jitter up to " + std::to_string(nu / 10.0) + ")");
    return nu;
}

/* the library's own landmarks: the first `rank` entries of a Fisher-Yates shuffle of 0 ... N-1 driven by splitmix64 from a fixed state (include/plssvm_amd.h) */
std::vector<uint64_t> default_landmarks(size_t N, size_t rank) {
    std::vector<uint64_t> perm(N);
    std::iota(perm.begin(), perm.end(), uint64_t{ 0 });
    uint64_t state = 0x243F6A8885A308D3ull;
    const auto next = [&state]() {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    for (size_t i = 0; i < rank; ++i) std::swap(perm[i], perm[i + static_cast<size_t>(next() % (N - i))]);
    perm.resize(rank);
    return perm;
}

std::vector<uint64_t> resolve_landmarks(const uint64_t *landmarks, size_t rank, size_t N) {
    if (landmarks == nullptr) return default_landmarks(N, rank);
    std::vector<uint64_t> lm(landmarks, landmarks + rank);
    std::vector<uint64_t> sorted(lm);
    std::sort(sorted.begin(), sorted.end());
    LSSVM_REQUIRE(sorted.back() < N, "Every landmark must be the index of a data point (< " + std::to_string(N) + "), but one is " + std::to_string(sorted.back()) + "!");
    LSSVM_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), "The landmarks must be distinct!");
    return lm;
}

void check_pcg_arguments(const void *Y, size_t num_rhs, double eps, uint64_t max_iter, const void *alphas_out, const double *rhos_out, const lssvm_pcg_info *infos_out) {
    LSSVM_REQUIRE(Y != nullptr, "The right hand side vector must not be empty!");
    LSSVM_REQUIRE(num_rhs > 0, "The number of right hand sides must be greater than 0!");
    LSSVM_REQUIRE(std::isfinite(eps) && eps > 0.0, "The stopping criterion in the CG algorithm must be greater than 0.0, but is " + std::to_string(eps) + "!");
    LSSVM_REQUIRE(max_iter > 0, "The number of CG iterations must be greater than 0!");
    LSSVM_REQUIRE(alphas_out != nullptr && rhos_out != nullptr && infos_out != nullptr, "alphas_out / rhos_out / infos_out must not be NULL");
}

void check_precond_rank(uint64_t rank, size_t num_points) {
    const uint64_t most = std::min<uint64_t>(num_points > 0 ? num_points - 1 : 0, PRECOND_MAX_RANK);
    LSSVM_REQUIRE(rank >= 1 && rank <= most, "The rank of the preconditioner must lie in [1, " + std::to_string(most) + "], but is " + std::to_string(rank) + "!");
}

template <typename T>
Problem<T> &Solver<T>::precond_problem(const char *what) {
    LSSVM_REQUIRE(shards_.size() == 1 && world_ == 1 && exchange_ == Exchange::none, std::string("the preconditioner (") + what + ") runs on a problem of one device and one rank");
    Problem<T> &p = *shards_[0];
    LSSVM_REQUIRE(!p.weighted_, std::string("the preconditioner (") + what + ") is built for the unweighted system: the problem has weights set (lssvm_mi355_problem_set_weights(p, NULL, 0) removes them)");
    LSSVM_REQUIRE(!in_cg_, std::string(what) + " cannot run between cg_begin and cg_finish");
    return p;
}

template <typename T>
void Solver<T>::build_preconditioner(uint64_t rank, const uint64_t *landmarks, lssvm_precond_info *info) {
    Problem<T> &p = precond_problem("build_preconditioner");
    const size_t N = p.N_;
    check_precond_rank(rank, N);
    const int m = static_cast<int>(rank), cols = m + 1, n = p.n_;
    const std::vector<uint64_t> lm = resolve_landmarks(landmarks, static_cast<size_t>(m), N);

    const double t0 = now_ms();
    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    auto pc = std::make_unique<Precond<T>>();
    pc->rank = m;
    pc->cols = cols;
    pc->ldn = static_cast<size_t>(round_up(n, 256));
    pc->landmarks = lm;
    pc->sigma = p.inv_cost_;
    const size_t ldN = static_cast<size_t>(round_up(static_cast<long>(N), 256));

    // ---- the landmark block K_Nm (all N points) from the resident data, and K_mm out of it ----
    const LandmarkBlock<T> block(p, lm, st);
    DevBuf<double> Kd, Bf, Kmm_dev, Linv_dev, G_dev;
    Kd.alloc_zero(static_cast<size_t>(m) * ldN, st);
    block.enqueue(0, static_cast<int>(ldN), Kd.p, ldN);  // (one slab of all the rows)
    Kmm_dev.alloc_zero(static_cast<size_t>(m) * m, st);
    block.enqueue_gather_kmm(Kd.p, ldN, 0, static_cast<int>(ldN), Kmm_dev.p);
    LSSVM_HIP_CHECK(hipGetLastError());
    std::vector<double> Kmm(static_cast<size_t>(m) * m);
    LSSVM_HIP_CHECK(hipMemcpyAsync(Kmm.data(), Kmm_dev.p, Kmm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));

    // ---- L L^T = K_mm + nu I on the host ----
    double host_ms = 0.0, t_host = now_ms();
    std::vector<double> L;
    pc->jitter = cholesky_with_jitter(Kmm, m, "the kernel matrix of the landmarks", L);
    const std::vector<double> Linv = invert_lower_by_reciprocal(L, m);
    host_ms += now_ms() - t_host;

    // ---- B_f = K_Nm L^-T, Bhat = [E B_f | sqrt(sigma) 1] in the real type ----
    Linv_dev.alloc_zero(Linv.size(), st);
    LSSVM_HIP_CHECK(hipMemcpyAsync(Linv_dev.p, Linv.data(), Linv.size() * sizeof(double), hipMemcpyHostToDevice, st));
    Bf.alloc_zero(static_cast<size_t>(m) * ldN, st);
    hipLaunchKernelGGL(k_nystrom_factor, dim3(static_cast<unsigned>(ldN / 256), m), dim3(256), 0, st, Kd.p, ldN, Linv_dev.p, m, Bf.p);
    pc->Bhat.alloc_zero(static_cast<size_t>(cols) * pc->ldn, st);
    hipLaunchKernelGGL(k_make_bhat<T>, dim3(static_cast<unsigned>(pc->ldn / 256), cols), dim3(256), 0, st, Bf.p, ldN, n, m, std::sqrt(pc->sigma), pc->Bhat.p, pc->ldn);

    // ---- G = Bhat^T Bhat + sigma I: the lower triangle from the device, the rest on the host ----
    const int tiles = (cols + 15) / 16, ldg = tiles * 16;
    G_dev.alloc_zero(static_cast<size_t>(ldg) * ldg, st);
    hipLaunchKernelGGL(k_precond_gram<T>, dim3(tiles, tiles), dim3(256), 0, st, pc->Bhat.p, pc->ldn, cols, G_dev.p, ldg);
    LSSVM_HIP_CHECK(hipGetLastError());
    std::vector<double> Gpad(static_cast<size_t>(ldg) * ldg);
    LSSVM_HIP_CHECK(hipMemcpyAsync(Gpad.data(), G_dev.p, Gpad.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    t_host = now_ms();
    std::vector<double> G(static_cast<size_t>(cols) * cols, 0.0);
    for (int j = 0; j < cols; ++j) {
        for (int k = 0; k <= j; ++k) G[static_cast<size_t>(j) * cols + k] = Gpad[static_cast<size_t>(j) * ldg + k];
        G[static_cast<size_t>(j) * cols + j] += pc->sigma;
    }
    if (!cholesky_lower(G, cols)) throw Error(LSSVM_ERR_INTERNAL, "Bhat^T Bhat + sigma I could not be factored");
    const std::vector<double> Ginv = inverse_from_lower_inverse(invert_lower_by_reciprocal(G, cols), cols);
    host_ms += now_ms() - t_host;
    pc->Ginv.alloc_zero(Ginv.size(), st);
    LSSVM_HIP_CHECK(hipMemcpyAsync(pc->Ginv.p, Ginv.data(), Ginv.size() * sizeof(double), hipMemcpyHostToDevice, st));
    pc->tpart.alloc_zero(static_cast<size_t>(RED_BLOCKS) * cols, st);
    pc->s.alloc_zero(static_cast<size_t>((cols + PC_SOLVE_COLS - 1) / PC_SOLVE_COLS) * cols, st);
    pc->part_rz.alloc_zero(static_cast<size_t>(RED_BLOCKS) * 2, st);
    const size_t vec_len = std::max(pc->ldn, static_cast<size_t>(p.nvec_) + TILE);
    pc->r_io.alloc_zero(vec_len, st);
    pc->z_io.alloc_zero(vec_len, st);
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (the temporaries are released on return)
    pc->build_ms = now_ms() - t0;
    if (info != nullptr) {
        lssvm_precond_info out{};
        out.rank = static_cast<uint64_t>(m);
        out.jitter = pc->jitter;
        out.build_ms = pc->build_ms;
        out.host_ms = host_ms;
        out.device_bytes = (pc->Bhat.count + pc->r_io.count + pc->z_io.count) * sizeof(T) + (pc->Ginv.count + pc->tpart.count + pc->s.count + pc->part_rz.count) * sizeof(double);
        *info = out;
    }
    precond_ = std::move(pc);
}

template <typename T>
void Solver<T>::precond_landmarks(uint64_t *out) {
    LSSVM_REQUIRE(out != nullptr, "out must not be NULL");
    LSSVM_REQUIRE(precond_ != nullptr, "the problem has no preconditioner (lssvm_mi355_problem_build_preconditioner builds one)");
    std::copy(precond_->landmarks.begin(), precond_->landmarks.end(), out);
}

/* z = r - Bhat G^-1 Bhat^T r: (a), (b), (c).  r and z hold at least ldn reals, exact zeros from row n on */
template <typename T>
void Solver<T>::enqueue_precond_apply(const T *r, T *z, double *part_rz) const {
    const Precond<T> &pc = *precond_;
    hipStream_t st = shards_[0]->stream();
    hipLaunchKernelGGL(k_precond_Btr<T>, dim3(RED_BLOCKS), dim3(PC_THREADS), 0, st, pc.Bhat.p, pc.ldn, pc.cols, r, pc.tpart.p);
    hipLaunchKernelGGL(k_precond_solve, dim3((pc.cols + PC_SOLVE_COLS - 1) / PC_SOLVE_COLS), dim3(RED_THREADS), 0, st, pc.tpart.p, pc.Ginv.p, pc.cols, pc.s.p);
    hipLaunchKernelGGL(k_precond_z<T>, dim3(RED_BLOCKS), dim3(PC_THREADS), 0, st, pc.Bhat.p, pc.ldn, pc.cols, pc.s.p, r, z, part_rz);
    LSSVM_HIP_CHECK(hipGetLastError());
}

template <typename T>
void Solver<T>::precond_apply(const void *r, void *z_out) {
    LSSVM_REQUIRE(r != nullptr && z_out != nullptr, "r / z_out must not be NULL");
    Problem<T> &p = precond_problem("precond_apply");
    LSSVM_REQUIRE(precond_ != nullptr, "the problem has no preconditioner (lssvm_mi355_problem_build_preconditioner builds one)");
    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    const size_t bytes = static_cast<size_t>(p.n_) * sizeof(T);
    LSSVM_HIP_CHECK(hipMemcpyAsync(precond_->r_io.p, r, bytes, hipMemcpyHostToDevice, st));
    enqueue_precond_apply(precond_->r_io.p, precond_->z_io.p, precond_->part_rz.p);
    LSSVM_HIP_CHECK(hipMemcpyAsync(z_out, precond_->z_io.p, bytes, hipMemcpyDeviceToHost, st));
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));
}

template <typename T>
void Solver<T>::solve_pcg(const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out_v, double *rhos_out, lssvm_pcg_info *infos_out) {
    check_pcg_arguments(Y, num_rhs, eps, max_iter, alphas_out_v, rhos_out, infos_out);
    LSSVM_REQUIRE(static_cast<T>(eps) > T(0), "The stopping criterion in the CG algorithm must be greater than 0.0, but is " + std::to_string(eps) + "!");  // csvm.cpp:77
    Problem<T> &p = precond_problem("solve_pcg");
    LSSVM_REQUIRE(precond_ != nullptr, "the problem has no preconditioner (lssvm_mi355_problem_build_preconditioner builds one)");
    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    const CgSteps<T> cg(p);
    const CgState<T> &s = p.lane(0);  // b, x, r, d, Ad and the recipe's scalars; its K*v vector holds z
    T *z = s.Kv.p;
    const int n = p.n_;
    const size_t N = p.N_;
    const T *q = p.q_.p;
    const dim3 gr(RED_BLOCKS), br(RED_THREADS);
    DevBuf<double> rz_sc;  // two sets of scalars for r.z (k_pcg_update_d), used in turn
    rz_sc.alloc_zero(2 * static_cast<size_t>(SC_COUNT), st);
    Event timer[2][2];  // around the apply of an iteration, two pairs in turn: a pair is read once the stream has passed the NEXT iteration's delta
    for (auto &pair : timer) {
        pair[0].create(true);
        pair[1].create(true);
    }
    const T *Yt = static_cast<const T *>(Y);
    T *alphas_out = static_cast<T *>(alphas_out_v);

    for (size_t c = 0; c < num_rhs; ++c) {
        const double t_rhs = now_ms();
        const double y_last = static_cast<double>(Yt[c * N + N - 1]);
        uint64_t gram_passes = 0, applies_timed = 0;
        double apply_ms = 0.0;
        bool apply_pending[2] = { false, false };
        const auto read_apply_time = [&](uint64_t slot) {  // (the stream has passed the pair's events)
            float ms = 0.0f;
            if (apply_pending[slot] && hipEventElapsedTime(&ms, timer[slot][0].e, timer[slot][1].e) == hipSuccess) {
                apply_ms += ms;
                ++applies_timed;
            }
            apply_pending[slot] = false;
        };
        const auto apply_and_direct = [&](uint64_t iteration, bool initial) {  // z = P^-1 r, r.z, d = z + beta d
            double *sc_now = rz_sc.p + (iteration & 1) * SC_COUNT, *sc_next = rz_sc.p + ((iteration + 1) & 1) * SC_COUNT;
            LSSVM_HIP_CHECK(hipEventRecord(timer[iteration & 1][0].e, st));
            enqueue_precond_apply(s.r.p, z, precond_->part_rz.p);
            LSSVM_HIP_CHECK(hipEventRecord(timer[iteration & 1][1].e, st));
            apply_pending[iteration & 1] = true;
            hipLaunchKernelGGL(k_pcg_update_d<T>, gr, br, 0, st, s.d.p, z, q, precond_->part_rz.p, sc_now, sc_next, n, initial ? 1 : 0, s.part_of(PART_D));
            LSSVM_HIP_CHECK(hipGetLastError());
        };

        // ---- cg_begin's statements: b = y - y_last, x = 1, r = b - Abar x, delta0 ----
        cg.begin(s, Yt + c * N);
        p.enqueue_apply_K_local(s.x.p, false);
        ++gram_passes;
        cg.residual(s, p.Kres_, s.x.p, s.r.p, PART_RR);
        cg.finish_delta(s, PART_RR, s.host_delta.dev, true);
        wait_for_deltas();
        p.drain_events();
        const double delta0 = static_cast<double>(static_cast<T>(s.delta_on_host()));
        const T target = static_cast<T>(eps) * static_cast<T>(eps) * static_cast<T>(delta0);  // as cg_step evaluates it
        double delta = delta0;
        bool converged = static_cast<T>(delta) <= target;  // (b = Abar 1: x0 is the solution)
        uint64_t iterations = 0;
        if (!converged) apply_and_direct(1, true);  // (the first iteration reads the scalar set of parity 0)

        while (!converged && iterations < max_iter) {
            double *sc_now = rz_sc.p + (iterations & 1) * SC_COUNT;
            const bool refresh = iterations % 50 == 49;
            p.enqueue_apply_K_local(s.d.p, false);
            ++gram_passes;
            cg.advance(s, p.Kres_, refresh, sc_now);  // (alpha's numerator is r.z of this iteration's set)
            if (refresh) {  // r = b - Abar x
                p.enqueue_apply_K_local(s.x.p, false);
                ++gram_passes;
                cg.residual(s, p.Kres_, s.x.p, s.r.p, PART_RR);
            }
            cg.finish_delta(s, PART_RR, s.host_delta.dev, false);
            LSSVM_HIP_CHECK(hipEventRecord(ev_delta_.e, st));
            // z, r.z and the direction go into the queue ahead of the stop test: they touch z and d only, never x or r
            if (iterations + 1 < max_iter) apply_and_direct(iterations, false);
            LSSVM_HIP_CHECK(hipEventSynchronize(ev_delta_.e));
            p.drain_events();
            read_apply_time((iterations + 1) & 1);  // (the apply before this iteration's Gram pass)
            ++iterations;
            delta = static_cast<double>(static_cast<T>(s.delta_on_host()));
            converged = static_cast<T>(delta) <= target;  // csvm.cpp:155-158
        }

        cg.finish_now(s, y_last, alphas_out + c * N, rhos_out + c);
        read_apply_time(0);
        read_apply_time(1);
        lssvm_pcg_info info{};
        info.iterations = iterations;
        info.gram_passes = gram_passes;
        info.converged = converged ? 1 : 0;
        info.rank = precond_->rank;
        info.initial_residuum = delta0;
        info.residuum = delta;
        info.target_residuum = static_cast<double>(target);
        info.jitter = precond_->jitter;
        info.build_ms = precond_->build_ms;
        info.apply_ms = applies_timed > 0 ? apply_ms / static_cast<double>(applies_timed) : 0.0;
        info.total_ms = now_ms() - t_rhs;
        infos_out[c] = info;
    }
}

template Problem<float> &Solver<float>::precond_problem(const char *);
template Problem<double> &Solver<double>::precond_problem(const char *);
template void Solver<float>::build_preconditioner(uint64_t, const uint64_t *, lssvm_precond_info *);
template void Solver<double>::build_preconditioner(uint64_t, const uint64_t *, lssvm_precond_info *);
template void Solver<float>::precond_landmarks(uint64_t *);
template void Solver<double>::precond_landmarks(uint64_t *);
template void Solver<float>::enqueue_precond_apply(const float *, float *, double *) const;
template void Solver<double>::enqueue_precond_apply(const double *, double *, double *) const;
template void Solver<float>::precond_apply(const void *, void *);
template void Solver<double>::precond_apply(const void *, void *);
template void Solver<float>::solve_pcg(const void *, size_t, double, uint64_t, void *, double *, lssvm_pcg_info *);
template void Solver<double>::solve_pcg(const void *, size_t, double, uint64_t, void *, double *, lssvm_pcg_info *);

}  // namespace lssvm
