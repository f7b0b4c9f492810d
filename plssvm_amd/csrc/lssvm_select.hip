/*
 * lssvm_select.hip -- landmark selection on a resident problem: the pivots of a partial Cholesky factorisation of the kernel matrix, chosen greedily or at random in
 * proportion to the residual diagonal (randomly pivoted Cholesky; lssvm_mi355_problem_select_landmarks, lssvm_mi355_select_landmarks_*).
 *
 * Over n candidates (all points, or a prefix of the library's fixed shuffle) the factor F (rank x ld, ld = n rounded up to 256, row j = column j of the partial
 * Cholesky factor) and the residual diagonal d live in HBM.  Step j is two launches on the problem's stream:
 *   k_select_pivot (one workgroup)   S = the sum of the block sums of d (blocks ascending), the pivot of step j, the stop test; writes the pivot, d_p, S, `done`;
 *   k_select_step  (256 rows each)   c_i = k(x_i, x_p) - sum_{t<j} F[t][i] F[t][p], F[j][i] = c_i / sqrt(d_p), d_i, the block's (sum, max, position of the max).
 * The host enqueues all of them back to back and reads once at the end; after `done` the remaining launches return at once.  A step streams j rows of F (coalesced:
 * thread i reads F[t][i]) and its own row of X_ in 16-byte pieces: n ldx sizeof(T) + 8 j n + O(n) bytes.  Every reduction has one fixed order, no atomics: DPP within
 * a 16-lane row, the sixteen rows of a block through LDS in ascending order, the blocks in ascending order.  Compiled for gfx950 only.
 */
#include "lssvm_landmark.hip.hpp"

#include <cfloat>
#include <cmath>
#include <limits>
#include <numeric>

namespace lssvm {

namespace {

constexpr int SEL_ROWS = 256;           // candidates per workgroup of the step kernel, as k_landmark_block
constexpr int SEL_FC = 128;             // features of the pivot's row in LDS at a time
constexpr int SEL_PIVOT_CHUNK = 2048;   // block sums in LDS at a time (k_select_pivot)

/* what k_select_pivot leaves for the step kernel and the host */
struct SelectState {
    double S;                 // the sum of d before the step that was last looked at
    double d0;                // max d_i before the first step
    double dp;                // d of the pivot
    double dmax;              // the largest d_i before the step that was last looked at
    unsigned long long rng;   // splitmix64's state
    int pivot;                // candidate position of the pivot
    int done;                 // the stop test fired
    int rank_found;           // ... at this step (rank where it never did)
    int pad;
};

/* v of the lane that CTRL names within this lane's 16-lane row (data-parallel primitives: no LDS, a double as its two dwords) */
template <int CTRL>
__device__ __forceinline__ int dpp_int(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ double dpp_double(double v) {
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = static_cast<unsigned>(dpp_int<CTRL>(static_cast<int>(static_cast<unsigned>(bits))));
    const unsigned hi = static_cast<unsigned>(dpp_int<CTRL>(static_cast<int>(static_cast<unsigned>(bits >> 32))));
    return __builtin_bit_cast(double, (static_cast<unsigned long long>(hi) << 32) | lo);
}

/* (m, pos) <- the larger of (m, pos) and (om, opos); among equal values the smaller position */
__device__ __forceinline__ void take_larger(double &m, int &pos, double om, int opos) {
    if (om > m || (om == m && opos < pos)) {
        m = om;
        pos = opos;
    }
}

template <int CTRL>
__device__ __forceinline__ void row_max_step(double &m, int &pos) {
    const double om = dpp_double<CTRL>(m);
    const int opos = dpp_int<CTRL>(pos);
    take_larger(m, pos, om, opos);
}
template <int CTRL>
__device__ __forceinline__ void row_step(double &sum, double &m, int &pos) {
    sum += dpp_double<CTRL>(sum);  // (both partners add the same two values: the same bits in both)
    row_max_step<CTRL>(m, pos);
}

/* The block's (sum of v, max of v, smallest position of the max) in thread 0: lanes l ^ 1, l ^ 2, then the mirrored halves of 8 and of 16 lanes (every lane of a
 * 16-lane row ends with the row's result), then the sixteen rows of the block through LDS, added in ascending row order. */
__device__ __forceinline__ void block_sum_max(double &sum, double &m, int &pos, double *lds_sum, double *lds_max, int *lds_pos) {
    row_step<0xB1>(sum, m, pos);   // quad_perm [1, 0, 3, 2]
    row_step<0x4E>(sum, m, pos);   // quad_perm [2, 3, 0, 1]
    row_step<0x141>(sum, m, pos);  // row_half_mirror
    row_step<0x140>(sum, m, pos);  // row_mirror
    if ((threadIdx.x & 15) == 0) {
        lds_sum[threadIdx.x >> 4] = sum;
        lds_max[threadIdx.x >> 4] = m;
        lds_pos[threadIdx.x >> 4] = pos;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sum = lds_sum[0];
        m = lds_max[0];
        pos = lds_pos[0];
        for (int r = 1; r < SEL_ROWS / 16; ++r) {
            sum += lds_sum[r];
            take_larger(m, pos, lds_max[r], lds_pos[r]);
        }
    }
}

/* d_i = k(x_i, x_i) for the candidates (exact zeros from n on) and the blocks' triples; a thread walks its own row as k_landmark_block walks it */
template <typename T>
__global__ __launch_bounds__(SEL_ROWS) void k_select_diag(const T *__restrict__ X, int ldx, const int *__restrict__ cand, int n, int kernel_type, int degree, double gamma, double coef0,
                                                          double *__restrict__ d, double *__restrict__ bsum, double *__restrict__ bmax, int *__restrict__ bpos) {
    constexpr int V = PcVec<T>::n;
    __shared__ double lds_sum[SEL_ROWS / 16], lds_max[SEL_ROWS / 16];
    __shared__ int lds_pos[SEL_ROWS / 16];
    const int i = blockIdx.x * SEL_ROWS + threadIdx.x;
    const T *xi = X + static_cast<size_t>(cand[min(i, n - 1)]) * ldx;
    double acc = 0.0;
    for (int f = 0; f < ldx; f += V) {
        const typename PcVec<T>::type v = *reinterpret_cast<const typename PcVec<T>::type *>(xi + f);
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const double a = static_cast<double>(v[u]);
            if (kernel_type == LSSVM_KERNEL_RBF) {
                acc += (a - a) * (a - a);
            } else {
                acc += a * a;
            }
        }
    }
    const double di = i < n ? landmark_kernel_value(kernel_type, degree, gamma, coef0, acc) : 0.0;
    d[i] = di;
    double sum = di, m = di;
    int pos = i;
    block_sum_max(sum, m, pos, lds_sum, lds_max, lds_pos);
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = sum;
        bmax[blockIdx.x] = m;
        bpos[blockIdx.x] = pos;
    }
}

/* One workgroup, before step j (and once after the last step, `last`): S and the largest d from the blocks' triples, then the pivot of step j and the stop test. */
__global__ __launch_bounds__(SEL_ROWS) void k_select_pivot(const double *__restrict__ d, const double *__restrict__ bsum, const double *__restrict__ bmax, const int *__restrict__ bpos,
                                                           int nblocks, int j, int method, int last, double tol, SelectState *__restrict__ state, int *__restrict__ pivots,
                                                           double *__restrict__ trace) {
    __shared__ double chunk[SEL_PIVOT_CHUNK];
    __shared__ double lds_max[SEL_ROWS / 16];
    __shared__ int lds_pos[SEL_ROWS / 16];
    __shared__ double sh_t, sh_rem;
    __shared__ int sh_block;
    if (state->done) return;

    // ---- the greedy pivot: the largest block maximum, among equal values the smallest position (no sum: the order does not matter) ----
    double m = -1.0;
    int pos = 0x7fffffff;
    for (int b = threadIdx.x; b < nblocks; b += SEL_ROWS) take_larger(m, pos, bmax[b], bpos[b]);
    row_max_step<0xB1>(m, pos);
    row_max_step<0x4E>(m, pos);
    row_max_step<0x141>(m, pos);
    row_max_step<0x140>(m, pos);
    if ((threadIdx.x & 15) == 0) {
        lds_max[threadIdx.x >> 4] = m;
        lds_pos[threadIdx.x >> 4] = pos;
    }

    // ---- S: the block sums in ascending order, through LDS in chunks, added by thread 0 ----
    double S = 0.0;
    for (int b0 = 0; b0 < nblocks; b0 += SEL_PIVOT_CHUNK) {
        __syncthreads();
        const int count = min(SEL_PIVOT_CHUNK, nblocks - b0);
        for (int e = threadIdx.x; e < count; e += SEL_ROWS) chunk[e] = bsum[b0 + e];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int e = 0; e < count; ++e) S += chunk[e];
        }
    }
    double u01 = 0.0;
    if (threadIdx.x == 0) {
        for (int r = 1; r < SEL_ROWS / 16; ++r) take_larger(m, pos, lds_max[r], lds_pos[r]);  // (rows 1 ... 15 were written before the first barrier above)
        trace[j] = S;
        state->S = S;
        state->dmax = m;
        if (j == 0) state->d0 = m;
        if (!last && method == LSSVM_LANDMARKS_RPCHOLESKY) {
            unsigned long long z = (state->rng += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            u01 = static_cast<double>(z >> 11) * 0x1.0p-53;
        }
        sh_t = u01 * S;
        sh_block = -1;
        sh_rem = 0.0;
    }
    if (last) return;  // (uniform)

    int pivot = pos;  // thread 0: the greedy pivot
    if (method == LSSVM_LANDMARKS_RPCHOLESKY) {
        // ---- the first block whose inclusive prefix exceeds t: the same ascending sums again ----
        double prefix = 0.0;
        for (int b0 = 0; b0 < nblocks; b0 += SEL_PIVOT_CHUNK) {
            __syncthreads();
            if (sh_block >= 0) break;  // (uniform: read after the barrier, written before it)
            const int count = min(SEL_PIVOT_CHUNK, nblocks - b0);
            for (int e = threadIdx.x; e < count; e += SEL_ROWS) chunk[e] = bsum[b0 + e];
            __syncthreads();
            if (threadIdx.x == 0) {
                const double t = sh_t;
                for (int e = 0; e < count; ++e) {
                    const double next = prefix + chunk[e];
                    if (next > t) {
                        sh_block = b0 + e;
                        sh_rem = t - prefix;
                        break;
                    }
                    prefix = next;
                }
            }
        }
        __syncthreads();
        const int block = sh_block;
        if (block >= 0) {  // (uniform)
            chunk[threadIdx.x] = d[static_cast<size_t>(block) * SEL_ROWS + threadIdx.x];
            __syncthreads();
            if (threadIdx.x == 0) {
                const double rem = sh_rem;
                double run = 0.0;
                for (int e = 0; e < SEL_ROWS; ++e) {
                    run += chunk[e];
                    if (run > rem) {
                        if (chunk[e] > 0.0) pivot = block * SEL_ROWS + e;
                        break;
                    }
                }
            }
        }
    }
    if (threadIdx.x == 0) {
        const bool none = pivot < 0 || pivot >= nblocks * SEL_ROWS;  // (no block maximum compared greater than -1: the diagonal is not a number)
        const double dp = none ? 0.0 : d[pivot];
        const double floor_rel = fmax(tol, 64.0 * DBL_EPSILON);
        if (none || !(dp > floor_rel * state->d0)) {
            state->done = 1;
            state->rank_found = j;
        } else {
            state->pivot = pivot;
            state->dp = dp;
            pivots[j] = pivot;
        }
    }
}

/* Step j for 256 candidates: the pivot's features through LDS in chunks of SEL_FC and the j values F[t][p] in LDS; a thread walks its own row in 16-byte pieces
 * (features ascending, as k_landmark_block) and streams its column of F (t ascending; the 256 threads of a block read 2 KB in a row per t). */
template <typename T>
__global__ __launch_bounds__(SEL_ROWS) void k_select_step(const T *__restrict__ X, int ldx, const int *__restrict__ cand, int n, size_t ld, int j, int kernel_type, int degree, double gamma,
                                                          double coef0, double *__restrict__ F, double *__restrict__ d, const SelectState *__restrict__ state,
                                                          double *__restrict__ bsum, double *__restrict__ bmax, int *__restrict__ bpos) {
    constexpr int V = PcVec<T>::n;
    __shared__ T xp[SEL_FC];
    __shared__ double fp[SELECT_MAX_RANK];
    __shared__ double lds_sum[SEL_ROWS / 16], lds_max[SEL_ROWS / 16];
    __shared__ int lds_pos[SEL_ROWS / 16];
    if (state->done) return;
    const int p = state->pivot;
    const double dp = state->dp;
    const int i = blockIdx.x * SEL_ROWS + threadIdx.x;
    const T *xi = X + static_cast<size_t>(cand[min(i, n - 1)]) * ldx;
    const T *xpiv = X + static_cast<size_t>(cand[p]) * ldx;
    for (int t = threadIdx.x; t < j; t += SEL_ROWS) fp[t] = F[static_cast<size_t>(t) * ld + p];
    double acc = 0.0;
    for (int f0 = 0; f0 < ldx; f0 += SEL_FC) {  // (ldx is a multiple of the k-chunk: 32 in fp32, 16 in fp64)
        __syncthreads();
        const int fend = min(SEL_FC, ldx - f0);
        if (static_cast<int>(threadIdx.x) < fend) xp[threadIdx.x] = xpiv[f0 + threadIdx.x];
        __syncthreads();
        for (int f = 0; f < fend; f += V) {
            const typename PcVec<T>::type v = *reinterpret_cast<const typename PcVec<T>::type *>(xi + f0 + f);
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const double a = static_cast<double>(v[u]);
                const double b = static_cast<double>(xp[f + u]);
                if (kernel_type == LSSVM_KERNEL_RBF) {
                    acc += (a - b) * (a - b);
                } else {
                    acc += a * b;
                }
            }
        }
    }
    const double k = landmark_kernel_value(kernel_type, degree, gamma, coef0, acc);
    double s = 0.0;  // (fp is complete: at least one pair of barriers has been passed)
    const double *Fi = F + i;
#pragma unroll 8
    for (int t = 0; t < j; ++t) s += Fi[static_cast<size_t>(t) * ld] * fp[t];
    const bool live = i < n;
    const double f = live ? (k - s) / sqrt(dp) : 0.0;
    double di = live ? fmax(d[i] - f * f, 0.0) : 0.0;
    if (i == p) di = 0.0;
    F[static_cast<size_t>(j) * ld + i] = f;
    d[i] = di;
    double sum = di, m = di;
    int pos = i;
    block_sum_max(sum, m, pos, lds_sum, lds_max, lds_pos);
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = sum;
        bmax[blockIdx.x] = m;
        bpos[blockIdx.x] = pos;
    }
}

}  // namespace

size_t check_select_arguments(uint64_t rank, int method, uint64_t pool, double tol, const uint64_t *landmarks_out, size_t num_points) {
    LSSVM_REQUIRE(method == LSSVM_LANDMARKS_GREEDY || method == LSSVM_LANDMARKS_RPCHOLESKY,
                  "The landmark rule must be LSSVM_LANDMARKS_GREEDY (1) or LSSVM_LANDMARKS_RPCHOLESKY (2), but is " + std::to_string(method) + "!");
    LSSVM_REQUIRE(std::isfinite(tol) && tol >= 0.0, "The tolerance of the landmark selection must be finite and not negative, but is " + std::to_string(tol) + "!");
    LSSVM_REQUIRE(landmarks_out != nullptr, "landmarks_out must not be NULL");
    LSSVM_REQUIRE(num_points == 0 || pool <= num_points, "The candidate pool must not exceed the number of data points (" + std::to_string(num_points) + "), but is " + std::to_string(pool) + "!");
    LSSVM_REQUIRE(pool == 0 || pool >= rank, "The candidate pool (" + std::to_string(pool) + ") must hold at least rank (" + std::to_string(rank) + ") points!");
    const uint64_t candidates = pool > 0 ? pool : num_points;
    const uint64_t most = candidates > 0 ? std::min<uint64_t>(candidates, SELECT_MAX_RANK) : SELECT_MAX_RANK;
    LSSVM_REQUIRE(rank >= 1 && rank <= most, "The number of landmarks to select must lie in [1, " + std::to_string(most) + "], but is " + std::to_string(rank) + "!");
    return static_cast<size_t>(candidates);
}

template <typename T>
void Solver<T>::select_landmarks(uint64_t rank, int method, uint64_t pool, uint64_t seed, double tol, uint64_t *landmarks_out, double *trace_out, double *residual_out,
                                 lssvm_landmark_select_info *info) {
    // ---- everything that needs no device ----
    LSSVM_REQUIRE(shards_.size() == 1 && world_ == 1 && exchange_ == Exchange::none, "landmarks are selected (select_landmarks) on a problem of one device and one rank");
    Problem<T> &p = *shards_[0];
    LSSVM_REQUIRE(!p.weighted_, "landmarks are selected (select_landmarks) for the unweighted kernel matrix: the problem has weights set (lssvm_mi355_problem_set_weights(p, NULL, 0) removes them)");
    LSSVM_REQUIRE(!in_cg_, "select_landmarks cannot run between cg_begin and cg_finish");
    const size_t N = p.N_;
    const size_t n = check_select_arguments(rank, method, pool, tol, landmarks_out, N);
    const int m = static_cast<int>(rank);
    std::vector<int> cand(n);
    if (pool == 0) {
        std::iota(cand.begin(), cand.end(), 0);
    } else {
        const std::vector<uint64_t> shuffled = default_landmarks(N, n);
        for (size_t i = 0; i < n; ++i) cand[i] = static_cast<int>(shuffled[i]);
    }

    const double t0 = now_ms();
    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    const size_t ld = static_cast<size_t>(round_up(static_cast<long>(n), SEL_ROWS));
    const int nblocks = static_cast<int>(ld / SEL_ROWS);
    double gamma = 0.0, coef0 = 0.0;
    LandmarkBlock<T>::kernel_scalars(p, gamma, coef0);

    DevBuf<int> cand_dev, bpos, pivots_dev;
    DevBuf<double> F, d, bsum, bmax, trace_dev;
    DevBuf<SelectState> state;
    cand_dev.alloc_zero(n, st);
    LSSVM_HIP_CHECK(hipMemcpyAsync(cand_dev.p, cand.data(), n * sizeof(int), hipMemcpyHostToDevice, st));
    F.alloc_zero(static_cast<size_t>(m) * ld, st);
    d.alloc_zero(ld, st);
    bsum.alloc_zero(static_cast<size_t>(nblocks), st);
    bmax.alloc_zero(static_cast<size_t>(nblocks), st);
    bpos.alloc_zero(static_cast<size_t>(nblocks), st);
    pivots_dev.alloc_zero(static_cast<size_t>(m), st);
    trace_dev.alloc_zero(static_cast<size_t>(m) + 1, st);
    state.alloc_zero(1, st);
    SelectState first{};
    first.rng = 0x243F6A8885A308D3ull ^ seed;
    first.rank_found = m;
    LSSVM_HIP_CHECK(hipMemcpyAsync(state.p, &first, sizeof(first), hipMemcpyHostToDevice, st));

    const int kt = p.params_.kernel_type, degree = p.params_.degree, ldx = p.X_.ldx, n_i = static_cast<int>(n);
    const T *X = p.X_.data.p;
    hipLaunchKernelGGL(k_select_diag<T>, dim3(nblocks), dim3(SEL_ROWS), 0, st, X, ldx, cand_dev.p, n_i, kt, degree, gamma, coef0, d.p, bsum.p, bmax.p, bpos.p);
    for (int j = 0; j < m; ++j) {  // (no host round trip: a step reads its pivot from device memory)
        hipLaunchKernelGGL(k_select_pivot, dim3(1), dim3(SEL_ROWS), 0, st, d.p, bsum.p, bmax.p, bpos.p, nblocks, j, method, 0, tol, state.p, pivots_dev.p, trace_dev.p);
        hipLaunchKernelGGL(k_select_step<T>, dim3(nblocks), dim3(SEL_ROWS), 0, st, X, ldx, cand_dev.p, n_i, ld, j, kt, degree, gamma, coef0, F.p, d.p, state.p, bsum.p, bmax.p, bpos.p);
    }
    hipLaunchKernelGGL(k_select_pivot, dim3(1), dim3(SEL_ROWS), 0, st, d.p, bsum.p, bmax.p, bpos.p, nblocks, m, method, 1, tol, state.p, pivots_dev.p, trace_dev.p);
    LSSVM_HIP_CHECK(hipGetLastError());

    SelectState end{};
    std::vector<int> pivots(static_cast<size_t>(m));
    std::vector<double> trace(static_cast<size_t>(m) + 1), d_host(residual_out != nullptr ? n : 0);
    LSSVM_HIP_CHECK(hipMemcpyAsync(&end, state.p, sizeof(end), hipMemcpyDeviceToHost, st));
    LSSVM_HIP_CHECK(hipMemcpyAsync(pivots.data(), pivots_dev.p, pivots.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    LSSVM_HIP_CHECK(hipMemcpyAsync(trace.data(), trace_dev.p, trace.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (residual_out != nullptr) LSSVM_HIP_CHECK(hipMemcpyAsync(d_host.data(), d.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (the work space is released on return)

    const int found = end.rank_found;
    for (int j = 0; j < m; ++j) landmarks_out[j] = j < found ? static_cast<uint64_t>(cand[static_cast<size_t>(pivots[static_cast<size_t>(j)])]) : UINT64_MAX;
    if (trace_out != nullptr) {
        for (int j = 0; j < m; ++j) trace_out[j] = trace[static_cast<size_t>(std::min(j + 1, found))];  // (trace[j]: S before step j; at a stop the last sum formed)
    }
    if (residual_out != nullptr) {
        std::fill(residual_out, residual_out + N, std::numeric_limits<double>::quiet_NaN());
        for (size_t i = 0; i < n; ++i) residual_out[cand[i]] = d_host[i];
    }
    if (info != nullptr) {
        lssvm_landmark_select_info out{};
        out.rank_found = static_cast<uint64_t>(found);
        out.candidates = n;
        out.trace0 = trace[0];
        out.trace = end.S;
        out.max_residual = end.dmax;
        out.select_ms = now_ms() - t0;
        out.device_bytes = static_cast<double>((F.count + d.count + bsum.count + bmax.count + trace_dev.count) * sizeof(double) + (cand_dev.count + bpos.count + pivots_dev.count) * sizeof(int) +
                                               sizeof(SelectState));
        *info = out;
    }
}

template void Solver<float>::select_landmarks(uint64_t, int, uint64_t, uint64_t, double, uint64_t *, double *, double *, lssvm_landmark_select_info *);
template void Solver<double>::select_landmarks(uint64_t, int, uint64_t, uint64_t, double, uint64_t *, double *, double *, lssvm_landmark_select_info *);

}  // namespace lssvm
