/*
 * lssvm_logistic.hip -- the fixed-size kernel logistic regression of a resident problem by iteratively reweighted least squares (lssvm_mi355_problem_fit_reduced_logistic,
 * _reduced_logistic_step, lssvm_mi355_fit_reduced_logistic_*).
 *
 * With labels y_i in {-1, +1}, prior weights a_i >= 0 and the cost C the model minimises J(beta, b) = 1/2 beta^T K_mm beta + C sum_i a_i log(1 + exp(-y_i eta_i)),
 * eta_i = Phi_i beta + b, over the m landmark coefficients and an unpenalised intercept.  One Newton step is the weighted fixed-size fit (lssvm_reduced.hip; DESIGN.md
 * section 16) with v_i = a_i max(mu_i, delta) and the working response z_i = eta_i + g_i / max(mu_i, delta): the slab plan, the landmark block, the Gram pass
 * (k_reduced_gram<true> / k_reduced_sum on the m + 2 columns [Phi | 1 | z] with q = sqrt(v) staged into both operands) and the dense steps of either `factor` are the
 * ones of that fit, through lssvm_dense.hip.hpp.  What this file adds: k_reduced_logistic_step, which turns the coefficients of up to four classes into eta, q, z and the
 * loss sums from ONE read of a Phi slab, without an N-sized array ever crossing to the host; and the loop around it, with a step-halving safeguard on J.
 *
 * Determinism: no atomics; eta_i is summed in an order that depends on m only (four column ranges, eight interleaved partial sums each, combined in a fixed tree), so
 * its bits do not depend on the slab size, the row's position, the number of classes or the other classes of a launch; the loss is summed per 64 rows by a fixed
 * butterfly and over the blocks in ascending row order on the host.  Compiled for gfx950 only.
 */
#include "lssvm_dense.hip.hpp"
#include "lssvm_landmark.hip.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <optional>
#include <type_traits>
#include <vector>

namespace lssvm {

namespace {

constexpr int LG_ROWS = 64;         // rows of a slab per workgroup: one per lane
constexpr int LG_WAVES = 4;         // the column ranges of a row's sum: one per wave
constexpr int LG_CLASSES = 4;       // classes per launch
constexpr int LG_UNROLL = 8;        // independent loads (and partial sums) per wave and step
constexpr int LG_PART = 3;          // doubles a workgroup leaves per class: the loss sum, the rows at the floor, max |eta|
constexpr double LG_DELTA = 0x1p-32;  // the floor of the curvature mu
constexpr int LG_MAX_HALVINGS = 30;

/* the classes of one launch: indices into the k classes of the call */
struct LogisticClasses {
    int c[LG_CLASSES];
};

/* column m of the slab: 1 for the rows of points, exact zeros from point N on */
__global__ __launch_bounds__(256) void k_logistic_ones(size_t N, size_t row0, double *__restrict__ out) {
    const size_t local = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    out[local] = row0 + local < N ? 1.0 : 0.0;
}

/* what a row of a class is turned into, from s = y eta and e = exp(-|s|) -- no p (1 - p) is formed from p, nothing cancels */
struct LogisticRow {
    double q, z, loss, mu;
};
__device__ __forceinline__ LogisticRow logistic_row(double y, double a, double eta) {
#pragma clang fp contract(off)
    const double s = y * eta;
    const double e = exp(-fabs(s));
    const double ope = 1.0 + e;
    LogisticRow r;
    r.mu = e / (ope * ope);
    r.loss = fmax(-s, 0.0) + log1p(e);
    const double g = y * (s >= 0.0 ? e / ope : 1.0 / ope);
    const double mf = fmax(r.mu, LG_DELTA);
    r.q = sqrt(a * mf);
    r.z = eta + g / mf;
    return r;
}

/* One workgroup: LG_ROWS rows of the column-major Phi `slab` (ld doubles between two columns; rows padded to 256 with zeros), KC classes.  Wave w sums the columns
 * [w cw, (w + 1) cw), cw = ceil(m / 4), of its lane's row against the betas of every class -- LG_UNROLL independent loads per step, each value of Phi read once and used
 * KC times -- and leaves its partial sums in LDS; wave c then adds the four ranges of class c in ascending order and the intercept, and forms q, z, and the loss.
 * betas: k x m, bias: k (b = -rho), Y: k x N in the problem's type, `a`: the prior weights of the slab's rows (NULL: 1).  q, z, eta: k x ld, indexed like the slab's rows;
 * rows from point N on get q = z = eta = 0.  part[(class * blocks_total + block0 + blockIdx.x) * LG_PART ...]: the workgroup's sum of a_i l_i (a fixed butterfly over the
 * lanes), its number of rows with mu < delta and its max |eta|.  Plain stores, no atomics. */
template <typename T, int KC>
__global__ __launch_bounds__(256) void k_reduced_logistic_step(const double *__restrict__ slab, size_t ld, int m, size_t N, size_t row0, const double *__restrict__ betas,
                                                               const double *__restrict__ bias, const T *__restrict__ Y, const double *__restrict__ a, LogisticClasses cls,
                                                               double *__restrict__ q, double *__restrict__ z, double *__restrict__ eta, double *__restrict__ part, int block0,
                                                               int blocks_total) {
    __shared__ double ps[LG_WAVES][LG_CLASSES][LG_ROWS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t local = static_cast<size_t>(blockIdx.x) * LG_ROWS + lane;

    const int cw = (m + LG_WAVES - 1) / LG_WAVES;
    const int jb = min(wave * cw, m), je = min(jb + cw, m);
    double acc[KC][LG_UNROLL];
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int u = 0; u < LG_UNROLL; ++u) acc[c][u] = 0.0;
    const double *col = slab + local;
    int j0 = jb;
    for (; j0 + LG_UNROLL <= je; j0 += LG_UNROLL) {
        double phi[LG_UNROLL];
#pragma unroll
        for (int u = 0; u < LG_UNROLL; ++u) phi[u] = col[static_cast<size_t>(j0 + u) * ld];
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const double *bc = betas + static_cast<size_t>(cls.c[c]) * m + j0;
#pragma unroll
            for (int u = 0; u < LG_UNROLL; ++u) acc[c][u] = fma(phi[u], bc[u], acc[c][u]);
        }
    }
    if (j0 < je) {  // the tail of the range: the same partial sums, the columns past it left out
        double phi[LG_UNROLL];
#pragma unroll
        for (int u = 0; u < LG_UNROLL; ++u) phi[u] = j0 + u < je ? col[static_cast<size_t>(j0 + u) * ld] : 0.0;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const double *bc = betas + static_cast<size_t>(cls.c[c]) * m;
#pragma unroll
            for (int u = 0; u < LG_UNROLL; ++u)
                if (j0 + u < je) acc[c][u] = fma(phi[u], bc[j0 + u], acc[c][u]);
        }
    }
#pragma unroll
    for (int c = 0; c < KC; ++c)
        ps[wave][c][lane] = ((acc[c][0] + acc[c][1]) + (acc[c][2] + acc[c][3])) + ((acc[c][4] + acc[c][5]) + (acc[c][6] + acc[c][7]));
    __syncthreads();
    if (wave >= KC) return;

    const int cc = wave == 0 ? cls.c[0] : (wave == 1 ? cls.c[1] : (wave == 2 ? cls.c[2] : cls.c[3]));  // (no indexed read of the argument: that would be scratch)
    const size_t i = row0 + local;
    const bool in = i < N;
    const double e_lin = ((ps[0][wave][lane] + ps[1][wave][lane]) + (ps[2][wave][lane] + ps[3][wave][lane])) + bias[cc];
    const double eta_v = in ? e_lin : 0.0;
    const double y = in ? static_cast<double>(Y[static_cast<size_t>(cc) * N + i]) : 1.0;
    const double a_v = in ? (a != nullptr ? a[local] : 1.0) : 0.0;
    const LogisticRow r = logistic_row(y, a_v, eta_v);
    const size_t at = static_cast<size_t>(cc) * ld + local;
    q[at] = in ? r.q : 0.0;
    z[at] = in ? r.z : 0.0;
    eta[at] = eta_v;

    double loss = in ? a_v * r.loss : 0.0;
    double floored = in && r.mu < LG_DELTA ? 1.0 : 0.0;
    double big = fabs(eta_v);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        loss += __shfl_xor(loss, d);
        floored += __shfl_xor(floored, d);
        big = fmax(big, __shfl_xor(big, d));
    }
    if (lane == 0) {
        double *out = part + (static_cast<size_t>(cc) * blocks_total + block0 + blockIdx.x) * LG_PART;
        out[0] = loss;
        out[1] = floored;
        out[2] = big;
    }
}

template <typename T>
void enqueue_step(int kc, const double *slab, size_t ld, int m, size_t N, size_t row0, int rows256, const double *betas, const double *bias, const T *Y, const double *a,
                  const LogisticClasses &cls, double *q, double *z, double *eta, double *part, int block0, int blocks_total, hipStream_t st) {
    const dim3 grid(rows256 / LG_ROWS), block(256);
    switch (kc) {
        case 1: hipLaunchKernelGGL((k_reduced_logistic_step<T, 1>), grid, block, 0, st, slab, ld, m, N, row0, betas, bias, Y, a, cls, q, z, eta, part, block0, blocks_total); break;
        case 2: hipLaunchKernelGGL((k_reduced_logistic_step<T, 2>), grid, block, 0, st, slab, ld, m, N, row0, betas, bias, Y, a, cls, q, z, eta, part, block0, blocks_total); break;
        case 3: hipLaunchKernelGGL((k_reduced_logistic_step<T, 3>), grid, block, 0, st, slab, ld, m, N, row0, betas, bias, Y, a, cls, q, z, eta, part, block0, blocks_total); break;
        default: hipLaunchKernelGGL((k_reduced_logistic_step<T, 4>), grid, block, 0, st, slab, ld, m, N, row0, betas, bias, Y, a, cls, q, z, eta, part, block0, blocks_total); break;
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}

/* What the passes of a call work on: the landmarks, the labels and the prior weights on the device once; one slab of m + 2 columns, q, z and eta of k classes for it
 * (3 k ld doubles), the Gram pass's partial tiles, St per class, K_mm, the coefficients and the workgroups' partial sums. */
template <typename T>
struct LogisticWork {
    const SlabPlan plan;
    const int m, k, cols, ntri, max_chunks, blocks_total;
    hipStream_t st;
    const LandmarkBlock<T> block;
    DevBuf<T> Y;
    DevBuf<double> a, slab, q, z, eta, part, St, Kmm, betas, bias, sums;
    std::vector<double> betas_host, bias_host, sums_host;
    std::vector<Event> ev;  // four per slab: before Phi, behind it, behind the step kernel, behind the Gram passes
    double landmark_ms = 0.0, step_ms = 0.0, gram_ms = 0.0;  // of the last walk

    LogisticWork(Problem<T> &problem, size_t num_points, const std::vector<uint64_t> &lm, const void *Y_host, int num_rhs, const double *weights, uint64_t slab_rows, bool with_gram,
                 hipStream_t stream) :
        plan(num_points, slab_rows), m(static_cast<int>(lm.size())), k(num_rhs), cols(m + 2), ntri(tiles_of(cols) * (tiles_of(cols) + 1) / 2),
        max_chunks(static_cast<int>((plan.ld + RG_RANGE - 1) / RG_RANGE)), blocks_total(static_cast<int>(static_cast<size_t>(plan.slabs) * plan.ld / LG_ROWS)), st(stream),
        block(problem, lm, stream), betas_host(static_cast<size_t>(k) * m), bias_host(static_cast<size_t>(k)), sums_host(static_cast<size_t>(k) * blocks_total * LG_PART),
        ev(static_cast<size_t>(4) * plan.slabs) {
        const size_t N = plan.N, ld = plan.ld;
        Y.alloc_zero(static_cast<size_t>(k) * N, st);
        LSSVM_HIP_CHECK(hipMemcpyAsync(Y.p, Y_host, static_cast<size_t>(k) * N * sizeof(T), hipMemcpyHostToDevice, st));
        if (weights != nullptr) {  // behind each other as the slabs' rows are, zeros from row N on
            a.alloc_zero(static_cast<size_t>(plan.slabs) * ld, st);
            LSSVM_HIP_CHECK(hipMemcpyAsync(a.p, weights, N * sizeof(double), hipMemcpyHostToDevice, st));
        }
        slab.alloc_zero(static_cast<size_t>(cols) * ld, st);
        q.alloc_zero(static_cast<size_t>(k) * ld, st);
        z.alloc_zero(static_cast<size_t>(k) * ld, st);
        eta.alloc_zero(static_cast<size_t>(k) * ld, st);
        betas.alloc_zero(betas_host.size(), st);
        bias.alloc_zero(bias_host.size(), st);
        sums.alloc_zero(sums_host.size(), st);
        if (with_gram) {
            part.alloc_zero(static_cast<size_t>(ntri) * max_chunks * RG_TILE, st);
            St.alloc_zero(static_cast<size_t>(k) * ntri * RG_TILE, st);
            Kmm.alloc_zero(static_cast<size_t>(m) * m, st);
        }
        for (Event &e : ev) e.create(true);
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (the caller's arrays have been read)
    }
    size_t device_bytes() const {
        return (a.count + slab.count + q.count + z.count + eta.count + part.count + St.count + Kmm.count + betas.count + bias.count + sums.count) * sizeof(double) + Y.count * sizeof(T) +
               block.device_bytes();
    }
    double *St_of(int c) const { return St.p + static_cast<size_t>(c) * ntri * RG_TILE; }

    /* One walk over the slabs at the coefficients in betas_host / bias_host for the classes `active` (ascending): Phi once per slab, the step kernel per group of up to
     * LG_CLASSES classes, then `per_slab(s)` -- everything enqueued, nothing waited for here.  gather_kmm: K_mm is picked out of the slabs on the way. */
    template <typename PerSlab>
    void walk(const std::vector<int> &active, bool gather_kmm, PerSlab per_slab) {
        LSSVM_HIP_CHECK(hipMemcpyAsync(betas.p, betas_host.data(), betas_host.size() * sizeof(double), hipMemcpyHostToDevice, st));
        LSSVM_HIP_CHECK(hipMemcpyAsync(bias.p, bias_host.data(), bias_host.size() * sizeof(double), hipMemcpyHostToDevice, st));
        const size_t ld = plan.ld;
        for (int s = 0; s < plan.slabs; ++s) {
            const size_t row0 = plan.row0(s);
            const int rows256 = plan.rows256(s);
            Event *e = &ev[static_cast<size_t>(4) * s];
            LSSVM_HIP_CHECK(hipEventRecord(e[0].e, st));
            block.enqueue(row0, rows256, slab.p, ld);
            if (gather_kmm) block.enqueue_gather_kmm(slab.p, ld, row0, plan.rows(s), Kmm.p);
            hipLaunchKernelGGL(k_logistic_ones, dim3(rows256 / 256), dim3(256), 0, st, plan.N, row0, slab.p + static_cast<size_t>(m) * ld);
            LSSVM_HIP_CHECK(hipGetLastError());
            LSSVM_HIP_CHECK(hipEventRecord(e[1].e, st));
            for (size_t g = 0; g < active.size(); g += LG_CLASSES) {
                const int kc = static_cast<int>(std::min<size_t>(LG_CLASSES, active.size() - g));
                LogisticClasses cls{};
                for (int c = 0; c < kc; ++c) cls.c[c] = active[g + c];
                enqueue_step<T>(kc, slab.p, ld, m, plan.N, row0, rows256, betas.p, bias.p, Y.p, a.p != nullptr ? a.p + row0 : nullptr, cls, q.p, z.p, eta.p, sums.p,
                                static_cast<int>(row0 / LG_ROWS), blocks_total, st);
            }
            LSSVM_HIP_CHECK(hipEventRecord(e[2].e, st));
            per_slab(s);
            LSSVM_HIP_CHECK(hipEventRecord(e[3].e, st));
        }
    }
    /* behind a wait for the stream: the device times of the walk */
    void read_times() {
        landmark_ms = step_ms = gram_ms = 0.0;
        for (int s = 0; s < plan.slabs; ++s) {
            const Event *e = &ev[static_cast<size_t>(4) * s];
            landmark_ms += elapsed_ms(e[0], e[1]);
            step_ms += elapsed_ms(e[1], e[2]);
            gram_ms += elapsed_ms(e[2], e[3]);
        }
    }
    /* the workgroups' sums of class c from sums_host, added in ascending row order: the loss sum, the rows at the floor, max |eta|.  (The blocks of the last slab
     * that no workgroup writes keep the zeros they were allocated with.) */
    void reduce_sums(int c, double &loss, uint64_t &floored, double &max_abs_eta) const {
        loss = 0.0;
        double fl = 0.0;
        max_abs_eta = 0.0;
        for (size_t b = 0; b < static_cast<size_t>(blocks_total); ++b) {
            const double *v = &sums_host[(static_cast<size_t>(c) * blocks_total + b) * LG_PART];
            loss += v[0];
            fl += v[1];
            max_abs_eta = std::max(max_abs_eta, v[2]);
        }
        floored = static_cast<uint64_t>(fl);
    }
};

/* 1/2 beta^T K_mm beta, every sum in index order */
double penalty_of(const std::vector<double> &Kmm, const double *beta, int m) {
    double total = 0.0;
    for (int j = 0; j < m; ++j) {
        double row = 0.0;
        for (int l = 0; l < m; ++l) row += Kmm[static_cast<size_t>(j) * m + l] * beta[l];
        total += beta[j] * row;
    }
    return 0.5 * total;
}

/* one class of the loop (include/plssvm_amd.h has its rules) */
struct ClassState {
    std::vector<double> cur, acc;  // m betas and rho: the iterate of the next pass, the last accepted one
    double J_acc = 0.0;
    bool have_acc = false, active = true;
    int consecutive = 0;
    lssvm_reduced_logistic_info info{};
};

}  // namespace

void check_reduced_logistic_arguments(double tol, uint64_t max_iter, const double *betas0, const double *rhos0, size_t num_rhs, uint64_t rank) {
    LSSVM_REQUIRE(std::isfinite(tol) && tol > 0.0, "tol must be finite and greater than 0, but is " + std::to_string(tol) + "!");
    LSSVM_REQUIRE(max_iter >= 1, "max_iter must be greater than 0!");
    LSSVM_REQUIRE((betas0 == nullptr) == (rhos0 == nullptr), "The start values betas0 and rhos0 must both be given or both be NULL!");
    if (betas0 == nullptr) return;
    for (size_t e = 0; e < num_rhs * rank; ++e) LSSVM_REQUIRE(std::isfinite(betas0[e]), "Every start value must be finite, but betas0[" + std::to_string(e) + "] is not!");
    for (size_t c = 0; c < num_rhs; ++c) LSSVM_REQUIRE(std::isfinite(rhos0[c]), "Every start value must be finite, but rhos0[" + std::to_string(c) + "] is not!");
}

void check_reduced_logistic_labels(const void *Y, int dtype, size_t num_rhs, size_t num_points) {
    for (size_t e = 0; e < num_rhs * num_points; ++e) {
        const double y = dtype == LSSVM_DTYPE_F32 ? static_cast<double>(static_cast<const float *>(Y)[e]) : static_cast<const double *>(Y)[e];
        LSSVM_REQUIRE(y == 1.0 || y == -1.0, "Every label of the logistic model must be exactly -1 or +1, but label " + std::to_string(e % num_points) + " of class " +
                                                 std::to_string(e / num_points) + " is " + std::to_string(y) + "!");
    }
}

namespace {

/* the checks of both entry points that need no device, in the order of the weighted fit; returns the landmarks */
template <typename T>
std::vector<uint64_t> check_logistic_call(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, size_t N) {
    check_reduced_arguments(Y, num_rhs, rank, slab_rows, N);
    LSSVM_REQUIRE(num_rhs <= 4096, "at most 4096 right hand sides per call");
    std::vector<uint64_t> lm = resolve_landmarks(landmarks, static_cast<size_t>(rank), N);
    if (weights != nullptr) (void) check_reduced_weights(weights, N);
    check_reduced_logistic_labels(Y, std::is_same_v<T, float> ? LSSVM_DTYPE_F32 : LSSVM_DTYPE_F64, num_rhs, N);
    return lm;
}

}  // namespace

template <typename T>
void Solver<T>::fit_reduced_logistic(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, int factor, double tol,
                                     uint64_t max_iter, const double *betas0, const double *rhos0, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                                     lssvm_reduced_logistic_info *infos) {
    // ---- everything that needs no device ----
    Problem<T> &p = reduced_problem("fit_reduced_logistic", true);
    const size_t N = p.N_;
    LSSVM_REQUIRE(betas_out != nullptr && rhos_out != nullptr, "betas_out / rhos_out must not be NULL");
    const std::vector<uint64_t> lm = check_logistic_call<T>(Y, num_rhs, weights, rank, landmarks, slab_rows, N);
    check_reduced_factor(factor);
    check_reduced_logistic_arguments(tol, max_iter, betas0, rhos0, num_rhs, rank);

    const double t0 = now_ms();
    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    const int m = static_cast<int>(rank), k = static_cast<int>(num_rhs);
    const double cost = p.params_.cost, sigma = 1.0 / cost;
    LogisticWork<T> w(p, N, lm, Y, k, weights, slab_rows, true, st);
    const int cols = w.cols;
    const size_t tile_doubles = static_cast<size_t>(w.ntri) * RG_TILE;

    std::vector<ClassState> cls(static_cast<size_t>(k));
    for (int c = 0; c < k; ++c) {
        cls[c].cur.assign(static_cast<size_t>(m) + 1, 0.0);
        if (betas0 != nullptr) {
            std::copy(betas0 + static_cast<size_t>(c) * m, betas0 + static_cast<size_t>(c + 1) * m, cls[c].cur.begin());
            cls[c].cur[m] = rhos0[c];
        }
        cls[c].acc = cls[c].cur;
    }
    std::vector<std::vector<double>> tiles(static_cast<size_t>(k), std::vector<double>(tile_doubles));
    std::vector<double> Kmm(static_cast<size_t>(m) * m), G, L, next(static_cast<size_t>(m) + 1);
    ReducedOnDevice dev;                    // factor 1: the class's St and K_mm where they lie (borrowed for the call of DenseFit::run, handed back behind it)
    std::optional<DenseFit> dense;
    if (factor == 1) dense.emplace(m, 1, st);
    auto finish = [&](int c, const std::vector<double> &result, double objective, bool converged) {
        std::copy(result.begin(), result.begin() + m, betas_out + static_cast<size_t>(c) * m);
        rhos_out[c] = result[m];
        cls[c].info.objective = objective;
        cls[c].info.converged = converged ? 1 : 0;
        cls[c].active = false;
    };

    for (uint64_t pass = 0;; ++pass) {
        std::vector<int> active;
        for (int c = 0; c < k; ++c)
            if (cls[c].active) active.push_back(c);
        if (active.empty()) break;
        for (const int c : active) {  // the iterate of this pass: b = -rho
            std::copy(cls[c].cur.begin(), cls[c].cur.begin() + m, w.betas_host.begin() + static_cast<size_t>(c) * m);
            w.bias_host[c] = -cls[c].cur[m];
            LSSVM_HIP_CHECK(hipMemsetAsync(w.St_of(c), 0, tile_doubles * sizeof(double), st));
        }
        w.walk(active, pass == 0, [&](int s) {
            for (const int c : active) {  // z_c into the slab's last column, q_c as the Gram pass's sqrt(w)
                LSSVM_HIP_CHECK(hipMemcpyAsync(w.slab.p + static_cast<size_t>(m + 1) * w.plan.ld, w.z.p + static_cast<size_t>(c) * w.plan.ld,
                                               static_cast<size_t>(w.plan.rows256(s)) * sizeof(double), hipMemcpyDeviceToDevice, st));
                enqueue_gram(w.slab.p, w.plan.ld, cols, w.plan.rows256(s), w.max_chunks, w.part.p, w.St_of(c), st, w.q.p + static_cast<size_t>(c) * w.plan.ld);
            }
        });
        for (const int c : active)
            LSSVM_HIP_CHECK(hipMemcpyAsync(tiles[c].data(), w.St_of(c), tile_doubles * sizeof(double), hipMemcpyDeviceToHost, st));
        LSSVM_HIP_CHECK(hipMemcpyAsync(w.sums_host.data(), w.sums.p, w.sums_host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        if (pass == 0) LSSVM_HIP_CHECK(hipMemcpyAsync(Kmm.data(), w.Kmm.p, Kmm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // the one wait of the pass
        w.read_times();

        for (const int c : active) {
            const double t_host = now_ms();
            ClassState &s = cls[c];
            lssvm_reduced_logistic_info &info = s.info;
            info.passes += 1;
            info.landmark_ms += w.landmark_ms;
            info.step_ms += w.step_ms;
            info.gram_ms += w.gram_ms;
            double loss = 0.0;
            w.reduce_sums(c, loss, info.floored, info.max_abs_eta);
            const double J = penalty_of(Kmm, s.cur.data(), m) + cost * loss;
            const bool last = info.passes >= max_iter;
            bool solve = true;
            if (s.have_acc) {
                const double decrease = s.J_acc - J;
                info.last_decrease = decrease;
                if (!(decrease >= -tol * s.J_acc)) {  // rejected (a J that is not finite as well): halfway back to the last accepted iterate
                    info.halvings += 1;
                    s.consecutive += 1;
                    if (s.consecutive >= LG_MAX_HALVINGS || last) {
                        finish(c, s.acc, s.J_acc, false);
                    } else {
                        for (int j = 0; j <= m; ++j) s.cur[j] = 0.5 * (s.cur[j] + s.acc[j]);
                    }
                    solve = false;
                } else if (std::fabs(decrease) <= tol * s.J_acc) {  // converged: the iterate of the smaller J -- the newer one unless it is worse beyond the rounding of both sums
                    if (J - s.J_acc <= 2.0 * (static_cast<double>(N) + 16.0) * DBL_EPSILON * s.J_acc) {
                        finish(c, s.cur, J, true);
                    } else {
                        finish(c, s.acc, s.J_acc, true);
                    }
                    solve = false;
                }
            }
            if (solve) {  // accepted: the next iterate from this pass's sums
                s.acc = s.cur;
                s.J_acc = J;
                s.have_acc = true;
                s.consecutive = 0;
                unpack_tiles(tiles[c], cols, G);
                const double W = G[static_cast<size_t>(m) * cols + m];  // the Gram pass's own sum of v
                if (factor == 1) {
                    dev.St.p = w.St_of(c);
                    dev.Kmm.p = w.Kmm.p;
                    try {
                        info.jitter = dense->run(dev, G, Kmm, cols, W, sigma, nullptr, 0, next.data(), &next[m], nullptr, nullptr);
                    } catch (...) {
                        dev.St.p = dev.Kmm.p = nullptr;
                        throw;
                    }
                    dev.St.p = dev.Kmm.p = nullptr;
                } else {
                    info.jitter = factor_reduced(G, Kmm, m, cols, W, sigma, L);
                    solve_reduced(G, L, m, 1, cols, W, next.data(), &next[m]);
                }
                s.cur = next;
                if (last) finish(c, s.cur, s.J_acc, false);
            }
            info.host_ms += now_ms() - t_host;
        }
    }
    if (landmarks_out != nullptr) std::copy(lm.begin(), lm.end(), landmarks_out);
    if (infos != nullptr) {
        const double total = now_ms() - t0;
        for (int c = 0; c < k; ++c) {
            cls[c].info.total_ms = total;
            infos[c] = cls[c].info;
        }
    }
}

template <typename T>
void Solver<T>::reduced_logistic_step(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *betas,
                                      const double *rhos, double *eta_out, double *q_out, double *z_out, double *loss_out, uint64_t *floored_out) {
    Problem<T> &p = reduced_problem("reduced_logistic_step", true);
    const size_t N = p.N_;
    LSSVM_REQUIRE(betas != nullptr && rhos != nullptr, "betas / rhos must not be NULL");
    LSSVM_REQUIRE(eta_out != nullptr && q_out != nullptr && z_out != nullptr && loss_out != nullptr, "eta_out / q_out / z_out / loss_out must not be NULL");
    const std::vector<uint64_t> lm = check_logistic_call<T>(Y, num_rhs, weights, rank, landmarks, slab_rows, N);
    check_reduced_logistic_arguments(1.0, 1, betas, rhos, num_rhs, rank);

    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    const int m = static_cast<int>(rank), k = static_cast<int>(num_rhs);
    LogisticWork<T> w(p, N, lm, Y, k, weights, slab_rows, false, st);
    std::copy(betas, betas + static_cast<size_t>(k) * m, w.betas_host.begin());
    for (int c = 0; c < k; ++c) w.bias_host[c] = -rhos[c];
    std::vector<int> all(static_cast<size_t>(k));
    for (int c = 0; c < k; ++c) all[c] = c;
    w.walk(all, false, [&](int s) {
        const size_t row0 = w.plan.row0(s), bytes = static_cast<size_t>(w.plan.rows(s)) * sizeof(double);
        for (int c = 0; c < k; ++c) {
            const size_t from = static_cast<size_t>(c) * w.plan.ld, to = static_cast<size_t>(c) * N + row0;
            LSSVM_HIP_CHECK(hipMemcpyAsync(eta_out + to, w.eta.p + from, bytes, hipMemcpyDeviceToHost, st));
            LSSVM_HIP_CHECK(hipMemcpyAsync(q_out + to, w.q.p + from, bytes, hipMemcpyDeviceToHost, st));
            LSSVM_HIP_CHECK(hipMemcpyAsync(z_out + to, w.z.p + from, bytes, hipMemcpyDeviceToHost, st));
        }
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (the next slab overwrites them)
    });
    LSSVM_HIP_CHECK(hipMemcpyAsync(w.sums_host.data(), w.sums.p, w.sums_host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    for (int c = 0; c < k; ++c) {
        uint64_t floored = 0;
        double big = 0.0;
        w.reduce_sums(c, loss_out[c], floored, big);
        if (floored_out != nullptr) floored_out[c] = floored;
    }
}

template void Solver<float>::fit_reduced_logistic(const void *, size_t, const double *, uint64_t, const uint64_t *, uint64_t, int, double, uint64_t, const double *, const double *, double *,
                                                  double *, uint64_t *, lssvm_reduced_logistic_info *);
template void Solver<double>::fit_reduced_logistic(const void *, size_t, const double *, uint64_t, const uint64_t *, uint64_t, int, double, uint64_t, const double *, const double *, double *,
                                                   double *, uint64_t *, lssvm_reduced_logistic_info *);
template void Solver<float>::reduced_logistic_step(const void *, size_t, const double *, uint64_t, const uint64_t *, uint64_t, const double *, const double *, double *, double *, double *,
                                                   double *, uint64_t *);
template void Solver<double>::reduced_logistic_step(const void *, size_t, const double *, uint64_t, const uint64_t *, uint64_t, const double *, const double *, double *, double *, double *,
                                                    double *, uint64_t *);

}  // namespace lssvm
