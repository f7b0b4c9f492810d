/*
 * lssvm_path.hip -- the cost path (lssvm_mi355_problem_solve_cost_path, lssvm_mi355_solve_cost_path_*): the solutions of one right-hand side for
 * every cost of a grid from ONE multi-shift CG sequence.  With sigma = 1 / C the reduced matrix is Abar(sigma) = A0 + sigma M, A0 v = K v + (k_ll S - q.v) 1 - S q
 * (S = sum v) and M = I + 1 1^T; with P = M^(-1/2) = I - theta 1 1^T the systems (B + sigma_s I) z_s = P b, B = P A0 P, differ by a shift only and share the Krylov
 * space of the seed sigma_0 = min sigma_s.  CG runs on the seed from z = 0 with ONE pass of the problem's own single-vector Gram kernel per iteration
 * (enqueue_apply_K_local: every kernel family, fp32 and fp64); every other shift follows by the scalar recurrences of k_path_scalars and the two vector updates of
 * k_path_update.  The rank-1 terms of P and A0, every reduction (RED_BLOCKS partial sums in fixed order, double accumulators) and every scalar stay on the device; the
 * host reads one mapped word per iteration, the number of shifts still active.
 *
 * THE STOP TEST IS NOT THE REFERENCE RECIPE'S.  cg_begin / cg_step start from x0 = 1 and stop at |r|^2 <= eps^2 |b - A 1|^2 in the 2-norm.  The path starts from
 * x0 = 0 and freezes shift s at zeta_s^2 |r|^2 <= eps^2 |P b|^2: the residual of cost s in the norm of M^-1, relative to the right-hand side in that norm.
 *
 * The kernels launched here are the path's own (below); the Gram pass is launched, not changed -- the verification's too (enqueue_apply_K_lanes where the two-vector
 * kernel applies: the same walk over the row-block bands, Problem::enqueue_sym_walk, so a verified residual is that of the pass the iteration ran).  Compiled for gfx950 only.
 */
#include "lssvm_problem.hip.hpp"

#include "lssvm_kernels.hip.hpp"

#include <algorithm>
#include <cmath>

namespace lssvm {

namespace {

constexpr int PATH_SHIFTS = static_cast<int>(PATH_MAX_COSTS);
/* the partial sums of the path's reductions: RED_BLOCKS x 4 doubles per set -- a kernel finishes its predecessor's set while its own blocks write another */
enum PathPart : int { PP_P = 0, PP_U = 1, PP_T = 2, PP_RR = 3, PP_SETS = 4 };
/* the device-resident scalars of the seed's CG (all double) */
enum PathScalar : int { PS_RR = 0, PS_RR0 = 1, PS_A = 2, PS_A_OLD = 3, PS_BETA = 4, PS_BETA_OLD = 5, PS_SP = 6, PS_PW = 7, PS_COUNT = 8 };
/* the state of the shifts: what k_path_scalars keeps and k_path_update reads */
struct PathShifts {
    double delta[PATH_SHIFTS];     // sigma_s - sigma_0 >= 0
    double zeta[PATH_SHIFTS], zeta_old[PATH_SHIFTS];
    double a_s[PATH_SHIFTS], b_s[PATH_SHIFTS], zeta_new[PATH_SHIFTS];  // of the iteration in flight
    double res[PATH_SHIFTS];       // zeta_s^2 r^T r when the shift froze
    unsigned long long iterations[PATH_SHIFTS];  // ... and the iteration at which it did
    int active[PATH_SHIFTS];       // not frozen yet
    int update[PATH_SHIFTS];       // active when the iteration in flight began: k_path_update moves its x_s and p_s
};

/* NV sums a PREVIOUS kernel left as RED_BLOCKS x 4 partials, reduced by every block for itself in block_reduce's fixed tree order (finish2_in_block's scheme) */
template <int NV>
__device__ __forceinline__ void path_finish_in_block(const double *__restrict__ part, double *lds /* [NV * 4] */, double *tot /* [NV] */, double (&out)[NV]) {
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = part[threadIdx.x * 4 + k];
    block_reduce<NV>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) tot[k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) out[k] = tot[k];
}
template <int NV>
__device__ __forceinline__ void path_store_partials(double (&acc)[NV], double *lds, double *__restrict__ part) {
    block_reduce<NV>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) part[blockIdx.x * 4 + k] = acc[k];
#pragma unroll
        for (int k = NV; k < 4; ++k) part[blockIdx.x * 4 + k] = 0.0;
    }
}

/* part = (sum v, q.v) */
template <typename T>
__global__ __launch_bounds__(RED_THREADS) void k_path_sums(const T *__restrict__ v, const T *__restrict__ q, int n, double *__restrict__ part) {
    __shared__ double lds[8];
    double acc[2] = { 0.0, 0.0 };
    for (int i = blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += RED_BLOCKS * RED_THREADS) {
        const double vi = static_cast<double>(v[i]);
        acc[0] += vi;
        acc[1] += vi * static_cast<double>(q[i]);
    }
    path_store_partials<2>(acc, lds, part);
}

/* r = p = p_s = P b = b - theta sum(b) for every shift (x_s = 0 from the allocation); part_rr = (r.r, 0), part_p = (0, sum p) */
template <typename T>
__global__ __launch_bounds__(RED_THREADS) void k_path_begin(const T *__restrict__ b, const double *__restrict__ part_b, double theta, int n, int m, size_t stride, T *__restrict__ r,
                                                            T *__restrict__ p, T *__restrict__ ps, double *__restrict__ part_rr, double *__restrict__ part_p) {
    __shared__ double lds[8];
    __shared__ double tot[2];
    double sb[2];
    path_finish_in_block<2>(part_b, lds, tot, sb);
    double acc[2] = { 0.0, 0.0 };
    for (int i = blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += RED_BLOCKS * RED_THREADS) {
        const T ri = static_cast<T>(static_cast<double>(b[i]) - theta * sb[0]);
        r[i] = ri;
        p[i] = ri;
        for (int s = 0; s < m; ++s) ps[static_cast<size_t>(s) * stride + i] = ri;
        acc[0] += static_cast<double>(ri) * static_cast<double>(ri);
        acc[1] += static_cast<double>(ri);
    }
    block_reduce<2>(acc, lds);
    if (threadIdx.x == 0) {
        part_rr[blockIdx.x * 4 + 0] = acc[0];
        part_rr[blockIdx.x * 4 + 1] = 0.0;
        part_p[blockIdx.x * 4 + 0] = 0.0;
        part_p[blockIdx.x * 4 + 1] = acc[1];
    }
}

/* u = P p = p - theta sum(p): the vector the Gram pass multiplies; part = (sum u, q.u), the rank-1 terms of A0 u */
template <typename T>
__global__ __launch_bounds__(RED_THREADS) void k_path_make_u(const T *__restrict__ p, const double *__restrict__ part_p, double theta, const T *__restrict__ q, int n, T *__restrict__ u,
                                                             double *__restrict__ sc, double *__restrict__ part) {
    __shared__ double lds[8];
    __shared__ double tot[2];
    double sp[2];
    path_finish_in_block<2>(part_p, lds, tot, sp);
    if (blockIdx.x == 0 && threadIdx.x == 0) sc[PS_SP] = sp[1];
    double acc[2] = { 0.0, 0.0 };
    for (int i = blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += RED_BLOCKS * RED_THREADS) {
        const T ui = static_cast<T>(static_cast<double>(p[i]) - theta * sp[1]);
        u[i] = ui;
        acc[0] += static_cast<double>(ui);
        acc[1] += static_cast<double>(ui) * static_cast<double>(q[i]);
    }
    path_store_partials<2>(acc, lds, part);
}

/* t = A0 u = K u + (k_ll S - q.u) 1 - S q with S = sum u, evaluated in double; part = (sum t, p.t, p.p): what w = P t + sigma_0 p and p.w need */
template <typename T>
__global__ __launch_bounds__(RED_THREADS) void k_path_t(const T *__restrict__ Ku, const T *__restrict__ p, const T *__restrict__ q, const double *__restrict__ part_u, double k_ll, int n,
                                                        T *__restrict__ t, double *__restrict__ part) {
    __shared__ double lds[12];
    __shared__ double tot[2];
    double su[2];
    path_finish_in_block<2>(part_u, lds, tot, su);
    const double shift = k_ll * su[0] - su[1];
    double acc[3] = { 0.0, 0.0, 0.0 };
    for (int i = blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += RED_BLOCKS * RED_THREADS) {
        const T ti = static_cast<T>(static_cast<double>(Ku[i]) + shift - su[0] * static_cast<double>(q[i]));
        t[i] = ti;
        const double pi = static_cast<double>(p[i]);
        acc[0] += static_cast<double>(ti);
        acc[1] += pi * static_cast<double>(ti);
        acc[2] += pi * pi;
    }
    path_store_partials<3>(acc, lds, part);
}

/* a = r.r / p.w with p.w = p.t - theta sum(t) sum(p) + sigma_0 p.p ; r -= a w, w = t - theta sum(t) + sigma_0 p ; part = (r.r, 0).  The scalar is rounded to T
 * first, as k_update_x_r rounds alpha_cd */
template <typename T>
__global__ __launch_bounds__(RED_THREADS) void k_path_update_r(const T *__restrict__ t, const T *__restrict__ p, T *__restrict__ r, const double *__restrict__ part_t,
                                                               double *__restrict__ sc, double theta, double sigma0, int n, double *__restrict__ part) {
    __shared__ double lds[12];
    __shared__ double tot[3];
    double st[3];
    path_finish_in_block<3>(part_t, lds, tot, st);
    const double pw = st[1] - theta * st[0] * sc[PS_SP] + sigma0 * st[2];
    const double a = sc[PS_RR] / pw;
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // (slots no block reads in this kernel)
        sc[PS_PW] = pw;
        sc[PS_A] = a;
    }
    const T aT = static_cast<T>(a);
    double acc[2] = { 0.0, 0.0 };
    for (int i = blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += RED_BLOCKS * RED_THREADS) {
        const T wi = static_cast<T>(static_cast<double>(t[i]) - theta * st[0] + sigma0 * static_cast<double>(p[i]));
        const T ri = r[i] - aT * wi;
        r[i] = ri;
        acc[0] += static_cast<double>(ri) * static_cast<double>(ri);
    }
    path_store_partials<2>(acc, lds, part);
}

/* ONE block: r.r of the iteration, beta, and per shift (thread s) zeta_new, a_s, beta_s and the freeze flag; the number of shifts still active goes to the host's
 * mapped word.  `initial`: the state before the first iteration (zeta = zeta_old = 1, a_old = 1, beta_old = 0, r.r = |P b|^2) */
__global__ __launch_bounds__(RED_THREADS) void k_path_scalars(const double *__restrict__ part_rr, double *__restrict__ sc, PathShifts *__restrict__ sh, int m, double eps2,
                                                              int initial, unsigned long long iteration, int *__restrict__ host_active) {
    __shared__ double lds[8];
    __shared__ double tot[2];
    __shared__ int still[PATH_SHIFTS];
    double rr[2];
    path_finish_in_block<2>(part_rr, lds, tot, rr);
    const double rr_new = rr[0];
    const double rr_old = initial ? rr_new : sc[PS_RR];
    const double rr0 = initial ? rr_new : sc[PS_RR0];
    const double a = initial ? 1.0 : sc[PS_A];
    const double a_old = sc[PS_A_OLD], beta_old = sc[PS_BETA_OLD];
    const double beta = initial ? 0.0 : rr_new / rr_old;
    const int s = threadIdx.x;
    if (s < m) {
        if (initial) {
            sh->zeta[s] = sh->zeta_old[s] = sh->zeta_new[s] = 1.0;
            sh->a_s[s] = sh->b_s[s] = 0.0;
            sh->update[s] = 0;
            const bool frozen = rr_new <= eps2 * rr0;  // (a zero right-hand side: x = 0 is the solution)
            sh->active[s] = frozen ? 0 : 1;
            sh->iterations[s] = 0;
            sh->res[s] = rr_new;
        } else if (sh->active[s] != 0) {
            const double z = sh->zeta[s], zo = sh->zeta_old[s];
            const double zn = z * zo * a_old / (a * beta_old * (zo - z) + zo * a_old * (1.0 + a * sh->delta[s]));
            const double ratio = zn / z;
            sh->zeta_new[s] = zn;
            sh->a_s[s] = a * ratio;
            sh->b_s[s] = beta * ratio * ratio;
            sh->zeta_old[s] = z;
            sh->zeta[s] = zn;
            sh->update[s] = 1;
            const double res = zn * zn * rr_new;
            if (res <= eps2 * rr0) {
                sh->active[s] = 0;
                sh->iterations[s] = iteration;
                sh->res[s] = res;
            }
        } else {
            sh->update[s] = 0;
        }
        still[s] = sh->active[s];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sc[PS_RR] = rr_new;
        if (initial) sc[PS_RR0] = rr_new;
        sc[PS_BETA] = beta;
        sc[PS_A_OLD] = a;
        sc[PS_BETA_OLD] = beta;
        int count = 0;
        for (int k = 0; k < m; ++k) count += still[k];
        *host_active = count;
    }
}

/* x_s += a_s p_s ; p_s = zeta_new_s r + beta_s p_s for every shift that was active when the iteration began ; p = r + beta p ; part = (0, sum p).  The scalars are
 * rounded to T first */
template <typename T>
__global__ __launch_bounds__(RED_THREADS) void k_path_update(const T *__restrict__ r, T *__restrict__ p, T *__restrict__ xs, T *__restrict__ ps, const PathShifts *__restrict__ sh,
                                                             const double *__restrict__ sc, int n, int m, size_t stride, double *__restrict__ part) {
    __shared__ double lds[8];
    __shared__ T a_s[PATH_SHIFTS], b_s[PATH_SHIFTS], zn[PATH_SHIFTS];
    __shared__ int upd[PATH_SHIFTS];
    if (threadIdx.x < m) {
        a_s[threadIdx.x] = static_cast<T>(sh->a_s[threadIdx.x]);
        b_s[threadIdx.x] = static_cast<T>(sh->b_s[threadIdx.x]);
        zn[threadIdx.x] = static_cast<T>(sh->zeta_new[threadIdx.x]);
        upd[threadIdx.x] = sh->update[threadIdx.x];
    }
    __syncthreads();
    const T beta = static_cast<T>(sc[PS_BETA]);
    double acc[2] = { 0.0, 0.0 };
    for (int i = blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += RED_BLOCKS * RED_THREADS) {
        const T ri = r[i];
        for (int s = 0; s < m; ++s) {
            if (upd[s] == 0) continue;
            const size_t k = static_cast<size_t>(s) * stride + i;
            const T psi = ps[k];
            xs[k] += a_s[s] * psi;
            ps[k] = zn[s] * ri + b_s[s] * psi;
        }
        const T pi = ri + beta * p[i];
        p[i] = pi;
        acc[1] += static_cast<double>(pi);
    }
    path_store_partials<2>(acc, lds, part);
}

/* x = P z = z - theta sum(z), in place; part = (sum x, q.x) */
template <typename T>
__global__ __launch_bounds__(RED_THREADS) void k_path_finish(T *__restrict__ z, const double *__restrict__ part_z, double theta, const T *__restrict__ q, int n, double *__restrict__ part) {
    __shared__ double lds[8];
    __shared__ double tot[2];
    double sz[2];
    path_finish_in_block<2>(part_z, lds, tot, sz);
    double acc[2] = { 0.0, 0.0 };
    for (int i = blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += RED_BLOCKS * RED_THREADS) {
        const T xi = static_cast<T>(static_cast<double>(z[i]) - theta * sz[0]);
        z[i] = xi;
        acc[0] += static_cast<double>(xi);
        acc[1] += static_cast<double>(xi) * static_cast<double>(q[i]);
    }
    path_store_partials<2>(acc, lds, part);
}

/* ONE block: out[0], out[1] = the two sums of `part` -- or, inv_N >= 0, out[0] = sum0 - sum1^2 / N = |P v|^2 from (v.v, sum v) */
__global__ __launch_bounds__(RED_THREADS) void k_path_store(const double *__restrict__ part, double inv_N, double *__restrict__ out) {
    __shared__ double lds[8];
    __shared__ double tot[2];
    double s[2];
    path_finish_in_block<2>(part, lds, tot, s);
    if (threadIdx.x == 0) {
        if (inv_N >= 0.0) {
            out[0] = s[0] - s[1] * s[1] * inv_N;
        } else {
            out[0] = s[0];
            out[1] = s[1];
        }
    }
}

/* the TRUE residual of one cost, res = b - Abar(sigma) x with Kx = K x and (sum x, q.x) in `sums`, evaluated in double and not stored; part = (res.res, sum res) */
template <typename T>
__global__ __launch_bounds__(RED_THREADS) void k_path_true_residual(const T *__restrict__ Kx, const T *__restrict__ x, const T *__restrict__ q, const T *__restrict__ y,
                                                                    const double *__restrict__ sums, double sigma, double k_ll, int n, double *__restrict__ part) {
    __shared__ double lds[8];
    const double S = sums[0], QX = sums[1];
    const double y_last = static_cast<double>(y[n]);
    double acc[2] = { 0.0, 0.0 };
    for (int i = blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += RED_BLOCKS * RED_THREADS) {
        const double ax = static_cast<double>(Kx[i]) + sigma * static_cast<double>(x[i]) + ((k_ll + sigma) * S - QX) - S * static_cast<double>(q[i]);
        const double res = (static_cast<double>(y[i]) - y_last) - ax;
        acc[0] += res * res;
        acc[1] += res;
    }
    path_store_partials<2>(acc, lds, part);
}

}  // namespace

void check_cost_path_arguments(const void *y, const double *costs, size_t num_costs, double eps, uint64_t max_iter, const void *alphas_out, const double *rhos_out,
                               const lssvm_path_info *infos_out) {
    LSSVM_REQUIRE(y != nullptr, "The right hand side vector must not be empty!");
    LSSVM_REQUIRE(num_costs > 0, "The number of costs must be greater than 0!");
    LSSVM_REQUIRE(num_costs <= PATH_MAX_COSTS, "A cost path takes at most " + std::to_string(PATH_MAX_COSTS) + " costs, but got " + std::to_string(num_costs) + "!");
    LSSVM_REQUIRE(costs != nullptr, "costs must not be NULL");
    for (size_t s = 0; s < num_costs; ++s) {
        LSSVM_REQUIRE(std::isfinite(costs[s]) && costs[s] > 0.0, "Every cost of the path must be finite and greater than 0.0, but cost " + std::to_string(s) + " is " + std::to_string(costs[s]) + "!");
    }
    LSSVM_REQUIRE(std::isfinite(eps) && eps > 0.0, "The stopping criterion in the CG algorithm must be greater than 0.0, but is " + std::to_string(eps) + "!");
    LSSVM_REQUIRE(max_iter > 0, "The number of CG iterations must be greater than 0!");
    LSSVM_REQUIRE(alphas_out != nullptr && rhos_out != nullptr && infos_out != nullptr, "alphas_out / rhos_out / infos_out must not be NULL");
}

template <typename T>
void Solver<T>::solve_cost_path(const void *y_host, const double *costs, size_t num_costs, double eps, uint64_t max_iter, bool verify, void *alphas_out_v, double *rhos_out,
                                lssvm_path_info *infos_out, uint64_t *passes_out) {
    check_cost_path_arguments(y_host, costs, num_costs, eps, max_iter, alphas_out_v, rhos_out, infos_out);
    LSSVM_REQUIRE(shards_.size() == 1 && world_ == 1 && exchange_ == Exchange::none, "the cost path runs on a problem of one device and one rank");
    Problem<T> &p = *shards_[0];
    LSSVM_REQUIRE(!p.weighted_, "the cost path solves the unweighted system: the problem has weights set (lssvm_mi355_problem_set_weights(p, NULL, 0) removes them)");
    LSSVM_REQUIRE(!in_cg_, "solve_cost_path cannot run between cg_begin and cg_finish");
    const int m = static_cast<int>(num_costs);
    // sigma_s = 1 / C_s as every solve forms it, in the real type; the seed is the smallest
    std::vector<double> sigma(num_costs);
    for (int s = 0; s < m; ++s) {
        const T c = static_cast<T>(costs[s]);
        sigma[s] = static_cast<double>(T(1) / c);
        LSSVM_REQUIRE(std::isfinite(static_cast<double>(c)) && sigma[s] > 0.0 && std::isfinite(sigma[s]), "cost " + std::to_string(s) + " and its inverse must be finite and positive in the real type");
    }
    const double sigma0 = *std::min_element(sigma.begin(), sigma.end());
    if (passes_out != nullptr) passes_out[0] = passes_out[1] = 0;

    const SetOnExit<bool> busy = hold_busy();
    p.activate();
    hipStream_t st = p.stream();
    const int n = p.n_;
    const size_t N = p.N_;
    const size_t stride = static_cast<size_t>(p.nvec_) + TILE;  // (as the problem's own vectors: the Gram pass reads whole tiles, exact zeros beyond n)
    const double theta = (1.0 - 1.0 / std::sqrt(static_cast<double>(N))) / static_cast<double>(n);
    const double k_ll = p.self_last_;
    const T *q = p.q_.p;
    T *alphas_out = static_cast<T *>(alphas_out_v);

    // the iteration vectors: r, p, u, w and x_s, p_s per shift -- 2 m + 4 vectors of n reals, for this call
    DevBuf<T> vecs, ydev;
    vecs.alloc_zero((2 * static_cast<size_t>(m) + 4) * stride, st);
    ydev.alloc_zero(N, st);
    T *r = vecs.p, *pv = r + stride, *u = pv + stride, *w = u + stride, *xs = w + stride, *ps = xs + static_cast<size_t>(m) * stride;
    DevBuf<double> part, sc, sums, true_res;
    part.alloc_zero(static_cast<size_t>(PP_SETS) * RED_BLOCKS * 4, st);
    sc.alloc_zero(PS_COUNT, st);
    sums.alloc_zero(2 * static_cast<size_t>(m), st);
    true_res.alloc_zero(static_cast<size_t>(m), st);
    DevBuf<PathShifts> shifts;
    shifts.alloc_zero(1, st);
    PinnedBuf<int> host_active;
    host_active.alloc_mapped(1);
    *host_active.p = m;
    const auto part_of = [&](PathPart s) { return part.p + static_cast<size_t>(s) * RED_BLOCKS * 4; };
    const dim3 gr(RED_BLOCKS), br(RED_THREADS);
    const double eps2 = eps * eps;

    PathShifts host_shifts{};
    for (int s = 0; s < m; ++s) host_shifts.delta[s] = sigma[s] - sigma0;
    LSSVM_HIP_CHECK(hipMemcpyAsync(shifts.p, &host_shifts, sizeof(PathShifts), hipMemcpyHostToDevice, st));
    const double ones[2] = { 1.0, 0.0 };  // a_old = 1, beta_old = 0
    LSSVM_HIP_CHECK(hipMemcpyAsync(sc.p + PS_A_OLD, &ones[0], sizeof(double), hipMemcpyHostToDevice, st));
    LSSVM_HIP_CHECK(hipMemcpyAsync(ydev.p, y_host, N * sizeof(T), hipMemcpyHostToDevice, st));

    // ---- start: b = y - y_last (in w, until the first iteration needs it), r = p = p_s = P b, r.r ----
    hipLaunchKernelGGL(k_make_b<T>, dim3((n + 255) / 256), dim3(256), 0, st, ydev.p, n, w);
    hipLaunchKernelGGL(k_path_sums<T>, gr, br, 0, st, w, q, n, part_of(PP_U));
    hipLaunchKernelGGL(k_path_begin<T>, gr, br, 0, st, w, part_of(PP_U), theta, n, m, stride, r, pv, ps, part_of(PP_RR), part_of(PP_P));
    hipLaunchKernelGGL(k_path_scalars, dim3(1), br, 0, st, part_of(PP_RR), sc.p, shifts.p, m, eps2, 1, 0ull, host_active.dev);
    LSSVM_HIP_CHECK(hipGetLastError());
    wait_for_deltas();
    int active = *static_cast<volatile int *>(host_active.p);

    // ---- the seed's CG, every shift following: one Gram pass per iteration ----
    uint64_t iterations = 0;
    while (active > 0 && iterations < max_iter) {
        ++iterations;
        hipLaunchKernelGGL(k_path_make_u<T>, gr, br, 0, st, pv, part_of(PP_P), theta, q, n, u, sc.p, part_of(PP_U));
        p.enqueue_apply_K_local(u, false);
        hipLaunchKernelGGL(k_path_t<T>, gr, br, 0, st, p.Kres_, pv, q, part_of(PP_U), k_ll, n, w, part_of(PP_T));
        hipLaunchKernelGGL(k_path_update_r<T>, gr, br, 0, st, w, pv, r, part_of(PP_T), sc.p, theta, sigma0, n, part_of(PP_RR));
        hipLaunchKernelGGL(k_path_scalars, dim3(1), br, 0, st, part_of(PP_RR), sc.p, shifts.p, m, eps2, 0, static_cast<unsigned long long>(iterations), host_active.dev);
        hipLaunchKernelGGL(k_path_update<T>, gr, br, 0, st, r, pv, xs, ps, shifts.p, sc.p, n, m, stride, part_of(PP_P));
        LSSVM_HIP_CHECK(hipGetLastError());
        wait_for_deltas();
        p.drain_events();
        active = *static_cast<volatile int *>(host_active.p);
    }

    // ---- x_s = P z_s, its sums; the outcome of every shift ----
    double host_sc[PS_COUNT];
    LSSVM_HIP_CHECK(hipMemcpyAsync(&host_shifts, shifts.p, sizeof(PathShifts), hipMemcpyDeviceToHost, st));
    LSSVM_HIP_CHECK(hipMemcpyAsync(host_sc, sc.p, sizeof(host_sc), hipMemcpyDeviceToHost, st));
    for (int s = 0; s < m; ++s) {
        T *x = xs + static_cast<size_t>(s) * stride;
        hipLaunchKernelGGL(k_path_sums<T>, gr, br, 0, st, x, q, n, part_of(PP_U));
        hipLaunchKernelGGL(k_path_finish<T>, gr, br, 0, st, x, part_of(PP_U), theta, q, n, part_of(PP_T));
        hipLaunchKernelGGL(k_path_store, dim3(1), br, 0, st, part_of(PP_T), -1.0, sums.p + 2 * s);
        LSSVM_HIP_CHECK(hipMemcpyAsync(alphas_out + static_cast<size_t>(s) * N, x, static_cast<size_t>(n) * sizeof(T), hipMemcpyDeviceToHost, st));
    }
    LSSVM_HIP_CHECK(hipGetLastError());
    std::vector<double> host_sums(2 * num_costs), host_true(num_costs, -1.0);
    LSSVM_HIP_CHECK(hipMemcpyAsync(host_sums.data(), sums.p, host_sums.size() * sizeof(double), hipMemcpyDeviceToHost, st));

    // ---- verification: the true residual b - Abar(sigma_s) x_s of every cost, one Gram pass each -- two costs per pass where the two-vector kernel applies ----
    uint64_t verify_passes = 0;
    if (verify) {
        const bool pairs = p.pair_kernel_applies();
        const double inv_N = 1.0 / static_cast<double>(N);
        const auto residual_of = [&](int s, const T *Kx) {
            hipLaunchKernelGGL(k_path_true_residual<T>, gr, br, 0, st, Kx, xs + static_cast<size_t>(s) * stride, q, ydev.p, sums.p + 2 * s, sigma[s], k_ll, n, part_of(PP_RR));
            hipLaunchKernelGGL(k_path_store, dim3(1), br, 0, st, part_of(PP_RR), inv_N, true_res.p + s);
        };
        for (int s = 0; s < m; s += pairs ? 2 : 1) {
            if (pairs) {
                const bool two = s + 1 < m;
                p.enqueue_apply_K_lanes(xs + static_cast<size_t>(s) * stride, u, two ? xs + static_cast<size_t>(s + 1) * stride : nullptr, two ? w : nullptr, nullptr, nullptr);
                residual_of(s, u);
                if (two) residual_of(s + 1, w);
            } else {
                p.enqueue_apply_K_local(xs + static_cast<size_t>(s) * stride, false);
                residual_of(s, p.Kres_);
            }
            ++verify_passes;
        }
        LSSVM_HIP_CHECK(hipGetLastError());
        LSSVM_HIP_CHECK(hipMemcpyAsync(host_true.data(), true_res.p, host_true.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    p.drain_events();

    const double y_last = static_cast<double>(static_cast<const T *>(y_host)[N - 1]);
    const double rr0 = host_sc[PS_RR0], target = eps2 * rr0;
    for (int s = 0; s < m; ++s) {
        // alpha_N = -sum(x), rho = -bias = -(y_last + QA_cost(sigma_s) sum(x) - q.x), rounded as CgSteps::read_solution rounds them
        const double QA_cost = static_cast<double>(static_cast<T>(k_ll) + static_cast<T>(sigma[s]));
        const T sum_x = static_cast<T>(host_sums[2 * s]);
        const T bias = static_cast<T>(y_last + QA_cost * host_sums[2 * s] - host_sums[2 * s + 1]);
        alphas_out[static_cast<size_t>(s) * N + n] = -sum_x;
        rhos_out[s] = static_cast<double>(-bias);
        lssvm_path_info info{};
        const bool frozen = host_shifts.active[s] == 0;
        info.iterations = frozen ? host_shifts.iterations[s] : iterations;
        info.converged = frozen ? 1 : 0;
        info.initial_residuum = rr0;
        info.residuum = frozen ? host_shifts.res[s] : host_shifts.zeta[s] * host_shifts.zeta[s] * host_sc[PS_RR];
        info.target_residuum = target;
        info.true_residuum = verify ? host_true[s] : -1.0;
        info.verified = (verify && host_true[s] <= 4.0 * target) ? 1 : 0;
        infos_out[s] = info;
    }
    if (passes_out != nullptr) {
        passes_out[0] = iterations;
        passes_out[1] = verify_passes;
    }
}

template void Solver<float>::solve_cost_path(const void *, const double *, size_t, double, uint64_t, bool, void *, double *, lssvm_path_info *, uint64_t *);
template void Solver<double>::solve_cost_path(const void *, const double *, size_t, double, uint64_t, bool, void *, double *, lssvm_path_info *, uint64_t *);

}  // namespace lssvm
