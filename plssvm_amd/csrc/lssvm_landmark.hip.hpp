/*
 * lssvm_landmark.hip.hpp -- the landmark block K_Nm of a resident problem in double, shared by the Nystrom preconditioner (lssvm_precond.hip) and the fixed-size
 * model (lssvm_reduced.hip), and the host pieces both use (the factorisation, the library's landmark rule).
 */
#pragma once

#include "lssvm_problem.hip.hpp"

#include <cstdint>
#include <vector>

namespace lssvm {

template <typename T>
struct PcVec;
template <>
struct PcVec<float> {
    using type = f32x4;
    static constexpr int n = 4;
};
template <>
struct PcVec<double> {
    using type = f64x2;
    static constexpr int n = 2;
};

/* k(a, b) from the sum over the features (ascending) of (a_f - b_f)^2 (rbf) or a_f b_f (polynomial, linear): the one epilogue of the landmark block and of the
 * landmark selection's columns (lssvm_select.hip) */
__device__ __forceinline__ double landmark_kernel_value(int kernel_type, int degree, double gamma, double coef0, double acc) {
    double k;
    if (kernel_type == LSSVM_KERNEL_RBF) {
        k = exp(-gamma * acc);
    } else if (kernel_type == LSSVM_KERNEL_POLYNOMIAL) {
        const double base = gamma * acc + coef0;
        k = 1.0;
        for (int e = 0; e < abs(degree); ++e) k *= base;
        if (degree < 0) k = 1.0 / k;
    } else {
        k = gamma * acc;
    }
    return k;
}

/* The body of k_landmark_block and of k_landmark_acc, shared whole so that both walk THE SAME loop (same order, same LDS staging, same bits of acc): for the points
 * row0 <= i < N of this launch's row blocks and a tile of 16 landmarks, acc[l] = the sum over the features (ascending) of (a_f - b_f)^2 (rbf) or a_f b_f (polynomial,
 * linear), in double -- the landmarks' features go through LDS in chunks of 32, a thread walks its own row in 16-byte pieces.  VALUES: out[l][i - row0] =
 * landmark_kernel_value(acc[l]); else acc[l] itself.  Exact zeros from point N on.  (The kernel's whole body and not the loop alone: with the loop cut out on its own the
 * compiler schedules k_landmark_block differently; this way its instructions are the ones it had.) */
template <typename T, bool VALUES>
__device__ __forceinline__ void landmark_block_body(const T *__restrict__ X, int ldx, int N, int row0, const int *__restrict__ lm, int m, int kernel_type, int degree, double gamma,
                                                    double coef0, double *__restrict__ Kd, size_t ldN) {
    constexpr int FC = 32, V = PcVec<T>::n;
    __shared__ T xl[16][FC];
    const int local = blockIdx.x * 256 + threadIdx.x;
    const int i = row0 + local;
    const int l0 = blockIdx.y * 16;
    const T *xi = X + static_cast<size_t>(min(i, N - 1)) * ldx;
    double acc[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) acc[l] = 0.0;
    for (int f0 = 0; f0 < ldx; f0 += FC) {  // (ldx is a multiple of the k-chunk: 32 in fp32, 16 in fp64)
        __syncthreads();
        for (int e = threadIdx.x; e < 16 * FC; e += 256) {
            const int l = e / FC, f = e % FC;
            xl[l][f] = (l0 + l < m && f0 + f < ldx) ? X[static_cast<size_t>(lm[l0 + l]) * ldx + f0 + f] : T(0);
        }
        __syncthreads();
        const int fend = min(FC, ldx - f0);
        for (int f = 0; f < fend; f += V) {
            const typename PcVec<T>::type v = *reinterpret_cast<const typename PcVec<T>::type *>(xi + f0 + f);
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const double a = static_cast<double>(v[u]);
#pragma unroll
                for (int l = 0; l < 16; ++l) {
                    const double b = static_cast<double>(xl[l][f + u]);
                    if (kernel_type == LSSVM_KERNEL_RBF) {
                        acc[l] += (a - b) * (a - b);
                    } else {
                        acc[l] += a * b;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int l = 0; l < 16; ++l) {
        if (l0 + l >= m) continue;
        const double k = VALUES ? landmark_kernel_value(kernel_type, degree, gamma, coef0, acc[l]) : acc[l];
        Kd[static_cast<size_t>(l0 + l) * ldN + local] = i < N ? k : 0.0;
    }
}

/* Kd[l][i - row0] = k(x_i, x_lm[l]) for the points row0 <= i < N of this launch's row blocks (exact zeros from N on) and a tile of 16 landmarks, in double.  `gamma`: the
 * kernel function's, divided by the square of the factor X_ carries.  `ldN`: doubles between two landmarks' columns; the grid's x extent times 256 rows are written from
 * column offset 0 on. */
template <typename T>
__global__ __launch_bounds__(256) void k_landmark_block(const T *__restrict__ X, int ldx, int N, int row0, const int *__restrict__ lm, int m, int kernel_type, int degree, double gamma,
                                                        double coef0, double *__restrict__ Kd, size_t ldN) {
    landmark_block_body<T, true>(X, ldx, N, row0, lm, m, kernel_type, degree, gamma, coef0, Kd, ldN);
}

/* D[l][i - row0] = the sum k_landmark_block hands to landmark_kernel_value, stored instead (exact zeros from N on): what every gamma of a grid shares (lssvm_reduced.hip;
 * DESIGN.md section 17).  k_kernel_values on it gives k_landmark_block's bits.  Grid and layout as k_landmark_block. */
template <typename T>
__global__ __launch_bounds__(256) void k_landmark_acc(const T *__restrict__ X, int ldx, int N, int row0, const int *__restrict__ lm, int m, int kernel_type, double *__restrict__ D,
                                                      size_t ldN) {
    landmark_block_body<T, false>(X, ldx, N, row0, lm, m, kernel_type, 0, 0.0, 0.0, D, ldN);
}

/* Kmm[k][l] = slab[l][lm[k] - row0] for the landmarks that lie in the rows [row0, row0 + rows) of this column-major slab of the block (ld doubles between two columns); a
 * copy, no arithmetic.  The whole block at once: row0 = 0, rows = ld.  (static: a kernel that is no template cannot be inline, and both units that include this launch it) */
[[maybe_unused]] static __global__ void k_gather_kmm(const double *__restrict__ slab, size_t ld, int row0, int rows, const int *__restrict__ lm, int m, double *__restrict__ Kmm) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * m) return;
    const int r = lm[e / m] - row0;
    if (r >= 0 && r < rows) Kmm[e] = slab[static_cast<size_t>(e % m) * ld + r];
}

/* The landmark block K(X, X_L) of a problem's resident data: the landmarks' indices on the device and the kernel function's scalars for the data AS X_ HOLDS IT --
 * x' = x_scale (x - mean) leaves rbf distances and inner products scaled by x_scale^2, so gamma is divided by that; gamma and coef0 are the ones the problem's real type
 * holds.  The ONE place this rule stands: the preconditioner, the fixed-size fit and its leave-one-out pass evaluate the block through it, so their bits agree. */
template <typename T>
class LandmarkBlock {
  public:
    /* enqueues the upload of the indices on `st`; the problem outlives the block */
    LandmarkBlock(const Problem<T> &p, const std::vector<uint64_t> &landmarks, hipStream_t st) :
        p_(p), st_(st), m_(static_cast<int>(landmarks.size())), lm_host_(landmarks.begin(), landmarks.end()) {
        kernel_scalars(p, gamma_, coef0_);
        lm_dev_.alloc_zero(static_cast<size_t>(m_), st);
        LSSVM_HIP_CHECK(hipMemcpyAsync(lm_dev_.p, lm_host_.data(), static_cast<size_t>(m_) * sizeof(int), hipMemcpyHostToDevice, st));
    }
    /* out[l][i - row0] = k(x_i, x_lm[l]) for row0 <= i < row0 + rows256 (a multiple of 256; exact zeros from point N on), `ld` doubles between two landmarks' columns */
    void enqueue(size_t row0, int rows256, double *out, size_t ld) const {
        hipLaunchKernelGGL(k_landmark_block<T>, dim3(rows256 / 256, (m_ + 15) / 16), dim3(256), 0, st_, p_.X_.data.p, p_.X_.ldx, static_cast<int>(p_.N_), static_cast<int>(row0), lm_dev_.p, m_,
                           p_.params_.kernel_type, p_.params_.degree, gamma_, coef0_, out, ld);
    }
    /* K_mm's rows of the landmarks among the `rows` points from row0 on, out of the slab `enqueue` filled */
    void enqueue_gather_kmm(const double *slab, size_t ld, size_t row0, int rows, double *Kmm) const {
        hipLaunchKernelGGL(k_gather_kmm, dim3((m_ * m_ + 255) / 256), dim3(256), 0, st_, slab, ld, static_cast<int>(row0), rows, lm_dev_.p, m_, Kmm);
    }
    size_t device_bytes() const { return lm_dev_.count * sizeof(int); }
    /* gamma and coef0 for the data as X_ holds it (the rule above); the landmark selection evaluates its columns with them (lssvm_select.hip) */
    static void kernel_scalars(const Problem<T> &p, double &gamma, double &coef0) { kernel_scalars(p, p.params_.gamma, gamma, coef0); }
    /* the same rule for a gamma that is not the problem's own: a grid of them on one resident problem (lssvm_reduced.hip) */
    static void kernel_scalars(const Problem<T> &p, double gamma_in, double &gamma, double &coef0) {
        const double scale2 = p.x_scale_ * p.x_scale_;
        gamma = p.params_.kernel_type == LSSVM_KERNEL_LINEAR ? 1.0 / scale2 : static_cast<double>(static_cast<T>(gamma_in)) / scale2;
        coef0 = static_cast<double>(static_cast<T>(p.params_.coef0));
    }
    const int *landmarks_dev() const { return lm_dev_.p; }

  private:
    const Problem<T> &p_;
    hipStream_t st_;
    int m_;
    std::vector<int> lm_host_;  // (the source of the asynchronous upload)
    DevBuf<int> lm_dev_;
    double gamma_ = 0.0, coef0_ = 0.0;
};

/* G[j][k] = sum over i of Bhat[j][i] Bhat[k][i] for one 16 x 16 tile on or below the diagonal: ONE thread owns an entry and adds its products for i ascending, in
 * double -- a single fixed-order sum per entry, no partial sums to combine and no atomics.  64 rows of both column groups go through LDS per step. */
template <typename T>
__global__ __launch_bounds__(256) void k_precond_gram(const T *__restrict__ Bhat, size_t ldn, int cols, double *__restrict__ G, int ldg) {
    if (blockIdx.y > blockIdx.x) return;
    __shared__ double A[16][65], B[16][65];
    const int tj = threadIdx.x / 16, tk = threadIdx.x % 16;
    const int j0 = blockIdx.x * 16, k0 = blockIdx.y * 16;
    const int lr = threadIdx.x / 16, lc = (threadIdx.x % 16) * 4;
    double acc = 0.0;
    for (size_t i0 = 0; i0 < ldn; i0 += 64) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            A[lr][lc + u] = j0 + lr < cols ? static_cast<double>(Bhat[static_cast<size_t>(j0 + lr) * ldn + i0 + lc + u]) : 0.0;
            B[lr][lc + u] = k0 + lr < cols ? static_cast<double>(Bhat[static_cast<size_t>(k0 + lr) * ldn + i0 + lc + u]) : 0.0;
        }
        __syncthreads();
#pragma unroll 16
        for (int c = 0; c < 64; ++c) acc += A[tj][c] * B[tk][c];
    }
    G[static_cast<size_t>(j0 + tj) * ldg + k0 + tk] = acc;
}

/* A = L L^T in place (lower triangle; the upper one is left alone); false at a pivot that is not positive and finite   (lssvm_precond.hip) */
bool cholesky_lower(std::vector<double> &A, int m);
/* L L^T = M + nu I for the lower triangle of the m x m matrix M (row major): nu = eps64 trace(M), tenfold while the factorisation fails, seven attempts; returns the nu
 * that let it factor.  `subject` names M in the two refusals (no positive finite trace; not factored)   (lssvm_precond.hip) */
double cholesky_with_jitter(const std::vector<double> &M, int m, const char *subject, std::vector<double> &L);
/* the library's own landmarks: the first `rank` entries of a Fisher-Yates shuffle of 0 ... N-1 driven by splitmix64 from a fixed state (include/plssvm_amd.h) */
std::vector<uint64_t> default_landmarks(size_t N, size_t rank);

}  // namespace lssvm
