/*
 * lssvm_dense.hip.hpp -- the dense SPD toolbox on the device (lssvm_dense.hip): assembly of M + nu I, blocked Cholesky factorisation, triangular
 * solves and the triangular inverse, float64, 1 <= m <= 1024, on one stream.  Used by the device-factored fixed-size fits (lssvm_reduced.hip) and by the three testing
 * aids lssvm_mi355_dense_* (capi.hip).
 */
#pragma once

#include "lssvm_problem.hip.hpp"

#include <cstdint>

namespace lssvm {

constexpr int DENSE_BLOCK = 64;     // the block width B of the factorisation, the solves and the inverse
constexpr int DENSE_MAX_RANK = 1024;
constexpr int DENSE_ST_TILE = 128;  // St arrives as k_reduced_sum leaves it: packed 128 x 128 tiles of the lower triangle (lssvm_reduced.hip: RG_TW)

/* what one attempt took: device time between events, and the kernels it launched */
struct DenseTimes {
    double assemble_ms = 0.0, factor_ms = 0.0, solve_ms = 0.0, invert_ms = 0.0;
    uint64_t launches = 0;
};

/* One m x m system on the device.  The matrix lives in a padded buffer of mp x mp doubles, mp = m rounded up to DENSE_BLOCK, whose padding is the identity: every
 * kernel then works on whole blocks, and no entry of the leading m x m part ever meets a padded one with a nonzero factor.  Every kernel reads the status word first and
 * returns at once where it is not zero; k_dense_potrf_diag alone writes it (1 + the column of a pivot that is not positive and finite).  Everything is enqueued on the
 * stream given at construction; nothing here waits for the device but status(). */
class DenseSpd {
  public:
    DenseSpd(int m, int max_rhs, hipStream_t st);
    int m() const { return m_; }
    int mp() const { return mp_; }
    /* the status word back to zero, the launch count too: the start of an attempt */
    void begin_attempt();
    /* (a) from St (packed tiles, cols = m + 1 + k columns) and K_mm (m x m): the lower triangle of S - s s^T / N + sigma K_mm + nu I, s, and the k right-hand sides t_c - s eta_c / N */
    void enqueue_assemble(const double *St_tiles, const double *Kmm, int k, double Nd, double sigma, double nu);
    /* (a) for the testing aids: the lower triangle of the m x m row-major A_dev plus nu I; what stands above its diagonal is never read */
    void enqueue_load_lower(const double *A_dev, double nu);
    /* the k right-hand sides (k x m row major, on the device) for the testing aid of the solve; no s: no rho is formed */
    void enqueue_load_rhs(const double *B_dev, int k);
    /* (b) A = L L^T in place, left-looking by block columns */
    void enqueue_factor();
    /* (c) L z = rhs, L^T beta = z for the k right-hand sides loaded or assembled before; beta_c -> X_out[c * ldx ...] (m entries, zeros up to `fill`), and, with_rho,
     * rho_c = -(eta_c - s^T beta_c) / N -> rhos_out[c].  X2_out (may be NULL): a second copy of the rows, ld2 doubles apart, zeros up to ld2 */
    void enqueue_solve(int k, double *X_out, size_t ldx, double *X2_out, size_t ld2, bool with_rho, double Nd, double *rhos_out);
    /* (c) for the rank path: z_c alone, L z = rhs forward as enqueue_solve takes it, -> Z_out[c * ldz ...] (m entries, zeros up to ldz) */
    void enqueue_forward(int k, double *Z_out, size_t ldz);
    /* ... and per (checkpoint q, right-hand side c) beta = V[:r_q, :r_q]^T z_c[:r_q] -> betas_out[(q * k + c) * m ...] (zeros from r_q on), rho -> rhos_out[q * k + c], from
     * the rows of V (Vt, ldv doubles apart) and Z that enqueue_invert and enqueue_forward left; cond_out[q] = max_j L_jj^2 / min_j L_jj^2 over j < r_q, off the factor.
     * ranks_dev: num_ranks ascending checkpoints on the device */
    void enqueue_prefix_betas(const double *Vt, int ldv, const double *Z, size_t ldz, int k, const int *ranks_dev, int num_ranks, double Nd, double *betas_out, double *rhos_out,
                              double *cond_out);
    /* (d) row n of V = L^-1 -> Vt_out[n * ldv ...] for n < m, exact zeros above the diagonal up to ldv (>= m, a multiple of 16) */
    void enqueue_invert(double *Vt_out, int ldv);
    /* the factor (its lower triangle, zeros above) as m x m row major into L_dev */
    void enqueue_store_factor(double *L_dev);
    /* waits for the stream; 0, or 1 + the column whose pivot was not positive and finite */
    unsigned status();
    uint64_t launches() const { return launches_; }
    size_t device_bytes() const { return (A_.count + rhs_.count + s_.count + eta_.count) * sizeof(double) + sizeof(unsigned); }

  private:
    int m_, mp_, nb_, max_rhs_;
    hipStream_t st_;
    DevBuf<double> A_, rhs_, s_, eta_;
    DevBuf<unsigned> status_;
    uint64_t launches_ = 0;
};

/* the four stages of one attempt between timing events */
class DenseStopwatch {
  public:
    explicit DenseStopwatch(hipStream_t st);
    void mark(int i);  // event i (0 ... 4) on the stream
    /* after the stream has been waited for: the spans between the marks that were set, in order assemble, factor, solve, invert (an unset end: 0) */
    void read(bool with_invert, DenseTimes &t) const;

  private:
    hipStream_t st_;
    Event ev_[5];
};

/* lssvm_mi355_dense_cholesky / _solve / _invert_lower (include/plssvm_amd_testing.h): host arrays in, the toolbox on device 0, host arrays out; the arguments have been checked */
void dense_cholesky_aid(const double *A, int m, double nu, double *L_out, uint64_t *status_out, double *ms_out);
void dense_solve_aid(const double *L, int m, const double *B, int k, double *X_out, double *ms_out);
void dense_invert_lower_aid(const double *L, int m, double *V_out, double *ms_out);

}  // namespace lssvm
