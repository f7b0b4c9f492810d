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

/* ---- what the translation units of the fixed-size model share (defined in lssvm_reduced.hip; used there and by lssvm_logistic.hip) ---- */
constexpr int RG_TW = 128;                 // columns of Pt per operand of a tile
constexpr int RG_KC = 16;                  // rows of Pt per step
constexpr int RG_LS = RG_KC + 2;           // doubles between two columns in LDS: 144 bytes, conflict-free ds_read_b64 (as the fp64 tile kernels)
constexpr int RG_RANGE = 2048;             // rows of a slab per workgroup: a CONSTANT (lssvm_reduced.hip has why)
constexpr int RG_TILE = RG_TW * RG_TW;     // entries of a tile
static_assert(RG_TW == DENSE_ST_TILE, "k_dense_assemble (lssvm_dense.hip) reads St as the tiles k_reduced_sum leaves");

int tiles_of(int cols);
/* St of one slab into the running sum: `rows` (a multiple of 256) rows of the column-major slab; `q`: sqrt(w) of these rows (`rows` doubles) for the weighted sum, or NULL */
void enqueue_gram(const double *slab, size_t ld, int cols, int rows, int max_chunks, double *part, double *St, hipStream_t st, const double *q = nullptr);
/* the tiles of St on the host -> cols x cols row major, the upper triangle the copy of the lower */
void unpack_tiles(const std::vector<double> &tiles, int cols, std::vector<double> &G);

/* rows of a slab (= doubles between two of its columns: at most N rounded up to 256) and how many slabs cover the N points; slab s holds the rows(s) points from row0(s)
 * on, in rows256(s) <= ld rows */
struct SlabPlan {
    size_t N, ld;
    int slabs;
    SlabPlan(size_t num_points, uint64_t slab_rows) :
        N(num_points), ld(std::min<size_t>(slab_rows == 0 ? REDUCED_DEFAULT_SLAB_ROWS : slab_rows, static_cast<size_t>(round_up(static_cast<long>(num_points), 256)))),
        slabs(static_cast<int>((N + ld - 1) / ld)) {}
    size_t row0(int s) const { return static_cast<size_t>(s) * ld; }
    int rows(int s) const { return static_cast<int>(std::min(ld, N - row0(s))); }
    int rows256(int s) const { return round_up(rows(s), 256); }  // (<= ld: ld is a multiple of 256)
};

/* the host's part of a fit, in double (lssvm_reduced.hip has the formulas) */
double factor_reduced(const std::vector<double> &St, const std::vector<double> &Kmm, int m, int cols, double Nd, double sigma, std::vector<double> &L);
void solve_reduced(const std::vector<double> &St, const std::vector<double> &L, int m, int k, int cols, double Nd, double *betas_out, double *rhos_out);
/* trace(M) from the host copies, with factor_reduced's expression and cholesky_with_jitter's order: where no attempt fails, nu has the host path's bits */
double reduced_trace(const std::vector<double> &St, const std::vector<double> &Kmm, int m, int cols, double Nd, double sigma);

/* what one cost needs on the device besides St and K_mm, held over the costs of a grid */
struct DenseFit {
    DenseSpd dense;
    DenseStopwatch watch;
    DevBuf<double> betas, rhos;
    std::vector<double> betas_host, rhos_host;  // where an attempt's results land before it is known to have factored
    const int m, k;
    hipStream_t st;
    DenseFit(int rank, int num_rhs, hipStream_t stream);
    size_t device_bytes() const { return dense.device_bytes() + (betas.count + rhos.count) * sizeof(double); }

    /* One cost: the jitter rule of cholesky_with_jitter, each attempt assemble -> factor -> solve (-> invert into the operand Bt_op: rows of V, the betas behind them, ldb
     * doubles apart) and ONE wait, at which betas (k x m), rhos (k) and the status word come back.  Fills `d` (may be NULL); returns nu.  Z_op (the rank path, DESIGN.md
     * section 18; else NULL): z_c = L^-1 (t_c - s eta_c / N), k rows of ldb doubles, is left there too. */
    double run(const ReducedOnDevice &dev, const std::vector<double> &St, const std::vector<double> &Kmm, int cols, double Nd, double sigma, double *Bt_op, int ldb, double *betas_out,
               double *rhos_out, lssvm_dense_info *d, double *device_ms_out, double *Z_op = nullptr);
};

}  // namespace lssvm
