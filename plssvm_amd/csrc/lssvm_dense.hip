/*
 * lssvm_dense.hip -- the dense SPD toolbox on the device: what the fixed-size fits need between their two device passes, in float64, for
 * 1 <= m <= 1024, on the problem's stream.  B = DENSE_BLOCK = 64.
 *
 * The matrix lives in an mp x mp buffer (mp = m rounded up to B) whose padding is the identity, so every kernel works on whole blocks; a padded entry meets an entry of
 * the leading m x m part only through a factor that is an exact zero.
 *   (a) k_dense_assemble         M + nu I = S - s s^T / N + sigma K_mm + nu I (lower triangle), s, and the right-hand sides t_c - s eta_c / N, from St's packed tiles and K_mm.
 *   (b) per block column j, left-looking:  k_dense_gemm   A[j:, j] -= L[j:, :j] L[j, :j]^T, one v_mfma_f64_16x16x4_f64 chain per entry over the columns ascending, the
 *                                                          chain STARTING at a_ij (the accumulator is loaded from A);
 *                                          k_dense_potrf_diag  one workgroup factors the B x B diagonal block in LDS;
 *                                          k_dense_trsm   the panel below it: X L_jj^T = A[j+1:, j], one thread per row.
 *       Every entry of L is (a_ij - sum_k l_ik l_jk) / l_jj with the k ascending and a true division (the square root on the diagonal); no inverted block is multiplied in.
 *   (c) k_dense_solve            one workgroup per right-hand side: L z = rhs, L^T beta = z by blocks, then rho.  Column c never sees another column.
 *   (d) per block ROW i of V = L^-1 (Higham, Accuracy and Stability, Method 1B, by rows):  k_dense_gemm  W = -L[i, :i] V[:i, :i] (the triangle of V skipped),
 *                                          k_dense_trsm   L_ii X = [W | I], one thread per column, straight into the leverage kernel's operand.
 *   (e) the rank path:  k_dense_forward  z_c = L^-1 rhs_c alone, the forward half of (c), beside V;
 *                                          k_dense_prefix_beta  per (checkpoint r, right-hand side): beta = V[:r, :r]^T z[:r], rho, and max / min of the factor's squared diagonal.
 * Failure: a pivot that is not positive and finite makes k_dense_potrf_diag write 1 + its column into the status word (a plain store) and leave; every kernel reads the
 * word first and returns at once where it is not zero -- the whole workgroup alike, ahead of any barrier.  No workgroup waits for another, no atomics, no scratch: the
 * stream orders the launches, and the same arguments give the same bits.  Compiled for gfx950 only.
 */
#include "lssvm_dense.hip.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>

namespace lssvm {

namespace {

constexpr int DB = DENSE_BLOCK;
constexpr int DG_KC = 16;          // columns of the contraction per step of k_dense_gemm
constexpr int DG_LS = DG_KC + 2;   // doubles between two rows of an operand in LDS: 144 bytes, conflict-free ds_read_b64 (as k_reduced_gram)
constexpr int DT_LD = DB + 1;      // doubles between two rows of a B x B block in LDS where a thread walks a row of its own

/* the word is read by every lane and is the same for all of them: the branch on it is uniform over the workgroup */
__device__ __forceinline__ bool dense_failed(const unsigned *status) { return __builtin_amdgcn_readfirstlane(static_cast<int>(*status)) != 0; }

/* St[j][l], l <= j, out of k_reduced_sum's packed tiles */
__device__ __forceinline__ double st_entry(const double *__restrict__ St, int j, int l) {
    const int bj = j / DENSE_ST_TILE, bk = l / DENSE_ST_TILE;
    return St[static_cast<size_t>(bj * (bj + 1) / 2 + bk) * (DENSE_ST_TILE * DENSE_ST_TILE) + (j % DENSE_ST_TILE) * DENSE_ST_TILE + l % DENSE_ST_TILE];
}

/* blockIdx.y < mp: row y of the padded matrix (its lower triangle as factor_reduced forms it, nu on the diagonal, zeros above, the identity in the padding);
 * y == mp: s; y > mp: right-hand side y - mp - 1 as solve_reduced forms it, and its eta */
__global__ __launch_bounds__(256) void k_dense_assemble(const double *__restrict__ St, const double *__restrict__ Kmm, int m, int mp, double Nd, double sigma, double nu,
                                                        double *__restrict__ A, double *__restrict__ s_out, double *__restrict__ rhs, double *__restrict__ eta_out,
                                                        const unsigned *status) {
    if (dense_failed(status)) return;
    const int col = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (col >= mp) return;
    if (row < mp) {
        double v = row == col ? 1.0 : 0.0;
        if (row < m && col < m) {
            v = 0.0;
            if (col <= row) {
                v = st_entry(St, row, col) - st_entry(St, m, row) * st_entry(St, m, col) / Nd + sigma * Kmm[static_cast<size_t>(row) * m + col];
                if (row == col) v += nu;
            }
        }
        A[static_cast<size_t>(row) * mp + col] = v;
    } else if (row == mp) {
        s_out[col] = col < m ? st_entry(St, m, col) : 0.0;
    } else {
        const int c = row - mp - 1;
        const double eta = st_entry(St, m + 1 + c, m);
        rhs[static_cast<size_t>(c) * mp + col] = col < m ? st_entry(St, m + 1 + c, col) - st_entry(St, m, col) * eta / Nd : 0.0;
        if (col == 0) eta_out[c] = eta;
    }
}

/* the testing aids' matrix: the lower triangle of the m x m row-major `in` plus nu I into the padded buffer; what stands above the diagonal of `in` is never read */
__global__ __launch_bounds__(256) void k_dense_load_lower(const double *__restrict__ in, int m, int mp, double nu, double *__restrict__ A) {
    const int col = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (col >= mp) return;
    double v = row == col ? 1.0 : 0.0;
    if (row < m && col < m) {
        v = 0.0;
        if (col <= row) {
            v = in[static_cast<size_t>(row) * m + col];
            if (row == col) v += nu;
        }
    }
    A[static_cast<size_t>(row) * mp + col] = v;
}

/* rows of m doubles -> rows of mp doubles, zeros behind them (the right-hand sides of the testing aid) */
__global__ __launch_bounds__(256) void k_dense_pad_rows(const double *__restrict__ in, int m, int mp, double *__restrict__ out) {
    const int col = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (col < mp) out[static_cast<size_t>(row) * mp + col] = col < m ? in[static_cast<size_t>(row) * m + col] : 0.0;
}

/* the leading m x m part of the padded factor, row major, zeros above the diagonal */
__global__ __launch_bounds__(256) void k_dense_store_lower(const double *__restrict__ A, int m, int mp, double *__restrict__ out) {
    const int col = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (col < m) out[static_cast<size_t>(row) * m + col] = col <= row ? A[static_cast<size_t>(row) * mp + col] : 0.0;
}

/* C -= A Bt^T over the contraction range [kbeg, K), one 64 x 64 tile of C per workgroup: tile (blockIdx.x, blockIdx.y), rows from `c_rows` on are neither read nor
 * written.  A: row i of the tile's rows, lda doubles apart, the contraction index contiguous.  B_KMAJOR false: Bm[j][k] (row j = column j of C, the contraction index
 * contiguous); true: Bm[k][j] (the contraction index is the ROW, as for V in W = L V).  tri: the contraction of column tile cb starts at 64 cb (Bm is lower triangular:
 * V[k][j] = 0 for k < j).  K - kbeg is a multiple of 16; every operand entry the tile reads exists (the callers' buffers are padded to whole blocks).
 * Both operands go through LDS as in k_reduced_gram; the four waves hold 32 x 32 each as four accumulators of v_mfma_f64_16x16x4_f64, which START at C's entries: an
 * entry is one chain a_ij - l_i0 l_j0 - l_i1 l_j1 - ... in ascending k.  The A fragments are negated on their way out of LDS (exact). */
template <bool B_KMAJOR>
__global__ __launch_bounds__(256) void k_dense_gemm(double *C, size_t ldc, int c_rows, const double *A, size_t lda, const double *Bm, size_t ldb, int K, int tri,
                                                    const unsigned *status) {
    if (dense_failed(status)) return;
    __shared__ __attribute__((aligned(16))) double As[DB * DG_LS];
    __shared__ __attribute__((aligned(16))) double Bs[DB * DG_LS];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int r = lane & 15, qd = lane >> 4;
    const int row0 = blockIdx.x * DB, col0 = blockIdx.y * DB;
    const int kbeg = tri ? col0 : 0;
    const int nsteps = (K - kbeg) / DG_KC;

    // staging: thread -> (row srow [+ 32 p] of the tile, columns 2 sseg, 2 sseg + 1 of the step); a k-major B: (row kk of the step, columns j4 ... j4 + 3 of the tile)
    const int srow = tid >> 3, sseg = tid & 7;
    const int kk = tid >> 4, j4 = (tid & 15) * 4;
    f64x2 sa[2], sb[2];
    auto stage_load = [&](int s) {
        const int k0 = kbeg + s * DG_KC;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            sa[p] = *reinterpret_cast<const f64x2 *>(A + static_cast<size_t>(row0 + srow + 32 * p) * lda + k0 + 2 * sseg);
            if constexpr (B_KMAJOR) {
                sb[p] = *reinterpret_cast<const f64x2 *>(Bm + static_cast<size_t>(k0 + kk) * ldb + col0 + j4 + 2 * p);
            } else {
                sb[p] = *reinterpret_cast<const f64x2 *>(Bm + static_cast<size_t>(col0 + srow + 32 * p) * ldb + k0 + 2 * sseg);
            }
        }
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            *reinterpret_cast<f64x2 *>(As + (srow + 32 * p) * DG_LS + 2 * sseg) = sa[p];
            if constexpr (B_KMAJOR) {
                Bs[(j4 + 2 * p) * DG_LS + kk] = sb[p][0];
                Bs[(j4 + 2 * p + 1) * DG_LS + kk] = sb[p][1];
            } else {
                *reinterpret_cast<f64x2 *>(Bs + (srow + 32 * p) * DG_LS + 2 * sseg) = sb[p];
            }
        }
    };

    // a lane holds rows qd + 4 i of its two row tiles and column r of its two column tiles (the layout of k_reduced_gram's results)
    f64x4 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + wr * 32 + mt * 16 + qd + 4 * i;
                acc[mt][nt][i] = row < c_rows ? C[static_cast<size_t>(row) * ldc + col0 + wc * 32 + nt * 16 + r] : 0.0;
            }
            // the start values live in the accumulators' OWN registers (C == D for every MFMA of a chain): lssvm_tile_f64_wide.hip.hpp has the hazard this keeps away
            asm volatile("" : "+v"(acc[mt][nt]));
        }

    if (nsteps > 0) {
        stage_load(0);
        stage_store();
    }
    __syncthreads();
    const double *Ab = As + (wr * 32 + r) * DG_LS + qd;
    const double *Bb = Bs + (wc * 32 + r) * DG_LS + qd;
    for (int s = 0; s < nsteps; ++s) {
        const bool has_next = s + 1 < nsteps;
        if (has_next) stage_load(s + 1);
#pragma unroll
        for (int ks = 0; ks < DG_KC / 4; ++ks) {
            double av[2], bv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                av[t] = -Ab[t * 16 * DG_LS + ks * 4];
                bv[t] = Bb[t * 16 * DG_LS + ks * 4];
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
        }
        __syncthreads();  // (every wave has read this step)
        if (has_next) {
            stage_store();
            __syncthreads();
        }
    }

#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + wr * 32 + mt * 16 + qd + 4 * i;
                if (row < c_rows) C[static_cast<size_t>(row) * ldc + col0 + wc * 32 + nt * 16 + r] = acc[mt][nt][i];
            }
}

/* The B x B diagonal block at `A` (ld doubles between rows) = L L^T in place, in LDS, by one workgroup: column k is divided by l_kk = sqrt(a_kk), then the trailing
 * lower triangle loses its products with column k -- entry (i, j) ends as (a_ij - l_i0 l_j0 - ... - l_i,j-1 l_j,j-1) / l_jj, the k ascending.  The block's upper triangle
 * is written as zeros.  A pivot that is not positive and finite: 1 + its column (col_base + k) into the status word, and every thread leaves (all of them read the same
 * pivot out of LDS: the exit is uniform). */
__global__ __launch_bounds__(256) void k_dense_potrf_diag(double *__restrict__ A, size_t ld, int col_base, unsigned *status) {
    if (dense_failed(status)) return;
    __shared__ double S[DB * DT_LD];
    const int tid = threadIdx.x;
    for (int e = tid; e < DB * DB; e += 256) S[(e >> 6) * DT_LD + (e & 63)] = A[static_cast<size_t>(e >> 6) * ld + (e & 63)];
    for (int k = 0; k < DB; ++k) {
        __syncthreads();
        const double d = S[k * DT_LD + k];
        if (!(d > 0.0 && d <= DBL_MAX)) {
            if (tid == 0) *status = static_cast<unsigned>(col_base + k + 1);
            return;
        }
        const double l = sqrt(d);
        if (tid > k && tid < DB) S[tid * DT_LD + k] = S[tid * DT_LD + k] / l;
        __syncthreads();
        if (tid == 0) S[k * DT_LD + k] = l;  // (nobody reads the pivot again: the trailing part lies in the columns behind k)
#pragma unroll
        for (int u = 0; u < DB * DB / 256; ++u) {
            const int e = tid + 256 * u, i = e >> 6, j = e & 63;
            if (j > k && j <= i) S[i * DT_LD + j] = fma(-S[i * DT_LD + k], S[j * DT_LD + k], S[i * DT_LD + j]);
        }
    }
    __syncthreads();
    for (int e = tid; e < DB * DB; e += 256) {
        const int i = e >> 6, j = e & 63;
        A[static_cast<size_t>(i) * ld + j] = j <= i ? S[i * DT_LD + j] : 0.0;
    }
}

/* where column c of the packed lower triangle of a B x B block starts: its entries (c, c) ... (B - 1, c) are contiguous */
__device__ __host__ constexpr int packed_col(int c) { return DB * c - c * (c - 1) / 2; }

/* Sixty-four independent forward substitutions with the lower triangular B x B block Ld, one per thread, the unknowns in registers:
 *   x_c = (b_c - sum_{k < c} l_ck x_k) / l_cc, the k ascending (each x_c, once known, is taken out of the entries behind it), a true division.
 * LEFT false (the panel of the factorisation): the systems are the ROWS of the tile, X Ld^T = tile; tile blockIdx.x of the rows below `M`.
 * LEFT true (a block row of the inverse): the systems are the COLUMNS of the tile, Ld X = tile; tile blockIdx.x of the columns of the block row at `M`; tile `ident_tile`
 * is the diagonal one, whose right-hand side is the identity and is not read.  Rows from rows_valid on and columns from cols_valid on are neither read nor written.
 * The tile goes through LDS both ways, so that global memory is walked along rows; Ld's lower triangle lies packed by columns in LDS and is read as a broadcast. */
template <bool LEFT>
__global__ __launch_bounds__(64) void k_dense_trsm(double *M, size_t ld, int rows_valid, int cols_valid, int ident_tile, const double *Ld, size_t ldl, const unsigned *status) {
    if (dense_failed(status)) return;
    __shared__ double T[DB * DT_LD];
    __shared__ __attribute__((aligned(16))) double Lc[DB * (DB + 1) / 2];
    const int tid = threadIdx.x;
    const int trow0 = LEFT ? 0 : blockIdx.x * DB, tcol0 = LEFT ? blockIdx.x * DB : 0;
    const bool ident = LEFT && static_cast<int>(blockIdx.x) == ident_tile;

    for (int rr = 0; rr < DB; ++rr) {  // (thread tid: column tid of every row)
        if (tid <= rr) Lc[packed_col(tid) + rr - tid] = Ld[static_cast<size_t>(rr) * ldl + tid];
        const int grow = trow0 + rr, gcol = tcol0 + tid;
        double v;
        if (ident) {
            v = rr == tid ? 1.0 : 0.0;
        } else {
            v = (grow < rows_valid && gcol < cols_valid) ? M[static_cast<size_t>(grow) * ld + gcol] : 0.0;
        }
        T[LEFT ? tid * DT_LD + rr : rr * DT_LD + tid] = v;
    }
    __syncthreads();

    double x[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i) x[i] = T[tid * DT_LD + i];
#pragma unroll
    for (int c = 0; c < DB; ++c) {
        x[c] = x[c] / Lc[packed_col(c)];
#pragma unroll
        for (int k = c + 1; k < DB; ++k) x[k] = fma(-x[c], Lc[packed_col(c) + k - c], x[k]);
    }
#pragma unroll
    for (int i = 0; i < DB; ++i) T[tid * DT_LD + i] = x[i];
    __syncthreads();

    for (int rr = 0; rr < DB; ++rr) {
        const int grow = trow0 + rr, gcol = tcol0 + tid;
        if (grow < rows_valid && gcol < cols_valid) M[static_cast<size_t>(grow) * ld + gcol] = T[LEFT ? tid * DT_LD + rr : rr * DT_LD + tid];
    }
}

/* One workgroup per right-hand side c: L z = rhs_c forward and L^T beta = z backward, block by block over the padded factor (mp x mp).  Per block the part of the sum
 * that lies outside the diagonal block is taken first -- forward: four lanes per row, each one chain over its columns (2 q, 2 q + 1, 2 q + 8, ...) ascending, combined as
 * (p0 + p1) + (p2 + p3); backward: four threads per column, thread q one chain over the rows 64 (jb + 1) + q, + 4, ..., combined the same way -- then wave 0 substitutes
 * through the diagonal block (in LDS), the lanes exchanging the unknown of the step: a true division per unknown.  The order depends on m only.
 * beta -> X[c ldx ...] (zeros from m up to fill) and, X2 given, X2[c ld2 ...] (zeros up to fill2); s given: rho_c = -(eta_c - s^T beta_c) / N with the dot product as 256
 * chains (j = tid, tid + 256, ...) and a binary tree over them. */
__global__ __launch_bounds__(256) void k_dense_solve(const double *__restrict__ L, int mp, int m, const double *__restrict__ rhs, double *__restrict__ X, size_t ldx, int fill,
                                                     double *__restrict__ X2, size_t ld2, int fill2, const double *__restrict__ s, const double *__restrict__ eta, double Nd,
                                                     double *__restrict__ rhos, const unsigned *status) {
    if (dense_failed(status)) return;
    __shared__ double Ls[DB * DT_LD];
    __shared__ double zv[DENSE_MAX_RANK];
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, c = blockIdx.x;
    const int nb = mp / DB;
    const double *b = rhs + static_cast<size_t>(c) * mp;

    for (int jb = 0; jb < nb; ++jb) {
        __syncthreads();  // (wave 0 is done with the block before: Ls may be overwritten, its unknowns are in zv)
        for (int e = tid; e < DB * DB; e += 256) Ls[(e >> 6) * DT_LD + (e & 63)] = L[static_cast<size_t>(jb * DB + (e >> 6)) * mp + jb * DB + (e & 63)];
        {
            const int row = tid >> 2, q = tid & 3;
            const double *Lr = L + static_cast<size_t>(jb * DB + row) * mp;
            double acc = 0.0;
            for (int k = 2 * q; k < jb * DB; k += 8) {
                const f64x2 l2 = *reinterpret_cast<const f64x2 *>(Lr + k);
                acc = fma(l2[0], zv[k], acc);
                acc = fma(l2[1], zv[k + 1], acc);
            }
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            if (q == 0) red[row] = b[jb * DB + row] - acc;
        }
        __syncthreads();
        if (tid < DB) {
            double v = red[lane], mine = 0.0;
#pragma unroll
            for (int cc = 0; cc < DB; ++cc) {
                const double zc = __shfl(v, cc) / Ls[cc * DT_LD + cc];
                if (lane == cc) mine = zc;
                if (lane > cc) v = fma(-Ls[lane * DT_LD + cc], zc, v);
            }
            zv[jb * DB + lane] = mine;
        }
    }

    for (int jb = nb - 1; jb >= 0; --jb) {
        __syncthreads();
        for (int e = tid; e < DB * DB; e += 256) Ls[(e >> 6) * DT_LD + (e & 63)] = L[static_cast<size_t>(jb * DB + (e >> 6)) * mp + jb * DB + (e & 63)];
        {
            const int q = tid >> 6;
            double acc = 0.0;
            for (int l = (jb + 1) * DB + q; l < mp; l += 4) acc = fma(L[static_cast<size_t>(l) * mp + jb * DB + lane], zv[l], acc);
            red[q * DB + lane] = acc;
        }
        __syncthreads();
        if (tid < DB) {
            double v = zv[jb * DB + lane] - ((red[lane] + red[DB + lane]) + (red[2 * DB + lane] + red[3 * DB + lane])), mine = 0.0;
#pragma unroll
            for (int cc = DB - 1; cc >= 0; --cc) {
                const double bc = __shfl(v, cc) / Ls[cc * DT_LD + cc];
                if (lane == cc) mine = bc;
                if (lane < cc) v = fma(-Ls[cc * DT_LD + lane], bc, v);
            }
            zv[jb * DB + lane] = mine;
        }
    }
    __syncthreads();

    for (int j = tid; j < fill; j += 256) X[static_cast<size_t>(c) * ldx + j] = j < m ? zv[j] : 0.0;
    if (X2 != nullptr)
        for (int j = tid; j < fill2; j += 256) X2[static_cast<size_t>(c) * ld2 + j] = j < m ? zv[j] : 0.0;
    if (s != nullptr) {
        double acc = 0.0;
        for (int j = tid; j < m; j += 256) acc = fma(s[j], zv[j], acc);
        red[tid] = acc;
        __syncthreads();
        for (int stride = 128; stride > 0; stride >>= 1) {
            if (tid < stride) red[tid] += red[tid + stride];
            __syncthreads();
        }
        if (tid == 0) rhos[c] = -((eta[c] - red[0]) / Nd);
    }
}

/* One workgroup per right-hand side c: z_c alone -> Z[c ldz ...], zeros from m up to ldz.  The forward half of k_dense_solve, statement for
 * statement (a copy and not a shared function: k_dense_solve's generated code stays what it was). */
__global__ __launch_bounds__(256) void k_dense_forward(const double *__restrict__ L, int mp, int m, const double *__restrict__ rhs, double *__restrict__ Z, size_t ldz,
                                                       const unsigned *status) {
    if (dense_failed(status)) return;
    __shared__ double Ls[DB * DT_LD];
    __shared__ double zv[DENSE_MAX_RANK];
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, c = blockIdx.x;
    const int nb = mp / DB;
    const double *b = rhs + static_cast<size_t>(c) * mp;

    for (int jb = 0; jb < nb; ++jb) {
        __syncthreads();  // (wave 0 is done with the block before: Ls may be overwritten, its unknowns are in zv)
        for (int e = tid; e < DB * DB; e += 256) Ls[(e >> 6) * DT_LD + (e & 63)] = L[static_cast<size_t>(jb * DB + (e >> 6)) * mp + jb * DB + (e & 63)];
        {
            const int row = tid >> 2, q = tid & 3;
            const double *Lr = L + static_cast<size_t>(jb * DB + row) * mp;
            double acc = 0.0;
            for (int k = 2 * q; k < jb * DB; k += 8) {
                const f64x2 l2 = *reinterpret_cast<const f64x2 *>(Lr + k);
                acc = fma(l2[0], zv[k], acc);
                acc = fma(l2[1], zv[k + 1], acc);
            }
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            if (q == 0) red[row] = b[jb * DB + row] - acc;
        }
        __syncthreads();
        if (tid < DB) {
            double v = red[lane], mine = 0.0;
#pragma unroll
            for (int cc = 0; cc < DB; ++cc) {
                const double zc = __shfl(v, cc) / Ls[cc * DT_LD + cc];
                if (lane == cc) mine = zc;
                if (lane > cc) v = fma(-Ls[lane * DT_LD + cc], zc, v);
            }
            zv[jb * DB + lane] = mine;
        }
    }
    __syncthreads();
    for (int j = tid; j < static_cast<int>(ldz); j += 256) Z[static_cast<size_t>(c) * ldz + j] = j < m ? zv[j] : 0.0;
}

/* One workgroup per (checkpoint q = blockIdx.x, right-hand side c = blockIdx.y) of the rank path: with r = ranks[q],
 *   beta_j = sum_{n = j}^{r - 1} V[n][j] z_c[n]   (beta = V[:r, :r]^T z_c[:r]; thread j, j + 256, ... one chain each over the rows n ascending: the threads of a wave read
 *   one row of V side by side),   betas[(q k + c) m + j], exact zeros from r up to m;
 *   rho = -(eta_c - s[:r]^T beta) / N with the dot product as k_dense_solve takes it: 256 chains (j = tid, tid + 256, ...) and a binary tree over them.
 * The workgroups of c == 0 also leave cond[q] = max_j L_jj^2 / min_j L_jj^2 over j < r off the padded factor (mp x mp), a binary tree each for the maximum and the minimum.
 * Every order depends on r only.  No atomics. */
__global__ __launch_bounds__(256) void k_dense_prefix_beta(const double *__restrict__ Vt, int ldv, const double *__restrict__ Z, size_t ldz, int m, int k, const int *__restrict__ ranks,
                                                           const double *__restrict__ L, int mp, const double *__restrict__ s, const double *__restrict__ eta, double Nd,
                                                           double *__restrict__ betas, double *__restrict__ rhos, double *__restrict__ cond, const unsigned *status) {
    if (dense_failed(status)) return;
    __shared__ double red[256];
    __shared__ double red2[256];
    const int tid = threadIdx.x, q = blockIdx.x, c = blockIdx.y;
    const int r = ranks[q];
    const double *z = Z + static_cast<size_t>(c) * ldz;
    double *beta = betas + (static_cast<size_t>(q) * k + c) * m;
    double acc = 0.0;
    for (int j = tid; j < m; j += 256) {
        double b = 0.0;
        for (int n = j; n < r; ++n) b = fma(Vt[static_cast<size_t>(n) * ldv + j], z[n], b);
        beta[j] = b;  // (j >= r: the loop is empty, an exact zero)
        if (j < r) acc = fma(s[j], b, acc);
    }
    red[tid] = acc;
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
        if (tid < stride) red[tid] += red[tid + stride];
        __syncthreads();
    }
    if (tid == 0) rhos[static_cast<size_t>(q) * k + c] = -((eta[c] - red[0]) / Nd);
    if (c != 0) return;  // (uniform over the workgroup)
    double hi = 0.0, lo = DBL_MAX;
    for (int j = tid; j < r; j += 256) {
        const double d = L[static_cast<size_t>(j) * mp + j], d2 = d * d;
        hi = fmax(hi, d2);
        lo = fmin(lo, d2);
    }
    __syncthreads();
    red[tid] = hi;
    red2[tid] = lo;
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
        if (tid < stride) {
            red[tid] = fmax(red[tid], red[tid + stride]);
            red2[tid] = fmin(red2[tid], red2[tid + stride]);
        }
        __syncthreads();
    }
    if (tid == 0) cond[q] = red[0] / red2[0];
}

}  // namespace

DenseSpd::DenseSpd(int m, int max_rhs, hipStream_t st) : m_(m), mp_(round_up(m, DB)), nb_(round_up(m, DB) / DB), max_rhs_(std::max(max_rhs, 1)), st_(st) {
    A_.alloc_zero(static_cast<size_t>(mp_) * mp_, st);
    rhs_.alloc_zero(static_cast<size_t>(max_rhs_) * mp_, st);
    s_.alloc_zero(static_cast<size_t>(mp_), st);
    eta_.alloc_zero(static_cast<size_t>(max_rhs_), st);
    status_.alloc_zero(1, st);
}

void DenseSpd::begin_attempt() {
    LSSVM_HIP_CHECK(hipMemsetAsync(status_.p, 0, sizeof(unsigned), st_));
    launches_ = 0;
}

void DenseSpd::enqueue_assemble(const double *St_tiles, const double *Kmm, int k, double Nd, double sigma, double nu) {
    LSSVM_REQUIRE(k >= 1 && k <= max_rhs_, "DenseSpd: more right-hand sides than it was built for");
    hipLaunchKernelGGL(k_dense_assemble, dim3((mp_ + 255) / 256, mp_ + 1 + k), dim3(256), 0, st_, St_tiles, Kmm, m_, mp_, Nd, sigma, nu, A_.p, s_.p, rhs_.p, eta_.p, status_.p);
    LSSVM_HIP_CHECK(hipGetLastError());
    ++launches_;
}

void DenseSpd::enqueue_load_lower(const double *A_dev, double nu) {
    hipLaunchKernelGGL(k_dense_load_lower, dim3((mp_ + 255) / 256, mp_), dim3(256), 0, st_, A_dev, m_, mp_, nu, A_.p);
    LSSVM_HIP_CHECK(hipGetLastError());
    ++launches_;
}

void DenseSpd::enqueue_load_rhs(const double *B_dev, int k) {
    LSSVM_REQUIRE(k >= 1 && k <= max_rhs_, "DenseSpd: more right-hand sides than it was built for");
    hipLaunchKernelGGL(k_dense_pad_rows, dim3((mp_ + 255) / 256, k), dim3(256), 0, st_, B_dev, m_, mp_, rhs_.p);
    LSSVM_HIP_CHECK(hipGetLastError());
    ++launches_;
}

void DenseSpd::enqueue_factor() {
    const size_t ld = static_cast<size_t>(mp_);
    for (int jb = 0; jb < nb_; ++jb) {
        double *rows = A_.p + static_cast<size_t>(jb) * DB * ld;  // block row jb from column 0 on
        double *diag = rows + static_cast<size_t>(jb) * DB;
        if (jb > 0) {
            hipLaunchKernelGGL(k_dense_gemm<false>, dim3(nb_ - jb, 1), dim3(256), 0, st_, diag, ld, mp_ - jb * DB, rows, ld, rows, ld, jb * DB, 0, status_.p);
            ++launches_;
        }
        hipLaunchKernelGGL(k_dense_potrf_diag, dim3(1), dim3(256), 0, st_, diag, ld, jb * DB, status_.p);
        ++launches_;
        if (jb + 1 < nb_) {
            hipLaunchKernelGGL(k_dense_trsm<false>, dim3(nb_ - jb - 1), dim3(DB), 0, st_, diag + static_cast<size_t>(DB) * ld, ld, mp_ - (jb + 1) * DB, DB, -1, diag, ld, status_.p);
            ++launches_;
        }
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}

void DenseSpd::enqueue_solve(int k, double *X_out, size_t ldx, double *X2_out, size_t ld2, bool with_rho, double Nd, double *rhos_out) {
    LSSVM_REQUIRE(k >= 1 && k <= max_rhs_, "DenseSpd: more right-hand sides than it was built for");
    hipLaunchKernelGGL(k_dense_solve, dim3(k), dim3(256), 0, st_, A_.p, mp_, m_, rhs_.p, X_out, ldx, m_, X2_out, ld2, static_cast<int>(ld2), with_rho ? s_.p : nullptr, eta_.p, Nd, rhos_out,
                       status_.p);
    LSSVM_HIP_CHECK(hipGetLastError());
    ++launches_;
}

void DenseSpd::enqueue_forward(int k, double *Z_out, size_t ldz) {
    LSSVM_REQUIRE(k >= 1 && k <= max_rhs_ && ldz >= static_cast<size_t>(m_), "DenseSpd: more right-hand sides than it was built for, or rows of z shorter than m");
    hipLaunchKernelGGL(k_dense_forward, dim3(k), dim3(256), 0, st_, A_.p, mp_, m_, rhs_.p, Z_out, ldz, status_.p);
    LSSVM_HIP_CHECK(hipGetLastError());
    ++launches_;
}

void DenseSpd::enqueue_prefix_betas(const double *Vt, int ldv, const double *Z, size_t ldz, int k, const int *ranks_dev, int num_ranks, double Nd, double *betas_out, double *rhos_out,
                                    double *cond_out) {
    LSSVM_REQUIRE(k >= 1 && k <= max_rhs_ && num_ranks >= 1 && ldv >= m_ && ldz >= static_cast<size_t>(m_), "DenseSpd: the prefix betas take the operands enqueue_invert and enqueue_forward left");
    hipLaunchKernelGGL(k_dense_prefix_beta, dim3(num_ranks, k), dim3(256), 0, st_, Vt, ldv, Z, ldz, m_, k, ranks_dev, A_.p, mp_, s_.p, eta_.p, Nd, betas_out, rhos_out, cond_out, status_.p);
    LSSVM_HIP_CHECK(hipGetLastError());
    ++launches_;
}

void DenseSpd::enqueue_invert(double *Vt_out, int ldv) {
    LSSVM_REQUIRE(ldv >= m_ && ldv % 16 == 0, "DenseSpd: the rows of the inverse are a multiple of 16 doubles apart");
    LSSVM_HIP_CHECK(hipMemsetAsync(Vt_out, 0, static_cast<size_t>(m_) * ldv * sizeof(double), st_));
    const size_t ld = static_cast<size_t>(mp_), lv = static_cast<size_t>(ldv);
    for (int i = 0; i < nb_; ++i) {
        double *vrows = Vt_out + static_cast<size_t>(i) * DB * lv;        // block row i of V
        const double *lrows = A_.p + static_cast<size_t>(i) * DB * ld;    // block row i of L
        const int rows_valid = m_ - i * DB;
        if (i > 0) {
            hipLaunchKernelGGL(k_dense_gemm<true>, dim3(1, i), dim3(256), 0, st_, vrows, lv, rows_valid, lrows, ld, static_cast<const double *>(Vt_out), lv, i * DB, 1, status_.p);
            ++launches_;
        }
        hipLaunchKernelGGL(k_dense_trsm<true>, dim3(i + 1), dim3(DB), 0, st_, vrows, lv, rows_valid, ldv, i, lrows + static_cast<size_t>(i) * DB, ld, status_.p);
        ++launches_;
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}

void DenseSpd::enqueue_store_factor(double *L_dev) {
    hipLaunchKernelGGL(k_dense_store_lower, dim3((m_ + 255) / 256, m_), dim3(256), 0, st_, A_.p, m_, mp_, L_dev);
    LSSVM_HIP_CHECK(hipGetLastError());
    ++launches_;
}

unsigned DenseSpd::status() {
    unsigned word = 0;
    LSSVM_HIP_CHECK(hipMemcpyAsync(&word, status_.p, sizeof(unsigned), hipMemcpyDeviceToHost, st_));
    LSSVM_HIP_CHECK(hipStreamSynchronize(st_));
    return word;
}

DenseStopwatch::DenseStopwatch(hipStream_t st) : st_(st) {
    for (Event &e : ev_) e.create(true);
}

void DenseStopwatch::mark(int i) { LSSVM_HIP_CHECK(hipEventRecord(ev_[i].e, st_)); }

void DenseStopwatch::read(bool with_invert, DenseTimes &t) const {
    t.assemble_ms = elapsed_ms(ev_[0], ev_[1]);
    t.factor_ms = elapsed_ms(ev_[1], ev_[2]);
    t.solve_ms = elapsed_ms(ev_[2], ev_[3]);
    t.invert_ms = with_invert ? elapsed_ms(ev_[3], ev_[4]) : 0.0;
}

/* ---- the three testing aids (include/plssvm_amd_testing.h): host arrays in, the toolbox on device 0, host arrays out; the arguments have been checked ---- */
namespace {

struct AidStream {
    Stream stream;
    AidStream() {
        select_device_checked(0);
        stream.create();
    }
};

float span_ms(const Event &a, const Event &b, hipStream_t st) {
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    return elapsed_ms(a, b);
}

}  // namespace

void dense_cholesky_aid(const double *A, int m, double nu, double *L_out, uint64_t *status_out, double *ms_out) {
    AidStream s;
    hipStream_t st = s.stream.s;
    const size_t mm = static_cast<size_t>(m) * m;
    DevBuf<double> in, out;
    in.alloc_zero(mm, st);
    out.alloc_zero(mm, st);
    LSSVM_HIP_CHECK(hipMemcpyAsync(in.p, A, mm * sizeof(double), hipMemcpyHostToDevice, st));
    DenseSpd dense(m, 1, st);
    Event ev[2];
    for (Event &e : ev) e.create(true);
    dense.begin_attempt();
    dense.enqueue_load_lower(in.p, nu);
    LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
    dense.enqueue_factor();
    LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
    const unsigned status = dense.status();
    if (status == 0) {
        dense.enqueue_store_factor(out.p);
        LSSVM_HIP_CHECK(hipMemcpyAsync(L_out, out.p, mm * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    const float ms = span_ms(ev[0], ev[1], st);
    if (status != 0) std::fill(L_out, L_out + mm, 0.0);
    *status_out = status;
    if (ms_out != nullptr) *ms_out = ms;
}

void dense_solve_aid(const double *L, int m, const double *B, int k, double *X_out, double *ms_out) {
    AidStream s;
    hipStream_t st = s.stream.s;
    const size_t mm = static_cast<size_t>(m) * m, km = static_cast<size_t>(k) * m;
    DevBuf<double> in, rhs, out;
    in.alloc_zero(mm, st);
    rhs.alloc_zero(km, st);
    out.alloc_zero(km, st);
    LSSVM_HIP_CHECK(hipMemcpyAsync(in.p, L, mm * sizeof(double), hipMemcpyHostToDevice, st));
    LSSVM_HIP_CHECK(hipMemcpyAsync(rhs.p, B, km * sizeof(double), hipMemcpyHostToDevice, st));
    DenseSpd dense(m, k, st);
    Event ev[2];
    for (Event &e : ev) e.create(true);
    dense.begin_attempt();
    dense.enqueue_load_lower(in.p, 0.0);
    dense.enqueue_load_rhs(rhs.p, k);
    LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
    dense.enqueue_solve(k, out.p, static_cast<size_t>(m), nullptr, 0, false, 1.0, nullptr);
    LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
    LSSVM_HIP_CHECK(hipMemcpyAsync(X_out, out.p, km * sizeof(double), hipMemcpyDeviceToHost, st));
    const float ms = span_ms(ev[0], ev[1], st);
    if (ms_out != nullptr) *ms_out = ms;
}

void dense_invert_lower_aid(const double *L, int m, double *V_out, double *ms_out) {
    AidStream s;
    hipStream_t st = s.stream.s;
    const size_t mm = static_cast<size_t>(m) * m;
    const int ldv = round_up(m, 16);
    DevBuf<double> in, out;
    in.alloc_zero(mm, st);
    out.alloc_zero(static_cast<size_t>(m) * ldv, st);
    LSSVM_HIP_CHECK(hipMemcpyAsync(in.p, L, mm * sizeof(double), hipMemcpyHostToDevice, st));
    DenseSpd dense(m, 1, st);
    Event ev[2];
    for (Event &e : ev) e.create(true);
    dense.begin_attempt();
    dense.enqueue_load_lower(in.p, 0.0);
    LSSVM_HIP_CHECK(hipEventRecord(ev[0].e, st));
    dense.enqueue_invert(out.p, ldv);
    LSSVM_HIP_CHECK(hipEventRecord(ev[1].e, st));
    LSSVM_HIP_CHECK(hipMemcpy2DAsync(V_out, static_cast<size_t>(m) * sizeof(double), out.p, static_cast<size_t>(ldv) * sizeof(double), static_cast<size_t>(m) * sizeof(double),
                                     static_cast<size_t>(m), hipMemcpyDeviceToHost, st));
    const float ms = span_ms(ev[0], ev[1], st);
    if (ms_out != nullptr) *ms_out = ms;
}

}  // namespace lssvm
