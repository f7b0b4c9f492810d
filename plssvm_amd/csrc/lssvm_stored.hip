/*
 * lssvm_stored.hip -- the kernel matrix of a resident problem KEPT in HBM, and K * V for up to sixteen vectors from one pass over it (DESIGN.md section 21;
 * lssvm_mi355_problem_store_gram, _drop_gram, _matvec_stored, _solve_lockstep_stored).  Opt-in: every other path evaluates the matrix from the data in every pass.
 *
 * ASSEMBLY, once per problem: k_store_gram evaluates the (N-1) x (N-1) matrix K of the reduced system -- what CgSteps calls K in Kv; the diagonal term, q and QA_cost stay
 * in the O(n) kernels -- tile by tile on and below the diagonal.  The dot products run in double on v_mfma_f64_16x16x4_f64 through the tile loop of the fixed-size kernels
 * (lssvm_tile_loop_f64.hip.hpp) over the resident data as X_ holds it (centred and scaled; LandmarkBlock::kernel_scalars has the rule for gamma), the kernel function is
 * evaluated in double (landmark_kernel_value; rbf: the norm expansion clamped at 0, the diagonal exactly 1) and every entry is rounded ONCE to the real type T on the store.
 * Entries of rows or columns from N-1 on are exact zeros, so the pass carries no bounds test.  No atomics: a tile's bits depend on its two row blocks only.
 *
 * LAYOUT: the 128 x 128 tiles (I, J), J <= I, at tile index I (I + 1) / 2 + J, each contiguous.  Inside a tile the order is the one a wave of the pass loads:
 * wave w owns the rows 32 w ... 32 w + 31; its strip is sixteen 16 x 16 blocks in the order cb (column block, 0 ... 7), then rb (row block, 0 ... 1); a block is stored as
 * 16-byte pieces, piece h of lane 16 qd + r = the entries (row 16 rb + r, columns 16 cb + 4 qd + V h ... + V - 1), V = 16 / sizeof(T) -- so every load instruction of a
 * wave reads 1 KiB contiguous, and the lane's registers ARE the A operand of the row product (stored_index below).
 *
 * THE PASS, tile_symm_stored<T>: persistent workgroups of four waves walk work items (row block I, sixteen column tiles) dealt round robin, longest first.  A wave streams
 * its strip of every tile straight from HBM into registers, two groups of blocks deep (128 bytes per lane in flight under the MFMAs of the group before), and uses it twice:
 *   row product    out_I += K_IJ V_J: register e of a block is A[row r][k = qd] of column 16 cb + 4 qd + e, B comes from the packed vectors; two accumulators per wave, kept
 *                  across the work item, stored once to the item's plane of the row slab;
 *   mirror product K_IJ^T V_I: the block goes through a 16 x 16 scratch of the wave's own in LDS (20 reals between rows: the transposed read is conflict free) and
 *                  comes back as B[k = qd][column r] against A = V_I of the wave's rows; the four waves' sums over their rows meet in a staging area per half tile and
 *                  leave, added in wave order (w0 + w1) + (w2 + w3), as the tile's column record.
 * Both on v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32.  k_fold_stored adds, per entry of K * v, the row slabs of its block's items in ascending order and then the
 * column records of the row blocks below in ascending order (four interleaved partial sums, combined in a fixed order).  No atomics anywhere: the order of every sum depends
 * on the shape only, and a vector's result neither on its slot nor on the other vectors -- every pass runs all sixteen slots, the empty ones on exact zeros.
 */
#include "lssvm_dense.hip.hpp"
#include "lssvm_landmark.hip.hpp"

namespace lssvm {

constexpr int ST_JC = 16;                      // column tiles per work item
constexpr int ST_TILE_ELEMS = TILE * TILE;
constexpr int ST_LDP = 20;                     // reals between two rows of a transposition block
constexpr size_t ST_FREE_MARGIN = size_t(1) << 30;  // store_gram(0): what hipMemGetInfo reports free, less 1 GiB

namespace {

#include "lssvm_tile_loop_f64.hip.hpp"
#include "lssvm_stored_common.hip.hpp"  // StoredTraits, StoredVectors, stored_select, k_pack_stored_v

/* where entry (row, col) of a tile lives inside it (the layout above) */
template <typename T>
__device__ __forceinline__ int stored_index(int row, int col) {
    constexpr int V = StoredTraits<T>::V, H = StoredTraits<T>::H;
    const int w = row >> 5, rb = (row >> 4) & 1, r = row & 15, cb = col >> 4, qd = (col >> 2) & 3, e = col & 3;
    return ((((w * 8 + cb) * 2 + rb) * H + e / V) * 64 + 16 * qd + r) * V + e % V;
}

/* n[i] = |x_i|^2 of the data as held, in double, features ascending */
template <typename T>
__global__ __launch_bounds__(256) void k_stored_norms(const T *__restrict__ X, int ldx, int n, double *__restrict__ norms) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const T *xi = X + static_cast<size_t>(i) * ldx;
    double acc = 0.0;
    for (int f = 0; f < ldx; ++f) acc += static_cast<double>(xi[f]) * static_cast<double>(xi[f]);
    norms[i] = acc;
}

/* tile (I = blockIdx.y, J = blockIdx.x), J <= I, of the stored matrix: the dot products x_i . x_j over the ldx held features on the shared tile loop (A: the tile's columns,
 * B: its rows -- sixteen lanes then store neighbouring pieces), the kernel function in double, one rounding to T.  `n` = N - 1 points; `norms`: rbf only. */
template <typename T>
__global__ __launch_bounds__(256, 2) void k_store_gram(const T *__restrict__ X, int ldx, int n, int kernel_type, int degree, double gamma, double coef0,
                                                       const double *__restrict__ norms, T *__restrict__ tiles) {
    __shared__ __attribute__((aligned(16))) double As[RG_TW * RG_LS];
    __shared__ __attribute__((aligned(16))) double Bs[RG_TW * RG_LS];
    const int I = blockIdx.y, J = blockIdx.x;
    if (J > I) return;
    const TileLanes t;
    const T *Ag[4], *Bg[4];
    bool a_in[4], b_in[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int ja = J * TILE + t.srow + 32 * p, ib = I * TILE + t.srow + 32 * p;
        a_in[p] = ja < n;
        b_in[p] = ib < n;
        Ag[p] = X + static_cast<size_t>(a_in[p] ? ja : 0) * ldx + 2 * t.sseg;
        Bg[p] = X + static_cast<size_t>(b_in[p] ? ib : 0) * ldx + 2 * t.sseg;
    }
    const int lds_w = t.srow * RG_LS + 2 * t.sseg;
    f64x2 sa[4], sb[4];
    const f64x2 zero2 = { 0.0, 0.0 };
    auto stage_load = [&](int s) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            sa[p] = zero2;
            sb[p] = zero2;
            if (a_in[p]) sa[p] = f64x2{ static_cast<double>(Ag[p][s * RG_KC]), static_cast<double>(Ag[p][s * RG_KC + 1]) };
            if (b_in[p]) sb[p] = f64x2{ static_cast<double>(Bg[p][s * RG_KC]), static_cast<double>(Bg[p][s * RG_KC + 1]) };
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
    tile_zero(acc);
    tile_contract<16 * RG_LS, 4>(ldx / RG_KC, As + (t.wr * 64 + t.r) * RG_LS + t.qd, Bs + (t.wc * 64 + t.r) * RG_LS + t.qd, acc, stage_load, stage_store);

    // a lane holds columns wr 64 + mt 16 + qd + 4 i and row wc 64 + nt 16 + r of the tile
    const bool rbf = kernel_type == LSSVM_KERNEL_RBF;
    T *out = tiles + (static_cast<size_t>(I) * (I + 1) / 2 + J) * ST_TILE_ELEMS;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int lrow = t.wc * 64 + nt * 16 + t.r, row = I * TILE + lrow;
        const double ni = rbf && row < n ? norms[row] : 0.0;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int lcol = t.wr * 64 + mt * 16 + t.qd + 4 * i, col = J * TILE + lcol;
                double k = 0.0;
                if (row < n && col < n) {
                    double d = acc[mt][nt][i];
                    if (rbf) d = row == col ? 0.0 : fmax((ni + norms[col]) - 2.0 * d, 0.0);
                    k = landmark_kernel_value(kernel_type, degree, gamma, coef0, d);
                }
                out[stored_index<T>(lrow, lcol)] = static_cast<T>(k);
            }
    }
}

/* one group of G blocks of a wave's strip, as loaded: the kernel values and -- per column block -- the vectors' entries of its columns */
template <typename T>
struct StoredGroup {
    typename StoredTraits<T>::vec k[StoredTraits<T>::G][StoredTraits<T>::H];
    typename StoredTraits<T>::vec v[StoredTraits<T>::G / 2][StoredTraits<T>::H];
};

/* The pass (the file's head has the design).  items[it] = (row block I, column chunk c): the tiles (I, J), c ST_JC <= J < min((c + 1) ST_JC, I + 1).
 * rowpart[(c 16 + u) npad + 128 I + row]: the item's row sums of vector u; colrec[((I (I - 1) / 2 + J) 16 + u) 128 + column]: tile (I, J)'s mirror sums, J < I.
 * 256 threads, two workgroups per CU: at most 256 registers, LDS 52 KiB (fp64) / 26 KiB (fp32). */
template <typename T>
__global__ __launch_bounds__(256, 2) void tile_symm_stored(const T *__restrict__ tiles, const T *__restrict__ Vp, const int2 *__restrict__ items, int num_items, int npad,
                                                           T *__restrict__ rowpart, T *__restrict__ colrec) {
    using S = StoredTraits<T>;
    using vec = typename S::vec;
    using acc_t = typename S::acc;
    constexpr int V = S::V, H = S::H, G = S::G, NG = 16 / G;
    __shared__ __attribute__((aligned(16))) T stage[4 * BLOCK_VECTORS * 64];  // [wave][vector][column of the half tile]
    __shared__ __attribute__((aligned(16))) T scratch[4 * 2 * 16 * ST_LDP];   // [wave][2][row][ST_LDP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, qd = lane >> 4;
    T *my_scratch = scratch + wave * 2 * 16 * ST_LDP;
    const int sc_w = r * ST_LDP + 4 * qd;  // the write: row r, columns 4 qd ...
    const int sc_r = 4 * qd * ST_LDP + r;  // the read: rows 4 qd + e', column r

    for (int it = blockIdx.x; it < num_items; it += gridDim.x) {
        const int I = items[it].x, c = items[it].y;
        const int J0 = c * ST_JC, ntiles = min(J0 + ST_JC, I + 1) - J0;
        const int total = ntiles * NG;
        const T *row_tiles = tiles + (static_cast<size_t>(I) * (I + 1) / 2 + J0) * ST_TILE_ELEMS + wave * (ST_TILE_ELEMS / 4) + lane * V;
        // the wave's rows of V_I, the A operand of the mirror product: vi[rb][e'] = V_I[row 16 rb + 4 qd + e'][vector r]
        T vi[2][4];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const T *src = Vp + ((static_cast<size_t>(I) * 32 + wave * 8 + rb * 4 + qd) * BLOCK_VECTORS + r) * 4;
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const vec x = *reinterpret_cast<const vec *>(src + h * V);
#pragma unroll
                for (int e = 0; e < V; ++e) vi[rb][h * V + e] = x[e];
            }
        }
        acc_t out[2], colout;
#pragma unroll
        for (int i = 0; i < 4; ++i) out[0][i] = out[1][i] = colout[i] = T(0);
        asm volatile("" : "+v"(out[0]), "+v"(out[1]), "+v"(colout));  // (the start values live in the accumulators' own registers)

        auto load = [&](int gi, StoredGroup<T> &g) {
            const int jt = gi / NG, gg = gi % NG;
            const T *kp = row_tiles + static_cast<size_t>(jt) * ST_TILE_ELEMS + gg * (G * 256);
#pragma unroll
            for (int b = 0; b < G; ++b)
#pragma unroll
                for (int h = 0; h < H; ++h) g.k[b][h] = *reinterpret_cast<const vec *>(kp + (b * H + h) * 64 * V);
            const T *vp = Vp + ((static_cast<size_t>(J0 + jt) * 32 + gg * (G / 2) * 4 + qd) * BLOCK_VECTORS + r) * 4;
#pragma unroll
            for (int cbl = 0; cbl < G / 2; ++cbl)
#pragma unroll
                for (int h = 0; h < H; ++h) g.v[cbl][h] = *reinterpret_cast<const vec *>(vp + cbl * 4 * BLOCK_VECTORS * 4 + h * V);
        };
        auto compute = [&](int gi, const StoredGroup<T> &g) {
            const int jt = gi / NG, gg = gi % NG;
            const bool below = J0 + jt < I;  // (the diagonal tile is stored in full and serves the rows only)
#pragma unroll
            for (int b = 0; b < G; ++b) {
                const int rb = b & 1;
                const int cb = gg * (G / 2) + (b >> 1);
                T kv[4], vj[4];
#pragma unroll
                for (int h = 0; h < H; ++h)
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        kv[h * V + e] = g.k[b][h][e];
                        vj[h * V + e] = g.v[b >> 1][h][e];
                    }
                T *blk = my_scratch + rb * 16 * ST_LDP;
                if (below) {
#pragma unroll
                    for (int h = 0; h < H; ++h) *reinterpret_cast<vec *>(blk + sc_w + h * V) = g.k[b][h];
                    asm volatile("" ::: "memory");  // (a wave's LDS operations execute in order: the read below sees every lane's write)
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) out[rb] = S::mfma(kv[e], vj[e], out[rb]);
                if (below) {
                    T kt[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) kt[e] = blk[sc_r + e * ST_LDP];
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int e = 0; e < 4; ++e) colout = S::mfma(vi[rb][e], kt[e], colout);
                    if (rb == 1) {  // the column block is complete over this wave's rows: colout[i] = (vector acc_row(qd, i), column 16 cb + r)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            stage[(wave * BLOCK_VECTORS + S::acc_row(qd, i)) * 64 + 16 * (cb & 3) + r] = colout[i];
                            colout[i] = T(0);
                        }
                        asm volatile("" : "+v"(colout));
                        if ((cb & 3) == 3) {  // a half tile: the four waves' sums in wave order, out as 64 columns of the tile's record
                            __syncthreads();
                            T *rec = colrec + ((static_cast<size_t>(I) * (I - 1) / 2 + J0 + jt) * BLOCK_VECTORS) * TILE + (cb >> 2) * 64;
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const int idx = tid + 256 * q, u = idx >> 6, jj = idx & 63;
                                const T *p = stage + u * 64 + jj;
                                rec[u * TILE + jj] = (p[0] + p[BLOCK_VECTORS * 64]) + (p[2 * BLOCK_VECTORS * 64] + p[3 * BLOCK_VECTORS * 64]);
                            }
                            __syncthreads();
                        }
                    }
                }
            }
        };

        StoredGroup<T> ga, gb;
        load(0, ga);
        for (int gi = 0; gi < total; gi += 2) {
            if (gi + 1 < total) load(gi + 1, gb);
            compute(gi, ga);
            if (gi + 1 < total) {
                if (gi + 2 < total) load(gi + 2, ga);
                compute(gi + 1, gb);
            }
        }
        // out[rb][i] = (row 32 wave + 16 rb + acc_row(qd, i), vector r)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                rowpart[(static_cast<size_t>(c) * BLOCK_VECTORS + r) * npad + I * TILE + wave * 32 + rb * 16 + S::acc_row(qd, i)] = out[rb][i];
    }
}

/* Kv_u[j] = the row slabs of j's block (its items in ascending order) + the column records of the row blocks below (ascending: four interleaved partial sums, then
 * (s0 + s1) + (s2 + s3)), for u = blockIdx.y < nv and every j < npad */
template <typename T>
__global__ __launch_bounds__(256) void k_fold_stored(const T *__restrict__ rowpart, const T *__restrict__ colrec, int npad, int num_tiles, const StoredVectors<T> Kv) {
    const int j = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
    if (j >= npad) return;
    const int J = j / TILE, jl = j % TILE;
    T rows = rowpart[static_cast<size_t>(u) * npad + j];
    for (int c = 1; c <= J / ST_JC; ++c) rows += rowpart[(static_cast<size_t>(c) * BLOCK_VECTORS + u) * npad + j];
    auto rec = [&](int I) { return colrec[((static_cast<size_t>(I) * (I - 1) / 2 + J) * BLOCK_VECTORS + u) * TILE + jl]; };
    T s0 = T(0), s1 = T(0), s2 = T(0), s3 = T(0);
    int I = J + 1;
    for (; I + 3 < num_tiles; I += 4) {
        s0 += rec(I);
        s1 += rec(I + 1);
        s2 += rec(I + 2);
        s3 += rec(I + 3);
    }
    for (; I < num_tiles; ++I) s0 += rec(I);
    stored_select(Kv, u)[j] = rows + ((s0 + s1) + (s2 + s3));
}

}  // namespace

/* ------------------------------------------------------------------ Problem<T>: store, drop, apply ------------------------------------------------------------------ */
template <typename T>
size_t Problem<T>::stored_gram_bytes() const {
    const size_t nt = static_cast<size_t>(num_tiles_), npad = nt * TILE;
    const size_t tiles = nt * (nt + 1) / 2 * ST_TILE_ELEMS, recs = std::max<size_t>(nt * (nt - 1) / 2, 1) * BLOCK_VECTORS * TILE;
    const size_t rows = ((nt - 1) / ST_JC + 1) * BLOCK_VECTORS * npad, vp = npad * BLOCK_VECTORS;
    return (tiles + recs + rows + vp) * sizeof(T);
}

template <typename T>
bool Problem<T>::store_gram(size_t max_bytes, size_t *bytes_out, double *assemble_ms_out) {
    activate();
    hipStream_t st = stream_.s;
    drop_gram();
    if (bytes_out != nullptr) *bytes_out = 0;
    if (assemble_ms_out != nullptr) *assemble_ms_out = 0.0;
    if (world_ != 1 || num_tiles_ < 1) return false;
    const size_t need = stored_gram_bytes();
    size_t cap = max_bytes;
    if (cap == 0) {
        size_t free_b = 0, total_b = 0;
        LSSVM_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        cap = free_b > ST_FREE_MARGIN ? free_b - ST_FREE_MARGIN : 0;
    }
    if (need > cap) return false;  // declined: nothing allocated
    const size_t nt = static_cast<size_t>(num_tiles_), npad = nt * TILE;
    // the work items, longest first (row blocks descending; a block's full chunks before its clipped last one), dealt round robin to the persistent workgroups
    std::vector<int2> items;
    for (int I = num_tiles_ - 1; I >= 0; --I)
        for (int c = 0; c <= I / ST_JC; ++c) items.push_back(int2{ I, c });
    try {
        gram_.alloc_zero(nt * (nt + 1) / 2 * ST_TILE_ELEMS, st);
        gram_colrec_.alloc_zero(std::max<size_t>(nt * (nt - 1) / 2, 1) * BLOCK_VECTORS * TILE, st);
        gram_rowpart_.alloc_zero(((nt - 1) / ST_JC + 1) * BLOCK_VECTORS * npad, st);
        gram_vp_.alloc_zero(npad * BLOCK_VECTORS, st);
        gram_items_.alloc_zero(items.size(), st);
    } catch (const Error &e) {
        drop_gram();
        if (e.status == LSSVM_ERR_OUT_OF_MEMORY) return false;  // (the free memory went elsewhere between the question and the allocation: declined as well)
        throw;
    }
    LSSVM_HIP_CHECK(hipMemcpyAsync(gram_items_.p, items.data(), items.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    gram_num_items_ = static_cast<int>(items.size());
    int cus = 0;
    LSSVM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_));
    gram_grid_ = std::max(1, std::min(gram_num_items_, 2 * cus));

    double gamma = 0.0, coef0 = 0.0;
    LandmarkBlock<T>::kernel_scalars(*this, gamma, coef0);
    DevBuf<double> norms;
    Event a, b;
    a.create(true);
    b.create(true);
    LSSVM_HIP_CHECK(hipEventRecord(a.e, st));
    if (params_.kernel_type == LSSVM_KERNEL_RBF) {
        norms.alloc_zero(npad, st);
        hipLaunchKernelGGL(k_stored_norms<T>, dim3((n_ + 255) / 256), dim3(256), 0, st, X_.data.p, X_.ldx, n_, norms.p);
    }
    hipLaunchKernelGGL(k_store_gram<T>, dim3(num_tiles_, num_tiles_), dim3(256), 0, st, X_.data.p, X_.ldx, n_, params_.kernel_type, params_.degree, gamma, coef0, norms.p, gram_.p);
    LSSVM_HIP_CHECK(hipGetLastError());
    LSSVM_HIP_CHECK(hipEventRecord(b.e, st));
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (`items` and `norms` go out of scope)
    if (assemble_ms_out != nullptr) *assemble_ms_out = static_cast<double>(elapsed_ms(a, b));
    if (bytes_out != nullptr) *bytes_out = need;
    return true;
}

template <typename T>
void Problem<T>::drop_gram() {
    if (gram_.p == nullptr && gram_colrec_.p == nullptr) return;
    activate();
    (void) hipStreamSynchronize(stream_.s);
    for (DevBuf<T> *buf : { &gram_, &gram_colrec_, &gram_rowpart_, &gram_vp_ }) buf->release();
    gram_items_.release();
    gram_num_items_ = 0;
}

template <typename T>
void Problem<T>::enqueue_apply_K_stored(const T *const *v, T *const *Kv, int nv, hipEvent_t ev_begin, hipEvent_t ev_end) {
    LSSVM_REQUIRE(gram_stored(), "no stored kernel matrix on this problem");
    LSSVM_REQUIRE(nv >= 1 && nv <= BLOCK_VECTORS, "a stored pass takes 1 ... 16 vectors");
    hipStream_t st = stream_.s;
    const int npad = num_tiles_ * TILE;
    StoredVectors<const T> src{};
    StoredVectors<T> dst{};
    for (int u = 0; u < BLOCK_VECTORS; ++u) {
        src.p[u] = v[std::min(u, nv - 1)];
        dst.p[u] = Kv[std::min(u, nv - 1)];
    }
    hipLaunchKernelGGL(k_pack_stored_v<T>, dim3((static_cast<unsigned>(npad) * BLOCK_VECTORS + 255) / 256), dim3(256), 0, st, src, nv, n_, npad, gram_vp_.p);
    if (ev_begin != nullptr) LSSVM_HIP_CHECK(hipEventRecord(ev_begin, st));
    hipLaunchKernelGGL(tile_symm_stored<T>, dim3(gram_grid_), dim3(256), 0, st, gram_.p, gram_vp_.p, gram_items_.p, gram_num_items_, npad, gram_rowpart_.p, gram_colrec_.p);
    if (ev_end != nullptr) LSSVM_HIP_CHECK(hipEventRecord(ev_end, st));
    hipLaunchKernelGGL(k_fold_stored<T>, dim3((npad + 255) / 256, nv), dim3(256), 0, st, gram_rowpart_.p, gram_colrec_.p, npad, num_tiles_, dst);
    LSSVM_HIP_CHECK(hipGetLastError());
}

template size_t Problem<float>::stored_gram_bytes() const;
template size_t Problem<double>::stored_gram_bytes() const;
template bool Problem<float>::store_gram(size_t, size_t *, double *);
template bool Problem<double>::store_gram(size_t, size_t *, double *);
template void Problem<float>::drop_gram();
template void Problem<double>::drop_gram();
template void Problem<float>::enqueue_apply_K_stored(const float *const *, float *const *, int, hipEvent_t, hipEvent_t);
template void Problem<double>::enqueue_apply_K_stored(const double *const *, double *const *, int, hipEvent_t, hipEvent_t);

}  // namespace lssvm
