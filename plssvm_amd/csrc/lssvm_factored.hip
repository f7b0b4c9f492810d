/*
 * lssvm_factored.hip -- the factored linear-kernel operator of a resident problem: K V = X (X^T V) for up to sixteen vectors from TWO reads of the data (DESIGN.md
 * section 22; lssvm_mi355_problem_matvec_factored, _solve_lockstep_factored).  Opt-in: every other path evaluates the n x n kernel matrix, for the linear kernel too.
 *
 * For the linear kernel K = gamma' X X^T exactly (gamma' = 1 / x_scale^2 for data held scaled, LandmarkBlock::kernel_scalars; 1 otherwise), so a pass costs 4 n d flop per
 * vector instead of 2 n^2 d.  Everything reads the resident X_ as k_store_gram does: row major, ldx padded features, the first n = N - 1 rows.  With S =
 * LSSVM_FACTORED_SLAB_ROWS rows per slab and a 16-byte PIECE = V reals (4 floats / 2 doubles) of one row, loaded by one lane with one global_load_dwordx4:
 *
 *   k_factored_gather   W_s = X_s^T V_s per slab s, on v_mfma_*_16x16x4 with feature along M, vector along N, row along k.  Persistent workgroups of four waves take the
 *                       slabs in a fixed deal; wave w owns the rows 128 w ... 128 w + 127 of the slab as eight blocks of 16 rows and walks the features in panels of 16
 *                       pieces.  Lane 16 qd + r loads piece r of the panel from the rows 4 qd + e (e = 0 ... 3) of a block: a wave instruction reads four runs of 256
 *                       contiguous bytes, and register c of the piece IS the A operand A[feature V r + c][k = qd] -- a permuted feature set per register, undone only in the
 *                       index of the store.  B[k = qd][vector r] = row 4 qd + e of Vp, the k-major packed vectors (k_pack_stored_v), loaded once per slab and held.  No LDS
 *                       staging of X: two groups of loads (block, panel) are in flight under the MFMAs of the group before.  After a panel the four waves' sums meet in LDS
 *                       and leave added in wave order (w0 + w1) + (w2 + w3) as W_part[slab][feature][vector].
 *   k_factored_fold     W = sum over the slabs in ascending order (four interleaved partial sums, then (s0 + s1) + (s2 + s3)), times gamma', written k-major for the second
 *                       product: Wp[feature / 4][vector][feature % 4].
 *   k_factored_scatter  out_s = X_s W with row along M, vector along N, feature along k: lane 16 qd + r loads piece 4 c + qd of row r of a block (step c: 16 rows x 64
 *                       contiguous bytes per wave instruction), register e is A[row r][k = qd] of feature V (4 c + qd) + e and B comes from Wp with the same mapping, through
 *                       L1 / L2 (Wp is ldx x 16 reals: any width works).  One accumulator per 16 rows, stored once, straight into the sixteen result vectors.
 *
 * X is read exactly twice per pass whatever the vector count.  No atomics, no scratch, two workgroups per CU.  Every pass runs all sixteen slots, the empty ones on exact
 * zeros, and the order of every sum depends on (N, ldx, T) only -- not on the CU count, the slot or the other vectors.  Rows from N - 1 on meet exact zeros of Vp in the
 * gather (their loads are clamped to row n - 1, never out of bounds) and are not stored by the scatter.
 */
#include "lssvm_landmark.hip.hpp"

namespace lssvm {

constexpr int FT_SLAB = LSSVM_FACTORED_SLAB_ROWS;
constexpr int FT_BLOCKS = FT_SLAB / 4 / 16;  // 16-row blocks of a wave's share of a slab
static_assert(FT_SLAB % 64 == 0, "a slab is whole 16-row blocks for each of the four waves");

namespace {

#include "lssvm_stored_common.hip.hpp"  // StoredTraits, StoredVectors, stored_select, k_pack_stored_v

/* the four pieces a lane holds of one group: gather -- the rows 4 qd + e of a block at one panel; scatter -- four steps of one block, with Wp's pieces beside them */
template <typename T>
struct FactoredGroup {
    typename StoredTraits<T>::vec x[4];
    typename StoredTraits<T>::vec w[4];  // (scatter only)
};

/* W_part[(slab ldx + f) 16 + u] = sum over the slab's rows j of X[j][f] v_u[j].  Vp: k_pack_stored_v's, nslabs FT_SLAB rows.  256 threads, LDS 16 KiB. */
template <typename T>
__global__ __launch_bounds__(256, 2) void k_factored_gather(const T *__restrict__ X, int ldx, int n, int nslabs, const T *__restrict__ Vp, T *__restrict__ Wpart) {
    using S = StoredTraits<T>;
    using vec = typename S::vec;
    using acc_t = typename S::acc;
    constexpr int V = S::V, H = S::H, PF = 16 * V;                      // features of a panel: 64 / 32
    __shared__ __attribute__((aligned(16))) T stage[4 * PF * BLOCK_VECTORS];  // [wave][feature of the panel][vector]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, qd = lane >> 4;
    const int npanels = (ldx + PF - 1) / PF;

    for (int slab = blockIdx.x; slab < nslabs; slab += gridDim.x) {
        const int row0 = slab * FT_SLAB + wave * (FT_SLAB / 4);
        // B, held for the slab: vb[b][e] = v_r[row0 + 16 b + 4 qd + e]
        T vb[FT_BLOCKS][4];
#pragma unroll
        for (int b = 0; b < FT_BLOCKS; ++b) {
            const T *src = Vp + ((static_cast<size_t>(row0 / 4 + 4 * b + qd)) * BLOCK_VECTORS + r) * 4;
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const vec x = *reinterpret_cast<const vec *>(src + h * V);
#pragma unroll
                for (int e = 0; e < V; ++e) vb[b][h * V + e] = x[e];
            }
        }
        acc_t acc[V];  // acc[c][i] = (feature V acc_row(qd, i) + c of the panel, vector r)

        auto load = [&](int p, int b, FactoredGroup<T> &g) {
            const int f = p * PF + V * r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = min(row0 + 16 * b + 4 * qd + e, n - 1);  // (rows from n on: any valid row, against exact zeros of Vp)
#pragma unroll
                for (int c = 0; c < V; ++c) g.x[e][c] = T(0);
                if (f < ldx) g.x[e] = *reinterpret_cast<const vec *>(X + static_cast<size_t>(row) * ldx + f);
            }
        };
        auto compute = [&](int b, const FactoredGroup<T> &g) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int c = 0; c < V; ++c) acc[c] = S::mfma(g.x[e][c], vb[b][e], acc[c]);
        };

        FactoredGroup<T> ga, gb;
        load(0, 0, ga);
        for (int p = 0; p < npanels; ++p) {
#pragma unroll
            for (int c = 0; c < V; ++c) {
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[c][i] = T(0);
                asm volatile("" : "+v"(acc[c]));  // (the start values live in the accumulators' own registers)
            }
#pragma unroll
            for (int b = 0; b < FT_BLOCKS; b += 2) {
                load(p, b + 1, gb);
                compute(b, ga);
                if (b + 2 < FT_BLOCKS) {
                    load(p, b + 2, ga);
                } else if (p + 1 < npanels) {
                    load(p + 1, 0, ga);
                }
                compute(b + 1, gb);
            }
            // the panel is complete over this wave's rows: the four waves' sums in wave order, out as the slab's record of the panel
#pragma unroll
            for (int c = 0; c < V; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) stage[(wave * PF + V * S::acc_row(qd, i) + c) * BLOCK_VECTORS + r] = acc[c][i];
            __syncthreads();
            T *rec = Wpart + (static_cast<size_t>(slab) * ldx + p * PF) * BLOCK_VECTORS;
#pragma unroll
            for (int q = 0; q < PF * BLOCK_VECTORS / 256; ++q) {
                const int idx = tid + 256 * q;  // (feature idx / 16 of the panel, vector idx % 16)
                const T *s = stage + idx;
                if (p * PF + idx / BLOCK_VECTORS < ldx) rec[idx] = (s[0] + s[PF * BLOCK_VECTORS]) + (s[2 * PF * BLOCK_VECTORS] + s[3 * PF * BLOCK_VECTORS]);
            }
            __syncthreads();
        }
    }
}

/* Wp[(f / 4) 16 + u][f % 4] = scale * sum over s of W_part[s][f][u], s ascending: four interleaved partial sums, then (s0 + s1) + (s2 + s3) */
template <typename T>
__global__ __launch_bounds__(256) void k_factored_fold(const T *__restrict__ Wpart, int ldx, int nslabs, T scale, T *__restrict__ Wp) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= ldx * BLOCK_VECTORS) return;
    const int f = idx / BLOCK_VECTORS, u = idx % BLOCK_VECTORS;
    const size_t stride = static_cast<size_t>(ldx) * BLOCK_VECTORS;
    const T *src = Wpart + idx;
    T s0 = T(0), s1 = T(0), s2 = T(0), s3 = T(0);
    int s = 0;
#pragma unroll 4
    for (; s + 3 < nslabs; s += 4) {
        s0 += src[s * stride];
        s1 += src[(s + 1) * stride];
        s2 += src[(s + 2) * stride];
        s3 += src[(s + 3) * stride];
    }
    for (; s < nslabs; ++s) s0 += src[s * stride];
    Wp[((f >> 2) * BLOCK_VECTORS + u) * 4 + (f & 3)] = scale * ((s0 + s1) + (s2 + s3));
}

/* Kv_u[j] = sum over f of X[j][f] W[f][u] for j < n, u < nv.  Wp: k_factored_fold's, exact zeros from feature ldx on up to whole groups of 16 pieces.  No LDS. */
template <typename T>
__global__ __launch_bounds__(256, 2) void k_factored_scatter(const T *__restrict__ X, int ldx, int n, int nslabs, const T *__restrict__ Wp, int nv, const StoredVectors<T> Kv) {
    using S = StoredTraits<T>;
    using vec = typename S::vec;
    using acc_t = typename S::acc;
    constexpr int V = S::V, CF = 4 * V, GF = 4 * CF;  // features of a step (16 / 8) and of a group of four steps (64 / 32)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, qd = lane >> 4;
    const int ngroups = (ldx + GF - 1) / GF;
    T *dst = stored_select(Kv, r);

    for (int slab = blockIdx.x; slab < nslabs; slab += gridDim.x) {
        const int row0 = slab * FT_SLAB + wave * (FT_SLAB / 4);
        const int nblocks = min(FT_BLOCKS, (n - row0 + 15) / 16);  // (this wave's blocks with a row below n; <= 0: none)
        const int total = nblocks * ngroups;
        acc_t acc;

        auto load = [&](int b, int gq, FactoredGroup<T> &g) {
            const T *xr = X + static_cast<size_t>(min(row0 + 16 * b + r, n - 1)) * ldx;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int f = gq * GF + c * CF + V * qd;  // this lane's k: the features f ... f + V - 1
#pragma unroll
                for (int e = 0; e < V; ++e) g.x[c][e] = T(0);
                if (f < ldx) g.x[c] = *reinterpret_cast<const vec *>(xr + f);
                g.w[c] = *reinterpret_cast<const vec *>(Wp + (static_cast<size_t>(f >> 2) * BLOCK_VECTORS + r) * 4 + (f & 3));
            }
        };
        auto compute = [&](int b, int gq, const FactoredGroup<T> &g) {
            if (gq == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = T(0);
                asm volatile("" : "+v"(acc));
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int e = 0; e < V; ++e) acc = S::mfma(g.x[c][e], g.w[c][e], acc);
            if (gq == ngroups - 1) {  // acc[i] = (row 16 b + acc_row(qd, i) of the wave's share, vector r)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = row0 + 16 * b + S::acc_row(qd, i);
                    if (row < n && r < nv) dst[row] = acc[i];
                }
            }
        };
        // the groups (block b, feature group gq) in order, gq fastest
        auto next = [&](int &b, int &gq) {
            if (++gq == ngroups) {
                gq = 0;
                ++b;
            }
        };

        FactoredGroup<T> ga, gb;
        int lb = 0, lg = 0, cb = 0, cg = 0;  // the next group to load / to compute
        if (total > 0) {
            load(lb, lg, ga);
            next(lb, lg);
        }
        for (int gi = 0; gi < total; gi += 2) {
            if (gi + 1 < total) {
                load(lb, lg, gb);
                next(lb, lg);
            }
            compute(cb, cg, ga);
            next(cb, cg);
            if (gi + 1 < total) {
                if (gi + 2 < total) {
                    load(lb, lg, ga);
                    next(lb, lg);
                }
                compute(cb, cg, gb);
                next(cb, cg);
            }
        }
    }
}

}  // namespace

/* ------------------------------------------------------------------ Problem<T>: apply ------------------------------------------------------------------ */
template <typename T>
void Problem<T>::enqueue_apply_K_factored(const T *const *v, T *const *Kv, int nv, hipEvent_t ev_begin, hipEvent_t ev_end) {
    LSSVM_REQUIRE(factored_applies(), "the factored operator serves the linear kernel on an unsharded problem");
    LSSVM_REQUIRE(nv >= 1 && nv <= BLOCK_VECTORS, "a factored pass takes 1 ... 16 vectors");
    hipStream_t st = stream_.s;
    using S = StoredTraits<T>;
    const int ldx = X_.ldx, nslabs = (n_ + FT_SLAB - 1) / FT_SLAB, rows_padded = nslabs * FT_SLAB;
    const size_t wp_features = static_cast<size_t>(round_up(ldx, 16 * S::V));  // whole groups of the scatter: exact zeros from ldx on (never written)
    if (fact_vp_.p == nullptr) {
        int cus = 0;
        LSSVM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_));
        fact_grid_ = std::max(1, std::min(nslabs, 2 * cus));
        fact_wpart_.alloc_zero(static_cast<size_t>(nslabs) * ldx * BLOCK_VECTORS, st);
        fact_wp_.alloc_zero(wp_features * BLOCK_VECTORS, st);
        fact_vp_.alloc_zero(static_cast<size_t>(rows_padded) * BLOCK_VECTORS, st);
    }
    double gamma = 0.0, coef0 = 0.0;
    LandmarkBlock<T>::kernel_scalars(*this, gamma, coef0);  // (linear: 1 / x_scale^2)
    StoredVectors<const T> src{};
    StoredVectors<T> dst{};
    for (int u = 0; u < BLOCK_VECTORS; ++u) {
        src.p[u] = v[std::min(u, nv - 1)];
        dst.p[u] = Kv[std::min(u, nv - 1)];
    }
    hipLaunchKernelGGL(k_pack_stored_v<T>, dim3((static_cast<unsigned>(rows_padded) * BLOCK_VECTORS + 255) / 256), dim3(256), 0, st, src, nv, n_, rows_padded, fact_vp_.p);
    if (ev_begin != nullptr) LSSVM_HIP_CHECK(hipEventRecord(ev_begin, st));
    hipLaunchKernelGGL(k_factored_gather<T>, dim3(fact_grid_), dim3(256), 0, st, X_.data.p, ldx, n_, nslabs, fact_vp_.p, fact_wpart_.p);
    hipLaunchKernelGGL(k_factored_fold<T>, dim3((ldx * BLOCK_VECTORS + 255) / 256), dim3(256), 0, st, fact_wpart_.p, ldx, nslabs, static_cast<T>(gamma), fact_wp_.p);
    hipLaunchKernelGGL(k_factored_scatter<T>, dim3(fact_grid_), dim3(256), 0, st, X_.data.p, ldx, n_, nslabs, fact_wp_.p, nv, dst);
    if (ev_end != nullptr) LSSVM_HIP_CHECK(hipEventRecord(ev_end, st));
    LSSVM_HIP_CHECK(hipGetLastError());
}

template void Problem<float>::enqueue_apply_K_factored(const float *const *, float *const *, int, hipEvent_t, hipEvent_t);
template void Problem<double>::enqueue_apply_K_factored(const double *const *, double *const *, int, hipEvent_t, hipEvent_t);

}  // namespace lssvm
