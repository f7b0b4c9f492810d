/*
 * lssvm_tile_f64_blk.hip.hpp -- tile_matvec_f64_blk: the full-square fp64 tile kernel with SIXTEEN weight vectors per pass, the
 * resident predictor of a one-vs-all model behind lssvm_mi355_predictor_create_block.  Included by tile_launch_f64blk.hip only.
 */
#pragma once

#include "lssvm_tile_f64.hip.hpp"  // the ring's geometry (V2D_RING, V2D_SLOT_BYTES): the pipeline is tile_matvec_f64_v2's

namespace lssvm {

/* =====================================================================================================================
 * out[row, v] = sum_col k(row, col) alpha[col, v] for 16 vectors v is itself a matrix product, and v_mfma_f64_16x16x4_f64 leaves its result where the next
 * MFMA takes an operand: D[m = q + 4 i][n = r] sits in register i of lane (r, q) = (lane & 15, lane >> 4), and the same lane supplies B[k = q][n = r].
 *   FIRST PRODUCT, TRANSPOSED.  The two operands of tile_matvec_f64_v2's product are swapped (A = the column fragment from the ring, B = the row panel; both are
 *   "feature 4 s + q of point r" in lane (r, q), so neither is loaded differently): the accumulator block (rb, cb) then holds the transposed tile,
 *   acc[rb][cb][i] of lane (r, q) = K[row = 16 rb + r][col = 16 cb + 4 i + q].  rbf: its start value is c_i(row by r) + c_j(col by q + 4 i).
 *   KERNEL VALUE.  Per element on the vector ALU, in place, exactly as in tile_matvec_f64_v2 (exp2 / integer power / coef0 / the pad-column rule of a negative degree).
 *   SECOND PRODUCT.  For fixed i the four kernel values of the lanes (r, 0 .. 3) are B[k = q][n = row r] of columns 16 cb + 4 i + q; with
 *   A[m = v][k = q] = alpha[col = 16 cb + 4 i + q][v = r], one ds_read_b64 from the sub-tile's record, out2[rb] += A B is the 16-vector x 16-row block of the result:
 *   out2[rb][i] of lane (r, q) = out[v = q + 4 i][row = 16 rb + r].  16 MFMAs per (rb, sub-tile) beside the 16 NKC of the first product; the per-vector fma chains
 *   and the row butterflies of NV = 1 / 2 do not exist.  out2 is two f64x4 (16 VGPRs) carried across all sub-tiles of the work item: every chain starts from a
 *   zero in registers and is C = D throughout.
 *   RECORD of a sub-tile: (alpha[64 columns][16 vectors] | c_j[64]), 8.5 KiB (k_pack_ablock_f64), exact zeros in padded columns and padded vectors; by LDS-DMA, each
 *   wave its quarter (two full instructions of alpha; rbf: eight lanes of c_j).  The alpha reads of a wave are 512 contiguous bytes: conflict free.
 *   LDS: ring 32 KiB + 4 records 34 KiB = 66 KiB, twice per CU (NKC <= 4) within gfx950's 160 KiB.  c_i of the lane's two rows stays in registers.
 *   SUM ORDER of one value: the sub-tiles of the work item in order, inside a sub-tile cb, then i: one MFMA (four columns) per addition; then the column chunks'
 *   slabs in order (k_reduce_partials).  It depends on the shapes only, and on no other vector of the pass.
 * ===================================================================================================================== */
constexpr int V2B_REC_DOUBLES = 64 * BLOCK_VECTORS + 64;  // 1088
constexpr int V2B_REC_BYTES = V2B_REC_DOUBLES * 8;        // 8.5 KiB
constexpr int V2B_REC_SLOTS = 4;                          // (one chunk per sub-tile: the record of sub-tile t + 3 arrives while t .. t + 2 are held)
constexpr size_t V2B_LDS_BYTES = static_cast<size_t>(V2D_RING) * V2D_SLOT_BYTES + V2B_REC_SLOTS * V2B_REC_BYTES;  // 66 KiB

template <int KT, int NKC>
__global__ __launch_bounds__(TILE_THREADS, (NKC <= 4 ? 2 : 1)) void tile_matvec_f64_blk(const TileArgs<double> a) {
    static_assert(BLOCK_VECTORS == 16, "the second product is one 16 x 16 x 4 MFMA per four columns");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char *ring = smem_raw;
    char *recs = smem_raw + V2D_RING * V2D_SLOT_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15;
    const int q = lane >> 4;

    int ibl, jc;
    if (!decode_work_item(a, ibl, jc)) return;
    const int row0 = (a.ib_begin + ibl) * TILE;
    const int jt_begin = jc * a.jc_tiles;
    const int jt_end = min(jt_begin + a.jc_tiles, a.num_jt);
    const int nsub = 2 * (jt_end - jt_begin);  // 64-column sub-tiles
    if (nsub <= 0) return;
    const int st_begin = 2 * jt_begin;
    const int nsteps = nsub * NKC;

    // row panel: lane (r, q) holds X[row][4 s + q] for k-step s -- here the B operand B[k = q][n = r]
    double afrag[2][4 * NKC];
    [[maybe_unused]] double ci[2] = { 0.0, 0.0 };  // rbf: c_i of the lane's row in either row block
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const double *xr = a.Xr + static_cast<size_t>(row0 + wave * 32 + rb * 16 + r) * a.ldx + q;
#pragma unroll
        for (int s = 0; s < 4 * NKC; ++s) afrag[rb][s] = xr[4 * s];
        if constexpr (KT == KT_RBF) ci[rb] = a.cr[row0 + wave * 32 + rb * 16 + r];
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
        for (int s = 0; s < 4 * NKC; ++s) asm volatile("" : "+v"(afrag[rb][s]));
        if constexpr (KT == KT_RBF) asm volatile("" : "+v"(ci[rb]));
    }

    // chunk DMA and read addressing: tile_matvec_f64_v2's (LDS image [column block cb][16-byte k-slot ks][column r], see there)
    unsigned dma_off[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int col = wave * 16 + (lane & 15);
        const int ks = 4 * i + (lane >> 4);
        dma_off[i] = 8u * static_cast<unsigned>(col * a.ldx + 2 * ks);
    }
    const unsigned ring_lds = static_cast<unsigned>(reinterpret_cast<size_t>(ring));
    const unsigned dma_lds = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(ring_lds + static_cast<unsigned>(wave) * 2048u)));
    // this wave's quarter of record slot 0: 2 KiB of alpha (16 columns x 16 vectors), 128 bytes of c_j
    const unsigned rec_lds = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(ring_lds + V2D_RING * V2D_SLOT_BYTES + static_cast<unsigned>(wave) * 2048u)));
    [[maybe_unused]] const unsigned recc_lds = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(ring_lds + V2D_RING * V2D_SLOT_BYTES + 64 * BLOCK_VECTORS * 8 + static_cast<unsigned>(wave) * 128u)));
    auto issue_chunk = [&](int step) {
        const int t = step / NKC;
        const int kc = step - t * NKC;
        const char *base = sgpr_ptr(a.Xc + static_cast<size_t>(st_begin + t) * 64 * a.ldx + kc * 16);
        const unsigned slot = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(dma_lds + static_cast<unsigned>(step % V2D_RING) * V2D_SLOT_BYTES)));
        lds_dma16<0>(dma_off[0], base, slot);
        lds_dma16<1024>(dma_off[1], base, slot);
    };
    // (every record instruction is older than the chunk pieces issued behind it: the counted waits below, which leave only the youngest chunk's two pieces
    // outstanding, cover the records whatever their number of instructions)
    auto issue_rec = [&](int t) {
        const char *src = reinterpret_cast<const char *>(a.dc + static_cast<size_t>(st_begin + t) * V2B_REC_DOUBLES);
        const unsigned slot_off = static_cast<unsigned>(__builtin_amdgcn_readfirstlane((t % V2B_REC_SLOTS) * V2B_REC_BYTES));
        const char *al = sgpr_ptr(src + __builtin_amdgcn_readfirstlane(wave * 2048));
        const unsigned off = 16u * (lane_off(threadIdx.x) & 63u);
        lds_dma16<0>(off, al, rec_lds + slot_off);
        lds_dma16<1024>(off, sgpr_ptr(al + 1024), rec_lds + slot_off);
        if constexpr (KT == KT_RBF) {
            if (lane < 8) lds_dma16<0>(off, sgpr_ptr(src + 64 * BLOCK_VECTORS * 8 + __builtin_amdgcn_readfirstlane(wave * 128)), recc_lds + slot_off);
        }
    };
    const int lane_base = (q >> 1) * 256 + r * 16 + (q & 1) * 8;
    auto read_group = [&](const char *slot, int s, double (&b)[4]) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) b[cb] = *((const volatile __attribute__((address_space(3))) double *) (slot + cb * 2048 + s * 512));
    };

    f64x4 acc[2][4];
    f64x4 out2[2];  // [vector q + 4 i][row 16 rb + r]: the block of the result, across every sub-tile of the work item
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        out2[rb] = f64x4{ 0.0, 0.0, 0.0, 0.0 };
        asm volatile("" : "+v"(out2[rb]));  // a zero in registers: the chain's first MFMA is C = D like every later one
    }

    // ---- prologue: chunks 0, 1, 2 (each preceded by the record of the sub-tile that starts with it) ----
    issue_rec(0);
    issue_chunk(0);
#pragma unroll
    for (int pre = 1; pre <= 2; ++pre) {
        if (pre < nsteps) {
            if (pre % NKC == 0) issue_rec(pre / NKC);
            issue_chunk(pre);
        }
    }
    if (nsteps >= 3) {
        asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    } else if (nsteps == 2) {
        asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    double bcur[4];
    read_group(ring + lane_base, 0, bcur);

    // hand-over of the next chunk in the middle of a step: tile_matvec_f64_v2's
    auto handover = [&](int step, int kc_plus3_mod, auto checked) {
        constexpr bool CHECKED = decltype(checked)::value;
        if constexpr (!CHECKED) {
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (kc_plus3_mod == 0) issue_rec((step + 3) / NKC);
            issue_chunk(step + 3);
        } else {
            if (step + 1 < nsteps) {
                if (step + 2 < nsteps) {
                    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if (step + 3 < nsteps) {
                    if (kc_plus3_mod == 0) issue_rec((step + 3) / NKC);
                    issue_chunk(step + 3);
                }
            }
        }
    };

    auto tile_body = [&](int t, auto checked) {
        const int s0 = t * NKC;
        const char *rec = recs + (t % V2B_REC_SLOTS) * V2B_REC_BYTES;
        const double *alr = reinterpret_cast<const double *>(rec) + q * BLOCK_VECTORS + r;  // alpha[16 cb + 4 i + q][r] at + (16 cb + 4 i) * 16
        if constexpr (KT == KT_RBF) {
            const double *cjr = reinterpret_cast<const double *>(rec) + 64 * BLOCK_VECTORS + q;  // c_j[16 cb + 4 i + q]
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double cjv = cjr[cb * 16 + 4 * i];
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) acc[rb][cb][i] = ci[rb] + cjv;
                }
        }
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
            const int step = s0 + kc;
            const char *slot = ring + (step % V2D_RING) * V2D_SLOT_BYTES + lane_base;
            const char *slot_next = ring + ((step + 1) % V2D_RING) * V2D_SLOT_BYTES + lane_base;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                double bnext[4];
                if (s < 3) read_group(slot, s + 1, bnext);
                if (s == 2) handover(step, (kc + 3) % NKC, checked);
                if (s == 3) read_group(slot_next, 0, bnext);
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) {
                        if (KT != KT_RBF && kc == 0 && s == 0) {
                            const f64x4 zero = { 0.0, 0.0, 0.0, 0.0 };
                            acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(bcur[cb], afrag[rb][0], zero, 0, 0, 0);
                        } else {
                            acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(bcur[cb], afrag[rb][4 * kc + s], acc[rb][cb], 0, 0, 0);
                        }
                    }
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) bcur[cb] = bnext[cb];
            }
        }
        // ---- epilogue of the sub-tile: the kernel value per element on the vector ALU, then four columns x sixteen vectors per MFMA ----
        if constexpr (v2_base_kt(KT) == KT_POLY) {
            if (a.coef0 != 0.0) {  // uniform; the common coef0 = 0 costs nothing
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[rb][cb][i] += a.coef0;
            }
        }
        [[maybe_unused]] const int pad_from = (a.degree < 0) ? a.ncols_valid - (st_begin + t) * 64 - q : 64;  // KT_POLY: columns 16 cb + 4 i of this lane from here on are padding
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double al = alr[(cb * 16 + 4 * i) * BLOCK_VECTORS];
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    double kv;
                    if constexpr (v2_base_kt(KT) == KT_POLY) {
                        kv = poly_power<v2_degree_class(KT)>(acc[rb][cb][i], a.degree);  // (the data carries sqrt(gamma), coef0 was added above)
                    } else {
                        kv = exp2_f64(acc[rb][cb][i]);  // the data is pre-scaled: acc = log2(K)
                    }
                    if constexpr (KT == KT_POLY) {
                        if (cb * 16 + 4 * i >= pad_from) kv = 0.0;  // a negative power of a padded column's 0 is inf: times alpha = 0 it would be NaN
                    }
                    out2[rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(al, kv, out2[rb], 0, 0, 0);
                }
            }
    };

    // steady state: every sub-tile whose last step still has step + 3 < nsteps; then the tail sub-tiles with the checked hand-over
    constexpr int TAIL_TILES = (3 + NKC - 1) / NKC;
    const int nmain = nsub > TAIL_TILES ? nsub - TAIL_TILES : 0;
    int t = 0;
    for (; t < nmain; ++t) tile_body(t, std::false_type{});
    for (; t < nsub; ++t) tile_body(t, std::true_type{});

    // plane v of the row slabs takes vector v: lane (r, q) holds vectors q + 4 i of rows 16 rb + r (16 lanes = 128 contiguous bytes per store)
    double *dst = a.partial + static_cast<size_t>(jc) * a.part_stride + ibl * TILE + wave * 32 + r;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[static_cast<size_t>(q + 4 * i) * a.part_vstride + rb * 16] = out2[rb][i];
}

/* the records of tile_matvec_f64_blk for the `count` (1 ... 16) weight vectors alpha[v][ld], v = 0 .. count - 1: per 64-column sub-tile st
 * dc[st][16 l + u] = alpha_u[64 st + l] (u >= count: 0), dc[st][1024 + l] = c[64 st + l].  One thread per (column, vector slot). */
#ifdef LSSVM_KERNELS_BLOCK_PACK
__global__ void k_pack_ablock_f64(const double *__restrict__ alpha, size_t ld, int count, const double *__restrict__ cc, int ncols_padded, double *__restrict__ dc) {
    const size_t e = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const size_t j = e / BLOCK_VECTORS;
    const int u = static_cast<int>(e % BLOCK_VECTORS);
    if (j >= static_cast<size_t>(ncols_padded)) return;
    const size_t st = j >> 6, l = j & 63;
    dc[st * V2B_REC_DOUBLES + l * BLOCK_VECTORS + u] = (u < count) ? alpha[static_cast<size_t>(u) * ld + j] : 0.0;
    if (u == 0) dc[st * V2B_REC_DOUBLES + 64 * BLOCK_VECTORS + l] = (cc != nullptr) ? cc[j] : 0.0;
}
#endif  // LSSVM_KERNELS_BLOCK_PACK
}  // namespace lssvm
