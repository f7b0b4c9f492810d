/*
 * lssvm_tile_f32_blk.hip.hpp -- tile_matvec_f32_blk: the full-square fp32 split tile kernel with SIXTEEN weight vectors per pass, the
 * resident predictor of a one-vs-all model behind lssvm_mi355_predictor_create_block32.  Included by tile_launch_f32blk.hip only.
 */
#pragma once

#include "lssvm_tile_f32_split.hip.hpp"  // plane_mfma, the ring's geometry and s6w_body, whose pipeline this is

namespace lssvm {

/* =====================================================================================================================
 * out[point, v] = sum_col k(point, col) W[col, v] for 16 vectors v is itself a matrix product, and v_mfma_f32_16x16x32_{f16,bf16} leaves its result where
 * v_mfma_f32_16x16x4_f32 takes its A operand: D[row = 4 g + e][col = r] sits in register e of lane (r, g) = (lane & 15, lane >> 4), and the fp32 MFMA takes
 * A[i = r][k = g] from that very lane.
 *   FIRST PRODUCT, TRANSPOSED.  The operands of s6w_body's plane products are swapped (A = the support vectors' fragment from the ring, B = the row panel of points;
 *   both are "features 8 g .. 8 g + 7 of point r" in lane (r, g), so neither is loaded differently): acc[rb][cb][e] of lane (r, g) = K[point 16 rb + r][column
 *   16 cb + 4 g + e].  Folded rbf: the first MFMA's C operand is c_i of point r in all four registers.  Per element the plane products are those of the single-vector
 *   kernel, in its order (column plane by column plane, chunk by chunk, k32 step by k32 step), and the epilogue is its apply_kernel_function.
 *   SECOND PRODUCT.  Register e of the 16 x 16 block (rb, cb) is, as it stands, the A operand A[point r][k = g] of the four columns 16 cb + 4 g + e, g = 0 .. 3; with
 *   B[k = g][vector r] = W[16 cb + 4 g + e][r], out2[rb] += A B is the 16-point x 16-vector block of the result: out2[rb][e'] of lane (r, g) = out[point 16 rb + 4 g +
 *   e'][vector r].  Four v_mfma_f32_16x16x4_f32 per block, 64 per wave and tile beside the 32 PL (PL + 1) NK64 / 2 ... of the first product; out2 is two f32x4 carried
 *   across all tiles of the work item.  No per-vector fma chain, no row butterfly, no LDS round trip of kernel values, no atomics.
 *   (32x32x2 for the second product would need the kernel values of 32 points in one register across the lanes: the first product would have to be 32x32x16, the shape
 *   round 3 retired for its lower clock -- and it halves nothing: 2 x 16 passes per 8 columns instead of 4 x 8.)
 *   RECORD of a 64-column sub-tile: W[64 columns][16 vectors] as [column / 4][vector][column % 4], 4 KiB (k_pack_wblock_f32): W = alpha (polynomial), 2^c_j alpha (folded
 *   rbf: the value k_pack_dc writes), exact zeros in padded columns and padded vectors -- nothing else: no form here reads c_j.  A tile's two records are contiguous
 *   (8 KiB); lane (r, g) reads its four B values of block cb, e = 0 .. 3, as ONE ds_read_b128 at byte ((4 cb + g) 16 + r) 16: a wave reads 1 KiB contiguous, conflict
 *   free.  By LDS-DMA, each wave its quarter (two full instructions), under the ring's counted waits: the record of tile t + 1 is issued at the FIRST hand-over of tile
 *   t, in front of that step's chunk pieces -- older than them, so the next hand-over's wait (all but the youngest chunk) and barrier cover it, a whole tile before its
 *   epilogue.  (s6w_body issues a record with the chunk three steps ahead, which at NKC = 2 is two tiles ahead and would take a third slot.)
 *   LDS: ring 64 KiB + 2 record slots 16 KiB = 80 KiB: two workgroups fill gfx950's 160 KiB exactly.  c_i stays in registers (one value per row block and lane), which
 *   is what makes the second workgroup fit.
 *   SUM ORDER of one value: the tiles of the work item in order, inside a tile cb, then e: one MFMA (four columns) per addition; then the column chunks' slabs in
 *   order (k_reduce_partials).  It depends on the shapes only, and on no other vector of the pass.
 * ===================================================================================================================== */
constexpr int B32_REC_FLOATS = TILE * BLOCK_VECTORS;  // per 128-column tile: two sub-tile records of 64 x 16
constexpr int B32_REC_BYTES = B32_REC_FLOATS * 4;     // 8 KiB
constexpr int B32_REC_SLOTS = 2;                      // (tile t's record is read in its epilogue; tile t + 1's arrives during tile t)
constexpr size_t B32_LDS_BYTES = static_cast<size_t>(V2_RING) * V2_SLOT_BYTES + B32_REC_SLOTS * B32_REC_BYTES;  // 80 KiB

template <int KT, int NK64, int PL>
__global__ __launch_bounds__(TILE_THREADS, 2) void tile_matvec_f32_blk(const TileArgs<float> a) {
    static_assert(BLOCK_VECTORS == 16, "the second product is one 16 x 16 x 4 MFMA per four columns");
    static_assert(PL == 3 || PL == 2, "three bf16 planes (bf16x6) or two f16 planes (f16x3)");
    static_assert(NK64 == 1 || NK64 == 2, "the row panel in registers beside two workgroups per CU: at most 128 features");
    static_assert(KT == KT_RBFF || KT == KT_POLY || KT == KT_POLY2 || KT == KT_POLY3, "folded rbf and the polynomial forms: the forms whose epilogue needs no c_j");
    constexpr bool F16 = PL == 2;
    constexpr bool RBF = KT == KT_RBFF;
    constexpr int NKC = PL * NK64;  // steps per tile: for every 64-feature chunk the column planes hi, mid (, lo)
    static_assert(NKC >= 2, "the record of tile t + 1 lands at the second hand-over of tile t");
    // row planes in registers and the row plane of the q-th product of column plane p: s6w_body's (f16 rbf: the shifted planes P2, P1 against P0 and P0 against P1)
    constexpr int PLA = F16 ? (RBF ? 3 : 2) : 3;
    constexpr auto row_plane = [](int p, int q) constexpr { return (F16 && PLA == 3) ? (p == 0 ? (q == 0 ? 2 : 1) : 0) : q; };
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char *ring = smem_raw;                               // [V2_RING][128 columns][128 B]
    char *recs = smem_raw + V2_RING * V2_SLOT_BYTES;     // [B32_REC_SLOTS][32 column quads][16 vectors][4]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15;  // operands: point / column of the fragment; results: point (first product), vector (second product)
    const int g = lane >> 4;  // k group (operands), row group (results)

    int ibl, jc;
    if (!decode_work_item(a, ibl, jc)) return;
    const int row0 = (a.ib_begin + ibl) * TILE;
    const int jt_begin = jc * a.jc_tiles;
    const int ntiles = min(jt_begin + a.jc_tiles, a.num_jt) - jt_begin;
    if (ntiles <= 0) return;
    const int nsteps = ntiles * NKC;

    // ---- the row panel: the fragments of this wave's 32 points (two blocks of 16), all features, all row planes -- here the B operand B[k = 8 g + j][n = r] ----
    bf16x8 afrag[PLA][2 * NK64][2];
#pragma unroll
    for (int p = 0; p < PLA; ++p) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const uint16_t *xr = a.Xr16 + p * a.plane_stride_r + static_cast<size_t>(row0 + wave * 32 + 16 * rb + r) * a.ldx16 + 8 * g;
#pragma unroll
            for (int kk = 0; kk < 2 * NK64; ++kk) afrag[p][kk][rb] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const f32x4 *>(xr + 32 * kk));
        }
    }
    [[maybe_unused]] f32x4 civ0[2] = { { 0.f, 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f, 0.f } };  // folded rbf: c_i of point r, the C operand of every accumulator's first MFMA
    if constexpr (RBF) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const float ci = a.cr[row0 + wave * 32 + 16 * rb + r];
            civ0[rb] = f32x4{ ci, ci, ci, ci };
        }
    }
    // make the compiler retire these ordinary loads HERE, before any LDS-DMA is in flight
#pragma unroll
    for (int p = 0; p < PLA; ++p)
#pragma unroll
        for (int kk = 0; kk < 2 * NK64; ++kk)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) asm volatile("" : "+v"(afrag[p][kk][rb]));
    if constexpr (RBF) asm volatile("" : "+v"(civ0[0]), "+v"(civ0[1]));

    // ---- LDS-DMA addressing of the column planes: s6w_body's (the LDS image does not depend on which operand the fragment becomes) ----
    unsigned dma_off[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 8 * (4 * wave + i) + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        dma_off[i] = 2u * static_cast<unsigned>(row * a.ldx16 + 8 * c);
    }
    const unsigned ring_lds = static_cast<unsigned>(reinterpret_cast<size_t>(ring));
    const unsigned dma_lds = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(ring_lds + static_cast<unsigned>(wave) * 4096u)));
    // this wave's quarter of record slot 0: 2 KiB (8 column quads x 16 vectors x 4)
    const unsigned rec_lds = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(ring_lds + V2_RING * V2_SLOT_BYTES + static_cast<unsigned>(wave) * 2048u)));
    auto issue_chunk = [&](int step) {
        const int t = step / NKC;
        const int kc = step - t * NKC;
        const char *base = sgpr_ptr(a.Xc16 + (kc % PL) * a.plane_stride + static_cast<size_t>(jt_begin + t) * TILE * a.ldx16 + (kc / PL) * 64);
        const unsigned slot = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(dma_lds + static_cast<unsigned>(step % V2_RING) * V2_SLOT_BYTES)));
        static_for<0, 4>([&](auto i_c) {
            constexpr int i = decltype(i_c)::value;
            lds_dma16<i * 1024>(dma_off[i], base, slot);
        });
    };
    // steady state: two scalar adds per DMA instruction (s6w_body's issue_part_static)
    const size_t tile_bytes = static_cast<size_t>(TILE) * a.ldx16 * 2;
    const size_t plane_bytes = a.plane_stride * 2;
    const char *xc_tile = reinterpret_cast<const char *>(a.Xc16) + static_cast<size_t>(jt_begin) * tile_bytes;
    auto issue_part_static = [&](auto kc3_c, unsigned slot_idx, auto i_c) {  // kc3 = kc + 3 of the issuing step, slot_idx = (step + 3) % V2_RING
        constexpr int KC3 = decltype(kc3_c)::value;
        constexpr int KC = KC3 % NKC;
        constexpr int i = decltype(i_c)::value;
        const char *base = xc_tile + (KC3 / NKC) * tile_bytes + (KC % PL) * plane_bytes + (KC / PL) * 128;
        lds_dma16<i * 1024>(dma_off[i], sgpr_ptr(base), dma_lds + slot_idx * V2_SLOT_BYTES);
    };
    // (both record instructions are older than the chunk pieces issued behind them: the counted waits, which leave only the youngest chunk's four pieces outstanding,
    // cover them)
    auto issue_rec = [&](int t) {
        const char *src = sgpr_ptr(reinterpret_cast<const char *>(a.dc) + static_cast<size_t>(jt_begin + t) * B32_REC_BYTES + __builtin_amdgcn_readfirstlane(wave * 2048));
        const unsigned dst = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(rec_lds + static_cast<unsigned>(t % B32_REC_SLOTS) * B32_REC_BYTES)));
        const unsigned off = 16u * (lane_off(threadIdx.x) & 63u);
        lds_dma16<0>(off, src, dst);
        lds_dma16<1024>(off, sgpr_ptr(src + 1024), dst);
    };

    // ---- read addressing of the ring: s6w_body's ----
    int rd_off[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) rd_off[kk] = r * 128 + (((4 * kk + g) ^ ((r >> 1) & 7)) << 4);
    const int rec_off = (g * 16 + r) * 16;  // + 1024 cb: W[16 cb + 4 g + e][r], e = 0 .. 3

    f32x4 acc[2][8];
    f32x4 out2[2];  // [point 16 rb + 4 g + e][vector r]: the block of the result, across every tile of the work item
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        out2[rb] = f32x4{ 0.f, 0.f, 0.f, 0.f };
        asm volatile("" : "+v"(out2[rb]));  // a zero in registers: the chain's first MFMA is C = D like every later one
    }

    // ---- prologue: the first tile's record, then chunks 0, 1, 2 ----
    issue_rec(0);
    issue_chunk(0);
#pragma unroll
    for (int pre = 1; pre <= 2; ++pre) {
        if (pre < nsteps) issue_chunk(pre);
    }
    if (nsteps >= 3) {
        asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");  // (NKC >= 2: at least two steps)
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // column fragments: two buffers used alternately by the groups, ordinary loads under the compiler's own waits (s6w_body's compiler-scheduled groups)
    f32x4 bbuf[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) bbuf[0][c] = *reinterpret_cast<const f32x4 *>(ring + c * 2048 + rd_off[0]);

    // hand-over in the middle of a step: s6w_body's, with the NEXT tile's record at a tile's first one
    auto handover = [&](int step, int kc, int t, auto checked) {
        constexpr bool CHECKED = decltype(checked)::value;
        if constexpr (!CHECKED) {
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (kc == 0) issue_rec(t + 1);  // (a steady-state tile is never the last)
        } else {
            if (step + 1 < nsteps) {
                if (step + 2 < nsteps) {
                    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if (kc == 0 && t + 1 < ntiles) issue_rec(t + 1);  // (then step + 3 < nsteps as well: the chunk below follows it)
                if (step + 3 < nsteps) issue_chunk(step + 3);
            }
        }
    };

    auto tile_body = [&](int t, auto checked) {
        const int s0 = t * NKC;
        const unsigned phase = static_cast<unsigned>(s0) & (V2_RING - 1);  // ring slot of the tile's first step (uniform)
        static_for<0, NKC>([&](auto kc_c) {
            constexpr int kc = decltype(kc_c)::value;
            constexpr int chunk = kc / PL, plane = kc % PL;
            const int step = s0 + kc;
            const char *slot = ring + ((phase + kc) & (V2_RING - 1)) * V2_SLOT_BYTES;
            const char *slot_next = ring + ((phase + kc + 1) & (V2_RING - 1)) * V2_SLOT_BYTES;
            static_for<0, 4>([&](auto mm_c) {
                constexpr int mm = decltype(mm_c)::value;
                constexpr int kk = mm >> 1, cbh = mm & 1;
                const bool more = !decltype(checked)::value || mm < 3 || step + 1 < nsteps;
                f32x4(&bcur)[4] = bbuf[mm & 1];
                f32x4(&bnext)[4] = bbuf[(mm + 1) & 1];
                if constexpr (mm < 3) {  // next group of this chunk: (kk', cbh') = ((mm + 1) >> 1, (mm + 1) & 1)
#pragma unroll
                    for (int c = 0; c < 4; ++c) bnext[c] = *reinterpret_cast<const f32x4 *>(slot + (4 * ((mm + 1) & 1) + c) * 2048 + rd_off[(mm + 1) >> 1]);
                    if constexpr (mm != 2) LSSVM_SCHED_BARRIER();
                }
                if constexpr (mm == 2) {
                    handover(step, kc, t, checked);
                    LSSVM_SCHED_BARRIER();
                }
                if constexpr (mm == 3) {  // first group of the next chunk: visible since this step's hand-over
                    if (more) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) bnext[c] = *reinterpret_cast<const f32x4 *>(slot_next + c * 2048 + rd_off[0]);
                    }
                    LSSVM_SCHED_BARRIER();
                }
#pragma unroll
                for (int q = 0; q < PL; ++q) {
                    if (q + plane > PL - 1) continue;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int cb = 4 * cbh + c;
                        const bf16x8 bv = __builtin_bit_cast(bf16x8, bcur[c]);
#pragma unroll
                        for (int rb = 0; rb < 2; ++rb) {
                            const bf16x8 av = afrag[row_plane(plane, q)][2 * chunk + kk][rb];
                            // (transposed: the column fragment is A, the row panel B)
                            if (RBF && kc == 0 && kk == 0 && q == 0) {
                                acc[rb][cb] = plane_mfma<F16>(bv, av, civ0[rb]);
                            } else if (kc == 0 && kk == 0 && q == 0) {
                                const f32x4 zero = { 0.f, 0.f, 0.f, 0.f };
                                acc[rb][cb] = plane_mfma<F16>(bv, av, zero);
                            } else {
                                acc[rb][cb] = plane_mfma<F16>(bv, av, acc[rb][cb]);
                            }
                        }
                        if constexpr (!decltype(checked)::value && mm >= 2) {
                            if (q == 0 && c == 0) issue_part_static(std::integral_constant<int, kc + 3>{}, (phase + kc + 3) & (V2_RING - 1), std::integral_constant<int, (mm - 2) * 2 + 0>{});
                            if (q == 0 && c == 2) issue_part_static(std::integral_constant<int, kc + 3>{}, (phase + kc + 3) & (V2_RING - 1), std::integral_constant<int, (mm - 2) * 2 + 1>{});
                        }
                    }
                }
            });
        });
        xc_tile += tile_bytes;
        // ---- epilogue of the tile: the kernel value per element on the vector ALU, in place; then four columns x sixteen vectors per fp32 MFMA ----
        const char *rec = recs + (t % B32_REC_SLOTS) * B32_REC_BYTES + rec_off;  // (landed and published by the tile's second hand-over at the latest)
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) {
            const f32x4 w = *reinterpret_cast<const f32x4 *>(rec + cb * 1024);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    const float kv = apply_kernel_function<v2_base_kt(KT), v2_degree_class(KT)>(acc[rb][cb][e], a);
                    out2[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv, w[e], out2[rb], 0, 0, 0);
                }
        }
    };

    constexpr int TAIL_TILES = (3 + NKC - 1) / NKC;
    const int nmain = ntiles > TAIL_TILES ? ntiles - TAIL_TILES : 0;
    int t = 0;
    for (; t < nmain; ++t) tile_body(t, std::false_type{});
    for (; t < ntiles; ++t) tile_body(t, std::true_type{});

    // plane v of the row slabs takes vector v: lane (r, g) holds points 4 g .. 4 g + 3 of either row block for vector r -- one 16-byte store per row block
    float *dst = a.partial + static_cast<size_t>(r) * a.part_vstride + static_cast<size_t>(jc) * a.part_stride + ibl * TILE + wave * 32 + 4 * g;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) *reinterpret_cast<f32x4 *>(dst + 16 * rb) = out2[rb];
}

/* the records of tile_matvec_f32_blk for the `count` (1 ... 16) weight vectors alpha[v][ld], v = 0 .. count - 1: per 64-column sub-tile st
 * dc[st][((l >> 2) 16 + u) 4 + (l & 3)] = W_u[64 st + l] (u >= count: 0), W = alpha, or -- folded != 0 -- 2^c_j alpha with k_pack_dc's statements (the same bits).
 * One thread per (column, vector slot). */
#ifdef LSSVM_KERNELS_BLOCK_PACK
__global__ void k_pack_wblock_f32(const float *__restrict__ alpha, size_t ld, int count, const float *__restrict__ cc, int folded, int ncols_padded, float *__restrict__ dc) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const size_t j = i / BLOCK_VECTORS;
    const int u = static_cast<int>(i % BLOCK_VECTORS);
    if (j >= static_cast<size_t>(ncols_padded)) return;
    const size_t st = j >> 6, l = j & 63;
    float w = 0.0f;
    if (u < count) {
        const float d = alpha[static_cast<size_t>(u) * ld + j];
        if (folded) {
            const float c = (cc != nullptr) ? cc[j] : 0.0f;
            const float e = __builtin_amdgcn_exp2f(c);
            w = e * d;
        } else {
            w = d;
        }
    }
    dc[st * (64 * BLOCK_VECTORS) + ((l >> 2) * BLOCK_VECTORS + u) * 4 + (l & 3)] = w;
}
#endif  // LSSVM_KERNELS_BLOCK_PACK
}  // namespace lssvm
