/*
 * lssvm_tile_f32_blk_wide.hip.hpp -- tile_matvec_f32_blk_wide: the full-square fp32 split tile kernel with SIXTEEN weight vectors per pass for models of MORE than 128
 * padded features, the resident predictor of a one-vs-all model behind lssvm_mi355_predictor_create_block_panels.  Included by
 * tile_launch_f32blkx.hip only.
 */
#pragma once

#include "lssvm_tile_f32_blk.hip.hpp"  // the record's geometry (B32_*), whose second product this is; through it plane_mfma and the ring's geometry

namespace lssvm {

/* =====================================================================================================================
 * Two designs in one kernel.
 *   FROM s6x_body (lssvm_tile_f32_wide.hip.hpp): the walk of 128-feature panels INSIDE a tile.  A work item's tile is `panels` x (128 features) tile-panels; the
 *   accumulators of the 128 x 128 tile live across them; the row panel of the wave's 32 points (all row planes, 128 features) is re-loaded from global memory / L2 into
 *   the same registers, a 64-feature chunk as soon as the previous tile-panel is through with it; the column stream walks (tile, panel, 64-feature chunk, plane) through
 *   the LDS-DMA ring of 128-column x 64-feature plane-chunks with run-time addressing and the checked hand-over throughout; the accumulators are initialised explicitly
 *   at panel 0; the epilogue runs after the last panel.  Planes are padded to whole panels, so ONE instantiation per (kernel function, plane kind) serves every width
 *   above 128 features -- the 129 ... 512 range of the one-pass s6w_body layout included (the handle keeps the panel layout there as well: one layout, one kernel).
 *   FROM tile_matvec_f32_blk (lssvm_tile_f32_blk.hip.hpp): the TRANSPOSED first product and the second product on the matrix cores.  The operands of the plane products
 *   are swapped (A = the column fragment from the ring, B = the row panel): acc[rb][cb][e] of lane (r, g) = K[point 16 rb + r][column 16 cb + 4 g + e], which is where
 *   v_mfma_f32_16x16x4_f32 takes its A operand.  Folded rbf: c_i of point r is the start value at panel 0 (one register per row block and lane -- no c_i in LDS, which is
 *   what lets two workgroups share a CU).  After the epilogue's apply_kernel_function, four fp32 MFMAs per 16 x 16 block against the 64 x 16 record of the sub-tile
 *   ([column / 4][vector][column % 4], 4 KiB, k_pack_wblock_f32), lane (r, g) reading its four B values as one ds_read_b128; out2 is two f32x4 per wave carried across
 *   all tiles of the work item.  No per-vector fma chain, no row butterfly, no atomics, no scratch.
 *   RECORD TIMING.  s6x_body's rule is kept: the record of tile t' is issued with -- in front of -- the chunk of the tile's first step, three steps ahead, at a hand-over
 *   of tile t' - 1 (a tile has panels x NKC >= 8 steps here, so three steps ahead is never two tiles ahead and two slots suffice, unlike the narrow kernel at NKC = 2).
 *   Its two instructions are older than that chunk's four pieces, so the NEXT hand-over's counted wait (which leaves the four youngest outstanding) and barrier land and
 *   publish it, two steps before the tile begins and panels x NKC + 2 before its epilogue reads it.  The slot it overwrites was last read by the epilogue of tile
 *   t' - 2, which every wave left at least one barrier earlier.
 *   LDS: ring 64 KiB + 2 record slots 16 KiB = 80 KiB (B32_LDS_BYTES): two workgroups per CU.
 *   SUM ORDER of one value: the narrow kernel's -- the tiles of the work item in order, inside a tile cb, then e, one MFMA (four columns) per addition; then the column
 *   chunks' slabs in order (k_reduce_partials).  It depends on the shapes only, and on no other vector of the pass.  Per element the plane products are s6x_body's, in
 *   its order (panel by panel, chunk by chunk, column plane by column plane, k32 step by k32 step).
 * ===================================================================================================================== */
template <int KT, int PL>
__global__ __launch_bounds__(TILE_THREADS, 2) void tile_matvec_f32_blk_wide(const TileArgs<float> a) {
    static_assert(BLOCK_VECTORS == 16, "the second product is one 16 x 16 x 4 MFMA per four columns");
    static_assert(PL == 3 || PL == 2, "three bf16 planes (bf16x6) or two f16 planes (f16x3)");
    static_assert(KT == KT_RBFF || KT == KT_POLY || KT == KT_POLY2 || KT == KT_POLY3, "folded rbf and the polynomial forms: the forms whose epilogue needs no c_j");
    constexpr bool F16 = PL == 2;
    constexpr bool RBF = KT == KT_RBFF;
    constexpr int NK64 = 2;         // 64-feature chunks per panel
    constexpr int NKC = PL * NK64;  // plane-chunks (steps) per tile-panel
    constexpr int PLA = F16 ? (RBF ? 3 : 2) : 3;  // row planes in registers (s6w_body: the shifted rbf planes)
    constexpr auto row_plane = [](int p, int q) constexpr { return (F16 && PLA == 3) ? (p == 0 ? (q == 0 ? 2 : 1) : 0) : q; };
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char *ring = smem_raw;                            // [V2_RING][128 columns][128 B]
    char *recs = smem_raw + V2_RING * V2_SLOT_BYTES;  // [B32_REC_SLOTS][32 column quads][16 vectors][4]

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
    const int panels = a.nk64 / NK64;  // (uniform; the planes are padded to a multiple of 128 features; at least 2: the launcher checks)
    const int steps_per_tile = panels * NKC;
    const int nsteps = ntiles * steps_per_tile;

    // ---- the row panel of ONE feature panel: lane (r, g) holds features 128 p + 32 kk + 8 g .. + 7 of point 16 rb + r -- here the B operand B[k = 8 g + j][n = r] ----
    // (uniform base in SGPRs + ONE 32-bit lane offset, as s6x_body's full-square variant)
    bf16x8 afrag[PLA][2 * NK64][2];
    const unsigned row_lane_off = 2u * static_cast<unsigned>(r * a.ldx16 + 8 * g);
    auto load_row_chunk = [&](int p, auto chunk_c) {  // all row planes of the 64-feature chunk `chunk` of panel p: k32 steps 2 chunk, 2 chunk + 1
        constexpr int chunk = decltype(chunk_c)::value;
#pragma unroll
        for (int pl = 0; pl < PLA; ++pl) {
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                const char *base = sgpr_ptr(a.Xr16 + pl * a.plane_stride_r + static_cast<size_t>(row0 + wave * 32 + 16 * rb) * a.ldx16 + p * (64 * NK64) + 64 * chunk);
                const auto *xr = (const __attribute__((address_space(1))) char *) base + lane_off(row_lane_off);
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) afrag[pl][2 * chunk + kk][rb] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const __attribute__((address_space(1))) f32x4 *>(xr + 64 * kk));
            }
        }
    };
    static_for<0, NK64>([&](auto c) { load_row_chunk(0, c); });
    [[maybe_unused]] float ci[2] = { 0.f, 0.f };  // folded rbf: c_i of point r of either row block, the start value of every accumulator at panel 0
    if constexpr (RBF) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) ci[rb] = a.cr[row0 + wave * 32 + 16 * rb + r];
    }
    // make the compiler retire these ordinary loads HERE, before any LDS-DMA is in flight
#pragma unroll
    for (int pl = 0; pl < PLA; ++pl)
#pragma unroll
        for (int kk = 0; kk < 2 * NK64; ++kk)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) asm volatile("" : "+v"(afrag[pl][kk][rb]));
    if constexpr (RBF) asm volatile("" : "+v"(ci[0]), "+v"(ci[1]));

    // ---- LDS-DMA addressing of the column planes (the LDS image of a plane-chunk is that of s6w_body, whichever operand the fragment becomes) ----
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
    auto issue_chunk = [&](int step) {  // step = (tile t, panel p, plane-chunk kc): plane kc % PL of the 64-feature chunk kc / PL of panel p
        const int t = step / steps_per_tile;
        const int in_tile = step - t * steps_per_tile;
        const int p = in_tile / NKC;
        const int kc = in_tile - p * NKC;
        const int chunk = kc / PL;
        const int plane = kc % PL;
        const char *base = sgpr_ptr(a.Xc16 + plane * a.plane_stride + static_cast<size_t>(jt_begin + t) * TILE * a.ldx16 + (p * NK64 + chunk) * 64);
        const unsigned slot = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(dma_lds + static_cast<unsigned>(step % V2_RING) * V2_SLOT_BYTES)));
        static_for<0, 4>([&](auto i_c) { lds_dma16<decltype(i_c)::value * 1024>(dma_off[decltype(i_c)::value], base, slot); });
    };
    auto issue_rec = [&](int t) {  // each wave its quarter of the tile's two records: two full instructions, lane-linear in LDS
        const char *src = sgpr_ptr(reinterpret_cast<const char *>(a.dc) + static_cast<size_t>(jt_begin + t) * B32_REC_BYTES + __builtin_amdgcn_readfirstlane(wave * 2048));
        const unsigned dst = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(rec_lds + static_cast<unsigned>(t % B32_REC_SLOTS) * B32_REC_BYTES)));
        const unsigned off = 16u * (lane_off(threadIdx.x) & 63u);
        lds_dma16<0>(off, src, dst);
        lds_dma16<1024>(off, sgpr_ptr(src + 1024), dst);
    };

    // ---- read addressing of the ring (s6w_body's) and of the record (the narrow block kernel's) ----
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

    // ---- prologue: the first tile's record, then chunks 0, 1, 2 (a tile has at least 2 x NKC >= 8 steps) ----
    issue_rec(0);
    issue_chunk(0);
    issue_chunk(1);
    issue_chunk(2);
    asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    f32x4 bbuf[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) bbuf[0][c] = *reinterpret_cast<const f32x4 *>(ring + c * 2048 + rd_off[0]);

    // hand-over of the next chunk in the middle of a step: s6x_body's checked form, the record of a tile in front of the chunk of its first step
    auto handover = [&](int step) {
        if (step + 1 < nsteps) {
            if (step + 2 < nsteps) {
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (step + 3 < nsteps) {
                const int s3 = step + 3;
                const int t3 = s3 / steps_per_tile;
                if (s3 - t3 * steps_per_tile == 0) issue_rec(t3);
                issue_chunk(s3);
            }
        }
    };

    for (int t = 0; t < ntiles; ++t) {
        // start values of the chain: folded rbf c_i of the point (c_j is the factor 2^c_j inside the record), polynomial 0
#pragma unroll
        for (int cb = 0; cb < 8; ++cb)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) acc[rb][cb] = f32x4{ ci[rb], ci[rb], ci[rb], ci[rb] };
        for (int p = 0; p < panels; ++p) {
            // (the row panel of this tile-panel was requested chunk by chunk while the previous one was being multiplied: see below)
            const bool more_panels = t + 1 < ntiles || p + 1 < panels;
            const int p_next = p + 1 < panels ? p + 1 : 0;  // (the row panel depends on the feature panel only, not on the tile)
            const int s0 = t * steps_per_tile + p * NKC;
            const unsigned phase = static_cast<unsigned>(s0) & (V2_RING - 1);
            static_for<0, NKC>([&](auto kc_c) {
                constexpr int kc = decltype(kc_c)::value;
                constexpr int chunk = kc / PL, plane = kc % PL;
                const int step = s0 + kc;
                const char *slot = ring + ((phase + kc) & (V2_RING - 1)) * V2_SLOT_BYTES;
                const char *slot_next = ring + ((phase + kc + 1) & (V2_RING - 1)) * V2_SLOT_BYTES;
                static_for<0, 4>([&](auto mm_c) {
                    constexpr int mm = decltype(mm_c)::value;
                    constexpr int kk = mm >> 1, cbh = mm & 1;
                    f32x4(&bcur)[4] = bbuf[mm & 1];
                    f32x4(&bnext)[4] = bbuf[(mm + 1) & 1];
                    if constexpr (mm < 3) {  // next group of this chunk
#pragma unroll
                        for (int c = 0; c < 4; ++c) bnext[c] = *reinterpret_cast<const f32x4 *>(slot + (4 * ((mm + 1) & 1) + c) * 2048 + rd_off[(mm + 1) >> 1]);
                        if constexpr (mm != 2) LSSVM_SCHED_BARRIER();
                    }
                    if constexpr (mm == 2) {
                        handover(step);
                        LSSVM_SCHED_BARRIER();
                    }
                    if constexpr (mm == 3) {  // first group of the next chunk: visible since this step's hand-over
                        if (step + 1 < nsteps) {
#pragma unroll
                            for (int c = 0; c < 4; ++c) bnext[c] = *reinterpret_cast<const f32x4 *>(slot_next + c * 2048 + rd_off[0]);
                        }
                        LSSVM_SCHED_BARRIER();
                    }
                    // the row planes this column plane meets: those of equal or lower order
#pragma unroll
                    for (int q = 0; q < PL - plane; ++q) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const int cb = 4 * cbh + c;
                            const bf16x8 bv = __builtin_bit_cast(bf16x8, bcur[c]);
                            // (transposed: the column fragment is A, the row panel B)
#pragma unroll
                            for (int rb = 0; rb < 2; ++rb) acc[rb][cb] = plane_mfma<F16>(bv, afrag[row_plane(plane, q)][2 * chunk + kk][rb], acc[rb][cb]);
                        }
                    }
                });
                // the last plane of a 64-feature chunk is through: its row fragments are dead, the registers take the same chunk of the NEXT tile-panel
                if constexpr (plane == PL - 1) {
                    if (more_panels) load_row_chunk(p_next, std::integral_constant<int, chunk>{});
                }
            });
        }
        // ---- epilogue of the tile: the kernel value per element on the vector ALU, in place; then four columns x sixteen vectors per fp32 MFMA ----
        const char *rec = recs + (t % B32_REC_SLOTS) * B32_REC_BYTES + rec_off;  // (landed and published two steps before the tile's first)
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
    }

    // plane v of the row slabs takes vector v: lane (r, g) holds points 4 g .. 4 g + 3 of either row block for vector r -- one 16-byte store per row block
    float *dst = a.partial + static_cast<size_t>(r) * a.part_vstride + static_cast<size_t>(jc) * a.part_stride + ibl * TILE + wave * 32 + 4 * g;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) *reinterpret_cast<f32x4 *>(dst + 16 * rb) = out2[rb];
}

}  // namespace lssvm
