/*
 * lssvm_tile_f32_blk_sym.hip.hpp -- tile_matvec_f32_blk_sym: the SYMMETRIC fp32 split tile kernel with SIXTEEN vectors per pass, the Gram
 * pass of the fp32 block lockstep CG behind lssvm_mi355_problem_solve_lockstep_block32 / _matvec_block32.  Included by tile_launch_f32blks.hip only.
 */
#pragma once

#include "lssvm_tile_f32_blk.hip.hpp"  // the W record of a tile (B32_REC_*), the ring's geometry, plane_mfma: the pipeline is tile_matvec_f32_blk's on s6w_body<..., SYM = true>'s work items

namespace lssvm {

/* =====================================================================================================================
 * A tile K_IJ below the diagonal owes two products, out_I += K_IJ W_J and the mirror out_J += K_IJ^T V_I, sixteen vectors each: two matrix products on
 * v_mfma_f32_16x16x4_f32, which takes A[i = r][k = g] and B[k = g][j = r] from lane (r, g) = (lane & 15, lane >> 4) and leaves D[i = 4 g + e][j = r] in register e.
 *   FIRST PRODUCT: tile_matvec_f32_blk's, TRANSPOSED (A = the column fragment from the ring, B = the row panel in registers): acc[rb][cb][e] of lane (r, g) =
 *   K[row 16 rb + r][column 16 cb + 4 g + e]; the plane products per element, their order and the kernel function are those of the single-vector kernel.  Folded
 *   rbf: the first MFMA's C operand is c_i, the value in the accumulators is 2^(c_i + dot).
 *   ROW PRODUCT, straight from the accumulators: tile_matvec_f32_blk's second product.  Register e of block (rb, cb) is A[row r][k = g] of the four columns
 *   16 cb + 4 g + e; with B[k = g][vector r] = W[16 cb + 4 g + e][r] from the record (ONE ds_read_b128 per block and lane), out2[rb] += A B: out2[rb][e'] of lane
 *   (r, g) = out[row 16 rb + 4 g + e'][vector r], carried in registers across the work item and stored once.  64 MFMAs per wave and tile.
 *   MIRROR PRODUCT, after one transposition through LDS.  The wave writes the 16 x 16 block of kernel values to a scratch of its own -- the lane's four values are
 *   four consecutive columns of one row: ONE ds_write_b128 -- and reads it back transposed, kt[e'] = K[row 16 rb + 4 g + e'][column 16 cb + r], four ds_read_b32.
 *   Element (row p, column c) of a block lives at float  16 (p / 4 + 4 (p % 4)) + 4 ((c / 4) ^ (p % 4)) + c % 4.  The write (p = r, c = 4 g ..): 16-byte slot
 *   4 (r / 4 + 4 (r % 4)) + (g ^ (r % 4)) -- the 64 lanes cover the block's 64 slots once, and the sixteen lanes of one g cover sixteen different slots modulo 16
 *   (4 (r / 4) + (g ^ (r % 4))), i.e. all 64 banks once per quarter wave.  The read (p = 4 g + e', c = r): float 16 (g + 4 e') + 4 ((r / 4) ^ e') + r % 4, bank
 *   16 g + 4 ((r / 4) ^ e') + r % 4 -- 64 lanes, 64 banks.  Neither side conflicts, without padding.  With A[i = vector r][k = g] = V_I[row 16 rb + 4 g + e'][r] --
 *   eight floats per lane, loaded once per work item from the PLAIN vectors (TileArgs::dvec: [row][16]) -- colout[cb] += A B is the 16-vector x 16-column block of
 *   K_IJ^T V_I over this wave's 32 rows: colout[cb][e''] of lane (r, g) = out[vector 4 g + e''][column 16 cb + r]; it starts from the constant 0 in every tile, rb
 *   then e'.  64 more MFMAs.  Two scratch blocks per wave alternate: a block's read-back is in flight under the row MFMAs of the next.  No kernel value crosses lanes
 *   on the vector ALU, no atomics, no scratch memory.
 *   FOLDED RBF: the row product takes W = 2^c_j v_j from the record; the mirror takes the plain V_I, and the wave's column sums are multiplied by 2^c_j once per
 *   column before they are staged (the rule of the two-vector s6w_body).  RECORD of a 128-column tile: W[2 sub-tiles][64 columns][16 vectors] in k_pack_wblock_f32's
 *   layout, 8 KiB, then 2^c_j of its 128 columns, 512 bytes (the polynomial forms carry and fetch the W part only): k_pack_vblock_f32_sym.  By LDS-DMA under the
 *   ring's counted waits, issued where tile_matvec_f32_blk issues its record.
 *   MIRRORED COLUMN SUMS.  The four waves hold different rows of the same 128 columns x 16 vectors: each stores its colout to a staging area (wave, vector v,
 *   column c at c ^ 16 (v / 4 % 4): the four lane groups of a ds_write_b32 land in four different bank quarters), and behind the barrier of the next tile's first
 *   hand-over thread (vector half h, column c) adds the four waves' values of its eight (vector, column) pairs in wave order, (w0 + w1) + (w2 + w3), and stores them
 *   to plane v of the column slab (TileArgs::colslab_vstride).  The staging area is double buffered (the flush of tile t reads while the epilogue of t + 1 writes).
 *   The diagonal tile is evaluated in full and contributes to the rows only.
 *   LDS: ring 64 KiB | 2 records 17 KiB | staging 2 x 32 KiB | scratch 4 x 2 x 1 KiB = 153 KiB of gfx950's 160: ONE workgroup per CU, one wave per SIMD.
 *   SUM ORDER of one value.  Row product: tile_matvec_f32_blk's -- the tiles of the work item in order, inside a tile cb, then e, one MFMA (four columns) per
 *   addition; then the chunk slabs in order (k_reduce_partials_sym).  Mirror: inside a tile rb, then e', one MFMA (four rows) per addition; (rbf: the factor;) the four
 *   waves; then the row blocks' records in k_reduce_colslab's order; the rows' sum is added on top.  It depends on the shapes only, and on no other vector of the pass.
 * ===================================================================================================================== */
constexpr int B32S_REC_BYTES = B32_REC_BYTES + TILE * 4;              // W of the tile's two sub-tiles | 2^c_j of its 128 columns
constexpr int B32S_STAGE_FLOATS = 4 * BLOCK_VECTORS * TILE;           // one staging buffer: [wave][vector][column], 32 KiB
constexpr int B32S_SCRATCH_BLOCKS = 2;                                // 16 x 16 transposition blocks per wave
constexpr size_t B32S_LDS_BYTES = static_cast<size_t>(V2_RING) * V2_SLOT_BYTES + B32_REC_SLOTS * B32S_REC_BYTES + 2 * B32S_STAGE_FLOATS * 4 + 4 * B32S_SCRATCH_BLOCKS * 1024;  // 153 KiB

template <int KT, int NK64, int PL>
__global__ __launch_bounds__(TILE_THREADS, 1) void tile_matvec_f32_blk_sym(const TileArgs<float> a) {
    static_assert(BLOCK_VECTORS == 16, "both second products are 16 x 16 x 4 MFMAs");
    static_assert(PL == 3 || PL == 2, "three bf16 planes (bf16x6) or two f16 planes (f16x3)");
    static_assert(NK64 == 1 || NK64 == 2, "the row panel in registers: at most 128 features");
    static_assert(KT == KT_RBFF || KT == KT_POLY || KT == KT_POLY2 || KT == KT_POLY3, "folded rbf and the polynomial forms");
    constexpr bool F16 = PL == 2;
    constexpr bool RBF = KT == KT_RBFF;
    constexpr int NKC = PL * NK64;  // steps per tile: for every 64-feature chunk the column planes hi, mid (, lo)
    static_assert(NKC >= 2, "the record of tile t + 1 lands at the second hand-over of tile t");
    constexpr int PLA = F16 ? (RBF ? 3 : 2) : 3;  // row planes in registers and the row plane of the q-th product of column plane p: s6w_body's
    constexpr auto row_plane = [](int p, int q) constexpr { return (F16 && PLA == 3) ? (p == 0 ? (q == 0 ? 2 : 1) : 0) : q; };
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char *ring = smem_raw;                                                                   // [V2_RING][128 columns][128 B]
    char *recs = smem_raw + V2_RING * V2_SLOT_BYTES;                                         // [B32_REC_SLOTS][W 8 KiB | e 512 B]
    float *stage = reinterpret_cast<float *>(recs + B32_REC_SLOTS * B32S_REC_BYTES);         // [2][4 waves][16 vectors][128 columns]
    float *scratch = stage + 2 * B32S_STAGE_FLOATS;                                          // [4 waves][B32S_SCRATCH_BLOCKS][256]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15;
    const int g = lane >> 4;

    const int2 it = a.items[blockIdx.x];
    const int ibl = __builtin_amdgcn_readfirstlane(it.x);
    const int jc = __builtin_amdgcn_readfirstlane(it.y);
    const int ib = a.ib_begin + ibl;
    const int row0 = ib * TILE;
    const int jt_begin = jc * a.jc_tiles;
    const int ntiles = min(jt_begin + a.jc_tiles, ib + 1) - jt_begin;  // clipped at the diagonal: tile t is below it iff jt_begin + t < ib
    if (ntiles <= 0) return;
    const int nsteps = ntiles * NKC;
    const long rec0 = static_cast<long>(ib) * (ib - 1) / 2 - a.pair_origin;  // column-slab record of (ib, tile 0)

    // ---- the row panel: tile_matvec_f32_blk's (the B operand B[k = 8 g + j][n = r]) ----
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
    [[maybe_unused]] f32x4 civ0[2] = { { 0.f, 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f, 0.f } };  // folded rbf: c_i of row r, the C operand of every accumulator's first MFMA
    if constexpr (RBF) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const float ci = a.cr[row0 + wave * 32 + 16 * rb + r];
            civ0[rb] = f32x4{ ci, ci, ci, ci };
        }
    }
    // the row block's plain vectors, A operand of the mirror product: vi[rb][e] = V_I[row 16 rb + 4 g + e][vector r]
    float vi[2][4];
    {
        const float *vr = a.dvec + static_cast<size_t>(row0 + wave * 32 + 4 * g) * BLOCK_VECTORS + r;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int e = 0; e < 4; ++e) vi[rb][e] = vr[(16 * rb + e) * BLOCK_VECTORS];
    }
    // make the compiler retire these ordinary loads HERE, before any LDS-DMA is in flight
#pragma unroll
    for (int p = 0; p < PLA; ++p)
#pragma unroll
        for (int kk = 0; kk < 2 * NK64; ++kk)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) asm volatile("" : "+v"(afrag[p][kk][rb]));
    if constexpr (RBF) asm volatile("" : "+v"(civ0[0]), "+v"(civ0[1]));
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(vi[rb][e]));

    // ---- LDS-DMA addressing of the column planes and of the record: tile_matvec_f32_blk's ----
    unsigned dma_off[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 8 * (4 * wave + i) + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        dma_off[i] = 2u * static_cast<unsigned>(row * a.ldx16 + 8 * c);
    }
    const unsigned ring_lds = static_cast<unsigned>(reinterpret_cast<size_t>(ring));
    const unsigned dma_lds = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(ring_lds + static_cast<unsigned>(wave) * 4096u)));
    // this wave's quarter of record slot 0: 2 KiB of W, 128 bytes of the factors behind the W part
    const unsigned rec_lds = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(ring_lds + V2_RING * V2_SLOT_BYTES + static_cast<unsigned>(wave) * 2048u)));
    [[maybe_unused]] const unsigned rece_lds = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(ring_lds + V2_RING * V2_SLOT_BYTES + B32_REC_BYTES + static_cast<unsigned>(wave) * 128u)));
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
    // (every record instruction is older than the chunk pieces issued behind it: the counted waits, which leave only the youngest chunk's four pieces outstanding,
    // cover them -- and the column slab's stores of a flush, which count in vmcnt like the DMA: such a wait then covers more than it needs to, never less)
    auto issue_rec = [&](int t) {
        const char *rec = reinterpret_cast<const char *>(a.dc) + static_cast<size_t>(jt_begin + t) * B32S_REC_BYTES;
        const char *src = sgpr_ptr(rec + __builtin_amdgcn_readfirstlane(wave * 2048));
        const unsigned slot_off = static_cast<unsigned>(__builtin_amdgcn_readfirstlane((t % B32_REC_SLOTS) * B32S_REC_BYTES));
        const unsigned off = 16u * (lane_off(threadIdx.x) & 63u);
        lds_dma16<0>(off, src, rec_lds + slot_off);
        lds_dma16<1024>(off, sgpr_ptr(src + 1024), rec_lds + slot_off);
        if constexpr (RBF) {
            if (lane < 8) lds_dma16<0>(off, sgpr_ptr(rec + B32_REC_BYTES + __builtin_amdgcn_readfirstlane(wave * 128)), rece_lds + slot_off);
        }
    };

    // ---- read addressing of the ring and of the record: tile_matvec_f32_blk's ----
    int rd_off[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) rd_off[kk] = r * 128 + (((4 * kk + g) ^ ((r >> 1) & 7)) << 4);
    const int rec_off = (g * 16 + r) * 16;  // + 1024 cb: W[16 cb + 4 g + e][r], e = 0 .. 3

    // the transposition scratch of this wave: where the lane writes its four columns 4 g .. 4 g + 3 of row r, and reads element (row 4 g + e, column r) of a block
    float *scr = scratch + wave * (B32S_SCRATCH_BLOCKS * 256);
    const int wofs = 16 * ((r >> 2) + 4 * (r & 3)) + 4 * (g ^ (r & 3));
    int rofs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) rofs[e] = 16 * (g + 4 * e) + 4 * ((r >> 2) ^ e) + (r & 3);
    // the staging area: the lane's colout[cb][e] is (vector 4 g + e, column 16 cb + r)
    const int stage_w = wave * (BLOCK_VECTORS * TILE) + 4 * g * TILE + r;  // + e * TILE + ((16 cb) ^ (16 g))

    f32x4 acc[2][8];
    f32x4 out2[2];  // [row 16 rb + 4 g + e][vector r]: the block of the row product, across every tile of the work item
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

    f32x4 bbuf[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) bbuf[0][c] = *reinterpret_cast<const f32x4 *>(ring + c * 2048 + rd_off[0]);

    // hand-over in the middle of a step: tile_matvec_f32_blk's.  `must_sync`: the caller publishes staged column sums at this barrier (a tile's FIRST hand-over:
    // NKC >= 2, so a next step -- and with it the barrier -- always exists there)
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

    // fixed-order sum of the four waves' staged column sums of tile t -> sixteen planes of its slab record; thread: column tid % 128, vectors 8 (tid / 128) .. + 7
    auto flush_cols = [&](int t) {
        const float *sg = stage + (t & 1) * B32S_STAGE_FLOATS;
        const int c = tid & (TILE - 1);
        const int v0 = 8 * (tid >> 7);
        // (an explicit GLOBAL pointer: through the generic one the store is a flat_store, which counts in lgkmcnt as well and completes out of order)
        auto *rec = (__attribute__((address_space(1))) float *) (a.colslab + (rec0 + jt_begin + t) * TILE);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int v = v0 + k;
            const float *p = sg + v * TILE + (c ^ (16 * ((v >> 2) & 3)));
            const float s = (p[0] + p[BLOCK_VECTORS * TILE]) + (p[2 * BLOCK_VECTORS * TILE] + p[3 * BLOCK_VECTORS * TILE]);
            rec[static_cast<long>(v) * a.colslab_vstride + c] = s;
        }
    };

    auto tile_body = [&](int t, auto checked) {
        const int s0 = t * NKC;
        const bool below = jt_begin + t < ib;  // strictly below the diagonal (uniform)
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
                if constexpr (mm < 3) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) bnext[c] = *reinterpret_cast<const f32x4 *>(slot + (4 * ((mm + 1) & 1) + c) * 2048 + rd_off[(mm + 1) >> 1]);
                    if constexpr (mm != 2) LSSVM_SCHED_BARRIER();
                }
                if constexpr (mm == 2) {
                    // tile t - 1 was below the diagonal (only a work item's last tile is not): its staged column sums are published by this barrier
                    if (kc == 0 && t > 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    handover(step, kc, t, checked);
                    if (kc == 0 && t > 0) flush_cols(t - 1);
                    LSSVM_SCHED_BARRIER();
                }
                if constexpr (mm == 3) {
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
        // ---- epilogue of the tile: the kernel value per element on the vector ALU, in place; then both second products on the matrix cores ----
        const char *rec = recs + (t % B32_REC_SLOTS) * B32S_REC_BYTES;  // (landed and published by the tile's second hand-over at the latest)
        auto epilogue = [&](auto with_cols) {
            constexpr bool COLS = decltype(with_cols)::value;
            float *sw = stage + (t & 1) * B32S_STAGE_FLOATS + stage_w;
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) {
                const f32x4 w = *reinterpret_cast<const f32x4 *>(rec + rec_off + cb * 1024);
                f32x4 colout = { 0.f, 0.f, 0.f, 0.f };  // [vector 4 g + e][column 16 cb + r] over this wave's 32 rows
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    f32x4 kv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) kv[e] = apply_kernel_function<v2_base_kt(KT), v2_degree_class(KT)>(acc[rb][cb][e], a);
                    float *blk = scr + ((2 * cb + rb) % B32S_SCRATCH_BLOCKS) * 256;
                    if constexpr (COLS) {
                        *reinterpret_cast<f32x4 *>(blk + wofs) = kv;
                        asm volatile("" ::: "memory");  // the wave's LDS operations execute in order: the read-back below sees every lane's writes
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) out2[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[e], w[e], out2[rb], 0, 0, 0);
                    if constexpr (COLS) {
                        float kt[4];  // K[row 16 rb + 4 g + e][column 16 cb + r]
#pragma unroll
                        for (int e = 0; e < 4; ++e) kt[e] = blk[rofs[e]];
                        asm volatile("" ::: "memory");
#pragma unroll
                        for (int e = 0; e < 4; ++e) colout = __builtin_amdgcn_mfma_f32_16x16x4f32(vi[rb][e], kt[e], colout, 0, 0, 0);
                    }
                }
                if constexpr (COLS) {
                    if constexpr (RBF) {
                        const float ej = *reinterpret_cast<const float *>(rec + B32_REC_BYTES + (cb * 16 + r) * 4);  // K_ij = 2^acc * 2^c_j: the column's factor once per column
#pragma unroll
                        for (int e = 0; e < 4; ++e) colout[e] *= ej;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) sw[e * TILE + ((cb * 16) ^ (16 * g))] = colout[e];
                }
            }
        };
        if (below) {
            epilogue(std::true_type{});
        } else {
            epilogue(std::false_type{});
        }
    };

    constexpr int TAIL_TILES = (3 + NKC - 1) / NKC;
    const int nmain = ntiles > TAIL_TILES ? ntiles - TAIL_TILES : 0;
    int t = 0;
    for (; t < nmain; ++t) tile_body(t, std::false_type{});
    for (; t < ntiles; ++t) tile_body(t, std::true_type{});
    if (jt_begin + ntiles - 1 < ib) {  // the last tile was below the diagonal: publish its column sums
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        flush_cols(ntiles - 1);
    }

    // plane v of the row slabs takes vector v: lane (r, g) holds rows 4 g .. 4 g + 3 of either row block for vector r -- one 16-byte store per row block
    float *dst = a.partial + static_cast<size_t>(r) * a.part_vstride + static_cast<size_t>(jc) * a.part_stride + ibl * TILE + wave * 32 + 4 * g;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) *reinterpret_cast<f32x4 *>(dst + 16 * rb) = out2[rb];
}

/* the records of tile_matvec_f32_blk_sym for `count` (1 ... 16) vectors that live in buffers of their own.  Per 128-column tile jt, at float jt * (B32S_REC_BYTES / 4):
 * the W part in k_pack_wblock_f32's layout ([sub-tile][column / 4][vector][column % 4]: W = v, or -- folded != 0 -- 2^c_j v with k_pack_dc's statements, u >= count:
 * 0), then 2^c_j of the tile's 128 columns (folded != 0 only).  vp[j][u] = v_u[j] (u >= count: 0): the plain vectors row-major, the mirror product's A operand.  The
 * same launch clears the `nzero` leading entries of every result vector, which the symmetric pass adds into.  One thread per (column, vector slot). */
struct BlockVectors32 {
    const float *v[BLOCK_VECTORS];
    float *Kv[BLOCK_VECTORS];
};
#ifdef LSSVM_KERNELS_BLOCK_SYM_PACK
__global__ void k_pack_vblock_f32_sym(const BlockVectors32 bv, int count, const float *__restrict__ cc, int folded, int ncols_padded, float *__restrict__ dc, float *__restrict__ vp, int nzero) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const size_t j = i / BLOCK_VECTORS;
    const int u = static_cast<int>(i % BLOCK_VECTORS);
    // (the 16 pointers are kernel arguments: select with a uniform-free chain instead of a dynamic index, which would put the struct into scratch)
    const float *src = nullptr;
    float *dst = nullptr;
#pragma unroll
    for (int k = 0; k < BLOCK_VECTORS; ++k) {
        if (u == k) {
            src = bv.v[k];
            dst = bv.Kv[k];
        }
    }
    if (u < count && j < static_cast<size_t>(nzero)) dst[j] = 0.0f;
    if (j >= static_cast<size_t>(ncols_padded)) return;
    const float d = (u < count) ? src[j] : 0.0f;
    float w = d, e = 1.0f;
    if (folded) {
        const float c = (cc != nullptr) ? cc[j] : 0.0f;
        e = __builtin_amdgcn_exp2f(c);
        w = e * d;
    }
    float *rec = dc + (j >> 7) * (B32S_REC_BYTES / 4);
    const size_t l = j & 63;
    rec[((j >> 6) & 1) * (64 * BLOCK_VECTORS) + ((l >> 2) * BLOCK_VECTORS + u) * 4 + (l & 3)] = w;
    if (folded && u == 0) rec[B32_REC_FLOATS + (j & 127)] = e;
    vp[j * BLOCK_VECTORS + u] = d;
}
#endif  // LSSVM_KERNELS_BLOCK_SYM_PACK
}  // namespace lssvm
