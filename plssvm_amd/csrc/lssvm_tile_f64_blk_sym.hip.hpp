/*
 * lssvm_tile_f64_blk_sym.hip.hpp -- tile_matvec_f64_blk_sym: the SYMMETRIC fp64 tile kernel with SIXTEEN vectors per pass, the Gram pass of
 * the block lockstep CG behind lssvm_mi355_problem_solve_lockstep_block / _matvec_block.  Included by tile_launch_f64blks.hip only.
 */
#pragma once

#include "lssvm_tile_f64_blk.hip.hpp"  // the record of a sub-tile (V2B_REC_*), the ring's geometry: the pipeline is tile_matvec_f64_v2<..., SYM = true>'s

namespace lssvm {

/* =====================================================================================================================
 * A tile K_IJ below the diagonal owes two products, out_I += K_IJ V_J and the mirror out_J += K_IJ^T V_I, and an MFMA accumulator that becomes an operand of
 * the next MFMA contracts over its own m index (D[m = q + 4 i][n = r] in register i of lane (r, q) = (lane & 15, lane >> 4); the lane supplies B[k = q][n = r]).
 *   FIRST PRODUCT: tile_matvec_f64_v2's, un-transposed (A = the row panel in registers, B = the column fragment from the ring): acc[rb][cb][i] of lane (r, q) =
 *   K[row 16 rb + 4 i + q][col 16 cb + r].  rbf: start value c_i + c_j; the other forms: the constant 0 as the C operand.  KERNEL VALUE per element, in place.
 *   MIRROR PRODUCT, straight from the accumulators.  For fixed (rb, i) the lane's kernel value is B[k = q][n = col r] of the rows 16 rb + 4 i + q; with
 *   A[m = v][k = q] = V_I[row 16 rb + 4 i + q][v = r] -- eight doubles per lane, loaded once per work item from the records of sub-tiles 2 ib, 2 ib + 1 --
 *   colout[cb] += A B is the 16-vector x 16-column block of K_IJ^T V_I over this wave's 32 rows: colout[cb][i] of lane (r, q) = out[v = q + 4 i][col 16 cb + r].
 *   It starts from the constant 0 in every sub-tile.  32 MFMAs per wave and sub-tile.
 *   ROW PRODUCT, after one transposition through LDS.  The wave writes a 16 x 16 block of kernel values to a scratch of its own and reads it back transposed:
 *   element (a, b) of the block lives at double a * 16 + ((b + 2 (a >> 1)) & 15).  The write (a = 4 i + q, b = r) covers two whole rows per half-wave, the read
 *   (a = r, b = 4 i + q) eight disjoint pairs per row parity: neither side of the ds_*_b64 conflicts, without padding.  The block read back is the operand
 *   tile_matvec_f64_blk has (kt[i] = K[row 16 rb + r][col 16 cb + 4 i + q]), and out2[rb] += alpha^T kt is its second product, carried across the whole work
 *   item.  32 more MFMAs.  Nothing crosses lanes on the vector ALU: v_mfma_f64 does not overlap it, but it does overlap LDS traffic.  Two scratch blocks per
 *   wave alternate, so that a block's read-back is in flight under the mirror MFMAs of the next.
 *   MIRRORED COLUMN SUMS.  The four waves hold different rows of the same 64 columns x 16 vectors: each stores its colout to a staging area (plane v at 64 v,
 *   column c at c ^ 16 (v & 1): conflict free), and behind the barrier of the next sub-tile's hand-over every thread adds the four waves' values of four
 *   (vector, column) pairs in wave order, (w0 + w1) + (w2 + w3), and stores them to plane v of the column slab (TileArgs::colslab_vstride).  The staging area is
 *   double buffered (the flush of sub-tile t reads while the epilogue of t + 1 writes): 2 x 32 KiB.  With the ring, the records and the scratch that is 147 KiB of
 *   gfx950's 160 KiB: ONE workgroup per CU at every chunk count, where the pair kernel has two up to four chunks.
 *   Diagonal sub-tiles are evaluated in full, contribute to the rows only (their colout is never staged) -- as in tile_matvec_f64_v2.
 *   SUM ORDER of one value.  Row product: tile_matvec_f64_blk's -- the sub-tiles of the work item in order, inside one cb, then i, one MFMA (four columns) per
 *   addition; then the chunk slabs in order (k_reduce_partials_sym).  Mirror: inside a sub-tile rb, then i, one MFMA (four rows) per addition; the four waves;
 *   then the row blocks' records in k_reduce_colslab's order.  It depends on the shapes only, and on no other vector of the pass.
 * ===================================================================================================================== */
constexpr int V2BS_SCRATCH_BLOCKS = 2;                                                      // 16 x 16 transposition blocks per wave
constexpr size_t V2BS_STAGE_BYTES = static_cast<size_t>(2) * 4 * BLOCK_VECTORS * 64 * 8;    // [buffer][wave][vector][column]: 64 KiB
constexpr size_t V2BS_LDS_BYTES = V2B_LDS_BYTES + TILE * 8 + V2BS_STAGE_BYTES + 4 * V2BS_SCRATCH_BLOCKS * 2048;  // ring, records | c_i | staging | scratch: 147 KiB

template <int KT, int NKC>
__global__ __launch_bounds__(TILE_THREADS, 1) void tile_matvec_f64_blk_sym(const TileArgs<double> a) {
    static_assert(BLOCK_VECTORS == 16, "both second products are 16 x 16 x 4 MFMAs with the vectors in m");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char *ring = smem_raw;
    char *recs = smem_raw + V2D_RING * V2D_SLOT_BYTES;
    double *cis = reinterpret_cast<double *>(smem_raw + V2B_LDS_BYTES);  // [128] c_i of the row panel (rbf)
    double *stage = cis + TILE;                                         // [2][4 waves][16 vectors][64 columns]
    double *scratch = stage + V2BS_STAGE_BYTES / 8;                      // [4 waves][V2BS_SCRATCH_BLOCKS][256]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15;
    const int q = lane >> 4;

    const int2 it = a.items[blockIdx.x];
    const int ibl = __builtin_amdgcn_readfirstlane(it.x);
    const int jc = __builtin_amdgcn_readfirstlane(it.y);
    const int ib = a.ib_begin + ibl;
    const int row0 = ib * TILE;
    const int jt_begin = jc * a.jc_tiles;
    const int jt_end = min(jt_begin + a.jc_tiles, ib + 1);
    const int nsub = 2 * (jt_end - jt_begin);  // 64-column sub-tiles; sub-tile st is below the diagonal block iff st < 2 ib
    if (nsub <= 0) return;
    const int st_begin = 2 * jt_begin;
    const int nsteps = nsub * NKC;
    const long rec0 = static_cast<long>(ib) * (ib - 1) - 2 * a.pair_origin;  // column-slab record of (ib, sub-tile 0)

    // row panel: A operand of lane (r, q) for k-step s is X[row][4 s + q]
    double afrag[2][4 * NKC];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const double *xr = a.Xr + static_cast<size_t>(row0 + wave * 32 + rb * 16 + r) * a.ldx + q;
#pragma unroll
        for (int s = 0; s < 4 * NKC; ++s) afrag[rb][s] = xr[4 * s];
    }
    // the row block's vectors, A operand of the mirror product: vi[rb][i] = V_I[row wave * 32 + 16 rb + 4 i + q][vector r], from the records of sub-tiles 2 ib, 2 ib + 1
    double vi[2][4];
    {
        const double *vr = a.dc + static_cast<size_t>(2 * ib + (wave >> 1)) * V2B_REC_DOUBLES + ((wave & 1) * 32 + q) * BLOCK_VECTORS + r;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int i = 0; i < 4; ++i) vi[rb][i] = vr[(rb * 16 + 4 * i) * BLOCK_VECTORS];
    }
    if constexpr (KT == KT_RBF) {
        if (tid < TILE) cis[tid] = a.cr[row0 + tid];
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
        for (int s = 0; s < 4 * NKC; ++s) asm volatile("" : "+v"(afrag[rb][s]));
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(vi[rb][i]));
    }

    // chunk DMA, record DMA and read addressing: tile_matvec_f64_blk's (LDS image [column block cb][16-byte k-slot ks][column r], see tile_matvec_f64_v2)
    unsigned dma_off[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int col = wave * 16 + (lane & 15);
        const int ks = 4 * i + (lane >> 4);
        dma_off[i] = 8u * static_cast<unsigned>(col * a.ldx + 2 * ks);
    }
    const unsigned ring_lds = static_cast<unsigned>(reinterpret_cast<size_t>(ring));
    const unsigned dma_lds = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(ring_lds + static_cast<unsigned>(wave) * 2048u)));
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

    // the transposition scratch of this wave: where the lane writes element (a = 4 i + q, b = r) and reads element (a = r, b = 4 i + q) of a block
    double *scr = scratch + wave * (V2BS_SCRATCH_BLOCKS * 256);
    int wofs[4], rofs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        wofs[i] = (4 * i + q) * 16 + ((r + 4 * i + 2 * (q >> 1)) & 15);
        rofs[i] = r * 16 + ((4 * i + q + 2 * (r >> 1)) & 15);
    }
    // the staging area: the lane's colout[cb][i] is (vector q + 4 i, column 16 cb + r)
    const int stage_w = wave * (BLOCK_VECTORS * 64) + q * 64 + r;  // + i * 256 + ((16 cb) ^ stage_x)
    const int stage_x = 16 * (q & 1);

    f64x4 acc[2][4];
    f64x4 out2[2];  // [vector q + 4 i][row 16 rb + r]: the block of the row product, across every sub-tile of the work item
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

    // hand-over of the next chunk in the middle of a step: tile_matvec_f64_v2's.  `must_sync`: the caller publishes staged column sums at this barrier, so the
    // checked form keeps the barrier where no chunk is left to hand over.  (The column slab's stores count in vmcnt like the DMA: a wait that leaves the two youngest
    // operations outstanding then covers more than it needs to, never less.)
    auto handover = [&](int step, int kc_plus3_mod, bool must_sync, auto checked) {
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
            } else if (must_sync) {
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
        }
    };

    // fixed-order sum of the four waves' staged column sums of sub-tile t -> sixteen planes of its slab record; thread (wave, lane): vectors 4 wave .. 4 wave + 3 of column `lane`
    auto flush_cols = [&](int t) {
        const double *sg = stage + (t & 1) * (4 * BLOCK_VECTORS * 64);
        // (an explicit GLOBAL pointer: through the generic one the store is a flat_store, which counts in lgkmcnt as well and completes out of order)
        auto *rec = (__attribute__((address_space(1))) double *) (a.colslab + (rec0 + st_begin + t) * 64);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = 4 * wave + k;
            const double *p = sg + v * 64 + (lane ^ (16 * (k & 1)));
            const double s = (p[0] + p[BLOCK_VECTORS * 64]) + (p[2 * BLOCK_VECTORS * 64] + p[3 * BLOCK_VECTORS * 64]);
            rec[static_cast<long>(v) * a.colslab_vstride + lane] = s;
        }
    };

    auto tile_body = [&](int t, auto checked) {
        const int s0 = t * NKC;
        const char *rec = recs + (t % V2B_REC_SLOTS) * V2B_REC_BYTES;
        const double *alr = reinterpret_cast<const double *>(rec) + q * BLOCK_VECTORS + r;  // alpha[16 cb + 4 i + q][r] at + (16 cb + 4 i) * 16
        if constexpr (KT == KT_RBF) {
            const double *cjr = reinterpret_cast<const double *>(rec) + 64 * BLOCK_VECTORS + r;  // c_j[16 cb + r]
            double cj[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) cj[cb] = cjr[cb * 16];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double civ = cis[wave * 32 + rb * 16 + q + 4 * i];
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) acc[rb][cb][i] = civ + cj[cb];
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
                if (s == 2) {
                    // sub-tile t - 1 was off-diagonal unless it is the first of the diagonal pair: its staged column sums are published by this barrier
                    const bool flush = kc == 0 && t > 0 && (st_begin + t - 1 < 2 * ib);
                    if (kc == 0 && t > 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (and the reads of the flush before: the buffer is written again after the NEXT barrier)
                    handover(step, (kc + 3) % NKC, flush, checked);
                    if (flush) flush_cols(t - 1);
                }
                if (s == 3) read_group(slot_next, 0, bnext);
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) {
                        if (KT != KT_RBF && kc == 0 && s == 0) {
                            const f64x4 zero = { 0.0, 0.0, 0.0, 0.0 };
                            acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(afrag[rb][0], bcur[cb], zero, 0, 0, 0);
                        } else {
                            acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(afrag[rb][4 * kc + s], bcur[cb], acc[rb][cb], 0, 0, 0);
                        }
                    }
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) bcur[cb] = bnext[cb];
            }
        }
        // ---- epilogue of the sub-tile: the kernel value per element on the vector ALU, then both second products on the matrix cores ----
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
        double *sw = stage + (t & 1) * (4 * BLOCK_VECTORS * 64) + stage_w;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            f64x4 colout;  // [vector q + 4 i][column 16 cb + r] over this wave's 32 rows
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                double *blk = scr + ((2 * cb + rb) % V2BS_SCRATCH_BLOCKS) * 256;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    double kv;
                    if constexpr (v2_base_kt(KT) == KT_POLY) {
                        kv = poly_power<v2_degree_class(KT)>(acc[rb][cb][i], a.degree);  // (the data carries sqrt(gamma), coef0 was added above)
                    } else {
                        kv = exp2_f64(acc[rb][cb][i]);  // the data is pre-scaled: acc = log2(K)
                    }
                    blk[wofs[i]] = kv;
                    if (rb == 0 && i == 0) {
                        const f64x4 zero = { 0.0, 0.0, 0.0, 0.0 };
                        colout = __builtin_amdgcn_mfma_f64_16x16x4f64(vi[0][0], kv, zero, 0, 0, 0);
                    } else {
                        colout = __builtin_amdgcn_mfma_f64_16x16x4f64(vi[rb][i], kv, colout, 0, 0, 0);
                    }
                }
                asm volatile("" ::: "memory");  // the wave's LDS operations execute in order: the read-back below sees every lane's writes
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double kt = blk[rofs[i]];                                // K[row 16 rb + r][col 16 cb + 4 i + q]
                    const double al = alr[(cb * 16 + 4 * i) * BLOCK_VECTORS];     // alpha[col 16 cb + 4 i + q][vector r]
                    out2[rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(al, kt, out2[rb], 0, 0, 0);
                }
                asm volatile("" ::: "memory");
            }
            // (a diagonal sub-tile stages nothing: whoever writes a buffer has a flush of its predecessor, hence a barrier, behind the last reads of that buffer)
            if (st_begin + t < 2 * ib) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sw[i * 256 + ((cb * 16) ^ stage_x)] = colout[i];
            }
        }
    };

    // steady state: every sub-tile whose last step still has step + 3 < nsteps; then the tail sub-tiles with the checked hand-over
    constexpr int TAIL_TILES = (3 + NKC - 1) / NKC;
    const int nmain = nsub > TAIL_TILES ? nsub - TAIL_TILES : 0;
    int t = 0;
    for (; t < nmain; ++t) tile_body(t, std::false_type{});
    for (; t < nsub; ++t) tile_body(t, std::true_type{});
    if (st_begin + nsub - 1 < 2 * ib) {  // the last sub-tile was off-diagonal: publish its column sums
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        flush_cols(nsub - 1);
    }

    // plane v of the row slabs takes vector v: lane (r, q) holds vectors q + 4 i of rows 16 rb + r (16 lanes = 128 contiguous bytes per store)
    double *dst = a.partial + static_cast<size_t>(jc) * a.part_stride + ibl * TILE + wave * 32 + r;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[static_cast<size_t>(q + 4 * i) * a.part_vstride + rb * 16] = out2[rb][i];
}

/* the records of tile_matvec_f64_blk_sym for `count` (1 ... 16) vectors that live in buffers of their own: k_pack_ablock_f64's layout (dc[st][16 l + u] = v_u[64 st + l],
 * u >= count: 0; dc[st][1024 + l] = c[64 st + l]); the same launch clears the `nzero` leading entries of every result vector, which the symmetric pass adds into */
struct BlockVectors {
    const double *v[BLOCK_VECTORS];
    double *Kv[BLOCK_VECTORS];
};
#ifdef LSSVM_KERNELS_BLOCK_SYM_PACK
__global__ void k_pack_vblock_f64(const BlockVectors bv, int count, const double *__restrict__ cc, int ncols_padded, double *__restrict__ dc, int nzero) {
    const size_t e = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const size_t j = e / BLOCK_VECTORS;
    const int u = static_cast<int>(e % BLOCK_VECTORS);
    // (the 16 pointers are kernel arguments: select with a uniform-free chain instead of a dynamic index, which would put the struct into scratch)
    const double *src = nullptr;
    double *dst = nullptr;
#pragma unroll
    for (int k = 0; k < BLOCK_VECTORS; ++k) {
        if (u == k) {
            src = bv.v[k];
            dst = bv.Kv[k];
        }
    }
    if (u < count && j < static_cast<size_t>(nzero)) dst[j] = 0.0;
    if (j >= static_cast<size_t>(ncols_padded)) return;
    const size_t st = j >> 6, l = j & 63;
    dc[st * V2B_REC_DOUBLES + l * BLOCK_VECTORS + u] = (u < count) ? src[j] : 0.0;
    if (u == 0) dc[st * V2B_REC_DOUBLES + 64 * BLOCK_VECTORS + l] = (cc != nullptr) ? cc[j] : 0.0;
}
#endif  // LSSVM_KERNELS_BLOCK_SYM_PACK
}  // namespace lssvm
