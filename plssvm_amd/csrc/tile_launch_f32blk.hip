/*
 * tile_launch_f32blk.hip -- instantiates and launches tile_matvec_f32_blk (sixteen weight vectors per full-square fp32 pass: lssvm_tile_f32_blk.hip.hpp) and packs
 * its records.  Compiled for gfx950 only, as TWO translation units (tile_launch_f32blk_a.hip: LSSVM_TU_HALF 1 = the f16x3 planes, the entry points and the packing
 * kernel; tile_launch_f32blk_b.hip: LSSVM_TU_HALF 2 = the bf16x6 planes), eight instantiations each, so that the build spreads over more cores.
 */
#ifndef LSSVM_TU_HALF
#error "compile tile_launch_f32blk_a.hip / _b.hip"
#endif
#if LSSVM_TU_HALF == 1
#define LSSVM_KERNELS_BLOCK_PACK
#endif

#include "tile_launch.hip.hpp"

#include "lssvm_tile_f32_blk.hip.hpp"

namespace lssvm {

constexpr int B32_PL = LSSVM_TU_HALF == 1 ? 2 : 3;  // the plane kind this unit holds

/* 80 KiB of dynamic LDS: opted into per kernel and device */
template <int KT, int NK64>
static void launch_blk32(const TileArgs<float> &a, dim3 grid, hipStream_t s) {
    ensure_dynamic_lds(tile_matvec_f32_blk<KT, NK64, B32_PL>, B32_LDS_BYTES);
    hipLaunchKernelGGL((tile_matvec_f32_blk<KT, NK64, B32_PL>), grid, dim3(TILE_THREADS), B32_LDS_BYTES, s, a);
}

template <int KT>
static void launch_blk32_kt(const TileArgs<float> &a, dim3 grid, hipStream_t s) {
    switch (a.nk64) {
        case 1: launch_blk32<KT, 1>(a, grid, s); break;
        case 2: launch_blk32<KT, 2>(a, grid, s); break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no sixteen-vector fp32 tile kernel for this number of features");
    }
}

static void launch_f32_block_here(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s) {
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree < 0) throw Error(LSSVM_ERR_INTERNAL, "the sixteen-vector fp32 tile kernel has no pad-column rule: degree >= 0");
            if (a.degree == 3) {
                launch_blk32_kt<KT_POLY3>(a, grid, s);
            } else if (a.degree == 2) {
                launch_blk32_kt<KT_POLY2>(a, grid, s);
            } else {
                launch_blk32_kt<KT_POLY>(a, grid, s);
            }
            break;
        case KT_RBF:
            if (a.dc_folded == 0 || a.rbf_grid != 0) throw Error(LSSVM_ERR_INTERNAL, "the sixteen-vector fp32 rbf kernel needs the folded records");
            launch_blk32_kt<KT_RBFF>(a, grid, s);
            break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no sixteen-vector fp32 tile kernel for this kernel function");  // (the linear kernel predicts through w)
    }
}

void launch_f32_block_bf16(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s);  // tile_launch_f32blk_b.hip: the bf16x6 planes
#if LSSVM_TU_HALF == 1
void launch_f32_block(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s) {
    if (a.items != nullptr || a.row_pair != 0 || a.wide_panels != 0) throw Error(LSSVM_ERR_INTERNAL, "sixteen weight vectors per fp32 pass: the 128-row full-square variant only");
    if (a.dc == nullptr || a.Xc16 == nullptr || a.Xr16 == nullptr || a.partial == nullptr || a.part_vstride < static_cast<long>(a.num_jc) * a.part_stride || a.part_vstride % 4 != 0)
        throw Error(LSSVM_ERR_INTERNAL, "the sixteen-vector kernel needs its planes, its records and sixteen planes of row slabs");
    if (a.planes_f16 != 0) {
        launch_f32_block_here(a, kernel_type, grid, s);
    } else {
        launch_f32_block_bf16(a, kernel_type, grid, s);
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}

void enqueue_pack_block_records(const float *alpha, size_t ld, int count, const float *cc, int folded, int ncols_padded, float *dc, hipStream_t s) {
    if (count < 1 || count > BLOCK_VECTORS || ncols_padded % TILE != 0) throw Error(LSSVM_ERR_INTERNAL, "a block record holds 1 ... 16 vectors over whole tiles");
    const size_t threads = static_cast<size_t>(ncols_padded) * BLOCK_VECTORS;
    hipLaunchKernelGGL(k_pack_wblock_f32, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, s, alpha, ld, count, cc, folded, ncols_padded, dc);
}
#else
void launch_f32_block_bf16(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s) { launch_f32_block_here(a, kernel_type, grid, s); }
#endif

}  // namespace lssvm
