/*
 * tile_launch_f64blk.hip -- instantiates and launches tile_matvec_f64_blk (sixteen weight vectors per full-square fp64 pass: lssvm_tile_f64_blk.hip.hpp) and packs
 * its records.  Compiled for gfx950 only, as TWO translation units (tile_launch_f64blk_a.hip: LSSVM_TU_HALF 1 = 1 ... 6 chunks, the entry points and the packing
 * kernel; tile_launch_f64blk_b.hip: LSSVM_TU_HALF 2 = 7 ... 16 chunks), so that the build spreads over more cores.
 */
#ifndef LSSVM_TU_HALF
#error "compile tile_launch_f64blk_a.hip / _b.hip"
#endif
#if LSSVM_TU_HALF == 1
#define LSSVM_KERNELS_BLOCK_PACK
#endif

#include "tile_launch.hip.hpp"

#include "lssvm_tile_f64_blk.hip.hpp"

namespace lssvm {

/* 66 KiB of dynamic LDS: opted into per kernel and device */
template <int KT, int NKC>
static void launch_blk(const TileArgs<double> &a, dim3 grid, hipStream_t s) {
    ensure_dynamic_lds(tile_matvec_f64_blk<KT, NKC>, V2B_LDS_BYTES);
    hipLaunchKernelGGL((tile_matvec_f64_blk<KT, NKC>), grid, dim3(TILE_THREADS), V2B_LDS_BYTES, s, a);
}

template <int KT>
static void launch_blk_kt(const TileArgs<double> &a, dim3 grid, hipStream_t s) {
    switch (a.kchunks) {
#if LSSVM_TU_HALF == 1
        case 1: launch_blk<KT, 1>(a, grid, s); break;
        case 2: launch_blk<KT, 2>(a, grid, s); break;
        case 3: launch_blk<KT, 3>(a, grid, s); break;
        case 4: launch_blk<KT, 4>(a, grid, s); break;
        case 5: launch_blk<KT, 5>(a, grid, s); break;
        case 6: launch_blk<KT, 6>(a, grid, s); break;
#else
        case 7: launch_blk<KT, 7>(a, grid, s); break;
        case 8: launch_blk<KT, 8>(a, grid, s); break;
        case 10: launch_blk<KT, 10>(a, grid, s); break;
        case 12: launch_blk<KT, 12>(a, grid, s); break;
        case 14: launch_blk<KT, 14>(a, grid, s); break;
        case 16: launch_blk<KT, 16>(a, grid, s); break;
#endif
        default: throw Error(LSSVM_ERR_INTERNAL, "no sixteen-vector fp64 tile kernel for this number of k-chunks");
    }
}

static void launch_v2d_block_here(const TileArgs<double> &a, int kernel_type, dim3 grid, hipStream_t s) {
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree == 3) {
                launch_blk_kt<KT_POLY3>(a, grid, s);
            } else if (a.degree == 2) {
                launch_blk_kt<KT_POLY2>(a, grid, s);
            } else {
                launch_blk_kt<KT_POLY>(a, grid, s);
            }
            break;
        case KT_RBF: launch_blk_kt<KT_RBF>(a, grid, s); break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no sixteen-vector fp64 tile kernel for this kernel function");  // (the linear kernel predicts through w)
    }
}

void launch_v2d_block_wide(const TileArgs<double> &a, int kernel_type, dim3 grid, hipStream_t s);  // tile_launch_f64blk_b.hip: 7 ... 16 chunks
#if LSSVM_TU_HALF == 1
void launch_v2d_block(const TileArgs<double> &a, int kernel_type, dim3 grid, hipStream_t s) {
    if (a.dc == nullptr || a.partial == nullptr || a.part_vstride < static_cast<long>(a.num_jc) * a.part_stride) throw Error(LSSVM_ERR_INTERNAL, "the sixteen-vector kernel needs its records and sixteen planes of row slabs");
    if (a.kchunks > 6) {
        launch_v2d_block_wide(a, kernel_type, grid, s);
    } else {
        launch_v2d_block_here(a, kernel_type, grid, s);
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}

void enqueue_pack_block_records(const double *alpha, size_t ld, int count, const double *cc, int ncols_padded, double *dc, hipStream_t s) {
    if (count < 1 || count > BLOCK_VECTORS || ncols_padded % 64 != 0) throw Error(LSSVM_ERR_INTERNAL, "a block record holds 1 ... 16 vectors over whole sub-tiles");
    const size_t threads = static_cast<size_t>(ncols_padded) * BLOCK_VECTORS;
    hipLaunchKernelGGL(k_pack_ablock_f64, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, s, alpha, ld, count, cc, ncols_padded, dc);
}
#else
void launch_v2d_block_wide(const TileArgs<double> &a, int kernel_type, dim3 grid, hipStream_t s) { launch_v2d_block_here(a, kernel_type, grid, s); }
#endif

}  // namespace lssvm
