/*
 * tile_launch_f64blks.hip -- instantiates and launches tile_matvec_f64_blk_sym (sixteen vectors per SYMMETRIC fp64 pass: lssvm_tile_f64_blk_sym.hip.hpp) and packs
 * its records.  Compiled for gfx950 only, as TWO translation units (tile_launch_f64blks_a.hip: LSSVM_TU_HALF 1 = 1 ... 6 chunks, the entry points and the packing
 * kernel; tile_launch_f64blks_b.hip: LSSVM_TU_HALF 2 = 7 ... 16 chunks), so that the build spreads over more cores.
 */
#ifndef LSSVM_TU_HALF
#error "compile tile_launch_f64blks_a.hip / _b.hip"
#endif
#if LSSVM_TU_HALF == 1
#define LSSVM_KERNELS_BLOCK_SYM_PACK
#endif

#include "tile_launch.hip.hpp"

#include "lssvm_tile_f64_blk_sym.hip.hpp"

namespace lssvm {

/* 147 KiB of dynamic LDS: opted into per kernel and device */
template <int KT, int NKC>
static void launch_blks(const TileArgs<double> &a, dim3 grid, hipStream_t s) {
    ensure_dynamic_lds(tile_matvec_f64_blk_sym<KT, NKC>, V2BS_LDS_BYTES);
    hipLaunchKernelGGL((tile_matvec_f64_blk_sym<KT, NKC>), grid, dim3(TILE_THREADS), V2BS_LDS_BYTES, s, a);
}

template <int KT>
static void launch_blks_kt(const TileArgs<double> &a, dim3 grid, hipStream_t s) {
    switch (a.kchunks) {
#if LSSVM_TU_HALF == 1
        case 1: launch_blks<KT, 1>(a, grid, s); break;
        case 2: launch_blks<KT, 2>(a, grid, s); break;
        case 3: launch_blks<KT, 3>(a, grid, s); break;
        case 4: launch_blks<KT, 4>(a, grid, s); break;
        case 5: launch_blks<KT, 5>(a, grid, s); break;
        case 6: launch_blks<KT, 6>(a, grid, s); break;
#else
        case 7: launch_blks<KT, 7>(a, grid, s); break;
        case 8: launch_blks<KT, 8>(a, grid, s); break;
        case 10: launch_blks<KT, 10>(a, grid, s); break;
        case 12: launch_blks<KT, 12>(a, grid, s); break;
        case 14: launch_blks<KT, 14>(a, grid, s); break;
        case 16: launch_blks<KT, 16>(a, grid, s); break;
#endif
        default: throw Error(LSSVM_ERR_INTERNAL, "no sixteen-vector symmetric fp64 tile kernel for this number of k-chunks");
    }
}

static void launch_v2d_block_sym_here(const TileArgs<double> &a, int kernel_type, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(a.num_items));
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree == 3) {
                launch_blks_kt<KT_POLY3>(a, grid, s);
            } else if (a.degree == 2) {
                launch_blks_kt<KT_POLY2>(a, grid, s);
            } else {
                launch_blks_kt<KT_POLY>(a, grid, s);
            }
            break;
        case KT_RBF: launch_blks_kt<KT_RBF>(a, grid, s); break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no sixteen-vector symmetric fp64 tile kernel for this kernel function");
    }
}

void launch_v2d_block_sym_wide(const TileArgs<double> &a, int kernel_type, hipStream_t s);  // tile_launch_f64blks_b.hip: 7 ... 16 chunks
#if LSSVM_TU_HALF == 1
void launch_v2d_block_sym(const TileArgs<double> &a, int kernel_type, hipStream_t s) {
    if (a.items == nullptr || a.num_items <= 0 || a.dc == nullptr || a.partial == nullptr || a.colslab == nullptr || a.part_vstride < static_cast<long>(a.num_jc) * a.part_stride || a.colslab_vstride <= 0
        || (kernel_type == KT_POLY && a.degree < 0)) {
        throw Error(LSSVM_ERR_INTERNAL, "the sixteen-vector symmetric kernel needs its work items, its records, sixteen planes of both slabs and a non-negative degree");
    }
    if (a.kchunks > 6) {
        launch_v2d_block_sym_wide(a, kernel_type, s);
    } else {
        launch_v2d_block_sym_here(a, kernel_type, s);
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}

void enqueue_pack_block_sym_records(const double *const *v, double *const *Kv, int count, const double *cc, int ncols_padded, double *dc, int nzero, hipStream_t s) {
    if (count < 1 || count > BLOCK_VECTORS || ncols_padded % 64 != 0) throw Error(LSSVM_ERR_INTERNAL, "a block record holds 1 ... 16 vectors over whole sub-tiles");
    BlockVectors bv{};
    for (int u = 0; u < count; ++u) {
        bv.v[u] = v[u];
        bv.Kv[u] = Kv[u];
    }
    const size_t threads = static_cast<size_t>(std::max(ncols_padded, nzero)) * BLOCK_VECTORS;
    hipLaunchKernelGGL(k_pack_vblock_f64, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, s, bv, count, cc, ncols_padded, dc, nzero);
}
#else
void launch_v2d_block_sym_wide(const TileArgs<double> &a, int kernel_type, hipStream_t s) { launch_v2d_block_sym_here(a, kernel_type, s); }
#endif

}  // namespace lssvm
