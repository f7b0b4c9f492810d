/*
 * tile_launch_f32blks.hip -- instantiates and launches tile_matvec_f32_blk_sym (sixteen vectors per SYMMETRIC fp32 pass: lssvm_tile_f32_blk_sym.hip.hpp) and packs
 * its records.  Compiled for gfx950 only, as TWO translation units (tile_launch_f32blks_a.hip: LSSVM_TU_HALF 1 = the f16x3 planes, the entry points and the packing
 * kernel; tile_launch_f32blks_b.hip: LSSVM_TU_HALF 2 = the bf16x6 planes), eight instantiations each, so that the build spreads over more cores.
 */
#ifndef LSSVM_TU_HALF
#error "compile tile_launch_f32blks_a.hip / _b.hip"
#endif
#if LSSVM_TU_HALF == 1
#define LSSVM_KERNELS_BLOCK_SYM_PACK
#endif

#include "tile_launch.hip.hpp"

#include "lssvm_tile_f32_blk_sym.hip.hpp"

namespace lssvm {

constexpr int B32S_PL = LSSVM_TU_HALF == 1 ? 2 : 3;  // the plane kind this unit holds

/* 153 KiB of dynamic LDS: opted into per kernel and device */
template <int KT, int NK64>
static void launch_blks32(const TileArgs<float> &a, dim3 grid, hipStream_t s) {
    ensure_dynamic_lds(tile_matvec_f32_blk_sym<KT, NK64, B32S_PL>, B32S_LDS_BYTES);
    hipLaunchKernelGGL((tile_matvec_f32_blk_sym<KT, NK64, B32S_PL>), grid, dim3(TILE_THREADS), B32S_LDS_BYTES, s, a);
}

template <int KT>
static void launch_blks32_kt(const TileArgs<float> &a, dim3 grid, hipStream_t s) {
    switch (a.nk64) {
        case 1: launch_blks32<KT, 1>(a, grid, s); break;
        case 2: launch_blks32<KT, 2>(a, grid, s); break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no sixteen-vector symmetric fp32 tile kernel for this number of features");
    }
}

static void launch_f32_block_sym_here(const TileArgs<float> &a, int kernel_type, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(a.num_items));
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree == 3) {
                launch_blks32_kt<KT_POLY3>(a, grid, s);
            } else if (a.degree == 2) {
                launch_blks32_kt<KT_POLY2>(a, grid, s);
            } else {
                launch_blks32_kt<KT_POLY>(a, grid, s);
            }
            break;
        case KT_RBF: launch_blks32_kt<KT_RBFF>(a, grid, s); break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no sixteen-vector symmetric fp32 tile kernel for this kernel function");
    }
}

void launch_f32_block_sym_bf16(const TileArgs<float> &a, int kernel_type, hipStream_t s);  // tile_launch_f32blks_b.hip: the bf16x6 planes
#if LSSVM_TU_HALF == 1
void launch_f32_block_sym(const TileArgs<float> &a, int kernel_type, hipStream_t s) {
    if (a.items == nullptr || a.num_items <= 0 || a.queue != nullptr || a.jc_head_count != 0 || a.wide_panels != 0)
        throw Error(LSSVM_ERR_INTERNAL, "sixteen vectors per symmetric fp32 pass: a list of 128-row work items over uniform column chunks");
    if (a.dc == nullptr || a.dvec == nullptr || a.Xc16 == nullptr || a.Xr16 == nullptr || a.partial == nullptr || a.colslab == nullptr || a.part_vstride < static_cast<long>(a.num_jc) * a.part_stride
        || a.part_vstride % 4 != 0 || a.colslab_vstride <= 0)
        throw Error(LSSVM_ERR_INTERNAL, "the sixteen-vector symmetric kernel needs its planes, its records, the plain vectors and sixteen planes of both slabs");
    if ((kernel_type == KT_POLY && a.degree < 0) || (kernel_type == KT_RBF && (a.dc_folded == 0 || a.rbf_grid != 0)))
        throw Error(LSSVM_ERR_INTERNAL, "the sixteen-vector symmetric fp32 kernel: a non-negative degree, or rbf with the folded records");
    if (a.planes_f16 != 0) {
        launch_f32_block_sym_here(a, kernel_type, s);
    } else {
        launch_f32_block_sym_bf16(a, kernel_type, s);
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}

void enqueue_pack_block_sym_records_f32(const float *const *v, float *const *Kv, int count, const float *cc, int folded, int ncols_padded, float *dc, float *vp, int nzero, hipStream_t s) {
    if (count < 1 || count > BLOCK_VECTORS || ncols_padded % TILE != 0) throw Error(LSSVM_ERR_INTERNAL, "a block record holds 1 ... 16 vectors over whole tiles");
    BlockVectors32 bv{};
    for (int u = 0; u < count; ++u) {
        bv.v[u] = v[u];
        bv.Kv[u] = Kv[u];
    }
    const size_t threads = static_cast<size_t>(std::max(ncols_padded, nzero)) * BLOCK_VECTORS;
    hipLaunchKernelGGL(k_pack_vblock_f32_sym, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, s, bv, count, cc, folded, ncols_padded, dc, vp, nzero);
}
#else
void launch_f32_block_sym_bf16(const TileArgs<float> &a, int kernel_type, hipStream_t s) { launch_f32_block_sym_here(a, kernel_type, s); }
#endif

}  // namespace lssvm
