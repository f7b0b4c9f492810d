/*
 * tile_launch_f32blkx.hip -- instantiates and launches tile_matvec_f32_blk_wide (sixteen weight vectors per full-square fp32 pass on models of more than 128 padded
 * features, feature panels of 128 walked inside a tile: lssvm_tile_f32_blk_wide.hip.hpp), the resident predictor behind lssvm_mi355_predictor_create_block_panels.  The
 * polynomial forms and rbf with folded records, on f16x3 and bf16x6 planes: eight instantiations, two waves per SIMD, 80 KiB of dynamic LDS.  The records are the narrow
 * block kernel's (enqueue_pack_block_records, tile_launch_f32blk_a.hip).  Compiled for gfx950 only.
 */
#include "tile_launch.hip.hpp"

#include "lssvm_tile_f32_blk_wide.hip.hpp"

namespace lssvm {

template <int KT>
static void launch_blk32_panels_kt(const TileArgs<float> &a, dim3 grid, hipStream_t s) {
    const dim3 block(TILE_THREADS);
    if (a.planes_f16 != 0) {
        ensure_dynamic_lds(tile_matvec_f32_blk_wide<KT, 2>, B32_LDS_BYTES);
        hipLaunchKernelGGL((tile_matvec_f32_blk_wide<KT, 2>), grid, block, B32_LDS_BYTES, s, a);
    } else {
        ensure_dynamic_lds(tile_matvec_f32_blk_wide<KT, 3>, B32_LDS_BYTES);
        hipLaunchKernelGGL((tile_matvec_f32_blk_wide<KT, 3>), grid, block, B32_LDS_BYTES, s, a);
    }
}

/* reached through launch_tile_kernel<float> (TileArgs::wide_panels with nvec == BLOCK_VECTORS and no work-item list); `grid` from finish_mapping */
void launch_f32_block_panels(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s) {
    if (a.items != nullptr || a.row_pair != 0) throw Error(LSSVM_ERR_INTERNAL, "sixteen weight vectors per pass of the panel kernel: the 128-row full-square variant only");
    if (a.nk64 < 4 || a.nk64 % 2 != 0 || a.ldx16 != 64 * a.nk64) throw Error(LSSVM_ERR_INTERNAL, "the sixteen-vector panel kernel needs planes padded to a multiple of 128 features, two panels at least");
    if (a.dc == nullptr || a.Xc16 == nullptr || a.Xr16 == nullptr || a.partial == nullptr || a.part_vstride < static_cast<long>(a.num_jc) * a.part_stride || a.part_vstride % 4 != 0)
        throw Error(LSSVM_ERR_INTERNAL, "the sixteen-vector panel kernel needs its planes, its records and sixteen planes of row slabs");
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree < 0) throw Error(LSSVM_ERR_INTERNAL, "the sixteen-vector panel kernel has no pad-column rule: degree >= 0");
            if (a.degree == 3) {
                launch_blk32_panels_kt<KT_POLY3>(a, grid, s);
            } else if (a.degree == 2) {
                launch_blk32_panels_kt<KT_POLY2>(a, grid, s);
            } else {
                launch_blk32_panels_kt<KT_POLY>(a, grid, s);
            }
            break;
        case KT_RBF:
            if (a.dc_folded == 0 || a.rbf_grid != 0 || a.cr == nullptr) throw Error(LSSVM_ERR_INTERNAL, "the sixteen-vector panel rbf kernel needs the folded records and the points' norms");
            launch_blk32_panels_kt<KT_RBFF>(a, grid, s);
            break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no sixteen-vector panel kernel for this kernel function");  // (the linear kernel predicts through w)
    }
    LSSVM_HIP_CHECK(hipGetLastError());  // (a failed launch surfaces HERE, not at an unrelated later call)
}

}  // namespace lssvm
