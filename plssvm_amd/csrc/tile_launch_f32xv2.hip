/*
 * tile_launch_f32xv2.hip -- instantiates and launches the fp32 panel kernel (lssvm_tile_f32_wide.hip.hpp: feature panels of 128 walked inside a tile) with TWO weight
 * vectors per pass (NV = 2), full-square variant: the resident predictor of a one-vs-all model beyond the one-pass split kernels (lssvm_mi355_predictor_create_panels).
 * The polynomial forms and rbf with folded records, on f16x3 and bf16x6 planes: eight instantiations, two waves per SIMD as their single-vector siblings.  A translation
 * unit of its own, so that tile_launch_f32x.hip stays the code it was.  Compiled for gfx950 only.
 */
#include "tile_launch.hip.hpp"

#include "lssvm_tile_f32_wide.hip.hpp"

namespace lssvm {

template <int KT>
static void launch_nv2_panel_kt(const TileArgs<float> &a, dim3 grid, hipStream_t s) {
    const dim3 block(TILE_THREADS);
    const size_t lds = lssvm::V2_LDS_BYTES;  // (the record (d0_j | d1_j) is the 1 KiB of (d_j | c_j))
    if (a.planes_f16 != 0) {
        ensure_dynamic_lds(tile_matvec_f32_wide_nv2<KT, 2>, lds);
        hipLaunchKernelGGL((tile_matvec_f32_wide_nv2<KT, 2>), grid, block, lds, s, a);
    } else {
        ensure_dynamic_lds(tile_matvec_f32_wide_nv2<KT, 3>, lds);
        hipLaunchKernelGGL((tile_matvec_f32_wide_nv2<KT, 3>), grid, block, lds, s, a);
    }
}

/* reached through launch_tile_kernel<float> (TileArgs::wide_panels with nvec == 2 and no work-item list); `grid` from finish_mapping */
void launch_nv2_panel_tile_kernel(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s) {
    if (a.items != nullptr || a.row_pair != 0) throw Error(LSSVM_ERR_INTERNAL, "two vectors per pass of the panel kernel: the full-square variant only");
    if (a.nk64 < 4 || a.nk64 % 2 != 0) throw Error(LSSVM_ERR_INTERNAL, "the wide split tile kernel needs planes padded to a multiple of 128 features");
    if (a.part_vstride <= 0) throw Error(LSSVM_ERR_INTERNAL, "two vectors per pass need the second plane of the row slabs (TileArgs::part_vstride)");
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree < 0) throw Error(LSSVM_ERR_INTERNAL, "the wide split tile kernel does not take a negative polynomial degree");
            if (a.degree == 3) {
                launch_nv2_panel_kt<KT_POLY3>(a, grid, s);
            } else if (a.degree == 2) {
                launch_nv2_panel_kt<KT_POLY2>(a, grid, s);
            } else {
                launch_nv2_panel_kt<KT_POLY>(a, grid, s);
            }
            break;
        case KT_RBF:
            if (a.dc_folded == 0 || a.rbf_grid != 0) throw Error(LSSVM_ERR_INTERNAL, "the two-vector panel rbf kernel needs the folded records");
            launch_nv2_panel_kt<KT_RBFF>(a, grid, s);
            break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no two-vector panel kernel for this kernel function");  // (the linear kernel predicts through w)
    }
    LSSVM_HIP_CHECK(hipGetLastError());  // (a failed launch surfaces HERE, not at an unrelated later call)
}

}  // namespace lssvm
