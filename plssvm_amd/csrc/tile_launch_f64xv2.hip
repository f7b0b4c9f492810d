/*
 * tile_launch_f64xv2.hip -- instantiates and launches the fp64 panel kernel (lssvm_tile_f64_wide.hip.hpp: feature panels of 64 walked inside a sub-tile) with TWO weight
 * vectors per pass (NV = 2), full-square variant: the resident predictor of a one-vs-all model on more than 256 features (lssvm_mi355_predictor_create_panels).  rbf and
 * the three polynomial forms: four instantiations, two workgroups per CU as their single-vector siblings.  A translation unit of its own, so that tile_launch_f64x.hip
 * stays the code it was.  Compiled for gfx950 only.
 */
#include "tile_launch.hip.hpp"

#include "lssvm_tile_f64_wide.hip.hpp"

namespace lssvm {

static_assert(V2D_LDS_BYTES_NV2 <= 64 * 1024, "the launches below do not opt into more dynamic LDS than the default limit");

/* reached through launch_tile_kernel<double> (TileArgs::wide_panels with nvec == 2 and no work-item list); `grid` from finish_mapping */
void launch_nv2_panel_tile_kernel_f64(const TileArgs<double> &a, int kernel_type, dim3 grid, hipStream_t s) {
    if (a.items != nullptr) throw Error(LSSVM_ERR_INTERNAL, "two vectors per pass of the fp64 panel kernel: the full-square variant only");
    if (a.kchunks < 8 || a.kchunks % 4 != 0) throw Error(LSSVM_ERR_INTERNAL, "the wide fp64 tile kernel needs data padded to a multiple of 64 features");
    if (a.part_vstride <= 0) throw Error(LSSVM_ERR_INTERNAL, "two vectors per pass need the second plane of the row slabs (TileArgs::part_vstride)");
    const dim3 block(TILE_THREADS);
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree < 0) throw Error(LSSVM_ERR_INTERNAL, "the wide fp64 tile kernel does not take a negative polynomial degree");
            if (a.degree == 3) {
                hipLaunchKernelGGL((tile_matvec_f64_wide<KT_POLY3, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a);
            } else if (a.degree == 2) {
                hipLaunchKernelGGL((tile_matvec_f64_wide<KT_POLY2, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a);
            } else {
                hipLaunchKernelGGL((tile_matvec_f64_wide<KT_POLY, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a);
            }
            break;
        case KT_RBF: hipLaunchKernelGGL((tile_matvec_f64_wide<KT_RBF, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        default: throw Error(LSSVM_ERR_INTERNAL, "the wide fp64 tile kernel exists for the rbf and polynomial kernels");
    }
    LSSVM_HIP_CHECK(hipGetLastError());  // (a failed launch surfaces HERE, not at an unrelated later call)
}

}  // namespace lssvm
