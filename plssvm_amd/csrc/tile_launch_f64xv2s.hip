/*
 * tile_launch_f64xv2s.hip -- instantiates and launches the fp64 panel kernel (lssvm_tile_f64_wide.hip.hpp: feature panels of 64 walked inside a sub-tile) with TWO
 * vectors per pass (NV = 2), SYMMETRIC variant: a pair of right-hand sides of the lockstep CG on more than 256 features (Problem<double>::enqueue_apply_K_lanes where
 * panel_pair_applies).  rbf and the three polynomial forms: four instantiations, two workgroups per CU as their single-vector siblings.  A translation unit of its own,
 * so that tile_launch_f64x.hip and tile_launch_f64xv2.hip stay the code they were.  Compiled for gfx950 only.
 */
#include "tile_launch.hip.hpp"

#include "lssvm_tile_f64_wide.hip.hpp"

namespace lssvm {

static_assert(V2D_WIDE_LDS_BYTES_SYM_NV2 <= 64 * 1024, "the launches below do not opt into more dynamic LDS than the default limit");

/* reached through launch_tile_kernel<double> (TileArgs::wide_panels with nvec == 2 and a work-item list): one workgroup per listed item, as the single-vector launch */
void launch_nv2_sym_panel_tile_kernel_f64(const TileArgs<double> &a, int kernel_type, hipStream_t s) {
    if (a.items == nullptr) throw Error(LSSVM_ERR_INTERNAL, "two vectors per symmetric pass of the fp64 panel kernel need the work-item list");
    if (a.kchunks < 8 || a.kchunks % 4 != 0) throw Error(LSSVM_ERR_INTERNAL, "the wide fp64 tile kernel needs data padded to a multiple of 64 features");
    if (a.Xrf == nullptr || a.frag_rows16 <= 0) throw Error(LSSVM_ERR_INTERNAL, "the symmetric wide fp64 tile kernel needs the fragment-major rows");
    if (a.dvec1 == nullptr || a.part_vstride <= 0 || a.colslab_vstride <= 0) {
        throw Error(LSSVM_ERR_INTERNAL, "two vectors per symmetric pass need the second vector and the second planes of the slabs (TileArgs::dvec1, part_vstride, colslab_vstride)");
    }
    if (a.num_items <= 0) return;
    const dim3 grid(static_cast<unsigned>(a.num_items));
    const dim3 block(TILE_THREADS);
    constexpr size_t lds = V2D_WIDE_LDS_BYTES_SYM_NV2;
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree < 0) throw Error(LSSVM_ERR_INTERNAL, "the wide fp64 tile kernel does not take a negative polynomial degree");
            if (a.degree == 3) {
                hipLaunchKernelGGL((tile_matvec_f64_wide<KT_POLY3, true, 2>), grid, block, lds, s, a);
            } else if (a.degree == 2) {
                hipLaunchKernelGGL((tile_matvec_f64_wide<KT_POLY2, true, 2>), grid, block, lds, s, a);
            } else {
                hipLaunchKernelGGL((tile_matvec_f64_wide<KT_POLY, true, 2>), grid, block, lds, s, a);
            }
            break;
        case KT_RBF: hipLaunchKernelGGL((tile_matvec_f64_wide<KT_RBF, true, 2>), grid, block, lds, s, a); break;
        default: throw Error(LSSVM_ERR_INTERNAL, "the wide fp64 tile kernel exists for the rbf and polynomial kernels");
    }
    LSSVM_HIP_CHECK(hipGetLastError());  // (a failed launch surfaces HERE, not at an unrelated later call)
}

}  // namespace lssvm
