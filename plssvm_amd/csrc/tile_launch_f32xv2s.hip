/*
 * tile_launch_f32xv2s.hip -- instantiates and launches the fp32 panel kernel (lssvm_tile_f32_wide.hip.hpp: feature panels of 128 walked inside a tile) with TWO vectors
 * per pass (NV = 2), SYMMETRIC variant: a pair of right-hand sides of the lockstep CG beyond the one-pass split kernels (Problem<float>::enqueue_apply_K_lanes where
 * panel_pair_applies).  The polynomial forms and rbf with folded records, on f16x3 and bf16x6 planes: eight instantiations.  A translation unit of its own, so that
 * tile_launch_f32x.hip and tile_launch_f32xv2.hip stay the code they were.  Compiled for gfx950 only.
 */
#include "tile_launch.hip.hpp"

#include "lssvm_tile_f32_wide.hip.hpp"

namespace lssvm {

template <int KT>
static void launch_nv2s_panel_kt(const TileArgs<float> &a, dim3 grid, hipStream_t s) {
    const dim3 block(TILE_THREADS);
    const size_t lds = lssvm::V2S_LDS_BYTES;  // (record slots of 1.5 KiB, two planes of dis and of colred)
    if (a.planes_f16 != 0) {
        ensure_dynamic_lds(tile_matvec_f32_wide_nv2s<KT, 2>, lds);
        hipLaunchKernelGGL((tile_matvec_f32_wide_nv2s<KT, 2>), grid, block, lds, s, a);
    } else {
        ensure_dynamic_lds(tile_matvec_f32_wide_nv2s<KT, 3>, lds);
        hipLaunchKernelGGL((tile_matvec_f32_wide_nv2s<KT, 3>), grid, block, lds, s, a);
    }
}

/* reached through launch_tile_kernel<float> (TileArgs::wide_panels with nvec == 2 and a work-item list): one workgroup per listed item, as the single-vector launch */
void launch_nv2_sym_panel_tile_kernel(const TileArgs<float> &a, int kernel_type, hipStream_t s) {
    if (a.items == nullptr || a.row_pair != 0) throw Error(LSSVM_ERR_INTERNAL, "two vectors per symmetric pass of the panel kernel need the work-item list of the 128-row kernels");
    if (a.nk64 < 4 || a.nk64 % 2 != 0) throw Error(LSSVM_ERR_INTERNAL, "the wide split tile kernel needs planes padded to a multiple of 128 features");
    if (a.Xr16f == nullptr) throw Error(LSSVM_ERR_INTERNAL, "the symmetric wide split tile kernel needs the fragment-major row planes");
    if (a.dvec1 == nullptr || a.part_vstride <= 0 || a.colslab_vstride <= 0) {
        throw Error(LSSVM_ERR_INTERNAL, "two vectors per symmetric pass need the second vector and the second planes of the slabs (TileArgs::dvec1, part_vstride, colslab_vstride)");
    }
    if (a.num_items <= 0) return;
    const dim3 grid(static_cast<unsigned>(a.num_items));
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree < 0) throw Error(LSSVM_ERR_INTERNAL, "the wide split tile kernel does not take a negative polynomial degree");
            if (a.degree == 3) {
                launch_nv2s_panel_kt<KT_POLY3>(a, grid, s);
            } else if (a.degree == 2) {
                launch_nv2s_panel_kt<KT_POLY2>(a, grid, s);
            } else {
                launch_nv2s_panel_kt<KT_POLY>(a, grid, s);
            }
            break;
        case KT_RBF:
            if (a.dc_folded == 0 || a.rbf_grid != 0) throw Error(LSSVM_ERR_INTERNAL, "the two-vector symmetric panel rbf kernel needs the folded records");
            launch_nv2s_panel_kt<KT_RBFF>(a, grid, s);
            break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no two-vector symmetric panel kernel for this kernel function");
    }
    LSSVM_HIP_CHECK(hipGetLastError());  // (a failed launch surfaces HERE, not at an unrelated later call)
}

}  // namespace lssvm
