/*
 * tile_launch_f32v2.hip -- instantiates and launches the 128-row full-square split tile kernels (lssvm_tile_f32_split.hip.hpp) with TWO weight vectors per pass
 * (NV = 2: the resident predictor of a one-vs-all model on batches below the rectangular 256-row kernel's 64 row blocks).  Both plane kinds (f16x3, bf16x6), one and
 * two 64-feature chunks (more: tile_launch_f32v2w.hip, reached through the entry point below); the polynomial forms and rbf with folded records -- the forms whose kernel leaves the second half of the column record free for the second
 * vector.  A translation unit of its own, so that it builds beside the single-vector instantiations.  Compiled for gfx950 only.
 */
#include "tile_launch.hip.hpp"

#include "lssvm_tile_f32_split.hip.hpp"

namespace lssvm {

/* <= 128 features: the hand-scheduled groups; the run-time integer power stays on the compiler-scheduled groups, as with one vector (tile_launch_f32h.hip) */
template <int KT, int N, int PL>
static void launch_nv2_one(const TileArgs<float> &a, dim3 grid, hipStream_t s) {
    const dim3 block(TILE_THREADS);
    if constexpr (PL == 2) {
        if constexpr (KT != KT_POLY) {
            ensure_dynamic_lds(tile_matvec_f32_f3h_nv2<KT, N>, V2_LDS_BYTES);
            hipLaunchKernelGGL((tile_matvec_f32_f3h_nv2<KT, N>), grid, block, V2_LDS_BYTES, s, a);
        } else {
            ensure_dynamic_lds(tile_matvec_f32_f3w_nv2<KT, N>, V2_LDS_BYTES);
            hipLaunchKernelGGL((tile_matvec_f32_f3w_nv2<KT, N>), grid, block, V2_LDS_BYTES, s, a);
        }
    } else {
        if constexpr (KT != KT_POLY) {
            ensure_dynamic_lds(tile_matvec_f32_s6h_nv2<KT, N>, V2_LDS_BYTES);
            hipLaunchKernelGGL((tile_matvec_f32_s6h_nv2<KT, N>), grid, block, V2_LDS_BYTES, s, a);
        } else {
            ensure_dynamic_lds(tile_matvec_f32_s6w_nv2<KT, N>, V2_LDS_BYTES);
            hipLaunchKernelGGL((tile_matvec_f32_s6w_nv2<KT, N>), grid, block, V2_LDS_BYTES, s, a);
        }
    }
}
template <int KT, int PL>
static void launch_nv2_kt(const TileArgs<float> &a, dim3 grid, hipStream_t s) {
    switch (a.nk64) {
#ifndef LSSVM_DEV_SUBSET
        case 1: launch_nv2_one<KT, 1, PL>(a, grid, s); break;
#endif
        case 2: launch_nv2_one<KT, 2, PL>(a, grid, s); break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no two-vector 128-row tile kernel for this number of features");
    }
}
template <int PL>
static void launch_nv2(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s) {
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree == 3) {
                launch_nv2_kt<KT_POLY3, PL>(a, grid, s);
            } else if (a.degree == 2) {
                launch_nv2_kt<KT_POLY2, PL>(a, grid, s);
            } else {
                launch_nv2_kt<KT_POLY, PL>(a, grid, s);
            }
            break;
        case KT_RBF:
            if (a.dc_folded == 0 || a.rbf_grid != 0) throw Error(LSSVM_ERR_INTERNAL, "the two-vector 128-row rbf kernel needs the folded records");
            launch_nv2_kt<KT_RBFF, PL>(a, grid, s);
            break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no two-vector 128-row tile kernel for this kernel function");  // (the linear kernel predicts through w)
    }
}

void launch_nv2_tile_kernel(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s) {
    if (a.items != nullptr) throw Error(LSSVM_ERR_INTERNAL, "two weight vectors per pass: the full-square variant only");
    if (a.part_vstride <= 0) throw Error(LSSVM_ERR_INTERNAL, "two weight vectors per pass need the second plane of the row slabs (TileArgs::part_vstride)");
    if (a.nk64 > 2) {  // beyond 128 features: the one-workgroup-per-CU instantiations of tile_launch_f32v2w.hip
        launch_nv2_wide_tile_kernel(a, kernel_type, grid, s);
    } else if (a.planes_f16 != 0) {
        launch_nv2<2>(a, kernel_type, grid, s);
    } else {
        launch_nv2<3>(a, kernel_type, grid, s);
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}

}  // namespace lssvm
