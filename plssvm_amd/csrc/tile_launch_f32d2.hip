/*
 * tile_launch_f32d2.hip -- instantiates and launches the RECTANGULAR 256-row kernel (lssvm_tile_f32_pair.hip.hpp, RECT) with TWO weight vectors per pass
 * (NV = 2: predict_values_multi, a one-vs-all model's classifiers over the same support vectors).  A translation unit of its own beside
 * tile_launch_f32d.hip, so that the two sets of instantiations build in parallel.  Compiled for gfx950 only.
 */
#include "tile_launch.hip.hpp"

#include "lssvm_tile_f32_pair.hip.hpp"

namespace lssvm {

template <int KT, int PL>
static void launch_rect2_kt(const TileArgs<float> &a, hipStream_t s) {
    const dim3 grid = sym_grid(a, 1), block(PR_THREADS);
    switch (a.nk64) {
#ifndef LSSVM_DEV_SUBSET
        case 1:
            ensure_dynamic_lds(tile_matvec_f32_pair_rect<KT, 1, PL, 2>, PR_LDS_BYTES);
            hipLaunchKernelGGL((tile_matvec_f32_pair_rect<KT, 1, PL, 2>), grid, block, PR_LDS_BYTES, s, a);
            break;
#endif
        case 2:
            ensure_dynamic_lds(tile_matvec_f32_pair_rect<KT, 2, PL, 2>, PR_LDS_BYTES);
            hipLaunchKernelGGL((tile_matvec_f32_pair_rect<KT, 2, PL, 2>), grid, block, PR_LDS_BYTES, s, a);
            break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no rectangular 256-row tile kernel for this number of features");
    }
}
template <int PL>
static void launch_rect2(const TileArgs<float> &a, int kernel_type, hipStream_t s) {
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree == 3) {
                launch_rect2_kt<KT_POLY3, PL>(a, s);
            } else if (a.degree == 2) {
                launch_rect2_kt<KT_POLY2, PL>(a, s);
            } else {
                throw Error(LSSVM_ERR_INTERNAL, "no rectangular 256-row tile kernel for the run-time integer power");
            }
            break;
        case KT_RBF:
            if (a.dc_folded == 0) throw Error(LSSVM_ERR_INTERNAL, "the rectangular 256-row rbf kernel needs the folded records");
            launch_rect2_kt<KT_RBFF, PL>(a, s);
            break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no rectangular 256-row tile kernel for this kernel function");  // (the linear kernel predicts through w)
    }
}

void launch_rect2_tile_kernel(const TileArgs<float> &a, int kernel_type, hipStream_t s) {
    if (a.part_vstride <= 0) throw Error(LSSVM_ERR_INTERNAL, "two weight vectors per pass need the second plane of the row slabs (TileArgs::part_vstride)");
    if (a.planes_f16 != 0) {
        launch_rect2<2>(a, kernel_type, s);
    } else {
#ifdef LSSVM_DEV_SUBSET
        throw Error(LSSVM_ERR_INTERNAL, "development build: 256-row kernels for the f16 planes only");
#else
        launch_rect2<3>(a, kernel_type, s);
#endif
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}

}  // namespace lssvm
