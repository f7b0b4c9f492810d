/*
 * tile_launch_f32v2w.hip -- instantiates and launches the 128-row full-square split tile kernels (lssvm_tile_f32_split.hip.hpp) with TWO weight vectors per pass
 * (NV = 2) BEYOND 128 features: the resident predictor of a one-vs-all model on 129 ... 512 features.  Compiler-scheduled groups, one workgroup per CU, as the
 * single-vector tile_matvec_f32_f3w / _s6w beyond two chunks.  f16x3 planes: the polynomial forms on 3 ... 8 chunks of 64 features, rbf with folded records on
 * 3 ... 6 (f16_max_nk64); bf16x6 planes: all four on 3 ... 6.  A translation unit of its own, so that it builds beside tile_launch_f32v2.hip, which sends wider
 * launches here.  Compiled for gfx950 only.
 */
#include "tile_launch.hip.hpp"

#include "lssvm_tile_f32_split.hip.hpp"

namespace lssvm {

template <int KT, int PL>
static void launch_nv2w_kt(const TileArgs<float> &a, dim3 grid, hipStream_t s) {
    const dim3 block(TILE_THREADS);
#define LSSVM_NV2W_CASE(N)                                                                                     \
    case N:                                                                                                    \
        if constexpr (PL == 2 && N <= f16_max_nk64(KT)) {                                                      \
            ensure_dynamic_lds(tile_matvec_f32_f3w_nv2w<KT, N>, V2_LDS_BYTES);                                 \
            hipLaunchKernelGGL((tile_matvec_f32_f3w_nv2w<KT, N>), grid, block, V2_LDS_BYTES, s, a);            \
        } else if constexpr (PL == 3 && N <= 6) {                                                              \
            ensure_dynamic_lds(tile_matvec_f32_s6w_nv2w<KT, N>, V2_LDS_BYTES);                                 \
            hipLaunchKernelGGL((tile_matvec_f32_s6w_nv2w<KT, N>), grid, block, V2_LDS_BYTES, s, a);            \
        } else {                                                                                               \
            throw Error(LSSVM_ERR_INTERNAL, "no two-vector 128-row tile kernel for this number of features");  \
        }                                                                                                      \
        break;
    switch (a.nk64) {
#ifdef LSSVM_DEV_SUBSET  // development builds (make DEV=1): 256 features only, as the single-vector units
        LSSVM_NV2W_CASE(4)
#else
        LSSVM_NV2W_CASE(3) LSSVM_NV2W_CASE(4) LSSVM_NV2W_CASE(5) LSSVM_NV2W_CASE(6) LSSVM_NV2W_CASE(7) LSSVM_NV2W_CASE(8)
#endif
        default: throw Error(LSSVM_ERR_INTERNAL, "no two-vector 128-row tile kernel for this number of features");
    }
#undef LSSVM_NV2W_CASE
}
template <int PL>
static void launch_nv2w(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s) {
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree == 3) {
                launch_nv2w_kt<KT_POLY3, PL>(a, grid, s);
            } else if (a.degree == 2) {
                launch_nv2w_kt<KT_POLY2, PL>(a, grid, s);
            } else {
                launch_nv2w_kt<KT_POLY, PL>(a, grid, s);
            }
            break;
        case KT_RBF:
            if (a.dc_folded == 0 || a.rbf_grid != 0) throw Error(LSSVM_ERR_INTERNAL, "the two-vector 128-row rbf kernel needs the folded records");
            launch_nv2w_kt<KT_RBFF, PL>(a, grid, s);
            break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no two-vector 128-row tile kernel for this kernel function");  // (the linear kernel predicts through w)
    }
}

/* reached through launch_nv2_tile_kernel (tile_launch_f32v2.hip), which has checked the variant and the second plane of the row slabs */
void launch_nv2_wide_tile_kernel(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s) {
    if (a.planes_f16 != 0) {
        launch_nv2w<2>(a, kernel_type, grid, s);
    } else {
        launch_nv2w<3>(a, kernel_type, grid, s);
    }
}

}  // namespace lssvm
