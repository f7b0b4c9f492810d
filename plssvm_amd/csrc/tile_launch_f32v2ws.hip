/*
 * tile_launch_f32v2ws.hip -- instantiates and launches the 128-row SYMMETRIC split tile kernels (lssvm_tile_f32_split.hip.hpp) with TWO vectors per pass (NV = 2)
 * beyond 128 features: a pair of right-hand sides of the lockstep CG on 129 ... 512 features (Problem<float>::enqueue_apply_K_lanes).  Compiler-scheduled groups, one
 * workgroup per CU, as the single-vector tile_matvec_f32_f3w / _s6w<KT, NK64, SYM = true> beyond two chunks.  f16x3 planes: the polynomial forms on 3 ... 8 chunks of
 * 64 features, rbf with folded records on 3 ... 6 (f16_max_nk64); bf16x6 planes: all four on 3 ... 6.  Compiled for gfx950 only.
 */
#include "tile_launch.hip.hpp"

#include "lssvm_tile_f32_split.hip.hpp"

/* compiled as TWO translation units, one per plane kind, so that neither builds longer than the single-vector units beside it: tile_launch_f32v2ws_f16.hip
 * (LSSVM_TU_HALF 1: the 22 f16x3 instantiations) and tile_launch_f32v2ws_bf16.hip (LSSVM_TU_HALF 2: the 16 bf16x6 ones and the entry point) */
#ifndef LSSVM_TU_HALF
#error "compile tile_launch_f32v2ws_f16.hip / tile_launch_f32v2ws_bf16.hip"
#endif

namespace lssvm {

template <int KT, int PL>
static void launch_nv2ws_kt(const TileArgs<float> &a, dim3 grid, hipStream_t s) {
    const dim3 block(TILE_THREADS);
#define LSSVM_NV2WS_CASE(N)                                                                                              \
    case N:                                                                                                              \
        if constexpr (PL == 2 && N <= f16_max_nk64(KT)) {                                                                \
            ensure_dynamic_lds(tile_matvec_f32_f3w_nv2s<KT, N>, V2S_LDS_BYTES);                                          \
            hipLaunchKernelGGL((tile_matvec_f32_f3w_nv2s<KT, N>), grid, block, V2S_LDS_BYTES, s, a);                     \
        } else if constexpr (PL == 3 && N <= 6) {                                                                        \
            ensure_dynamic_lds(tile_matvec_f32_s6w_nv2s<KT, N>, V2S_LDS_BYTES);                                          \
            hipLaunchKernelGGL((tile_matvec_f32_s6w_nv2s<KT, N>), grid, block, V2S_LDS_BYTES, s, a);                     \
        } else {                                                                                                         \
            throw Error(LSSVM_ERR_INTERNAL, "no two-vector symmetric 128-row tile kernel for this number of features");  \
        }                                                                                                                \
        break;
    switch (a.nk64) {
#ifdef LSSVM_DEV_SUBSET  // development builds (make DEV=1): 256 features only, as the single-vector units
        LSSVM_NV2WS_CASE(4)
#else
        LSSVM_NV2WS_CASE(3) LSSVM_NV2WS_CASE(4) LSSVM_NV2WS_CASE(5) LSSVM_NV2WS_CASE(6) LSSVM_NV2WS_CASE(7) LSSVM_NV2WS_CASE(8)
#endif
        default: throw Error(LSSVM_ERR_INTERNAL, "no two-vector symmetric 128-row tile kernel for this number of features");
    }
#undef LSSVM_NV2WS_CASE
}
template <int PL>
static void launch_nv2ws(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s) {
    switch (kernel_type) {
        case KT_POLY:
            if (a.degree == 3) {
                launch_nv2ws_kt<KT_POLY3, PL>(a, grid, s);
            } else if (a.degree == 2) {
                launch_nv2ws_kt<KT_POLY2, PL>(a, grid, s);
            } else {
                launch_nv2ws_kt<KT_POLY, PL>(a, grid, s);
            }
            break;
        case KT_RBF:
            if (a.dc_folded == 0 || a.rbf_grid != 0) throw Error(LSSVM_ERR_INTERNAL, "the two-vector symmetric 128-row rbf kernel needs the folded records");
            launch_nv2ws_kt<KT_RBFF, PL>(a, grid, s);
            break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no two-vector symmetric 128-row tile kernel for this kernel function");
    }
}

void launch_nv2ws_f16(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s);  // tile_launch_f32v2ws_f16.hip

#if LSSVM_TU_HALF == 1
void launch_nv2ws_f16(const TileArgs<float> &a, int kernel_type, dim3 grid, hipStream_t s) {
    launch_nv2ws<2>(a, kernel_type, grid, s);
}
#else
/* reached through launch_tile_kernel<float> (TileArgs::nvec == 2 with a work-item list): one workgroup per listed item, as the single-vector symmetric launch */
void launch_nv2_sym_wide_tile_kernel(const TileArgs<float> &a, int kernel_type, hipStream_t s) {
    if (a.items == nullptr || a.row_pair != 0 || a.wide_panels != 0) throw Error(LSSVM_ERR_INTERNAL, "two vectors per symmetric pass: the 128-row one-pass split kernels only");
    if (a.dvec1 == nullptr || a.part_vstride <= 0 || a.colslab_vstride <= 0) {
        throw Error(LSSVM_ERR_INTERNAL, "two vectors per symmetric pass need the second vector and the second planes of the slabs (TileArgs::dvec1, part_vstride, colslab_vstride)");
    }
    const dim3 grid(static_cast<unsigned>(a.num_items));
    if (a.planes_f16 != 0) {
        launch_nv2ws_f16(a, kernel_type, grid, s);
    } else {
        launch_nv2ws<3>(a, kernel_type, grid, s);
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}
#endif

}  // namespace lssvm
