/*
 * tile_launch_f64.hip -- instantiates and launches the fp64 tile kernels (launch_tile_kernel<double>, declared in
 * lssvm_problem.hip.hpp).  Compiled for gfx950 only.
 */
#include "tile_launch.hip.hpp"

#include "lssvm_tile_f64.hip.hpp"

/* This source is compiled as SIX translation units (tile_launch_f64_sym.hip: LSSVM_TU_HALF 1 = the symmetric instantiations, tile_launch_f64_full.hip:
 * LSSVM_TU_HALF 2 = the full-square ones, the generic kernel and the entry point, tile_launch_f64_sym2a.hip / _sym2b.hip: LSSVM_TU_HALF 3 / 4 = the symmetric
 * instantiations with two vectors per pass for 1 ... 6 / 7 ... 16 chunks, tile_launch_f64_full2a.hip / _full2b.hip: LSSVM_TU_HALF 5 / 6 = the full-square
 * instantiations with two vectors per pass, split alike), so that the build spreads over more cores. */
#ifndef LSSVM_TU_HALF
#error "compile tile_launch_f64_sym.hip / _full.hip / _sym2a.hip / _sym2b.hip / _full2a.hip / _full2b.hip"
#endif

namespace lssvm {

template <int KT, bool SYM>
static void launch_v2d_kt(const TileArgs<double> &a, dim3 grid, hipStream_t s) {
    const dim3 block(TILE_THREADS);
    switch (a.kchunks) {
        case 1: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 1, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        case 2: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 2, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        case 3: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 3, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        case 4: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 4, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        case 5: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 5, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        case 6: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 6, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        case 7: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 7, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        case 8: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 8, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        case 10: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 10, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        case 12: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 12, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        case 14: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 14, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        case 16: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 16, SYM>), grid, block, V2D_LDS_BYTES, s, a); break;
        default: throw Error(LSSVM_ERR_INTERNAL, "no v2 tile kernel for this number of k-chunks");
    }
}

void launch_v2d_sym(const TileArgs<double> &a, int kernel_type, hipStream_t s);  // tile_launch_f64_sym.hip

#if LSSVM_TU_HALF == 3 || LSSVM_TU_HALF == 4
/* two vectors per pass (TileArgs::nvec == 2): every kernel function and chunk count the single-vector kernel has; V2D_LDS_BYTES_NV2 < 64 KiB */
template <int KT>
static void launch_v2d_kt2(const TileArgs<double> &a, dim3 grid, hipStream_t s) {
    const dim3 block(TILE_THREADS);
    switch (a.kchunks) {
#if LSSVM_TU_HALF == 3
        case 1: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 1, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 2: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 2, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 3: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 3, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 4: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 4, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 5: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 5, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 6: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 6, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
#else
        case 7: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 7, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 8: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 8, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 10: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 10, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 12: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 12, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 14: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 14, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 16: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 16, true, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
#endif
        default: throw Error(LSSVM_ERR_INTERNAL, "no two-vector v2 tile kernel for this number of k-chunks");
    }
}
static void launch_v2d_sym2_here(const TileArgs<double> &a, int kernel_type, hipStream_t s) {
    const dim3 sgrid(static_cast<unsigned>(a.num_items));
    switch (kernel_type) {
        case KT_LINEAR: launch_v2d_kt2<KT_LINEAR>(a, sgrid, s); break;
        case KT_POLY:
            if (a.degree == 3) {
                launch_v2d_kt2<KT_POLY3>(a, sgrid, s);
            } else if (a.degree == 2) {
                launch_v2d_kt2<KT_POLY2>(a, sgrid, s);
            } else {
                launch_v2d_kt2<KT_POLY>(a, sgrid, s);
            }
            break;
        default: launch_v2d_kt2<KT_RBF>(a, sgrid, s); break;
    }
}
void launch_v2d_sym2_wide(const TileArgs<double> &a, int kernel_type, hipStream_t s);  // tile_launch_f64_sym2b.hip: 7 ... 16 chunks
#if LSSVM_TU_HALF == 3
void launch_v2d_sym2(const TileArgs<double> &a, int kernel_type, hipStream_t s) {
    if (a.kchunks > 6) {
        launch_v2d_sym2_wide(a, kernel_type, s);
    } else {
        launch_v2d_sym2_here(a, kernel_type, s);
    }
}
#else
void launch_v2d_sym2_wide(const TileArgs<double> &a, int kernel_type, hipStream_t s) { launch_v2d_sym2_here(a, kernel_type, s); }
#endif
#elif LSSVM_TU_HALF == 5 || LSSVM_TU_HALF == 6
/* two vectors per pass on the full square (the resident fp64 predictor: rows = points, columns = support vectors): rbf and polynomial -- the linear kernel predicts
 * through w -- for every chunk count the single-vector kernel has */
template <int KT>
static void launch_v2d_full_kt2(const TileArgs<double> &a, dim3 grid, hipStream_t s) {
    const dim3 block(TILE_THREADS);
    switch (a.kchunks) {
#if LSSVM_TU_HALF == 5
        case 1: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 1, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 2: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 2, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 3: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 3, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 4: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 4, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 5: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 5, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 6: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 6, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
#else
        case 7: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 7, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 8: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 8, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 10: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 10, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 12: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 12, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 14: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 14, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
        case 16: hipLaunchKernelGGL((tile_matvec_f64_v2<KT, 16, false, 2>), grid, block, V2D_LDS_BYTES_NV2, s, a); break;
#endif
        default: throw Error(LSSVM_ERR_INTERNAL, "no two-vector v2 tile kernel for this number of k-chunks");
    }
}
static void launch_v2d_full2_here(const TileArgs<double> &a, int kernel_type, dim3 grid, hipStream_t s) {
    switch (kernel_type) {
        case KT_LINEAR: throw Error(LSSVM_ERR_INTERNAL, "no two-vector fp64 tile kernel for the full square of the linear kernel");
        case KT_POLY:
            if (a.degree == 3) {
                launch_v2d_full_kt2<KT_POLY3>(a, grid, s);
            } else if (a.degree == 2) {
                launch_v2d_full_kt2<KT_POLY2>(a, grid, s);
            } else {
                launch_v2d_full_kt2<KT_POLY>(a, grid, s);
            }
            break;
        default: launch_v2d_full_kt2<KT_RBF>(a, grid, s); break;
    }
}
void launch_v2d_full2_wide(const TileArgs<double> &a, int kernel_type, dim3 grid, hipStream_t s);  // tile_launch_f64_full2b.hip: 7 ... 16 chunks
#if LSSVM_TU_HALF == 5
void launch_v2d_full2(const TileArgs<double> &a, int kernel_type, dim3 grid, hipStream_t s) {
    if (a.kchunks > 6) {
        launch_v2d_full2_wide(a, kernel_type, grid, s);
    } else {
        launch_v2d_full2_here(a, kernel_type, grid, s);
    }
}
#else
void launch_v2d_full2_wide(const TileArgs<double> &a, int kernel_type, dim3 grid, hipStream_t s) { launch_v2d_full2_here(a, kernel_type, grid, s); }
#endif
#elif LSSVM_TU_HALF == 1
void launch_v2d_sym(const TileArgs<double> &a, int kernel_type, hipStream_t s) {
    const dim3 sgrid(static_cast<unsigned>(a.num_items));
    switch (kernel_type) {
        case KT_LINEAR: launch_v2d_kt<KT_LINEAR, true>(a, sgrid, s); break;
        case KT_POLY:
            if (a.degree == 3) {
                launch_v2d_kt<KT_POLY3, true>(a, sgrid, s);
            } else if (a.degree == 2) {
                launch_v2d_kt<KT_POLY2, true>(a, sgrid, s);
            } else {
                launch_v2d_kt<KT_POLY, true>(a, sgrid, s);
            }
            break;
        default: launch_v2d_kt<KT_RBF, true>(a, sgrid, s); break;
    }
}
#else
template <>
void launch_tile_kernel<double>(TileArgs<double> &a, int kernel_type, bool /*rbf_direct*/, int num_jc, hipStream_t s) {
    const dim3 grid(a.num_ib > 0 && num_jc > 0 ? finish_mapping(a, num_jc) : 0u);
    const dim3 block(TILE_THREADS);
    if (grid.x == 0) return;
    constexpr size_t lds = static_cast<size_t>(4) * TILE * F64_LS * sizeof(double);
    if (a.dc != nullptr && a.wide_panels != 0) {
        if (a.nvec == 2 && a.items == nullptr) {  // two vectors per full-square pass of the panel kernel (the resident Predictor<double>)
            launch_nv2_panel_tile_kernel_f64(a, kernel_type, grid, s);
        } else {
            launch_wide_tile_kernel_f64(a, kernel_type, grid, s);
        }
        return;
    }
    if (a.dc != nullptr) {  // the records exist only where the v2 kernel was chosen when the data was prepared; V2D_LDS_BYTES < 64 KiB
        if (a.nvec == 2) {  // two vectors per pass: the symmetric variant (Problem<double>::enqueue_apply_K_lanes), the full square (the resident Predictor<double>)
            if (a.items == nullptr) {
                launch_v2d_full2(a, kernel_type, grid, s);
            } else {
                launch_v2d_sym2(a, kernel_type, s);
            }
        } else if (a.items != nullptr) {
            launch_v2d_sym(a, kernel_type, s);
        } else {
            switch (kernel_type) {
                case KT_LINEAR: launch_v2d_kt<KT_LINEAR, false>(a, grid, s); break;
                case KT_POLY:
                    if (a.degree == 3) {
                        launch_v2d_kt<KT_POLY3, false>(a, grid, s);
                    } else if (a.degree == 2) {
                        launch_v2d_kt<KT_POLY2, false>(a, grid, s);
                    } else {
                        launch_v2d_kt<KT_POLY, false>(a, grid, s);
                    }
                    break;
                default: launch_v2d_kt<KT_RBF, false>(a, grid, s); break;
            }
        }
        LSSVM_HIP_CHECK(hipGetLastError());
        return;
    }
    switch (kernel_type) {
        case KT_LINEAR:
            ensure_dynamic_lds(tile_matvec_f64<KT_LINEAR>, lds);
            hipLaunchKernelGGL(tile_matvec_f64<KT_LINEAR>, grid, block, lds, s, a);
            break;
        case KT_POLY:
            ensure_dynamic_lds(tile_matvec_f64<KT_POLY>, lds);
            hipLaunchKernelGGL(tile_matvec_f64<KT_POLY>, grid, block, lds, s, a);
            break;
        default:
            ensure_dynamic_lds(tile_matvec_f64<KT_RBF>, lds);
            hipLaunchKernelGGL(tile_matvec_f64<KT_RBF>, grid, block, lds, s, a);
            break;
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}
#endif

}  // namespace lssvm
