/*
 * lssvm_problem.hip -- Problem<T>: one device's shard of the device-resident LS-SVM problem (see lssvm_problem.hip.hpp) -- the data in its HBM layouts, the
 * operand planes, the work-item geometry, the tile-kernel launches of one implicit matvec -- and the one-shot predict path, a rectangular instance of the same
 * tile kernels.  The CG driver over the shards is lssvm_solver.hip, the exchange between them lssvm_exchange.hip.  Compiled for gfx950 only.
 */
#include "lssvm_problem.hip.hpp"

#define LSSVM_KERNELS_SETUP
#include "lssvm_kernels.hip.hpp"

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>

namespace lssvm {

Options &options() {
    static Options o;
    return o;
}
std::mutex &options_mutex() {
    static std::mutex m;
    return m;
}

void check_params(const lssvm_params *params) {
    LSSVM_REQUIRE(params != nullptr, "params must not be NULL!");
    LSSVM_REQUIRE(params->kernel_type == LSSVM_KERNEL_LINEAR || params->kernel_type == LSSVM_KERNEL_POLYNOMIAL || params->kernel_type == LSSVM_KERNEL_RBF,
                  "Invalid kernel function " + std::to_string(params->kernel_type) + " given!");  // csvm.hpp:379
    if (params->kernel_type != LSSVM_KERNEL_LINEAR) {
        LSSVM_REQUIRE(params->gamma > 0.0, "gamma must be greater than 0, but is " + std::to_string(params->gamma) + "!");  // svm_kernel.cpp:68, :77
    }
    LSSVM_REQUIRE(params->cost != 0.0 && std::isfinite(1.0 / params->cost), "cost must not be 0.0 since it is 1 / plssvm::cost!");  // svm_kernel.cpp:27
}

template <typename T>
void check_weights(const double *weights, size_t num_points, double cost) {
    LSSVM_REQUIRE(weights != nullptr, "weights must not be NULL");
    for (size_t i = 0; i < num_points; ++i) {
        const double w = weights[i];
        LSSVM_REQUIRE(std::isfinite(w) && w > 0.0, "weight " + std::to_string(i) + " is " + std::to_string(w) + ": every weight must be finite and greater than 0.0!");
        // (the diagonal term is formed in the real type, as 1 / C is: a weight that is positive in double may not be in float)
        const T inv = T(1) / (static_cast<T>(cost) * static_cast<T>(w));
        LSSVM_REQUIRE(static_cast<T>(w) > T(0) && std::isfinite(static_cast<double>(inv)), "weight " + std::to_string(i) + " is " + std::to_string(w) + ": 1 / (C * weight) is not finite in the real type!");
    }
}
template void check_weights<float>(const double *, size_t, double);
template void check_weights<double>(const double *, size_t, double);

static int device_count_checked() {
    int count = 0;
    const hipError_t err = hipGetDeviceCount(&count);
    if (err != hipSuccess || count <= 0) {
        (void) hipGetLastError();
        throw Error(LSSVM_ERR_NO_DEVICE, "HIP backend selected but no HIP capable devices were found!");  // csvm.hip.cpp:70-72
    }
    return count;
}

int select_device_checked(int device) {
    const int count = device_count_checked();
    LSSVM_REQUIRE(device >= 0 && device < count, "Invalid device " + std::to_string(device) + " (" + std::to_string(count) + " available)!");
    LSSVM_HIP_CHECK(hipSetDevice(device));
    return count;
}

std::vector<int> resolve_devices(const int *devices, int num_devices, size_t num_points) {
    const int count = device_count_checked();
    LSSVM_REQUIRE(num_devices >= 0 && num_devices <= MAX_LOCAL_DEVICES, "num_devices must be between 0 (automatic) and " + std::to_string(MAX_LOCAL_DEVICES) + "!");
    std::vector<int> out;
    if (num_devices == 0) {
        // automatic: every visible device, as the reference's backends do (csvm.hip.cpp:66-75), but never fewer than 32 row blocks
        // (4096 points) per device -- below that the exchange and the launch latencies outweigh the split
        LSSVM_REQUIRE(devices == nullptr, "a device list needs its length (num_devices > 0)");
        const long tiles = (static_cast<long>(num_points) - 1 + TILE - 1) / TILE;
        const int use = static_cast<int>(std::max<long>(1, std::min<long>(std::min(count, MAX_LOCAL_DEVICES), tiles / 32)));
        for (int r = 0; r < use; ++r) out.push_back(r);
        return out;
    }
    for (int r = 0; r < num_devices; ++r) {
        const int dev = devices != nullptr ? devices[r] : r;
        LSSVM_REQUIRE(dev >= 0 && dev < count, "Invalid device " + std::to_string(dev) + " (" + std::to_string(count) + " available)!");
        out.push_back(dev);
    }
    return out;
}

/* ------------------------------------------------------------------ tile kernel selection ------------------------------------------------------------------ */
/* the v2 kernels exist for 1..8 and 10, 12, 14, 16 k-chunks (padded_features() never produces an odd count above 8) */
static bool v2_chunk_count_ok(int kchunks, int single_up_to = 8) {
    return kchunks <= single_up_to || (kchunks <= 16 && kchunks % 2 == 0);
}
bool v2_eligible(const Options &o, int ldx, bool rbf_direct) {
    return !rbf_direct && v2_chunk_count_ok(ldx / F32_KC, 4) && o.tile_kernel != 1;
}
bool v2_eligible_f64(const Options &o, int ldx) {
    return v2_chunk_count_ok(ldx / F64_KC) && o.tile_kernel != 1;
}

constexpr int F64_ONE_PASS_FEATURES = 256;

/* fp64 rbf / polynomial on more than 256 features: feature panels of 64 inside a sub-tile (lssvm_tile_f64_wide.hip.hpp; the data carries the
   kernel's scale as on the one-pass v2 kernel, so gamma > 0 -- a precondition of the kernels anyway -- and a non-negative degree are required) */
bool wide_nonlinear_f64(const Options &o, const lssvm_params &p, size_t num_features) {
    const bool nonlinear = p.kernel_type == LSSVM_KERNEL_RBF || (p.kernel_type == LSSVM_KERNEL_POLYNOMIAL && p.degree >= 0);
    return nonlinear && p.gamma > 0.0 && o.tile_kernel != 1 && padded_features<double>(num_features) > F64_ONE_PASS_FEATURES;
}

/* fp32 rbf / polynomial beyond the feature count the one-pass split kernels take (row panel in registers): the panel kernel applies */
bool wide_nonlinear(const Options &o, const lssvm_params &p, bool rbf_direct, size_t num_features) {
    const bool nonlinear = (p.kernel_type == LSSVM_KERNEL_RBF && !rbf_direct) || (p.kernel_type == LSSVM_KERNEL_POLYNOMIAL && p.degree >= 0);
    const long one_pass_limit = (p.kernel_type == LSSVM_KERNEL_RBF || o.gram_mode == 1) ? 384 : 512;  // SPLIT_MAX_FEATURES / F16_MAX_FEATURES (rbf: F16_RBF_MAX_FEATURES)
    return nonlinear && o.gram_mode != 0 && o.tile_kernel != 1 && round_up(static_cast<long>(num_features), 64) > one_pass_limit;
}

/* The resident fp32 predictor beyond 128 features (Predictor<float>, lssvm_predict.hip): whether a pair of weight vectors is dispatched as ONE launch of the wide
 * two-vector kernels (tile_launch_f32v2w.hip) -- by plane kind (PlaneSet::mode: 1 bf16x6, 2 f16x3), kernel function (polynomial: its degree selects the instantiation)
 * and the number of 64-feature chunks.  The project's routing condition: a pair launch is dispatched where it was measured to take less than two single-vector launches
 * by more than the single-vector kernel's own run-to-run spread (tests/tools/predictor_f32_wide_timing.py, profiles/predictor_f32_wide.json); an instantiation that
 * fails it is named here and served by two single-vector launches on the same resident data.  None is named: all 38 meet it at 4 096 points x 30 000 support vectors
 * -- 0.49 ... 0.53 of two launches, the worst ratio + spread 0.60 (bf16x6, polynomial of degree 2, three chunks) -- and are dispatched. */
bool wide_pair_routed(int plane_mode, int kernel_type, int /*degree*/, int nk64) {
    const int max_nk64 = (plane_mode == 2 && kernel_type != LSSVM_KERNEL_RBF) ? 8 : 6;  // (what tile_launch_f32v2w.hip instantiates)
    return (plane_mode == 1 || plane_mode == 2) && nk64 >= 3 && nk64 <= max_nk64;
}

/* The resident predictors beyond the one-pass kernels (lssvm_mi355_predictor_create_panels; lssvm_predict.hip): whether a pair of weight vectors is dispatched as ONE
 * launch of the two-vector panel kernels (tile_launch_f32xv2.hip: f16x3 and bf16x6 planes x polynomial of a run-time degree, degree 2, degree 3, folded rbf;
 * tile_launch_f64xv2.hip: rbf and the three polynomial forms) -- by real type, plane kind (fp32; PlaneSet::mode), kernel function and number of feature panels (128
 * features in fp32, 64 in fp64; one instantiation serves every panel count).  Same routing condition as wide_pair_routed, measured by
 * tests/tools/predictor_panels_timing.py (profiles/predictor_panels.json) against two single-vector launches of the build before; an instantiation that fails it, or that
 * the compiler does not fit into its single-vector sibling's register budget without scratch, is named here and served by two single-vector launches on the same resident
 * data.  None is named: all twelve compile without scratch at their siblings' occupancy.  (Unfolded fp32 rbf has no pair record and never gets here.) */
bool panel_pair_routed(int dtype, int plane_mode, int kernel_type, int /*degree*/, int panels) {
    const bool nonlinear = kernel_type == LSSVM_KERNEL_RBF || kernel_type == LSSVM_KERNEL_POLYNOMIAL;
    if (dtype == LSSVM_DTYPE_F64) return nonlinear && panels >= 5;
    return nonlinear && (plane_mode == 1 || plane_mode == 2) && panels >= 2;
}

/* The lockstep CG in fp32 on 129 ... 512 features (Problem<float>::pair_kernel_applies): whether a pair of right-hand sides is dispatched as ONE launch of the symmetric
 * two-vector kernels (tile_launch_f32v2ws.hip) -- same arguments, same routing condition as wide_pair_routed, measured by tests/tools/lockstep_f32_wide_timing.py
 * (profiles/lockstep_f32_wide.json) against two single-vector symmetric passes of the build before.  An instantiation that fails the condition, or that the compiler
 * does not fit into the register file without scratch, is named here and takes two single passes.  None is named: all 38 compile without scratch and meet the condition
 * at 30 000 points -- 0.50 ... 0.54 of two passes, the worst ratio + spread 0.66 (f16x3, folded rbf, four chunks) -- and are dispatched. */
bool sym_pair_routed(int plane_mode, int kernel_type, int /*degree*/, int nk64) {
    const int max_nk64 = (plane_mode == 2 && kernel_type != LSSVM_KERNEL_RBF) ? 8 : 6;  // (what tile_launch_f32v2ws.hip instantiates)
    return (plane_mode == 1 || plane_mode == 2) && nk64 >= 3 && nk64 <= max_nk64;
}

/* kernel-function specific scalars of TileArgs */
template <typename T>
void set_kernel_scalars(TileArgs<T> &a, const lssvm_params &p, bool rbf_direct) {
    a.degree = p.degree;
    a.coef0 = static_cast<T>(p.coef0);
    constexpr double log2e = 1.4426950408889634073599246810019;
    if (p.kernel_type == LSSVM_KERNEL_RBF) {
        const T g = static_cast<T>(p.gamma);  // gamma is rounded to the real type first, as in parameter<T>
        if (rbf_direct) {
            a.gamma = static_cast<T>(-static_cast<double>(g) * log2e);
        } else if (std::is_same_v<T, float>) {
            a.gamma = T(1);  // folded into the data (rbf_prescale)
        } else {
            a.gamma = static_cast<T>(2.0 * static_cast<double>(g));
        }
    } else {
        a.gamma = static_cast<T>(p.gamma);
    }
}

/* the launch-related knobs travel inside TileArgs: the launchers never read the process-wide defaults */
template <typename T>
void set_launch_options(TileArgs<T> &a, const Options &o) {
    a.dbg = static_cast<int>(o.debug_ablate);
    a.mfma_shape = static_cast<int>(o.mfma_shape);
    a.pair_lag = static_cast<int>(o.pair_lag);
}

/* rbf on the matrix cores: the data is scaled so that the MFMA chain leaves the exponent in the unit the epilogue wants:
 * fp32: x' = sqrt(2 gamma log2 e) (x - mean)  =>  x_i'.x_j' - (|x_i'|^2 + |x_j'|^2)/2 = -gamma log2(e) |x_i - x_j|^2 (epilogue v_exp_f32);
 * fp64 on the v2 kernel (`fp64_v2`): the same (epilogue exp2_f64); fp64 on the generic kernel: unscaled (epilogue fast_exp_f64(acc * 2 gamma)). */
template <typename T>
T rbf_prescale(const lssvm_params &p, bool fp64_v2) {
    constexpr double log2e = 1.4426950408889634073599246810019;
    if constexpr (std::is_same_v<T, float>) {
        return static_cast<T>(std::sqrt(2.0 * static_cast<double>(static_cast<T>(p.gamma)) * log2e));
    } else {
        return fp64_v2 ? static_cast<T>(std::sqrt(2.0 * p.gamma * log2e)) : T(1);
    }
}

/* column means of M's valid rows, in double, deterministic two-stage sum */
template <typename T>
void column_means(const DeviceMatrix<T> &M, DevBuf<T> &mean, hipStream_t s) {
    const int rows_per_block = 256;
    const int nblocks = (M.rows + rows_per_block - 1) / rows_per_block;
    DevBuf<double> part;
    part.alloc_zero(static_cast<size_t>(nblocks) * M.ldx, s);
    mean.alloc_zero(M.ldx, s);
    const dim3 g1(nblocks, (M.ldx + 255) / 256);
    hipLaunchKernelGGL(k_colsum_stage1<T>, g1, dim3(256), 0, s, M.data.p, M.ldx, M.rows, rows_per_block, part.p);
    hipLaunchKernelGGL(k_colsum_stage2<T>, dim3((M.ldx + 255) / 256), dim3(256), 0, s, part.p, nblocks, M.ldx, M.rows, mean.p);
    LSSVM_HIP_CHECK(hipGetLastError());
    LSSVM_HIP_CHECK(hipStreamSynchronize(s));  // part is released on return
}

/* max_i |x_i - mean|^2 over the valid rows of M (the data is NOT modified) */
template <typename T>
double max_centred_sqnorm(const DeviceMatrix<T> &M, const DevBuf<T> &mean, hipStream_t s) {
    DevBuf<double> sq;
    sq.alloc_zero(static_cast<size_t>(M.rows), s);
    hipLaunchKernelGGL(k_centred_sqnorm<T>, dim3((M.rows + 3) / 4), dim3(256), 0, s, M.data.p, M.ldx, M.dfeat, M.rows, mean.p, sq.p);
    LSSVM_HIP_CHECK(hipGetLastError());
    std::vector<double> host(static_cast<size_t>(M.rows));
    LSSVM_HIP_CHECK(hipMemcpyAsync(host.data(), sq.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    LSSVM_HIP_CHECK(hipStreamSynchronize(s));
    return host.empty() ? 0.0 : *std::max_element(host.begin(), host.end());
}

template <typename T>
void center_columns(DeviceMatrix<T> &M, DeviceMatrix<T> *M2, T scale, hipStream_t s) {
    DevBuf<T> mean;
    column_means<T>(M, mean, s);
    hipLaunchKernelGGL(k_center<T>, dim3((M.dfeat + 255) / 256, M.rows), dim3(256), 0, s, M.data.p, M.ldx, M.dfeat, M.rows, mean.p, scale);
    if (M2 != nullptr) {
        hipLaunchKernelGGL(k_center<T>, dim3((M2->dfeat + 255) / 256, M2->rows), dim3(256), 0, s, M2->data.p, M2->ldx, M2->dfeat, M2->rows, mean.p, scale);
    }
    LSSVM_HIP_CHECK(hipGetLastError());
    LSSVM_HIP_CHECK(hipStreamSynchronize(s));  // mean is released on return
}

/* fp32 rbf, option rbf_form = 0 (automatic): the matrix-core form evaluates the exponent as c_i + c_j + x_i'.x_j' on data scaled by
 * sqrt(2 gamma log2 e), so its ABSOLUTE error is about 2^-24 times the size of the terms that cancel, R2 = 2 gamma log2(e) max |x - mean|^2,
 * whatever the distance of the pair -- for nearby points (K close to 1) that is a relative error of K of ~R2 * 2^-24, where the reference's
 * direct (x_i - x_j)^2 chain keeps all its digits.  [-1, 1]-scaled data with gamma = 1 / num_features has R2 <= 3; gamma = 1 at 128
 * features has R2 ~ 100.  Above RBF_DIRECT_ABOVE the formula-exact vector-ALU kernel is used instead (5x slower, same accuracy class as
 * the reference).  Returns true for the direct form.  `M2` (predict: the points beside the support vectors) may be NULL. */
template <typename T>
bool rbf_wants_direct_form(const Options &o, const lssvm_params &p, const DeviceMatrix<T> &M, const DeviceMatrix<T> *M2, hipStream_t s, double *r2_out) {
    if (r2_out != nullptr) *r2_out = 0.0;
    if (!std::is_same_v<T, float> || p.kernel_type != LSSVM_KERNEL_RBF) return false;
    if (o.rbf_form == 1) return true;
    DevBuf<T> mean;
    column_means<T>(M, mean, s);
    double sq = max_centred_sqnorm<T>(M, mean, s);
    if (M2 != nullptr) sq = std::max(sq, max_centred_sqnorm<T>(*M2, mean, s));
    const double r2 = 2.0 * static_cast<double>(static_cast<T>(p.gamma)) * 1.4426950408889634 * sq;
    if (r2_out != nullptr) *r2_out = r2;
    if (o.rbf_form == 2) return false;  // the norm expansion whatever the scale (r2 is still reported: it decides the record form)
    return r2 > RBF_DIRECT_ABOVE;       // (0 and 3: the caller then moves to the grid planes where they exist -- rbf_wants_grid_planes -- and stays here where they do not)
}

/* fp32: reorder the features of every group of 8 to 0,2,4,6,1,3,5,7 (the operand order of the MFMA kernels); fp64: nothing */
template <typename T>
void interleave_features(DeviceMatrix<T> &M, hipStream_t s) {
    if constexpr (std::is_same_v<T, float>) {
        const size_t ngroups = static_cast<size_t>(M.rows_alloc) * M.ldx / 8;
        hipLaunchKernelGGL(k_interleave_features, dim3(static_cast<unsigned>((ngroups + 255) / 256)), dim3(256), 0, s, M.data.p, ngroups);
        LSSVM_HIP_CHECK(hipGetLastError());
    }
}

template <typename T>
void half_neg_norms(const DeviceMatrix<T> &M, DevBuf<T> &c, hipStream_t s) {
    c.alloc_zero(M.rows_alloc, s);
    hipLaunchKernelGGL(k_half_neg_norms<T>, dim3((M.rows_alloc + 3) / 4), dim3(256), 0, s, M.data.p, M.ldx, M.rows_alloc, c.p);
    LSSVM_HIP_CHECK(hipGetLastError());
}

/* fp32: the (centred, scaled) data once more as operand planes of the split kernels; `M2` (predict: the points beside the support vectors)
 * may be NULL and gets planes of the same kind and scale.
 *   f16x3 (mode 2): two f16 planes, x ~ hi + mid (11 + 11 significant bits).  What limits them is f16's exponent range: mid ~ 2^-12 |x| turns
 *     subnormal (loses bits) for |x| < 2^-2.  Linear and polynomial kernels: the planes carry 2^k x, k moves the largest entry to [2^14, 2^15)
 *     so that mid stays a NORMAL f16 for entries down to 2^-17 of it -- undone exactly on the finished sums (TileArgs::out_scale) or inside
 *     gamma.  rbf cannot pre-scale (the chain must leave the exponent itself, and a multiply per element in the epilogue costs matrix-core
 *     time): it uses the SHIFTED planes (2^-6 hi, 2^6 mid, 2^6 hi) -- every product of a row plane and a column plane carries the net scale 1,
 *     mid is normal for |x| in [2^-8, 2^10), which covers everything the exponent scale allows (|x| <= sqrt(RBF_DIRECT_ABOVE)); the price is a
 *     third row plane in registers, none in the column stream.  Whether the planes carry THIS data as well as fp32 does is measured, not
 *     assumed: k_split_f16x2 returns the largest relative representation error of a row; above 2^-22 (data with a dynamic range beyond the
 *     planes', or planes that overflow) the answer is no -- for rbf an absolute bound on the exponent's error is accepted as well.
 *   bf16x6 (mode 1): three bf16 planes, exact for every fp32 input (8 exponent bits), twice the matrix-core work.
 * option gram_mode: 0 = none (native v_mfma_f32 kernels), 1 = bf16x6, 2 = f16x3 without the check (A/B, tests), 3 = f16x3 if the data passes, else bf16x6. */
void make_planes(const Options &o, const lssvm_params &p, bool rbf_direct, const DeviceMatrix<float> &M, const DeviceMatrix<float> *M2, PlaneSet &out, PlaneSet *out2, hipStream_t s,
                 bool wide_nl, bool linear_panels, bool f16_known_bad) {
    out.mode = 0;
    if (out2 != nullptr) out2->mode = 0;
    // (wide_nl: rbf / polynomial beyond the register-resident row panel -- the kernel walks feature panels of 128 inside a tile and exists for
    // both plane kinds, so neither feature limit below applies; planes padded to whole panels)
    const int ldx16 = static_cast<int>(round_up(static_cast<long>(M.dfeat), wide_nl ? 128 : 64));
    // linear_panels: the CALLER says whether the linear kernel's panel passes will run (symmetric variant, f16x3 only) -- the decision is not
    // re-derived here (a full-square problem of more than 512 features got planes that nobody read).  f16_known_bad: an earlier call
    // on the same data has already seen the representability check fail.
    const bool wide_linear = linear_panels && p.kernel_type == LSSVM_KERNEL_LINEAR && ldx16 > LINEAR_PANEL_FEATURES && o.tile_kernel != 1;
    if (o.gram_mode == 0 || rbf_direct || (!v2_eligible(o, M.ldx, false) && !wide_linear && !wide_nl)) return;
    auto alloc = [&](int nplanes) {
        out.ldx16 = ldx16;
        out.nplanes = nplanes;
        if (out2 != nullptr) out2->nplanes = nplanes;
        out.buf.alloc_zero(static_cast<size_t>(nplanes) * M.rows_alloc * ldx16, s);
        if (M2 != nullptr) {
            out2->ldx16 = ldx16;
            out2->buf.alloc_zero(static_cast<size_t>(nplanes) * M2->rows_alloc * ldx16, s);
        }
    };
    const bool rbf = p.kernel_type == LSSVM_KERNEL_RBF;
    const int f16_limit = rbf ? F16_RBF_MAX_FEATURES : (wide_linear ? F16_LINEAR_MAX_FEATURES : F16_MAX_FEATURES);
    if ((o.gram_mode == 2 || o.gram_mode == 3) && (ldx16 <= f16_limit || wide_nl) && !(f16_known_bad && o.gram_mode == 3)) {
        DevBuf<unsigned> stats;
        stats.alloc_zero(4, s);
        int shift = 0;
        unsigned host[4] = { 0, 0, 0, 0 };
        if (p.kernel_type != LSSVM_KERNEL_RBF) {
            absmax_f32(M.data.p, M.ldx, M.dfeat, static_cast<size_t>(M.rows), stats.p + 3, s);
            if (M2 != nullptr) absmax_f32(M2->data.p, M2->ldx, M2->dfeat, static_cast<size_t>(M2->rows), stats.p + 3, s);
            LSSVM_HIP_CHECK(hipMemcpyAsync(host, stats.p, sizeof(host), hipMemcpyDeviceToHost, s));
            LSSVM_HIP_CHECK(hipStreamSynchronize(s));
            float amax = 0.0f;
            std::memcpy(&amax, &host[3], sizeof(float));
            if (amax > 0.0f && std::isfinite(amax)) shift = std::min(std::max(F16_TARGET_EXP - std::ilogb(amax), -F16_MAX_SHIFT), F16_MAX_SHIFT);
        }
        alloc(rbf ? 3 : 2);
        const float scale = std::ldexp(1.0f, shift);
        const int pshift = rbf ? F16_RBF_SHIFT : 0;
        split_f16_planes(M.data.p, M.ldx, M.dfeat, static_cast<size_t>(M.rows_alloc), ldx16, scale, pshift, out.buf.p, static_cast<size_t>(M.rows_alloc) * ldx16, stats.p, s);
        if (M2 != nullptr) {
            split_f16_planes(M2->data.p, M2->ldx, M2->dfeat, static_cast<size_t>(M2->rows_alloc), ldx16, scale, pshift, out2->buf.p, static_cast<size_t>(M2->rows_alloc) * ldx16, stats.p, s);
        }
        LSSVM_HIP_CHECK(hipMemcpyAsync(host, stats.p, sizeof(host), hipMemcpyDeviceToHost, s));
        LSSVM_HIP_CHECK(hipStreamSynchronize(s));
        float rel2 = 0.0f, rest2 = 0.0f, x2 = 0.0f;
        std::memcpy(&rel2, &host[0], sizeof(float));
        std::memcpy(&rest2, &host[1], sizeof(float));
        std::memcpy(&x2, &host[2], sizeof(float));
        out.f16_row_rel_error = std::sqrt(static_cast<double>(rel2));  // (NaN: an overflowing plane)
        out.f16_rel2 = rel2;
        out.f16_rest2 = rest2;
        out.f16_x2 = x2;
        const bool ok = f16_planes_pass(p.kernel_type == LSSVM_KERNEL_RBF, rel2, rest2, x2);
        if (const char *dbg = std::getenv("LSSVM_MI355_DEBUG"); dbg != nullptr && dbg[0] == '1') {
            std::fprintf(stderr, "[plssvm_amd] f16 planes: shift %d, max relative representation error of a row %.3g (accepted up to %.3g), max |rest| %.3g, max |x| %.3g -> %s\n", shift,
                         std::sqrt(static_cast<double>(rel2)), std::sqrt(static_cast<double>(F16_REL2_MAX)), std::sqrt(static_cast<double>(rest2)), std::sqrt(static_cast<double>(x2)),
                         ok ? "f16x3" : (o.gram_mode == 2 ? "f16x3 (forced)" : "bf16x6"));
        }
        if (ok || o.gram_mode == 2) {
            out.mode = 2;
            out.shift = shift;
            if (out2 != nullptr) {
                out2->mode = 2;
                out2->shift = shift;
            }
            return;
        }
        // Round 6, linear kernel (training): what ONE scale for the matrix cannot hold is data whose ROWS differ by orders of magnitude (tests/tools/gram_mode_by_data.py:
        // the only shape that failed) -- the small rows' mid plane falls into f16's subnormals.  A power-of-two scale PER ROW holds them: K = D (Xs Xs^T) D with D = diag(2^-k_i),
        // so the tile kernels run unchanged on Xs and Problem<float> multiplies the vector by D in front of the product and the result by D behind it (two O(n) launches)
        // instead of running twice the matrix-core work as bf16x6.
        if (p.kernel_type == LSSVM_KERNEL_LINEAR && M2 == nullptr && o.gram_mode == 3 && std::isfinite(rel2)) {
            out.row_inv_scale.alloc_zero(static_cast<size_t>(M.rows_alloc), s);
            LSSVM_HIP_CHECK(hipMemsetAsync(stats.p, 0, 4 * sizeof(unsigned), s));
            split_f16_planes(M.data.p, M.ldx, M.dfeat, static_cast<size_t>(M.rows_alloc), ldx16, 1.0f, 0, out.buf.p, static_cast<size_t>(M.rows_alloc) * ldx16, stats.p, s, out.row_inv_scale.p);
            LSSVM_HIP_CHECK(hipMemcpyAsync(host, stats.p, sizeof(host), hipMemcpyDeviceToHost, s));
            LSSVM_HIP_CHECK(hipStreamSynchronize(s));
            float rel2_rows = 0.0f;
            std::memcpy(&rel2_rows, &host[0], sizeof(float));
            if (const char *dbg = std::getenv("LSSVM_MI355_DEBUG"); dbg != nullptr && dbg[0] == '1') {
                std::fprintf(stderr, "[plssvm_amd] f16 planes with a scale per row: max relative representation error of a row %.3g -> %s\n", std::sqrt(static_cast<double>(rel2_rows)),
                             rel2_rows <= F16_REL2_MAX ? "f16x3 (row scaled)" : "bf16x6");
            }
            if (rel2_rows <= F16_REL2_MAX) {
                out.mode = 2;
                out.shift = 0;
                out.f16_row_rel_error = std::sqrt(static_cast<double>(rel2_rows));
                return;
            }
            out.row_inv_scale.release();
        }
        out.buf.release();
        if (out2 != nullptr) out2->buf.release();
    }
    if ((o.gram_mode == 1 || o.gram_mode == 3) && (ldx16 <= SPLIT_MAX_FEATURES || wide_nl)) {
        alloc(3);
        split_bf16_planes(M.data.p, M.ldx, M.dfeat, static_cast<size_t>(M.rows_alloc), ldx16, out.buf.p, static_cast<size_t>(M.rows_alloc) * ldx16, s);
        out.mode = 1;
        if (M2 != nullptr) {
            split_bf16_planes(M2->data.p, M2->ldx, M2->dfeat, static_cast<size_t>(M2->rows_alloc), ldx16, out2->buf.p, static_cast<size_t>(M2->rows_alloc) * ldx16, s);
            out2->mode = 1;
        }
    }
}

/* rbf on GRID planes (KT_RBFG): the rule that chooses them, and the planes of one (centred, scaled) matrix */
bool rbf_wants_grid_planes(const Options &o, const lssvm_params &p, size_t num_features, double r2) {
    const bool shape = p.kernel_type == LSSVM_KERNEL_RBF && o.gram_mode != 0 && o.tile_kernel != 1;  // (<= 128 features: _g6h, <= 384: _g6w, beyond: the panels-inside-a-tile kernel)
    // (the cross terms |h||s| grow like R2 sqrt(d): the limit is RBF_GRID_MAX_R2 at 128 features and sqrt(128 / d) of it beyond -- 2 365 at 384; a 300-case random run at the
    // flat limit had its worst case, 15.7 eps, on wide data at the top of the range: profiles/r05_grid_stress_seed31.log)
    const double limit = RBF_GRID_MAX_R2 * std::sqrt(128.0 / static_cast<double>(std::max<size_t>(num_features, 128)));
    return shape && std::isfinite(r2) && r2 <= limit && (o.rbf_form == 3 || (o.rbf_form == 0 && r2 > RBF_DIRECT_ABOVE));
}
/* g from the exponent scale alone (max|x_k| <= sqrt(R2), so |h / g| <= 2048 holds with it; (R2 + 160) / (g^2 / 2) <= 2^24 keeps the h.h chain of every pair that matters -- |t| <= 150,
 * beyond that 2^t is 0 in fp32 -- exact); sigma moves the largest |h| below f16's maximum.  `chg` (rows_alloc floats, allocated) receives sigma^2 ch_i, `efac` is allocated here. */
float make_grid_planes(const DeviceMatrix<float> &M, double r2_in, PlaneSet &out, float *chg, DevBuf<float> &efac, hipStream_t s, bool wide_nl) {
    const double r2 = std::max(r2_in, 1.0);
    const double g = std::exp2(std::ceil(std::log2(std::max(std::sqrt((r2 + 160.0) * 0x1p-23), std::sqrt(r2) / 2048.0))));
    const float sigma = static_cast<float>(std::exp2(std::floor(std::log2(60000.0 / (std::sqrt(r2) + g)))));
    out.ldx16 = static_cast<int>(round_up(static_cast<long>(M.dfeat), wide_nl ? 128 : 64));  // (the panels-inside-a-tile kernel walks panels of 128 features)
    out.nplanes = 3;
    out.shift = 0;
    out.buf.alloc_zero(static_cast<size_t>(3) * M.rows_alloc * out.ldx16, s);
    efac.alloc_zero(M.rows_alloc, s);
    DevBuf<unsigned> stats;
    stats.alloc_zero(4, s);
    split_grid_planes(M.data.p, M.ldx, M.dfeat, static_cast<size_t>(M.rows_alloc), out.ldx16, static_cast<float>(g), sigma, out.buf.p, static_cast<size_t>(M.rows_alloc) * out.ldx16, chg, efac.p, stats.p, s);
    unsigned bad = 0;
    LSSVM_HIP_CHECK(hipMemcpyAsync(&bad, stats.p, sizeof(bad), hipMemcpyDeviceToHost, s));
    LSSVM_HIP_CHECK(hipStreamSynchronize(s));
    // (no valid input is known to get here -- |h / g| <= 2048 follows from the exponent scale the planes were sized with -- so the tests reach the path through this hook)
    if (const char *hook = std::getenv("LSSVM_MI355_TEST_GRID_UNFIT"); hook != nullptr && hook[0] == '1') bad = 1;
    if (bad != 0) throw GridPlanesUnfit();  // (rbf_form 0: the owner builds the problem again on the formula-exact kernel; rbf_form 3: the error is the caller's)
    out.mode = 2;  // f16 planes (the launcher picks the grid kernel from TileArgs::rbf_grid)
    if (const char *dbg = std::getenv("LSSVM_MI355_DEBUG"); dbg != nullptr && dbg[0] == '1') {
        std::fprintf(stderr, "[plssvm_amd] rbf on grid planes: exponent scale %.1f, g = 2^%d, sigma = 2^%d\n", r2_in, static_cast<int>(std::log2(g)), static_cast<int>(std::log2(sigma)));
    }
    return sigma;
}

/* the plane fields of TileArgs; `gamma` must hold the kernel's own gamma already */
void set_plane_args(TileArgs<float> &a, const lssvm_params &p, const PlaneSet &cols, const PlaneSet &rows, size_t col_rows_alloc, size_t row_rows_alloc) {
    a.Xr16 = rows.buf.p;
    a.Xc16 = cols.buf.p;
    a.plane_stride = col_rows_alloc * cols.ldx16;
    a.plane_stride_r = row_rows_alloc * rows.ldx16;
    a.ldx16 = cols.ldx16;
    a.nk64 = cols.ldx16 / 64;
    a.planes_f16 = cols.mode == 2 ? 1 : 0;
    a.out_scale = 1.0f;
    if (cols.mode == 2 && cols.shift != 0) {
        const float undo = std::ldexp(1.0f, -2 * cols.shift);
        if (p.kernel_type == LSSVM_KERNEL_LINEAR) a.out_scale = undo;
        if (p.kernel_type == LSSVM_KERNEL_POLYNOMIAL) a.gamma *= undo;
    }
}

/* host restatement of kernel_function(x, x) for QA_cost (csvm.cpp:86): the same fma chain in the same precision */
template <typename T>
static T host_self_kernel(const lssvm_params &p, const std::vector<T> &x) {
    T val = T(0);
    if (p.kernel_type == LSSVM_KERNEL_RBF) {
        for (const T v : x) {
            const T diff = v - v;
            val = std::fma(diff, diff, val);
        }
        return std::exp(-static_cast<T>(p.gamma) * val);
    }
    for (const T v : x) val = std::fma(v, v, val);
    if (p.kernel_type == LSSVM_KERNEL_LINEAR) return val;
    return std::pow(std::fma(static_cast<T>(p.gamma), val, static_cast<T>(p.coef0)), static_cast<T>(p.degree));
}

/* ------------------------------------------------------------------ Problem: one device's shard ------------------------------------------------------------------ */
/* The part of a problem that depends on WHICH row blocks this shard evaluates (constructor; reshard): the shard's blocks, the column chunks of its work items. */
template <typename T>
void Problem<T>::choose_shard_geometry() {
    const size_t num_features = num_features_;
    const int ldx_probe = ldx_probe_;
    {
        int ib_end = 0;
        shard_blocks(num_tiles_, world_, rank_, sym_, ib_begin_, ib_end, &opt_.shard_weights);
        num_ib_ = ib_end - ib_begin_;
    }
    {
        // the column chunks of the work items (shard_chunks, lssvm_geometry.cpp); `split`: the fp32 split kernels, whose chunks may be longer
        const bool split = wide_linear_ || wide_nl_
                           || (std::is_same_v<T, float> && opt_.gram_mode != 0 && v2_eligible(opt_, ldx_probe, rbf_direct_)
                               && round_up(static_cast<long>(num_features), 64) <= ((opt_.gram_mode == 1 || tile_params_.kernel_type == LSSVM_KERNEL_RBF) ? SPLIT_MAX_FEATURES : F16_MAX_FEATURES));
        int cus = 256;  // 256-row workgroups: one per CU
        if (pair_ && opt_.j_chunk_tiles <= 0) LSSVM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_));
        const PairChunks c = shard_chunks(geometry_options(opt_), ib_begin_, ib_begin_ + num_ib_, num_tiles_, sizeof(T), sym_, split, pair_, wide_nl_, std::max(cus, 1));
        jc_tiles_ = c.tiles;
        jc_head_tiles_ = c.head_tiles;
        jc_head_count_ = c.head_count;
    }
    if (wide_nl_ && sym_) {
        // These kernels re-load a work item's row panel at EVERY column tile.  In the column-chunk major orders each of the 64 workgroups an XCD runs
        // at a time has a row panel of its own -- 64 x 0.4 ... 1.6 MB against 4 MB of L2: the re-loads came from beyond L2 at HBM rate (60 000 x 640
        // rbf: 54 GB of row planes per matvec, 6 TB/s).  Row-group major (band_items, order 4 / 5): an XCD works on FOUR (two, where a panel is
        // beyond 640 KB) row blocks x their column chunks at a time, so their panels stay in its L2 and every column tile is streamed for the
        // whole group: 60 000 x 640 rbf 8.5 -> 6.2 ms, 100 000 x 385 rbf 19.4 -> 12.4 ms.  Results do not depend on the order.
        const double panel_bytes = std::is_same_v<T, float>
                                       ? 128.0 * static_cast<double>(round_up(static_cast<long>(num_features), 128)) * ((tile_params_.kernel_type == LSSVM_KERNEL_RBF || opt_.gram_mode == 1) ? 3.0 : 2.0) * 2.0
                                       : 128.0 * static_cast<double>(ldx_probe) * 8.0;
        wide_order_ = panel_bytes <= 640e3 ? 4 : 5;
    }
    num_jc_ = num_chunks(num_tiles_, jc_tiles_, jc_head_tiles_, jc_head_count_);
    if (const char *dbg = std::getenv("LSSVM_MI355_DEBUG"); dbg != nullptr && dbg[0] == '1') {
        std::fprintf(stderr, "[plssvm_amd] shard %d/%d on device %d: row blocks [%d, %d) of %d, %d tiles per work item (head: %d chunks of %d), symmetric %d\n", rank_, world_, device_,
                     ib_begin_, ib_begin_ + num_ib_, num_tiles_, jc_tiles_, jc_head_count_, jc_head_tiles_, sym_ ? 1 : 0);
    }
}

/* ... and the device-side lists for it: the row slabs, the work items band by band, the column slab, the events around the band launches. */
template <typename T>
void Problem<T>::build_shard_lists(hipStream_t st) {
    partial_.alloc_zero(static_cast<size_t>(std::max(num_jc_, 1)) * part_blocks() * TILE, st);
    bands_.clear();
    if (sym_) {
        // Row-block BANDS.  Every evaluated off-diagonal tile leaves a 128-entry record of column sums (no atomics: one writer per record,
        // k_reduce_colslab adds the records of a column in a fixed order).  All records of the triangle would be n_tiles^2 / 2 * 512 bytes
        // (15.6 GB at 1M points in fp32); instead the device's row blocks are cut into bands of equal AREA whose records fit
        // colslab_band_mb, the tile kernel runs band by band into the SAME slab and the band's records are folded into K*v before the
        // next band overwrites them.  One band for up to ~360 000 points per device at the default 2 GiB.
        const int ib_end_all = ib_begin_ + num_ib_;
        const std::vector<int> edge = band_edges(ib_begin_, ib_end_all, sizeof(T), geometry_options(opt_));
        const int order = opt_.item_order_dev != 0 ? static_cast<int>(opt_.item_order_dev) : (wide_order_ != 0 ? wide_order_ : ITEM_ORDER);
        std::vector<WorkItem> items;  // the kernels read them as int2
        static_assert(sizeof(WorkItem) == sizeof(int2) && alignof(int2) % alignof(WorkItem) == 0 && offsetof(WorkItem, x) == offsetof(int2, x) && offsetof(WorkItem, y) == offsetof(int2, y));
        long max_records = 1;
        for (size_t k = 0; k + 1 < edge.size(); ++k) {
            Band band{};
            band.ib_begin = edge[k];
            band.ib_end = edge[k + 1];
            band.item_begin = static_cast<int>(items.size());
            band.pair_origin = pairs_below(band.ib_begin);
            for (const WorkItem &it : band_items(band.ib_begin, band.ib_end, jc_tiles_, num_jc_, order, pair_, jc_head_tiles_, jc_head_count_)) items.push_back({ it.x - ib_begin_, it.y });
            band.item_count = static_cast<int>(items.size()) - band.item_begin;
            // (block pairs: the records of the pair's SECOND block, which is padding behind an odd last block)
            max_records = std::max(max_records, pairs_below(pair_ ? round_up(band.ib_end, 2) : band.ib_end) - band.pair_origin);
            if (band.ib_end > band.ib_begin) bands_.push_back(band);
        }
        num_items_ = static_cast<int>(items.size());
        items_.alloc_zero(std::max<size_t>(items.size(), 1), st);
        if (!items.empty()) LSSVM_HIP_CHECK(hipMemcpyAsync(items_.p, items.data(), items.size() * sizeof(WorkItem), hipMemcpyHostToDevice, st));
        colslab_.alloc_zero(static_cast<size_t>(max_records) * TILE, st);
        LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // `items` goes out of scope
    }
    // (two matvecs can be in flight -- enqueue-ahead -- and each issues bands x feature-panel passes tile launches: ADVICE r03, the later panels of a wide
    // linear problem went untimed and the reported kernel time came out too low)
    // (created HERE: a reshard that needs one more band than before grows the list -- pairs without events would be handed out by free_event)
    events_.resize(4 * std::max<size_t>(bands_.size(), 1) * static_cast<size_t>(std::max(passes_per_matvec(), 1)));
    for (EvPair &e : events_) {
        if (e.a.e == nullptr) e.a.create(true);
        if (e.b.e == nullptr) e.b.create(true);
    }
}

/* New shares for the ranks of a sharded symmetric problem (lssvm_mi355_problem_rebalance): the row blocks of this shard, its work items, slabs and bands are
 * rebuilt for `weights`; the data, the operand planes, the vectors and the CG state are what they were -- the implicit matrix does not change, only who evaluates
 * which of its tiles.  The caller has drained the stream. */
template <typename T>
void Problem<T>::reshard(const std::vector<double> &weights) {
    LSSVM_REQUIRE(sym_ && world_ > 1 && static_cast<int>(weights.size()) == world_, "shares by weight exist for the symmetric variant of a sharded problem, one weight per rank");
    select_device_checked(device_);
    LSSVM_HIP_CHECK(hipStreamSynchronize(stream_.s));
    drain_events();
    opt_.shard_weights = weights;
    choose_shard_geometry();
    build_shard_lists(stream_.s);
    d_packed_ = false;  // (the records of d are shard independent, but K*v is cleared again by the next matvec: the plain path)
    pace_ms0_ = matvec_ms_;  // the pace of the NEW share is measured from here on; the counters lssvm_cg_info reports keep running
    pace_timed0_ = matvec_timed_;
    LSSVM_HIP_CHECK(hipStreamSynchronize(stream_.s));
}

template <typename T>
Problem<T>::Problem(const Options &opt, const lssvm_params &params, const void *X, int mem_kind, size_t num_points, size_t num_features, int device, int rank, int world) :
    opt_(opt), params_(params), device_(device), rank_(rank), world_(world) {
    check_params(&params_);
    LSSVM_REQUIRE(X != nullptr, "The data must not be empty!");                                           // csvm.cpp:73
    LSSVM_REQUIRE(num_points >= 2, "The data must contain at least two data points!");
    LSSVM_REQUIRE(num_features >= 1, "The data points must contain at least one feature!");               // csvm.cpp:74
    LSSVM_REQUIRE(num_points < (size_t(1) << 31) - 4 * TILE && num_features < (size_t(1) << 24), "problem too large for 32-bit tile indices");
    LSSVM_REQUIRE(mem_kind == LSSVM_MEM_HOST || mem_kind == LSSVM_MEM_DEVICE, "invalid mem_kind");
    LSSVM_REQUIRE(world_ >= 1 && rank_ >= 0 && rank_ < world_, "invalid shard descriptor");
    select_device_checked(device_);
    const double t0 = now_ms();
    stream_.create();
    hipStream_t st = stream_.s;
    const char *dbg_env = std::getenv("LSSVM_MI355_DEBUG");
    const bool dbg_laps = dbg_env != nullptr && dbg_env[0] == '1' && rank_ == 0;
    double t_lap = t0;
    auto lap = [&](const char *what) {  // LSSVM_MI355_DEBUG=1: where the set-up's time goes (the stream is drained at every lap, so the laps add up)
        if (!dbg_laps) return;
        (void) hipStreamSynchronize(st);
        const double t = now_ms();
        std::fprintf(stderr, "[plssvm_amd] set-up: %-44s %8.3f ms\n", what, t - t_lap);
        t_lap = t;
    };

    lap("stream");
    N_ = num_points;
    n_ = static_cast<int>(num_points - 1);
    num_tiles_ = (n_ + TILE - 1) / TILE;
    ib_per_rank_ = (num_tiles_ + world_ - 1) / world_;
    nvec_ = ib_per_rank_ * world_ * TILE;
    // data matrix: all N points (the last one is row n; it takes part in q and QA_cost only)
    // (+ TILE: an odd number of row blocks ends in a block pair whose second block is zero padding -- the 256-row workgroups read its rows, d_i and c_i)
    X_.upload(X, mem_kind, num_points, num_features, static_cast<size_t>(nvec_) + TILE, st);
    lap("data into the padded layout");
    // fp32 rbf: matrix cores (norm expansion) or the formula-exact vector-ALU kernel?  (every shard sees the same data: same decision)
    rbf_direct_ = rbf_wants_direct_form<T>(opt_, params_, X_, nullptr, st, &rbf_r2_);
    // Large exponent scales (round 5): between RBF_DIRECT_ABOVE and RBF_GRID_MAX_R2, at any width, with operand planes allowed, the matrix cores run the
    // rbf kernel on GRID planes (KT_RBFG, lssvm_tile_f32_split.hip.hpp) -- the direct form's accuracy at about twice the f16x3 time instead of five times.  A rule on
    // the data's scale, the shape and the options: every shard sees the same data and decides alike; predict_values takes the same decision.
    if constexpr (std::is_same_v<T, float>) {
        if (rbf_wants_grid_planes(opt_, params_, num_features, rbf_r2_)) {
            rbf_grid_ = true;
            rbf_direct_ = false;
        }
    }
    // symmetric variant: v2 kernels only; a negative polynomial degree can give inf on zero-padded rows -> full square
    const int ldx_probe = padded_features<T>(num_features);
    ldx_probe_ = ldx_probe;
    num_features_ = num_features;
    bool v2_ok = std::is_same_v<T, float> ? v2_eligible(opt_, ldx_probe, rbf_direct_) : v2_eligible_f64(opt_, ldx_probe);
    // FEW points, many features, linear kernel (fp32): the feature-panel passes below are launch-bound there -- 3 000 x 16 384: 128 passes 4.75 ms, the
    // polynomial kernel's ONE launch over the same panels 2.89 (profiles/r04_very_wide_probe.log).  Below LINEAR_IN_TILE_BELOW points and beyond 256
    // features the tile kernels therefore run the linear kernel AS the polynomial kernel of degree 1 with gamma = 1, coef0 = 0: K_ij = (1 * acc + 0)^1,
    // bit for bit the linear kernel's value (the planes' power-of-two pre-scale is undone inside gamma, exactly); above, the passes win (twice the
    // matrix-core rate of the panels-inside-a-tile kernels).  q, QA_cost and the data preparation keep the caller's kernel (params_); a rule on the
    // shape and the options only, so every rank of a sharded solve decides alike.
    tile_params_ = params_;
    if constexpr (std::is_same_v<T, float>) {
        if (params_.kernel_type == LSSVM_KERNEL_LINEAR && opt_.gram_mode != 0 && opt_.tile_kernel != 1 && round_up(static_cast<long>(num_features), 64) > 256
            && n_ < LINEAR_IN_TILE_BELOW) {
            tile_params_.kernel_type = LSSVM_KERNEL_POLYNOMIAL;
            tile_params_.degree = 1;
            tile_params_.gamma = 1.0;
            tile_params_.coef0 = 0.0;
        }
    }
    if constexpr (std::is_same_v<T, float>) {
        // linear kernel on more than 512 features: K*v = sum over feature panels of (X_p X_p^T) v, every panel one launch of the f16x3 kernels
        // (enqueue_apply_K_local).  Whether the data allows f16 planes decides it, so the planes are built HERE (the linear kernel needs the raw data).
        if (tile_params_.kernel_type == LSSVM_KERNEL_LINEAR && opt_.gram_mode >= 2 && opt_.tile_kernel != 1
            && round_up(static_cast<long>(num_features), 64) > LINEAR_PANEL_FEATURES) {
            if (opt_.symmetric != 0 && opt_.colslab_limit_mb != 0) {  // (the panel passes exist for the symmetric variant: no probe, no planes otherwise)
                make_planes(opt_, tile_params_, false, X_, nullptr, planes_, nullptr, st, false, true);
                if (planes_.mode == 2) {
                    v2_ok = wide_linear_ = true;
                } else {
                    f16_probe_failed_ = true;  // (the planes of the one-pass kernels below do not repeat the split and the check)
                    planes_.buf.release();
                    planes_.mode = 0;
                }
            }
        }
    }
    if constexpr (std::is_same_v<T, double>) {
        // fp64 linear kernel on more than 256 features (the widest row panel the resident-row-panel kernel holds): the same sum over feature
        // panels, one pass of that kernel per panel of 128 features (a remainder of 1 ... 8 sixteen-feature chunks always has its instantiation)
        // -- the symmetric variant instead of the generic full-square kernel: 40 000 x 512 35.1 -> 12.3 ms per iteration, 20 000 x 2 000
        // 34.2 -> 13.4 ms.  The panel width hardly matters (64 and 256 measure within 2 %: the linear epilogue is two fmas per element);
        // up to 256 features the one pass stays.
        if (params_.kernel_type == LSSVM_KERNEL_LINEAR && opt_.tile_kernel != 1 && opt_.symmetric != 0 && opt_.colslab_limit_mb != 0 && ldx_probe > F64_ONE_PASS_FEATURES) {
            v2_ok = wide_linear_ = true;
        }
        // rbf / polynomial beyond 256 features: the panels inside a sub-tile, either variant
        if (wide_nonlinear_f64(opt_, params_, num_features)) v2_ok = wide_nl_ = true;
    }
    if constexpr (std::is_same_v<T, float>) {
        // rbf / polynomial on more features than the row panel of the split kernels holds in registers (f16x3: 384 rbf, 512 polynomial; bf16x6:
        // 384): feature panels of 128 walked inside a tile (lssvm_tile_f32_wide.hip.hpp), either variant, either plane kind -- decided from
        // the shape and the options alone, so every rank of a sharded solve decides alike.  (The linear kernel has its panel passes above.)
        if (wide_nonlinear(opt_, tile_params_, rbf_direct_, num_features)) v2_ok = wide_nl_ = true;
    }
    sym_ = opt_.symmetric != 0 && v2_ok && !(tile_params_.kernel_type == LSSVM_KERNEL_POLYNOMIAL && tile_params_.degree < 0);
    // the symmetric variant keeps one 128-entry record per evaluated off-diagonal tile of the row-block BAND in flight (see the bands
    // below); colslab_limit_mb = 0 switches the variant off (a rule in the options only, so every rank of a sharded solve decides alike)
    if (sym_ && opt_.colslab_limit_mb == 0) sym_ = false;
    if constexpr (std::is_same_v<T, float>) {
        // 256-row workgroups on block pairs (lssvm_tile_f32_pair.hip.hpp): the symmetric variant of the split kernels on at most 128 features per
        // pass with a hand-scheduled epilogue -- decided from the shape and the options alone (both plane kinds have the kernel), so that the
        // geometry below does not wait for the planes and every rank of a sharded solve decides alike
        const bool poly_generic = tile_params_.kernel_type == LSSVM_KERNEL_POLYNOMIAL && tile_params_.degree != 2 && tile_params_.degree != 3;
        const bool narrow = wide_linear_ ? true : (round_up(static_cast<long>(num_features), 64) <= 128 && v2_eligible(opt_, ldx_probe, rbf_direct_));
        // (rbf: that kernel folds BOTH exponent terms out of the chain -- only while |c| = R2 / 2 stays small and the folded records are on)
        // (round 6: rbf on GRID planes has its 256-row form too -- start values instead of folded terms, so neither condition applies to it)
        const bool rbf_ok = tile_params_.kernel_type != LSSVM_KERNEL_RBF || rbf_grid_ || (opt_.rbf_fold != 0 && rbf_r2_ <= 2.0 * PAIR_FOLD_MAX_C);
        // (below 64 row blocks -- 8 192 points -- the 128-row workgroups have more items to spread over the chip: 3 000 points 13.8 against 19.7 us)
        pair_ = sym_ && opt_.gram_mode != 0 && opt_.mfma_shape >= 3 && !wide_nl_ && !poly_generic && narrow && rbf_ok && num_tiles_ >= PAIR_MIN_TILES;
    }
    lap("exponent scale, path decisions");
    choose_shard_geometry();
    lap("shard geometry (chunk choice by replay)");
    // 256-row workgroups: PERSISTENT launches, the work items drawn from per-XCD counters (for_each_work_item, lssvm_device_common.hip.hpp) instead of one workgroup per
    // item dealt by the hardware -- whose deal is static per XCD (every eighth workgroup, whatever the XCD's pace: the eight clocks of one chip differ by 3-5 %) and in
    // order.  Same box, interleaved, bit-identical: 1 000 000 x 128 rbf 264.9 -> 256.8 ms per iteration (-3.0 %), 200 000 x 256 linear 20.05 -> 19.49 (-3.0 %),
    // 50 000 x 128 unchanged (profiles/r05_ab_pair_queue.log).  LSSVM_MI355_PAIR_QUEUE=0 in the environment: the former launches (A/B runs).
    if (const char *pq = std::getenv("LSSVM_MI355_PAIR_QUEUE"); pair_ && !(pq != nullptr && pq[0] == '0')) {
        queue_.alloc_zero(512, st);
        LSSVM_HIP_CHECK(hipDeviceGetAttribute(&queue_min_items_, hipDeviceAttributeMultiprocessorCount, device_));
    }
    inv_cost_ = static_cast<double>(T(1) / static_cast<T>(params_.cost));  // "1 / params.cost" in real_type, csvm.cpp:297

    // QA_cost = k(x_last, x_last) + 1/C, evaluated on the host in the real type (csvm.cpp:86)
    std::vector<T> last(num_features);
    LSSVM_HIP_CHECK(hipMemcpyAsync(last.data(), X_.data.p + static_cast<size_t>(n_) * X_.ldx, num_features * sizeof(T), hipMemcpyDeviceToHost, st));
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    self_last_ = static_cast<double>(host_self_kernel<T>(params_, last));
    QA_cost_ = static_cast<double>(static_cast<T>(self_last_) + T(1) / static_cast<T>(params_.cost));

    // vectors (zero padded to nvec_)
    for (DevBuf<T> *v : { &q_, &Kv_, &tmp_ }) v->alloc_zero(static_cast<size_t>(nvec_) + TILE, st);
    Kres_ = Kv_.p;
    own_.alloc(static_cast<size_t>(nvec_) + TILE, num_points, false, st);

    lap("QA_cost, vectors");
    // q from the raw (un-centred) data: bit-compatible fma chains (q_kernel.cpp:18-55)
    {
        const T *xlast = X_.data.p + static_cast<size_t>(n_) * X_.ldx;
        const dim3 grid((n_ + 127) / 128), block(128);
        const T g = static_cast<T>(params_.gamma), c0 = static_cast<T>(params_.coef0);
        switch (params_.kernel_type) {
            case LSSVM_KERNEL_LINEAR: hipLaunchKernelGGL((k_q<KT_LINEAR, T>), grid, block, 0, st, X_.data.p, X_.ldx, X_.dfeat, n_, xlast, params_.degree, g, c0, q_.p); break;
            case LSSVM_KERNEL_POLYNOMIAL: hipLaunchKernelGGL((k_q<KT_POLY, T>), grid, block, 0, st, X_.data.p, X_.ldx, X_.dfeat, n_, xlast, params_.degree, g, c0, q_.p); break;
            default: hipLaunchKernelGGL((k_q<KT_RBF, T>), grid, block, 0, st, X_.data.p, X_.ldx, X_.dfeat, n_, xlast, params_.degree, g, c0, q_.p); break;
        }
        LSSVM_HIP_CHECK(hipGetLastError());
    }
    lap("q");
    // rbf on the matrix cores: centre the data, then c_i = -|x_i|^2 / 2
    if (params_.kernel_type == LSSVM_KERNEL_RBF && !rbf_direct_) {
        const T prescale = rbf_prescale<T>(params_, v2_eligible_f64(opt_, X_.ldx) || wide_nl_);
        center_columns<T>(X_, nullptr, prescale, st);
        x_scale_ = static_cast<double>(prescale);
        half_neg_norms<T>(X_, c_, st);
    }
    lap("centring, norms");
    // polynomial in fp64 on the v2 kernel: fold gamma into the data (x' = sqrt(gamma) x, after q was computed from the raw data), so
    // that the MFMA chain leaves gamma * <x_i, x_j> and the epilogue is the bare integer power -- every vector ALU instruction
    // beside v_mfma_f64 costs matrix-core time (gamma > 0 is a precondition of the kernel, parameter.hpp / csvm.cpp:77)
    if constexpr (std::is_same_v<T, double>) {
        if (params_.kernel_type == LSSVM_KERNEL_POLYNOMIAL && (v2_eligible_f64(opt_, X_.ldx) || wide_nl_) && params_.gamma > 0.0) {
            hipLaunchKernelGGL(k_center<T>, dim3((X_.dfeat + 255) / 256, X_.rows), dim3(256), 0, st, X_.data.p, X_.ldx, X_.dfeat, X_.rows,
                               static_cast<const T *>(nullptr), static_cast<T>(std::sqrt(params_.gamma)));
            LSSVM_HIP_CHECK(hipGetLastError());
            poly_prescaled_ = true;
            x_scale_ = static_cast<double>(static_cast<T>(std::sqrt(params_.gamma)));
        }
    }
    if constexpr (std::is_same_v<T, float>) {
        // the (centred, scaled) data once more as operand planes of the split kernels (features in natural order): see make_planes
        if (rbf_grid_) {
            grid_sigma_ = make_grid_planes(X_, rbf_r2_, planes_, c_.p, efac_, st, wide_nl_);
        } else if (!wide_linear_) make_planes(opt_, tile_params_, rbf_direct_, X_, nullptr, planes_, nullptr, st, wide_nl_, false, f16_probe_failed_);
        f16_row_rel_error_ = planes_.f16_row_rel_error;
        row_scaled_ = planes_.row_inv_scale.p != nullptr;
        if (row_scaled_) vs_.alloc_zero(static_cast<size_t>(nvec_) + TILE, st);
        if ((wide_nl_ || pair_) && planes_.mode == 0) throw Error(LSSVM_ERR_INTERNAL, "no operand planes for a path that was chosen from the shape alone");
        if ((wide_nl_ && sym_) || pair_) {
            // the row side of the panels-inside-a-tile kernel: the planes once more, every 16 x 32 block stored as the A fragment a wave loads
            // (lssvm_tile_f32_wide.hip.hpp: the row fragments are re-loaded at every tile-panel -- whole cache lines instead of half lines);
            // the 256-row workgroups load a work item's row panel from it (1 KiB contiguous per load instruction instead of 64 bytes of each of 16 rows)
            const size_t plane_elems = static_cast<size_t>(X_.rows_alloc) * planes_.ldx16;
            planes_frag_.alloc_zero(static_cast<size_t>(planes_.nplanes) * plane_elems, st);
            const size_t pieces = static_cast<size_t>(planes_.nplanes) * X_.rows_alloc * (planes_.ldx16 / 8);
            hipLaunchKernelGGL(k_planes_fragment_major, dim3(static_cast<unsigned>((pieces + 255) / 256)), dim3(256), 0, st, planes_.buf.p, plane_elems, static_cast<int>(X_.rows_alloc), planes_.ldx16,
                               planes_.nplanes, planes_frag_.p);
            LSSVM_HIP_CHECK(hipGetLastError());
        }
        // rbf: folded records while the exponent terms stay small (rbf_r2_ = 2 max|c| in the exponent's unit)
        if (planes_.mode != 0) dc_folded_ = tile_params_.kernel_type == LSSVM_KERNEL_RBF && opt_.rbf_fold != 0 && rbf_r2_ <= FOLD_MAX_R2 && !rbf_grid_;
    }
    lap("operand planes, fragment-major copy");
    interleave_features<T>(X_, st);
    if constexpr (std::is_same_v<T, double>) {
        if (wide_nl_ && sym_) {
            // the row side of the fp64 panels-inside-a-sub-tile kernel: the (prepared) data once more, every 16 x 4 block stored as the A fragment a wave
            // loads (lssvm_tile_f64_wide.hip.hpp) -- after every in-place transformation of X_ above
            Xfrag_.alloc_zero(static_cast<size_t>(X_.rows_alloc) * X_.ldx, st);
            const size_t elems = static_cast<size_t>(X_.rows_alloc) * X_.ldx;
            hipLaunchKernelGGL(k_rows_fragment_major_f64, dim3(static_cast<unsigned>((elems + 255) / 256)), dim3(256), 0, st, X_.data.p, static_cast<int>(X_.rows_alloc), X_.ldx, Xfrag_.p);
            LSSVM_HIP_CHECK(hipGetLastError());
        }
    }
    if ((std::is_same_v<T, float> && (v2_eligible(opt_, X_.ldx, rbf_direct_) || wide_linear_ || wide_nl_)) || (std::is_same_v<T, double> && (v2_eligible_f64(opt_, X_.ldx) || wide_linear_ || wide_nl_))) {
        dc_.alloc_zero(static_cast<size_t>(std::max(num_tiles_, 1)) * 256, st);  // (d_j | c_j) records: 256 reals per 128 columns
    }
    lap("interleave, records");
    build_shard_lists(st);
    lap("work-item lists, slabs, events");
    ev_ready_.create(false);
    ev_consumed_.create(false);
    LSSVM_HIP_CHECK(hipStreamSynchronize(st));
    setup_ms_ = now_ms() - t0;
}

template <typename T>
Problem<T>::~Problem() {
    (void) hipSetDevice(device_);
    if (stream_.s != nullptr) (void) hipStreamSynchronize(stream_.s);
    // members release themselves (events, pinned words, device buffers, then the stream)
}

template <typename T>
TileArgs<T> Problem<T>::tile_args(const T *v_dev) const {
    TileArgs<T> a{};
    a.Xr = X_.data.p;
    a.Xrf = Xfrag_.p;
    a.frag_rows16 = static_cast<int>(X_.rows_alloc / 16);
    a.Xc = X_.data.p;
    a.cr = c_.p;
    a.cc = c_.p;
    a.dvec = v_dev;
    a.dc = dc_.p;
    a.items = sym_ ? items_.p : nullptr;  // (the symmetric variant launches band by band: enqueue_apply_K_local offsets these two)
    a.num_items = num_items_;
    a.colslab = colslab_.p;
    a.pair_origin = 0;
    a.partial = partial_.p;
    a.part_stride = static_cast<long>(part_blocks()) * TILE;
    a.ldx = X_.ldx;
    a.kchunks = X_.ldx / kchunk_of<T>();
    a.ib_begin = ib_begin_;
    a.num_ib = num_ib_;
    a.num_jt = num_tiles_;
    a.jc_tiles = jc_tiles_;
    a.jc_head_tiles = jc_head_tiles_;
    a.jc_head_count = jc_head_count_;
    a.ncols_valid = n_;
    set_kernel_scalars(a, tile_params_, rbf_direct_);
    if (rbf_grid_) {
        a.gamma = static_cast<T>(1.0 / (static_cast<double>(grid_sigma_) * static_cast<double>(grid_sigma_)));  // the chain carries sigma^2 t
        a.er = efac_.p;
        a.rbf_grid = 1;
    }
    if (poly_prescaled_) a.gamma = T(1);
    if constexpr (std::is_same_v<T, float>) {
        a.Xr16f = planes_frag_.p;
        if (planes_.mode != 0) set_plane_args(a, tile_params_, planes_, planes_, static_cast<size_t>(X_.rows_alloc), static_cast<size_t>(X_.rows_alloc));
    }
    a.wide_panels = wide_nl_ ? 1 : 0;
    set_launch_options(a, opt_);
    a.row_pair = pair_ ? 1 : 0;
    a.dc_folded = dc_folded_ ? 1 : 0;
    return a;
}

template <typename T>
void Problem<T>::drain_events() {
    for (EvPair &e : events_) {
        if (e.pending && hipEventQuery(e.b.e) == hipSuccess) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, e.a.e, e.b.e) == hipSuccess) {
                matvec_ms_ += ms;  // the band launches of one matvec add up; the matvec is counted once
                if (e.first_of_matvec) ++matvec_timed_;
            }
            e.pending = false;
        }
    }
}

/* the single-vector records of a problem's pass: rbf on grid planes carries E_j, the other forms the folded or plain (d_j | c_j) */
template <typename T>
void Problem<T>::enqueue_pack_dc(const T *v, T *zero, int nzero) {
    const int ncols = num_tiles_ * TILE;
    const int nthreads = std::max(ncols, nzero);
    if constexpr (std::is_same_v<T, float>) {
        hipLaunchKernelGGL(k_pack_dc, dim3((nthreads + 255) / 256), dim3(256), 0, stream_.s, v, c_.p, ncols, dc_.p, rbf_grid_ ? 2 : (dc_folded_ ? 1 : 0), zero, nzero, rbf_grid_ ? efac_.p : static_cast<const float *>(nullptr));
    } else {
        hipLaunchKernelGGL(k_pack_dc_f64, dim3((nthreads + 255) / 256), dim3(256), 0, stream_.s, v, c_.p, ncols, dc_.p, zero, nzero);
    }
}

template <typename T>
template <typename Around>
void Problem<T>::enqueue_sym_walk(const TileArgs<T> &a, int nv, T *const *Kv, int npanels, Around &&around) {
    hipStream_t st = stream_.s;
    const int nrows = num_ib_ * TILE;
    // wide linear problems: one pass per panel of LINEAR_PANEL_FEATURES features, every pass ADDS its K_p * v (rows and mirrored columns) into K*v
    const int panel_features = LINEAR_PANEL_FEATURES;
    for (int panel = 0; panel < npanels; ++panel) {
        TileArgs<T> ap = a;
        if constexpr (std::is_same_v<T, float>) {
            if (wide_linear_) {
                if (ap.Xr16f != nullptr) ap.Xr16f += static_cast<size_t>(panel) * (panel_features / 64) * (X_.rows_alloc / 16) * 1024;  // (the 64-feature chunk is the outermost index of a plane)
                ap.Xr16 += static_cast<size_t>(panel) * panel_features;
                ap.Xc16 += static_cast<size_t>(panel) * panel_features;
                ap.nk64 = std::min(panel_features, planes_.ldx16 - panel * panel_features) / 64;
            }
        } else {
            if (wide_linear_) {  // (row-major fp64 data: a panel is a column range of X, the row stride stays)
                ap.Xr += static_cast<size_t>(panel) * panel_features;
                ap.Xc += static_cast<size_t>(panel) * panel_features;
                ap.kchunks = std::min(panel_features, X_.ldx - panel * panel_features) / F64_KC;
            }
        }
        for (const Band &band : bands_) {
            TileArgs<T> ab = ap;
            ab.items = items_.p + band.item_begin;
            ab.num_items = band.item_count;
            ab.pair_origin = band.pair_origin;
            if (queue_.p != nullptr && band.item_count > queue_min_items_) {  // (a launch of no more items than CUs: one workgroup per item, no counters -- 2 % faster there)
                ab.queue = queue_.p + 256 * queue_set_;
                ab.queue_next = queue_.p + 256 * (1 - queue_set_);
                ab.queue_grid = queue_min_items_;
                queue_set_ ^= 1;
            }
            around([&]() { launch_tile_kernel<T>(ab, tile_params_.kernel_type, rbf_direct_, num_jc_, st); }, panel == 0 && &band == &bands_.front(), panel == npanels - 1 && &band == &bands_.back());
            // fold the band's mirrored column sums into K*v before the next band re-uses the slab
            if (band.ib_end > 1) {
                for (int u = 0; u < nv; ++u) {
                    if constexpr (std::is_same_v<T, float>) {
                        // (block pairs: one record per pair and column tile, kept as the record of the pair's second -- odd -- block)
                        hipLaunchKernelGGL((k_reduce_colslab<T, 128>), dim3(band.ib_end - 1), dim3(1024), 0, st, a.colslab + u * a.colslab_vstride, band.pair_origin, band.ib_begin, pair_ ? round_up(band.ib_end, 2) : band.ib_end, pair_ ? 2 : 1, Kv[u], rbf_grid_ ? efac_.p : static_cast<const T *>(nullptr));
                    } else {  // fp64: records per 64-column sub-tile
                        hipLaunchKernelGGL((k_reduce_colslab<T, 64>), dim3(2 * (band.ib_end - 1)), dim3(1024), 0, st, a.colslab + u * a.colslab_vstride, band.pair_origin, band.ib_begin, band.ib_end, 1, Kv[u]);
                    }
                }
            }
        }
        // rows of this device's blocks: the slabs of the column chunks that exist for each block, added on top
        for (int u = 0; u < nv; ++u) {
            hipLaunchKernelGGL(k_reduce_partials_sym<T>, dim3((nrows + 255) / 256), dim3(256), 0, st, a.partial + u * a.part_vstride, a.part_stride, jc_tiles_, jc_head_tiles_, jc_head_count_, ib_begin_, nrows, Kv[u], 1);
        }
    }
}

template <typename T>
void Problem<T>::enqueue_apply_K_local(const T *v_dev, bool zero_first) {
    // this shard's part of the implicit K * v: tile kernel over its row blocks (band by band), slabs added in a fixed order
    hipStream_t st = stream_.s;
    // sampled matvecs: every `stride`-th, starting with the LAST of each run of `stride`, plus launches 1 ... 4 (a run of a few iterations still reports a
    // kernel time; no more than four: the first launches of a solve run a few per cent slow and would weigh on the average of a run of a hundred) -- never launch 0, the cold first matvec of cg_begin, which would otherwise carry `stride` times its weight in the average
    const uint64_t stride = static_cast<uint64_t>(event_stride());
    const bool timed = matvec_launches_ != 0 && (matvec_launches_ % stride == stride - 1 || matvec_launches_ <= 4);  // (short runs: every one of the first four after launch 0)
    ++matvec_launches_;
    auto free_event = [&]() -> EvPair * {
        if (!timed) return nullptr;
        for (int attempt = 0; attempt < 2; ++attempt) {
            for (EvPair &e : events_) {
                if (!e.pending) return &e;
            }
            drain_events();
        }
        return nullptr;
    };
    // symmetric variant: row sums of the device's blocks and the mirrored column sums of every band are ADDED into K*v (and, sharded, every rank
    // adds into all earlier rows): start from zero -- by the kernel that packs the records where there is one, by a memset otherwise
    const bool clear = zero_first || sym_;
    if constexpr (std::is_same_v<T, float>) {
        if (row_scaled_) {  // K v = D (Xs Xs^T) (D v): the tile kernels see D v (make_planes: a power-of-two scale per row)
            hipLaunchKernelGGL(k_scale_vector, dim3((nvec_ + 255) / 256), dim3(256), 0, st, v_dev, planes_.row_inv_scale.p, nvec_, vs_.p);
            v_dev = vs_.p;
        }
    }
    const bool prepacked = d_packed_ && v_dev == own_.d.p;  // k_update_d has left the records of the own state's d and cleared K*v (pack_for_d)
    d_packed_ = false;                                  // (either they are consumed now, or dc_ is about to hold another vector's)
    const bool pack = dc_.p != nullptr && num_ib_ > 0 && !prepacked;
    if (clear && !pack && !prepacked) LSSVM_HIP_CHECK(hipMemsetAsync(Kv_.p, 0, static_cast<size_t>(nvec_) * sizeof(T), st));
    if (num_ib_ <= 0) return;
    TileArgs<T> a = tile_args(v_dev);
    if (pack) enqueue_pack_dc(v_dev, Kv_.p, clear ? static_cast<int>(nvec_) : 0);  // v2 kernels: (d_j | c_j) records for the LDS-DMA
    if (sym_) {
        T *const Kv[1] = { Kv_.p };
        // (sampled events around every band launch of every feature panel; the matvec is counted once, at its first launch)
        enqueue_sym_walk(a, 1, Kv, passes_per_matvec(), [&](auto &&launch, bool first, bool) {
            EvPair *ev = free_event();
            if (ev != nullptr) LSSVM_HIP_CHECK(hipEventRecord(ev->a.e, st));
            launch();
            if (ev != nullptr) {
                LSSVM_HIP_CHECK(hipEventRecord(ev->b.e, st));
                ev->pending = true;
                ev->first_of_matvec = first;
            }
        });
    } else {
        EvPair *ev = free_event();
        if (ev != nullptr) LSSVM_HIP_CHECK(hipEventRecord(ev->a.e, st));
        launch_tile_kernel<T>(a, tile_params_.kernel_type, rbf_direct_, num_jc_, st);
        if (ev != nullptr) {
            LSSVM_HIP_CHECK(hipEventRecord(ev->b.e, st));
            ev->pending = true;
            ev->first_of_matvec = true;
        }
        const int nrows = num_ib_ * TILE;
        hipLaunchKernelGGL(k_reduce_partials<T>, dim3((nrows + 255) / 256), dim3(256), 0, st, partial_.p, a.part_stride, num_jc_, ib_begin_ * TILE, nrows, Kv_.p);
    }
    if constexpr (std::is_same_v<T, float>) {
        // (every entry this shard has added into: the symmetric variant mirrors into the rows of earlier blocks too; a sharded solve exchanges the scaled partial vectors)
        if (row_scaled_) hipLaunchKernelGGL(k_scale_vector, dim3((nvec_ + 255) / 256), dim3(256), 0, st, Kv_.p, planes_.row_inv_scale.p, nvec_, Kv_.p);
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}

/* The records of the NEXT implicit matvec -- always K * d in the CG loop -- are packed by the kernel that updates d (k_update_d) instead of a k_pack_dc launch
 * in front of the tile kernel: what that kernel needs, and the note that it has been done.  `zero_first` as enqueue_apply_K_local's. */
template <typename T>
PackDc<T> Problem<T>::pack_for_d(bool zero_first) {
    PackDc<T> pk;
    if (dc_.p == nullptr || num_ib_ <= 0 || row_scaled_) return pk;  // (row-scaled planes: the records are those of D d, packed per matvec)
    pk.dc = dc_.p;
    pk.cc = c_.p;
    pk.ncols = num_tiles_ * TILE;
    pk.zero = Kv_.p;
    pk.nzero = (zero_first || sym_) ? static_cast<int>(nvec_) : 0;
    if constexpr (std::is_same_v<T, float>) {
        pk.folded = rbf_grid_ ? 2 : (dc_folded_ ? 1 : 0);
        pk.efac = rbf_grid_ ? efac_.p : nullptr;
    }
    d_packed_ = true;
    return pk;
}

/* ------------------------------------------------------------------ lanes ------------------------------------------------------------------ */
template <typename T>
CgState<T> &Problem<T>::lane(size_t k) {
    activate();
    while (lanes_.size() <= k) {
        lanes_.push_back(std::make_unique<CgState<T>>());
        lanes_.back()->alloc(static_cast<size_t>(nvec_) + TILE, N_, true, stream_.s);  // (as the problem's own vectors)
    }
    return *lanes_[k];
}

/* The (kernel function, chunk count) instantiations of the two-vector kernel that are dispatched: those whose pass was measured to take less than two single-vector
 * passes by more than the single-vector kernel's own run-to-run spread (tests/tools/lockstep_timing.py, profiles/lockstep_f64.json).  All 60 do: 0.507 ... 0.596 of two
 * passes at 30 000 points, the worst ratio + spread 0.667 (linear, one chunk) -- an instantiation that stops doing so is named here and falls back to two single passes. */
static bool pair_kernel_routed(int /*kernel_type*/, int /*degree*/, int /*kchunks*/) {
    return true;
}

template <typename T>
bool Problem<T>::pair_kernel_applies() const {
    if constexpr (std::is_same_v<T, double>) {
        return world_ == 1 && sym_ && dc_.p != nullptr && !wide_nl_ && !wide_linear_ && num_ib_ > 0
               && pair_kernel_routed(tile_params_.kernel_type, tile_params_.degree, X_.ldx / F64_KC);
    } else {
        // the symmetric one-pass 128-row split kernels beyond 128 features: the polynomial forms (the linear kernel where it runs as the polynomial of degree 1) and
        // rbf with folded records -- the forms s6w_body<..., SYM, ..., NV = 2> has
        const bool poly = tile_params_.kernel_type == LSSVM_KERNEL_POLYNOMIAL && tile_params_.degree >= 0;
        const bool rbf_folded = tile_params_.kernel_type == LSSVM_KERNEL_RBF && dc_folded_;
        return world_ == 1 && sym_ && dc_.p != nullptr && num_ib_ > 0 && !pair_ && !wide_nl_ && !wide_linear_ && !rbf_direct_ && !rbf_grid_ && !row_scaled_
               && (planes_.mode == 1 || planes_.mode == 2) && planes_.ldx16 / 64 >= 3 && (poly || rbf_folded)
               && sym_pair_routed(planes_.mode, tile_params_.kernel_type, tile_params_.degree, planes_.ldx16 / 64);
    }
}

template <typename T>
void Problem<T>::enqueue_apply_K_lanes(const T *v0, T *Kv0, const T *v1, T *Kv1, hipEvent_t ev_begin, hipEvent_t ev_end) {
    LSSVM_REQUIRE(pair_kernel_applies(), "no two-vector tile kernel on this problem");
    hipStream_t st = stream_.s;
    const int nzero = static_cast<int>(nvec_);  // (the symmetric variant ADDS rows and mirrored columns into K*v)
    TileArgs<T> a = tile_args(v0);
    if (v1 != nullptr) {
        if (pair_dc_.p == nullptr) {
            // fp64: (d0_j | d1_j | c_j), 192 reals per 64-column sub-tile; fp32: (w0_j | w1_j | e_j), 384 per column tile (folded rbf; the polynomial forms use 256 of them)
            pair_dc_.alloc_zero(static_cast<size_t>(num_tiles_) * 2 * 192, st);
            pair_partial_.alloc_zero(2 * partial_.count, st);
            pair_colslab_.alloc_zero(2 * colslab_.count, st);
        }
        const int ncols = num_tiles_ * TILE;
        const int nthreads = std::max(ncols, nzero);
        if constexpr (std::is_same_v<T, float>) {
            hipLaunchKernelGGL(k_pack_dc2_sym, dim3((nthreads + 255) / 256), dim3(256), 0, st, v0, v1, c_.p, ncols, pair_dc_.p, a.dc_folded, Kv0, Kv1, nzero);
        } else {
            hipLaunchKernelGGL(k_pack_dc2_f64, dim3((nthreads + 255) / 256), dim3(256), 0, st, v0, v1, c_.p, ncols, pair_dc_.p, Kv0, Kv1, nzero);
        }
        a.nvec = 2;
        a.dvec1 = v1;
        a.dc = pair_dc_.p;
        a.partial = pair_partial_.p;
        a.part_vstride = static_cast<long>(partial_.count);
        a.colslab = pair_colslab_.p;
        a.colslab_vstride = static_cast<long>(colslab_.count);
    } else {
        d_packed_ = false;  // (dc_ is about to hold another vector's records)
        enqueue_pack_dc(v0, Kv0, nzero);
    }
    T *const Kv[2] = { Kv0, Kv1 };
    if (ev_begin != nullptr) LSSVM_HIP_CHECK(hipEventRecord(ev_begin, st));
    // every reduction runs per vector on that vector's planes, into that vector's K*v (no feature panels where the pair kernel applies)
    enqueue_sym_walk(a, v1 != nullptr ? 2 : 1, Kv, 1, [&](auto &&launch, bool, bool last) {
        launch();
        if (last && ev_end != nullptr) LSSVM_HIP_CHECK(hipEventRecord(ev_end, st));
    });
    LSSVM_HIP_CHECK(hipGetLastError());
}

/* Weighted LS-SVM: Abar(w)_ij = k(x_i,x_j) + delta_ij / (C w_i) + QA_cost(w) - q_i - q_j with QA_cost(w) = k(x_last,x_last) + 1 / (C w_last).  Every diagonal term is
 * formed as inv_cost_ is, in the real type -- so w = 1 gives today's bits, and w = 2 those of the unweighted system at cost 2C (T(C) * T(2) is exact). */
template <typename T>
void Problem<T>::set_weights(const double *weights) {
    const T cost = static_cast<T>(params_.cost);
    if (weights == nullptr) {
        weighted_ = false;
        inv_cw_.release();
        QA_cost_ = static_cast<double>(static_cast<T>(self_last_) + T(1) / cost);
        return;
    }
    std::vector<double> inv(static_cast<size_t>(nvec_) + TILE, inv_cost_);
    for (int i = 0; i < n_; ++i) inv[static_cast<size_t>(i)] = static_cast<double>(T(1) / (cost * static_cast<T>(weights[i])));
    activate();
    if (inv_cw_.p == nullptr) inv_cw_.alloc_zero(inv.size(), stream_.s);
    LSSVM_HIP_CHECK(hipMemcpyAsync(inv_cw_.p, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice, stream_.s));
    LSSVM_HIP_CHECK(hipStreamSynchronize(stream_.s));
    QA_cost_ = static_cast<double>(static_cast<T>(self_last_) + T(1) / (cost * static_cast<T>(weights[n_])));
    weighted_ = true;
}

template class Problem<float>;
template class Problem<double>;

/* ------------------------------------------------------------------ shared with lssvm_predict.hip ------------------------------------------------------------------ */
template float rbf_prescale<float>(const lssvm_params &, bool);
template double rbf_prescale<double>(const lssvm_params &, bool);
template void center_columns<float>(DeviceMatrix<float> &, DeviceMatrix<float> *, float, hipStream_t);
template void center_columns<double>(DeviceMatrix<double> &, DeviceMatrix<double> *, double, hipStream_t);
template void half_neg_norms<float>(const DeviceMatrix<float> &, DevBuf<float> &, hipStream_t);
template void half_neg_norms<double>(const DeviceMatrix<double> &, DevBuf<double> &, hipStream_t);
template void interleave_features<float>(DeviceMatrix<float> &, hipStream_t);
template void interleave_features<double>(DeviceMatrix<double> &, hipStream_t);
template void set_kernel_scalars<float>(TileArgs<float> &, const lssvm_params &, bool);
template void set_kernel_scalars<double>(TileArgs<double> &, const lssvm_params &, bool);
template void set_launch_options<float>(TileArgs<float> &, const Options &);
template void set_launch_options<double>(TileArgs<double> &, const Options &);
template void column_means<float>(const DeviceMatrix<float> &, DevBuf<float> &, hipStream_t);
template void column_means<double>(const DeviceMatrix<double> &, DevBuf<double> &, hipStream_t);
template double max_centred_sqnorm<float>(const DeviceMatrix<float> &, const DevBuf<float> &, hipStream_t);
template double max_centred_sqnorm<double>(const DeviceMatrix<double> &, const DevBuf<double> &, hipStream_t);
template bool rbf_wants_direct_form<float>(const Options &, const lssvm_params &, const DeviceMatrix<float> &, const DeviceMatrix<float> *, hipStream_t, double *);
template bool rbf_wants_direct_form<double>(const Options &, const lssvm_params &, const DeviceMatrix<double> &, const DeviceMatrix<double> *, hipStream_t, double *);

/* the set-up kernels that are no templates live in this translation unit (LSSVM_KERNELS_SETUP): the predict path enqueues them through these */
void enqueue_pack_records(const float *dvec, const float *cc, int ncols_padded, float *dc, int folded, const float *efac, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_dc, dim3((ncols_padded + 255) / 256), dim3(256), 0, s, dvec, cc, ncols_padded, dc, folded, static_cast<float *>(nullptr), 0, efac);
    LSSVM_HIP_CHECK(hipGetLastError());
}
void enqueue_pack_records2(const float *dvec0, const float *dvec1, const float *cc, int ncols_padded, float *dc, int folded, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_dc2, dim3((ncols_padded + 255) / 256), dim3(256), 0, s, dvec0, dvec1, cc, ncols_padded, dc, folded);
    LSSVM_HIP_CHECK(hipGetLastError());
}
void enqueue_pack_records(const double *dvec, const double *cc, int ncols_padded, double *dc, int, const double *, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_dc_f64, dim3((ncols_padded + 255) / 256), dim3(256), 0, s, dvec, cc, ncols_padded, dc, static_cast<double *>(nullptr), 0);
    LSSVM_HIP_CHECK(hipGetLastError());
}
void enqueue_pack_records2(const double *dvec0, const double *dvec1, const double *cc, int ncols_padded, double *dc, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_dc2_f64, dim3((ncols_padded + 255) / 256), dim3(256), 0, s, dvec0, dvec1, cc, ncols_padded, dc, static_cast<double *>(nullptr), static_cast<double *>(nullptr), 0);
    LSSVM_HIP_CHECK(hipGetLastError());
}
void enqueue_planes_fragment_major(const uint16_t *planes, size_t plane_elems, int rows_alloc, int ldx16, int nplanes, uint16_t *frag, hipStream_t s) {
    const size_t pieces = static_cast<size_t>(nplanes) * rows_alloc * (ldx16 / 8);
    hipLaunchKernelGGL(k_planes_fragment_major, dim3(static_cast<unsigned>((pieces + 255) / 256)), dim3(256), 0, s, planes, plane_elems, rows_alloc, ldx16, nplanes, frag);
    LSSVM_HIP_CHECK(hipGetLastError());
}

}  // namespace lssvm
