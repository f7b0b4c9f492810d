/*
 * lssvm_problem.hip.hpp -- host side of the MI355X LS-SVM CG backend: device-resident problem + CG driver.
 *
 * Replaces (citations relative to the reference tree):
 *   gpu_csvm::setup_data_on_device        include/plssvm/backends/gpu_csvm.hpp:302-346   (SoA + 96 pad rows  -> row-major, k-chunk padded)
 *   gpu_csvm::generate_q                  gpu_csvm.hpp:349-384
 *   gpu_csvm::run_device_kernel           gpu_csvm.hpp:431-447
 *   gpu_csvm::device_reduction            gpu_csvm.hpp:449-475                           (host-staged sum -> RCCL all-reduce / peer kernels over xGMI)
 *   gpu_csvm::solve_system_of_linear_equations_impl   gpu_csvm.hpp:477-654               (host BLAS-1 + 3 PCIe copies / iteration
 *                                                                                          -> everything device resident, one 8-byte read-back)
 * with the CG recipe of src/plssvm/backends/OpenMP/csvm.cpp:71-183 (x0 = 1, residual refresh every 50 iterations,
 * stop test delta <= eps^2 delta0 before the direction update, bias / rho / alpha_N epilogue).
 */
#pragma once

#include "lssvm_error.hpp"
#include "lssvm_types.hpp"

#include "../../include/plssvm_amd.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only: the library is dlopen'ed lazily (single-GPU use needs no RCCL)

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace lssvm {

/* ------------------------------------------------------------------ errors (lssvm::Error, LSSVM_REQUIRE: lssvm_error.hpp) ------------------------------------------------------------------ */
#define LSSVM_HIP_CHECK(expr)                                                                                                         \
    do {                                                                                                                              \
        const hipError_t lssvm_err_ = (expr);                                                                                         \
        if (lssvm_err_ != hipSuccess) {                                                                                               \
            throw ::lssvm::Error(lssvm_err_ == hipErrorOutOfMemory ? LSSVM_ERR_OUT_OF_MEMORY : LSSVM_ERR_HIP,                         \
                                 std::string("HIP assert '") + hipGetErrorName(lssvm_err_) + "' (" + std::to_string((int) lssvm_err_) + \
                                     "): " + hipGetErrorString(lssvm_err_) + " at " #expr);                                           \
        }                                                                                                                             \
    } while (0)

/* ------------------------------------------------------------------ options ------------------------------------------------------------------ */
struct Options {
    // the 14 options of the product (lssvm_mi355_set_option; include/plssvm_amd.h documents them; round 4 retired xcd_map, lds_extra_kb, item_order,
    // linear_panel_features, check_shards, rbf_direct_above and mfma_shape = 1 -- measured, decided, now constants below)
    int64_t rbf_form = 0;        // fp32 rbf: 0 automatic (matrix cores: norm expansion up to the exponent scale RBF_DIRECT_ABOVE, grid planes up to RBF_GRID_MAX_R2 (times sqrt(128 / features) beyond 128 features); else direct), 3 = grid planes where they exist, 1 always the direct
                                 // (x_i - x_j)^2 kernel on the vector ALU, 2 always the norm expansion on the matrix cores
    int64_t rbf_fold = 1;        // fp32 rbf on the split kernels: 1 = folded column records (2^c_j d_j | 2^c_j), accumulators start from c_i as the C
                                 // operand of their first MFMA (default, while the exponent scale stays below 200); 0 = start values c_i + c_j by vector adds
    int64_t j_chunk_tiles = 0;   // 128-column tiles per work item; 0 = automatic (shard_chunks / product_chunk_tiles, lssvm_geometry.cpp)
    std::vector<double> shard_weights;  // symmetric variant, several ranks: rank r's share of the triangle's area is weight[r] / sum (empty or of another length: equal shares); lssvm_mi355_set_shard_weights
    int64_t j_chunk_head = 1;    // 256-row workgroups: 0 = none; 1 = chosen by the replayed dispatch (with j_chunk_tiles = 0; default); 1024 count + tiles = the first `count` column chunks have `tiles` tiles
    int64_t symmetric = 1;         // 1: evaluate only the tiles on/below the diagonal and mirror them, 0: full square
    int64_t tile_kernel = 0;       // 0: automatic (resident-row-panel kernels where they exist), 1: always the generic v1 kernel (the cross-checks' yardstick)
    int64_t gram_mode = 3;         // fp32 Gram tiles: 0 = v_mfma_f32 chains; 1 = "bf16x6"; 2 = "f16x3" without the representability check; 3 (default) = f16x3
                                   // where the data passes that check, else bf16x6
    int64_t mfma_shape = 3;        // split kernels, symmetric variant, <= 128 features per pass: 2 = 128-row workgroups (four waves), 3 (default) = 256-row
                                   // workgroups on block pairs (eight waves, one column stream per CU) from 64 row blocks on
    int64_t colslab_band_mb = 2048;    // symmetric variant: the column-sum records of ONE row-block band may take this many MiB; the tile kernel runs band by band
    int64_t colslab_limit_mb = 98304;  // symmetric variant only while its column slab (per device) stays below this many MiB (96 GiB of the 288 GB); 0 = off
    int64_t force_collective = 0;  // testing aid: run the per-matvec collective even for a world of one (needs lssvm_mi355_comm_init(.., 0, 1, ..))
    int64_t skip_collective = 0;   // testing aid: sharded problems (world > 1) need no communicator and leave their PARTIAL K*v un-exchanged
    int64_t exchange = 0;          // several devices in ONE process: 0 = automatic (RCCL when the devices are distinct, else peer kernels), 1 = RCCL all-reduce / all-gather
                                   // (ncclCommInitAll), 2 = peer kernels: every device sums the partial vectors of all devices over xGMI in rank order
    int64_t rebalance_after = 0;           // one-shot solves on several devices: after this many iterations the shards are given new shares by their measured pace (lssvm_mi355_problem_rebalance); 0 = never
    int64_t enqueue_ahead_below_us = 5000;  // CG: implicit matvecs shorter than this are enqueued ahead of the previous iteration's stop test (0 = never)
    int64_t ipc_timeout_s = 600;   // one process per GPU over HIP IPC: how long a rank waits for its peers at an exchange before it gives up
    // development builds only (the setter refuses them elsewhere)
    int64_t debug_ablate = 0;      // -DLSSVM_ENABLE_ABLATION: timing ablations of the fp32 tile kernels (results are wrong when != 0)
    int64_t item_order_dev = 0;    // make DEV=1: order of the work items of the symmetric variant (0 = ITEM_ORDER; 3 = XCD-aware lanes)
    int64_t pair_lag = 0;          // make DEV=1: plane-chunk steps waves 4-7 of a 256-row workgroup run behind waves 0-3 (0 = lock step: the shipped form; 1, 3
                                   // measured slower)
};
constexpr double RBF_GRID_MAX_R2 = 4096.0;    // rbf_form 0: grid planes (KT_RBFG) between RBF_DIRECT_ABOVE and this exponent scale (at any width): their error grows with the cross
                                              // terms |h||s| ~ R2 sqrt(d) 2^-12 (7 eps of a row's summands at R2 = 12 600, d = 128 in the model of tests/tools/grid_planes_model.py)
constexpr double RBF_DIRECT_ABOVE = 32.0;     // rbf_form 0: the formula-exact kernel above this exponent scale 2 gamma log2(e) max|x - mean|^2 (absolute error of the
                                              // matrix-core exponent ~ 2^-24 x that; [-1, 1]-scaled data with gamma = 1 / num_features has <= 3)
/* mixed-precision refinement (lssvm_refine.hip): the constants of its CPU model */
constexpr double REFINE_INNER_EPS_MIN = 0x1p-16;  // the inner fp32 solve is never asked for more than this (relative to its right-hand side): below it fp32's own residual stalls
constexpr double REFINE_INNER_EPS_MAX = 0x1p-4;   // ... nor for less: a step must pay for its fp64 pass
constexpr double REFINE_ACCEPT_RATIO = 0.5;       // a step is accepted if the true residual's norm fell to at most this share; otherwise fp64 CG takes over
constexpr uint64_t REFINE_INNER_CAP = 200;        // iterations of ONE inner solve at most
constexpr int LINEAR_IN_TILE_BELOW = 10000;   // fp32 linear kernel on more than 256 features and fewer points than this: ONE launch of the polynomial tile kernels with degree 1
                                              // instead of launch-bound feature-panel passes (Problem<float>::tile_params_)
constexpr int LINEAR_PANEL_FEATURES = 128;    // linear kernel beyond this many features: one pass of the <= 128-feature kernels per feature panel (fp32 f16x3: beats the
                                              // wider one-wave kernels by 5 ... 12 % at every width measured; fp64: 64- and 256-feature panels within 2 %)
/* process-wide DEFAULTS (lssvm_mi355_set_option); every problem / solve that is not handed options of its own (lssvm_mi355_options, ABI 4) takes a snapshot when it is
 * created.  The defaults are read and written under options_mutex() only: options_snapshot() for readers. */
Options &options();
std::mutex &options_mutex();
inline Options options_snapshot() {
    const std::lock_guard<std::mutex> lock(options_mutex());
    return options();
}
/* what the work-item geometry reads of them (lssvm_geometry.hpp; the shard weights and the item order travel as arguments) */
inline GeometryOptions geometry_options(const Options &o) { return { o.j_chunk_tiles, o.j_chunk_head, o.colslab_band_mb, o.colslab_limit_mb }; }
/* fp32 rbf, rbf_form 0 (automatic): the grid planes were chosen from the exponent scale but do not represent THIS data -- the owner of the problem builds it again
 * with the formula-exact kernel (Solver's constructor, predict_values); with an explicit rbf_form = 3 the error reaches the caller */
struct GridPlanesUnfit : Error {
    GridPlanesUnfit() : Error(LSSVM_ERR_INTERNAL, "the grid planes of the rbf kernel do not represent this data (option rbf_form = 1 selects the direct kernel)") {}
};

/* ------------------------------------------------------------------ RCCL (lazy) ------------------------------------------------------------------ */
struct Comm {  // the RCCL entry points (dlopen'ed once) + the communicator of a one-process-per-GPU launch
    void *lib = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1, device = 0;
    decltype(&ncclGetUniqueId) pGetUniqueId = nullptr;
    decltype(&ncclCommInitRank) pCommInitRank = nullptr;
    decltype(&ncclCommInitAll) pCommInitAll = nullptr;
    decltype(&ncclCommDestroy) pCommDestroy = nullptr;
    decltype(&ncclAllGather) pAllGather = nullptr;
    decltype(&ncclAllReduce) pAllReduce = nullptr;
    decltype(&ncclGroupStart) pGroupStart = nullptr;
    decltype(&ncclGroupEnd) pGroupEnd = nullptr;
    decltype(&ncclGetErrorString) pGetErrorString = nullptr;
    decltype(&ncclCommCount) pCommCount = nullptr;
    decltype(&ncclCommCuDevice) pCommCuDevice = nullptr;
    decltype(&ncclCommUserRank) pCommUserRank = nullptr;
};
Comm &comm();
void comm_load();
void nccl_check(ncclResult_t rc, const char *what);  // throws LSSVM_ERR_COMM with RCCL's own message
constexpr int MAX_LOCAL_DEVICES = 16;                // shards one process drives / ranks the peer exchange sums

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* ------------------------------------------------------------------ small RAII helpers ------------------------------------------------------------------ */
template <typename U>
struct DevBuf {
    U *p = nullptr;
    size_t count = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void alloc_zero(size_t n, hipStream_t s) {
        release();
        count = n;
        if (n == 0) return;
        LSSVM_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(U)));
        LSSVM_HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(U), s));
    }
    void release() {
        if (p != nullptr) (void) hipFree(p);
        p = nullptr;
        count = 0;
    }
};

inline int round_up(long v, int m) { return static_cast<int>(((v + m - 1) / m) * m); }

template <typename T>
constexpr int kchunk_of() {
    return std::is_same_v<T, float> ? F32_KC : F64_KC;
}

/* Padded feature count: a multiple of the k-chunk; between 8 (fp32: 4) and 16 chunks a multiple of TWO chunks, so that the v2 tile kernels
 * (fp64: instantiated for 1..8 and 10, 12, 14, 16 chunks; fp32: 1..4, 6, 8, 10, 12, 14, 16) cover num_features <= 512 in fp32 / <= 256 in fp64. */
template <typename T>
inline int padded_features(size_t nfeat) {
    const int kc = kchunk_of<T>();
    const int ldx = round_up(static_cast<long>(nfeat), kc);
    if (std::is_same_v<T, double> && ldx > 16 * kc) return round_up(static_cast<long>(nfeat), 64);  // fp64 beyond the one-pass kernels: whole feature panels of 64 (lssvm_tile_f64_wide.hip.hpp)
    // fp32: whole pairs of chunks already beyond 4 (the native v2 kernel -- the rare path without operand planes -- is instantiated for 1 ... 4, 6, 8 ... 16)
    const int single_up_to = std::is_same_v<T, float> ? 4 : 8;
    return (ldx > single_up_to * kc && ldx <= 16 * kc) ? round_up(static_cast<long>(nfeat), 2 * kc) : ldx;
}

/* A dense row-major point set in HBM: rows padded to a multiple of 128, features padded to a multiple of the k-chunk
 * (zeros), so that every global load of the tile kernel is an aligned 16-byte load of a full 128-byte line. */
template <typename T>
struct DeviceMatrix {
    DevBuf<T> data;
    int rows = 0;        // valid rows
    int rows_alloc = 0;  // multiple of TILE
    int dfeat = 0;       // valid features
    int ldx = 0;         // padded features

    void upload(const void *src, int mem_kind, size_t nrows, size_t nfeat, size_t min_rows_alloc, hipStream_t s) {
        rows = static_cast<int>(nrows);
        dfeat = static_cast<int>(nfeat);
        ldx = padded_features<T>(nfeat);
        rows_alloc = std::max(round_up(static_cast<long>(nrows), TILE), round_up(static_cast<long>(min_rows_alloc), TILE));
        data.alloc_zero(static_cast<size_t>(rows_alloc) * ldx, s);
        LSSVM_HIP_CHECK(hipMemcpy2DAsync(data.p, static_cast<size_t>(ldx) * sizeof(T), src, nfeat * sizeof(T), nfeat * sizeof(T), nrows,
                                         mem_kind == LSSVM_MEM_DEVICE ? hipMemcpyDefault : hipMemcpyHostToDevice, s));  // (a device source may live on another device of the process)
    }
};

/* ------------------------------------------------------------------ more RAII: stream, events, pinned host words ------------------------------------------------------------------ */
/* A non-blocking stream of the CURRENT device.  Creating one costs 2-4 ms on this runtime (a hardware queue behind it) -- more than everything else in the set-up of a
 * 50 000-point problem -- so an idle stream goes back to a small per-device pool instead of being destroyed, and the next problem takes it from there. */
struct Stream {
    hipStream_t s = nullptr;
    int device = -1;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() {
        if (s == nullptr) return;
        if (hipStreamSynchronize(s) == hipSuccess) {  // (only an idle stream without a pending error is kept)
            const std::lock_guard<std::mutex> lock(pool_mutex());
            std::vector<hipStream_t> &idle = pool()[device];
            if (idle.size() < 8) {
                idle.push_back(s);
                return;
            }
        }
        (void) hipStreamDestroy(s);
    }
    void create() {
        LSSVM_HIP_CHECK(hipGetDevice(&device));
        {
            const std::lock_guard<std::mutex> lock(pool_mutex());
            std::vector<hipStream_t> &idle = pool()[device];
            if (!idle.empty()) {
                s = idle.back();
                idle.pop_back();
                return;
            }
        }
        LSSVM_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }

  private:
    static std::mutex &pool_mutex() {
        static std::mutex m;
        return m;
    }
    static std::map<int, std::vector<hipStream_t>> &pool() {
        static std::map<int, std::vector<hipStream_t>> *p = new std::map<int, std::vector<hipStream_t>>();  // (never destroyed: streams outlive static destruction order)
        return *p;
    }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    ~Event() {
        if (e != nullptr) (void) hipEventDestroy(e);
    }
    void create(bool timing) { LSSVM_HIP_CHECK(hipEventCreateWithFlags(&e, timing ? hipEventDefault : hipEventDisableTiming)); }
};
/* milliseconds between two timing events the stream has passed */
inline float elapsed_ms(const Event &a, const Event &b) {
    float ms = 0.0f;
    LSSVM_HIP_CHECK(hipEventElapsedTime(&ms, a.e, b.e));
    return ms;
}
template <typename U>
struct PinnedBuf {
    U *p = nullptr;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() {
        if (p != nullptr) (void) hipHostFree(p);
    }
    void alloc(size_t n) { LSSVM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&p), n * sizeof(U), hipHostMallocDefault)); }
    /* host memory a KERNEL writes (fine-grained, mapped): `dev` is the address the device uses; the host reads `p` behind an event of the stream */
    U *dev = nullptr;
    void alloc_mapped(size_t n) {
        LSSVM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&p), n * sizeof(U), hipHostMallocMapped | hipHostMallocCoherent));
        LSSVM_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void **>(&dev), p, 0));
    }
};

/* `ref` <- `value` when the scope ends, however it ends: the handle's busy flag, an option changed for one call */
template <typename V>
struct SetOnExit {
    V &ref;
    V value;
    SetOnExit(V &r, V v) : ref(r), value(v) {}
    SetOnExit(const SetOnExit &) = delete;
    SetOnExit &operator=(const SetOnExit &) = delete;
    ~SetOnExit() { ref = value; }
};

/* ------------------------------------------------------------------ tile kernel launch ------------------------------------------------------------------ */
template <typename T>
void launch_tile_kernel(TileArgs<T> &a, int kernel_type, bool rbf_direct, int num_jc, hipStream_t s);
template <>
void launch_tile_kernel<float>(TileArgs<float> &a, int kernel_type, bool rbf_direct, int num_jc, hipStream_t s);   // tile_launch_f32.hip
template <>
void launch_tile_kernel<double>(TileArgs<double> &a, int kernel_type, bool rbf_direct, int num_jc, hipStream_t s);  // tile_launch_f64.hip

/* centre `M` (and optionally `M2` with the same means) by the column means of M's valid rows; rbf only */
template <typename T>
void center_columns(DeviceMatrix<T> &M, DeviceMatrix<T> *M2, T scale, hipStream_t s);
template <typename T>
void half_neg_norms(const DeviceMatrix<T> &M, DevBuf<T> &c, hipStream_t s);
template <typename T>
void interleave_features(DeviceMatrix<T> &M, hipStream_t s);
bool v2_eligible(const Options &o, int ldx, bool rbf_direct);
void split_bf16_planes(const float *X, int ldx, int dfeat, size_t rows, int ldx16, uint16_t *planes, size_t plane_stride, hipStream_t s);  // tile_launch_f32s.hip
/* the f16 planes of `scale` * X (scale = a power of two; shift = 0: two planes, shift > 0: the three shifted planes of the rbf kernels) + the representation
 * statistics {max rel^2, max |rest|^2, max |y|^2} as float bits */
void split_grid_planes(const float *X, int ldx, int dfeat, size_t rows, int ldx16, float g, float sigma, uint16_t *planes, size_t plane_stride, float *chg, float *efac, unsigned *stats,
                       hipStream_t s);  // tile_launch_f32h.hip
void split_f16_planes(const float *X, int ldx, int dfeat, size_t rows, int ldx16, float scale, int shift, uint16_t *planes, size_t plane_stride, unsigned *stats, hipStream_t s,
                      float *row_inv_scale = nullptr);  // row_inv_scale != NULL: a power-of-two scale per ROW, its inverse stored there  // tile_launch_f32h.hip
void absmax_f32(const float *X, int ldx, int dfeat, size_t rows, unsigned *out, hipStream_t s);  // tile_launch_f32h.hip
bool v2_eligible_f64(const Options &o, int ldx);

/* fp32: a data matrix once more as operand planes of the split tile kernels (make_planes in lssvm_problem.hip) */
struct PlaneSet {
    DevBuf<float> row_inv_scale;     // f16x3, linear kernel, round 6: 2^-k_i per row where the planes carry a scale PER ROW (empty: one scale for the matrix)
    double f16_row_rel_error = -1.0;  // what the representability check of the f16 planes measured (make_planes), -1 where it did not run
    float f16_rel2 = 0.0f, f16_rest2 = 0.0f, f16_x2 = 0.0f;  // the check's statistics {max rel^2, max |rest|^2, max |y|^2} over THIS matrix (and M2), where it ran: the resident
                                                              // predictor combines them with a batch's to decide as the one-shot call does (f16_planes_pass)
    DevBuf<uint16_t> buf;
    int ldx16 = 0;
    int mode = 0;   // 0 none, 1 bf16x6 (three bf16 planes), 2 f16x3 (two f16 planes)
    int shift = 0;  // f16x3: the planes carry 2^shift x
    int nplanes = 0;  // planes in `buf` (f16x3: 2, rbf 3 -- the shifted planes; bf16x6: 3)
};

/* ------------------------------------------------------------------ one device's share of the problem ------------------------------------------------------------------ */
/* Problem<T>: the data matrix resident on ONE device plus the CG vectors, and the row blocks `rank` of `world` of the implicit
 * matrix.  Every method only ENQUEUES work on the shard's stream (set-up excepted); the CG recipe and the exchange between
 * shards are driven by Solver<T>.  Replaces gpu_csvm::setup_data_on_device / generate_q / run_device_kernel (gpu_csvm.hpp:302-447). */
template <typename T>
class Solver;
template <typename T>
class CgSteps;
template <typename T>
class LandmarkBlock;  // K(X, X_L) of a resident problem (lssvm_landmark.hip.hpp)
template <typename T>
struct GridSlabs;  // what the slabs of a (gamma, cost) grid are made from: the sums every gamma shares (lssvm_reduced.hip)

/* The CG state of ONE right-hand side on one device: the vectors y, b, x, r, d, Ad, the scalars and the four sets of partial sums, the host copies of the scalars and a
 * mapped host word for the iteration's delta (k_finish_delta stores its 8 bytes straight into host memory: no copy per iteration).  A problem has one of its own (the
 * single solve: its K*v is the problem's exchanged vector, `Kv` stays empty) and one per lane (solve_lockstep, matvec_pair, the refinement: each with a K*v of its own). */
template <typename T>
struct CgState {
    DevBuf<T> y, b, x, r, d, Ad, Kv;
    DevBuf<double> part, sc;
    double *part_of(PartSet s) const { return part.p + static_cast<size_t>(s) * RED_BLOCKS * 2; }  // (lssvm_types.hpp)
    PinnedBuf<double> host_sc, host_delta;
    double delta_on_host() const { return *static_cast<volatile double *>(host_delta.p); }  // (behind an event of the stream)
    void alloc(size_t vec_len, size_t num_points, bool own_Kv, hipStream_t s) {
        for (DevBuf<T> *v : { &b, &x, &r, &d, &Ad }) v->alloc_zero(vec_len, s);
        if (own_Kv) Kv.alloc_zero(vec_len, s);
        y.alloc_zero(num_points, s);
        part.alloc_zero(static_cast<size_t>(PART_REGIONS) * RED_BLOCKS * 2, s);  // (four sets of partial sums: a kernel reduces its predecessor's while it writes its own)
        sc.alloc_zero(SC_COUNT, s);
        host_sc.alloc(SC_COUNT);
        host_delta.alloc_mapped(1);
    }
};

template <typename T>
class Problem {
  public:
    Problem(const Options &opt, const lssvm_params &params, const void *X, int mem_kind, size_t num_points, size_t num_features, int device, int rank, int world);
    ~Problem();
    Problem(const Problem &) = delete;
    Problem &operator=(const Problem &) = delete;

    void activate() const { LSSVM_HIP_CHECK(hipSetDevice(device_)); }
    /* Kv_ <- this shard's part of K * v (complete for a world of one): tile kernel + fixed-order reductions.  The symmetric variant is one call of enqueue_sym_walk,
     * with sampled HIP events around every band launch (matvec_ms_) */
    void enqueue_apply_K_local(const T *v_dev, bool zero_first);
    void reshard(const std::vector<double> &weights);  // new shares of the triangle (lssvm_mi355_problem_rebalance): the data, the vectors and the CG state stay
    void choose_shard_geometry();
    void build_shard_lists(hipStream_t st);
    PackDc<T> pack_for_d(bool zero_first);  // what k_update_d needs to pack the records of the own state's d (dc == NULL: this problem packs per matvec); marks them as present
    /* weighted LS-SVM (lssvm_mi355_problem_set_weights): inv_cw_ and QA_cost_ from the weights of all N points (validated by the caller), or back to the
     * unweighted system for NULL */
    void set_weights(const double *weights);
    void drain_events();
    hipStream_t stream() const { return stream_.s; }
    /* tile-kernel passes per row-block band: the feature panels of a wide fp32 linear problem, else 1 */
    int passes_per_matvec() const {  // feature panels of a wide linear problem: fp32 over the planes, fp64 over the row-major data
        if (!wide_linear_) return 1;
        if constexpr (std::is_same_v<T, float>) {
            return (planes_.ldx16 + LINEAR_PANEL_FEATURES - 1) / LINEAR_PANEL_FEATURES;
        } else {
            return (X_.ldx + LINEAR_PANEL_FEATURES - 1) / LINEAR_PANEL_FEATURES;
        }
    }

    /* full-square-equivalent rate (flop/s, 2 n^2 d per matvec) this shard's kernel path is expected to sustain -- a rule on the shape, the real type and
     * the options only (never a measurement: every rank of a sharded solve must come to the same number).  Round numbers from profiles/r03 / r04:
     * fp32 split kernels in the symmetric variant ~900 T (c5: 930, c3: 1 000), full square half of that; native fp32 v2 ~250 T (sym) / 125 T; panels
     * inside a tile ~250 T; generic fp32 / direct rbf ~45 T; fp64 v2 ~130 T (sym, c4: 134) / 65 T; fp64 panels ~110 T; generic fp64 ~45 T. */
    double nominal_full_square_rate() const {
        const double sym = sym_ ? 1.0 : 0.5;
        if constexpr (std::is_same_v<T, float>) {
            if (rbf_direct_) return 45e12;
            if (planes_.mode != 0 && dc_.p != nullptr) return (wide_nl_ ? 250e12 : 900e12) * sym;
            return dc_.p != nullptr ? 250e12 * sym : 45e12;
        } else {
            if (wide_nl_) return 110e12 * sym;
            return dc_.p != nullptr ? 130e12 * sym : 45e12;
        }
    }

    /* ---- lanes (Solver<T>::solve_lockstep, matvec_pair, the refinement): CG states beside the problem's own, each with its K*v.  Allocated on first use, freed with the
     * problem; the own state is not involved. ---- */
    CgState<T> &lane(size_t k);
    /* where one Gram pass can serve two vectors: the fp64 symmetric v2 kernel on an unsharded problem without feature panels -- and only the (kernel function, chunk
     * count) instantiations whose two-vector pass was measured faster than two single passes (profiles/lockstep_f64.json); fp32: the symmetric one-pass 128-row split
     * kernels on 129 ... 512 features, polynomial or rbf with folded records (sym_pair_routed, profiles/lockstep_f32_wide.json) */
    bool pair_kernel_applies() const;
    /* Kv0 <- K * v0 and, with v1, Kv1 <- K * v1 from ONE pass of the two-vector kernel (pair_kernel_applies; the caller falls back to two calls elsewhere); without v1
     * today's single-vector pass.  Each result has the bits enqueue_apply_K_local gives for that vector: both are enqueue_sym_walk on the arguments of that vector.
     * `ev`: HIP events around the tile-kernel launches (before the first band's, after the last band's), or NULL. */
    void enqueue_apply_K_lanes(const T *v0, T *Kv0, const T *v1, T *Kv1, hipEvent_t ev_begin, hipEvent_t ev_end);

  private:
    friend class Solver<T>;
    friend class CgSteps<T>;
    friend class LandmarkBlock<T>;
    friend struct GridSlabs<T>;
    TileArgs<T> tile_args(const T *v_dev) const;
    /* dc_ <- the single-vector records of v, and `zero[0 .. nzero)` cleared by the same kernel: the one k_pack_dc / k_pack_dc_f64 launch of a problem */
    void enqueue_pack_dc(const T *v, T *zero, int nzero);
    /* The symmetric pass over the row-block bands, the one walk behind enqueue_apply_K_local and enqueue_apply_K_lanes: per feature panel (`npanels`: wide_linear_, else
     * 1) and band the tile kernel on `a` with the band's work items, then per vector u < nv the band's mirrored column sums (a.colslab + u * a.colslab_vstride) folded
     * into Kv[u]; after a panel's bands the row slabs (a.partial + u * a.part_vstride) added into Kv[u].  around(launch, first, last) runs every tile launch -- it calls
     * launch() once, with whatever timing the caller keeps around it; first / last: the first / last tile launch of the walk. */
    template <typename Around>
    void enqueue_sym_walk(const TileArgs<T> &a, int nv, T *const *Kv, int npanels, Around &&around);

    Options opt_{};
    lssvm_params params_{};
    int wide_order_ = 0;            // panels inside a tile, symmetric variant: the row-group major item order (band_items 4 / 5: groups of four / two row blocks); 0 elsewhere
    DevBuf<T> Xfrag_;               // fp64 panels-inside-a-sub-tile kernel, symmetric variant: the data once more, fragment-major, for the row side (TileArgs::Xrf)
    DevBuf<uint16_t> planes_frag_;  // panels-inside-a-tile kernel, symmetric variant: the planes once more, fragment-major, for the row side (TileArgs::Xr16f)
    lssvm_params tile_params_{};   // what the TILE kernels evaluate: params_, except that a linear kernel on few points and many features runs as the polynomial
                                   // kernel of degree 1 (constructor; same values, one launch instead of feature-panel passes)
    int device_ = 0;
    int rank_ = 0, world_ = 1;
    Stream stream_;

    size_t N_ = 0;  // data points
    int n_ = 0;     // N - 1
    int num_tiles_ = 0;  // ceil(n / TILE): row blocks == column tiles
    int ib_begin_ = 0, num_ib_ = 0, ib_per_rank_ = 0;
    int jc_tiles_ = 16, num_jc_ = 1;
    int jc_head_tiles_ = 0, jc_head_count_ = 0;  // 256-row workgroups: a head of short column chunks (choose_pair_chunk)
    int nvec_ = 0;  // allocated vector length (multiple of TILE * world)
    bool rbf_direct_ = false;
    double rbf_r2_ = 0.0;  // fp32 rbf: 2 gamma log2(e) max|x - mean|^2
    bool rbf_grid_ = false;      // fp32 rbf on GRID planes (KT_RBFG): large exponent scales on the matrix cores at the direct form's accuracy (Problem<T>'s constructor)
    float grid_sigma_ = 1.0f;    // ... the planes carry sigma x (a power of two), the chain sigma^2 t
    DevBuf<T> efac_;             // ... E_i = 2^(c_i - ch_i) per row (c_ then holds sigma^2 ch_i)
    bool dc_folded_ = false;  // the (d_j | c_j) records carry (2^c_j d_j | 2^c_j): rbf on the 16x16x32 bf16x6 kernels
    bool pair_ = false;            // fp32 symmetric variant on the split kernels, <= 128 features per pass: 256-row workgroups on block pairs (lssvm_tile_f32_pair.hip.hpp)
    int part_blocks() const { return pair_ ? round_up(std::max(num_ib_, 1), 2) : std::max(num_ib_, 1); }  // row blocks of a row slab (whole pairs)
    double f16_row_rel_error_ = -1.0;  // fp32, gram_mode 2 / 3: the largest relative error of a row under two f16 planes, as measured at set-up (-1: not measured)
    bool row_scaled_ = false;        // fp32 linear kernel: the f16 planes carry a power-of-two scale per ROW (planes_.row_inv_scale): K v = D (Xs Xs^T) (D v)
    DevBuf<T> vs_;                   // ... D v, the vector the tile kernel multiplies
    bool f16_probe_failed_ = false;  // the probe for the linear kernel's panel passes found the data unfit for two f16 planes
    bool wide_nl_ = false;         // fp32 rbf / polynomial on more features than the one-pass split kernels take: feature panels inside a tile (lssvm_tile_f32_wide.hip.hpp)
    bool wide_linear_ = false;     // linear kernel over feature panels, one tile-kernel pass per panel: fp32 f16x3 beyond linear_panel_features, fp64 beyond 256 features
    bool poly_prescaled_ = false;  // fp64 polynomial on the v2 kernel: X_ carries sqrt(gamma), the kernel sees gamma = 1
    double x_scale_ = 1.0;         // the factor X_ was multiplied by in place after q was computed (rbf off the direct form: rbf_prescale, on centred data; poly_prescaled_:
                                   // sqrt(gamma)): what reads X_ directly -- the landmark block of the preconditioner, lssvm_precond.hip -- evaluates with gamma / x_scale_^2
    PlaneSet planes_;              // fp32 split kernels: X as three bf16 planes (bf16x6) or two f16 planes (f16x3), [planes][rows_alloc][ldx16]

    DeviceMatrix<T> X_;
    DevBuf<T> c_;  // -0.5 |x|^2 (rbf, centred data)
    DevBuf<T> q_, Kv_, Ksum_, tmp_;
    CgState<T> own_;     // the CG state of the single solve (cg_begin / cg_step / cg_finish, matvec); its K*v is Kres_
    T *Kres_ = nullptr;  // the exchanged K * v the O(n) kernels read: Kv_ itself, or Ksum_ when peer kernels do the exchange
    DevBuf<T> partial_;
    DevBuf<T> dc_;  // v2 kernels: packed (d_j | c_j) records
    std::vector<std::unique_ptr<CgState<T>>> lanes_;
    DevBuf<T> pair_dc_, pair_partial_, pair_colslab_;  // two-vector passes: (d0_j | d1_j | c_j) records (fp32: k_pack_dc2_sym's), and both vectors' planes of the row slabs / the column slab
    bool d_packed_ = false;  // dc_ holds the records of own_.d and K*v is cleared: k_update_d left them (pack_for_d), the next implicit matvec of that d launches no k_pack_dc
    // symmetric variant
    bool sym_ = false;
    DevBuf<int2> items_;
    int num_items_ = 0;
    int ldx_probe_ = 0;        // the padded feature count the kernel paths were chosen with (constructor), kept for reshard
    size_t num_features_ = 0;
    DevBuf<unsigned> queue_;  // 256-row workgroups, persistent launches: two sets of eight item counters (a launch draws from one and zeroes the other)
    int queue_set_ = 0;
    int queue_min_items_ = 256;  // launches of more items than this (the CU count) are persistent
    DevBuf<T> colslab_;  // the records of the band in flight
    struct Band {
        int ib_begin, ib_end;       // row blocks [begin, end) of the band (global block indices)
        int item_begin, item_count; // its work items in items_
        long pair_origin;           // record index of (ib_begin, 0) in the packed triangle: ib_begin (ib_begin - 1) / 2
    };
    std::vector<Band> bands_;
    double QA_cost_ = 0.0;
    double inv_cost_ = 1.0;
    double self_last_ = 0.0;  // k(x_last, x_last) in the real type: QA_cost_ = self_last_ + 1/(C w_last) (set_weights)
    bool weighted_ = false;   // the O(n) kernels read the diagonal 1/(C w_i) from inv_cw_ (their WEIGHTED instantiations) instead of inv_cost_
    DevBuf<double> inv_cw_;   // ... replicated on every shard like q_, padded with inv_cost_
    double setup_ms_ = 0.0;

    // statistics: HIP events around the tile kernel
    double matvec_ms_ = 0.0;       // tile-kernel time of the TIMED matvecs (HIP events around the band launches)
    uint64_t matvec_launches_ = 0; // matvecs enqueued
    double pace_ms0_ = 0.0;        // matvec_ms_ / matvec_timed_ at the last reshard: a rebalance by measured pace looks at what came after it
    uint64_t pace_timed0_ = 0;
    uint64_t matvec_timed_ = 0;    // ... of which timed: all of them where a matvec is long, every 8th where it is short (two event records cost ~6 us per
                                   // matvec on the stream: 9 % of a 10 000-point CG iteration, profiles/r04_event_record_cost.log)
    /* a rule on the shape only, like the enqueue-ahead decision: below ~1 ms per matvec the events are sampled */
    int event_stride() const {
        const double n_d = static_cast<double>(n_);
        return 2.0 * n_d * n_d * static_cast<double>(X_.dfeat) / static_cast<double>(world_) / nominal_full_square_rate() < 1e-3 ? 8 : 1;
    }
    struct EvPair {
        Event a, b;
        bool pending = false;
        bool first_of_matvec = true;
    };
    std::vector<EvPair> events_;
    Event ev_ready_, ev_consumed_;  // peer exchange: partial vector written / all partial vectors read
};

/* ------------------------------------------------------------------ the CG recipe, step by step ------------------------------------------------------------------ */
/* CgSteps<T>: the O(n) steps of the reference's CG recipe (csvm.cpp:71-183) on ONE CG state of ONE problem -- its stream, q, n, QA_cost and diagonal term.  Every step
 * only enqueues (finish_now excepted); a step that reads K * v is handed the pointer to it.  The drivers -- the sharded single solve, the lanes, the refinement, PCG -- decide
 * when the Gram passes run and where the host waits; which O(n) kernel runs on which arguments is written here and nowhere else, so their recurrences have the same
 * bits.  Defined by lssvm_solver.hip. */
template <typename T>
class CgSteps {
  public:
    using State = CgState<T>;
    explicit CgSteps(Problem<T> &p) : p_(p) {}
    hipStream_t stream() const { return p_.stream_.s; }
    int n() const { return p_.n_; }
    size_t num_points() const { return p_.N_; }
    const T *q() const { return p_.q_.p; }
    T *Kres() const { return p_.Kres_; }  // where the problem's own pass (enqueue_apply_K_local + the exchange) leaves K * v

    /* sc[slot_sum] = sum v, sc[slot_q] = q^T v; finish_sums: its second half alone, the partial sums are in PART_SUMS already (k_axpy_up) */
    void sum_and_qdot(const State &s, const T *v, int slot_sum, int slot_q) const;
    void finish_sums(const State &s, int slot_sum, int slot_q) const;
    /* b = y - y_last, x = 1 and the sums of x that r = b - A x needs (csvm.cpp:89-95); K * x and `residual` follow */
    void begin(const State &s, const T *y_host) const;
    /* b = r = r_dev / max|r_dev|, x = 0, the partial sums of r^T r (the inner solve of the refinement: no Gram pass) */
    void begin_from_zero(const State &s, const double *r_dev, const double *absmax_part_dev) const;
    /* r_out = b - A x with Kv = K * x and the sums of x in the scalars; the partial sums of r_out^T r_out into `part`   (csvm.cpp:101-107, :140-145) */
    void residual(const State &s, const T *Kv, const T *x, T *r_out, PartSet part) const;
    /* delta = the sum of `part`, published to `host_delta`   (csvm.cpp:107-108, :152-153) */
    void finish_delta(const State &s, PartSet part, double *host_delta, bool initial) const;
    /* d = r (initial) or beta d + r, and -- as partial sums that Ad_and_dAd finishes for itself -- the sums the next matvec's rank-1 terms need   (csvm.cpp:111, :161-163) */
    void update_d(const State &s, bool initial, const PackDc<T> &pack = PackDc<T>{}) const;
    /* one iteration up to its delta, with Kv = K * d: Ad = A d, alpha = delta / d.Ad, x += alpha d, r -= alpha Ad -- or with `refresh`, every 50th iteration, x only and
     * its sums: K * x and `residual` follow   (csvm.cpp:131-148).  `sc_alpha`: the scalar set alpha is formed in (SC_DELTA read, SC_DAD / SC_ALPHA written) where that is
     * not the state's own -- PCG keeps alpha's numerator r.z in two sets used in turn (lssvm_precond.hip) */
    void advance(const State &s, const T *Kv, bool refresh, double *sc_alpha = nullptr) const;
    /* Ad += add * A v with Kv = K * v and the sums of v in SC_S / SC_QD   (csvm.cpp:283-306) */
    void apply_ret(const State &s, const T *Kv, const T *v, double add) const;
    /* the sums of x and the scalars to the host, x to alpha_out (where given); after the stream has been waited for, read_solution: alpha_N = -sum(x),
     * rho = -bias = -(y_last + QA_cost * sum(x) - q^T x)   (csvm.cpp:179-182).  finish_now: both around a wait for the stream */
    void enqueue_finish(const State &s, T *alpha_out) const;
    void read_solution(const State &s, double y_last, T *alpha_out, double *rho_out) const;
    void finish_now(const State &s, double y_last, T *alpha_out, double *rho_out) const;

  private:
    template <typename Launch>
    void with_diag(Launch &&launch) const;  // the one place that chooses between the weighted and the unweighted instantiation of a kernel
    Problem<T> &p_;
};

/* the fields of lssvm_cg_info that describe how a solve went (describe_path fills in where it ran) */
inline void fill_cg_outcome(lssvm_cg_info *info, uint64_t iterations, uint64_t max_iterations, double residuum, double initial_residuum, double target_residuum, double epsilon,
                            double total_ms, bool converged) {
    info->iterations = iterations;
    info->max_iterations = max_iterations;
    info->residuum = residuum;
    info->initial_residuum = initial_residuum;
    info->target_residuum = target_residuum;
    info->epsilon = epsilon;
    info->total_ms = total_ms;
    info->avg_iteration_ms = iterations > 0 ? total_ms / static_cast<double>(iterations) : 0.0;
    info->converged = converged ? 1 : 0;
}

/* ------------------------------------------------------------------ the Nystrom preconditioner of a problem (lssvm_precond.hip) ------------------------------------------------------------------ */
constexpr int PRECOND_MAX_RANK = 512;
/* P = Bhat Bhat^T + sigma I with Bhat = [E K_Nm L^-T | sqrt(sigma) 1], n x (rank + 1), and what applying P^-1 r ~ r - Bhat G^-1 Bhat^T r needs, G = Bhat^T Bhat + sigma I.
 * Bhat is stored COLUMN by column (column j: ldn reals, exact zeros from row n on), so that both apply kernels stream it in 16-byte pieces along a column. */
template <typename T>
struct Precond {
    int rank = 0, cols = 0;           // landmarks m, columns m + 1
    size_t ldn = 0;                   // reals between two columns: n rounded up to 256
    std::vector<uint64_t> landmarks;  // the points in use
    DevBuf<T> Bhat;                   // [cols][ldn]
    DevBuf<double> Ginv;              // [cols][cols], symmetric to the bit
    DevBuf<double> tpart, s;          // the apply's RED_BLOCKS x cols partial sums of Bhat^T r, and s = G^-1 Bhat^T r as ceil(cols / 32) shares of cols doubles (added by the last kernel)
    DevBuf<double> part_rz;           // RED_BLOCKS x 2 partial sums of r.z
    DevBuf<T> r_io, z_io;             // lssvm_mi355_problem_precond_apply: the caller's vector and the result
    double sigma = 0.0, jitter = 0.0, build_ms = 0.0;
};

/* ------------------------------------------------------------------ the resident problem (what a C handle points to) ------------------------------------------------------------------ */
struct ProblemBase {
    int dtype = 0;
    virtual ~ProblemBase() = default;
    virtual void get_q(void *q_out, double *QA_cost_out) = 0;
    virtual void set_weights(const double *weights, size_t num_points) = 0;  // lssvm_mi355_problem_set_weights
    virtual void matvec(const void *d, void *ret_inout, double add) = 0;
    virtual void matvec_pair(const void *d0, const void *d1, void *ret0_inout, void *ret1_inout, double add, int *two_vector_out) = 0;  // lssvm_mi355_problem_matvec_pair
    virtual void solve_lockstep(const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out, double *rhos_out, lssvm_cg_info *infos_out,
                                uint64_t *passes_out) = 0;  // lssvm_mi355_problem_solve_lockstep
    virtual void solve_cost_path(const void *y, const double *costs, size_t num_costs, double eps, uint64_t max_iter, bool verify, void *alphas_out, double *rhos_out,
                                 lssvm_path_info *infos_out, uint64_t *passes_out) = 0;  // lssvm_mi355_problem_solve_cost_path
    /* the Nystrom preconditioner and PCG on it (lssvm_precond.hip) */
    virtual void build_preconditioner(uint64_t rank, const uint64_t *landmarks, lssvm_precond_info *info) = 0;  // lssvm_mi355_problem_build_preconditioner
    virtual void precond_landmarks(uint64_t *out) = 0;                                                          // lssvm_mi355_problem_precond_landmarks
    virtual void precond_apply(const void *r, void *z_out) = 0;                                                 // lssvm_mi355_problem_precond_apply
    virtual void solve_pcg(const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out, double *rhos_out, lssvm_pcg_info *infos_out) = 0;  // lssvm_mi355_problem_solve_pcg
    /* the fixed-size model (lssvm_reduced.hip) */
    virtual void fit_reduced(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out,
                             uint64_t *landmarks_out, lssvm_reduced_info *info, const double *weights = nullptr) = 0;  // lssvm_mi355_problem_fit_reduced
    virtual void landmark_gram(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *gram_out, const double *weights = nullptr) = 0;  // lssvm_mi355_problem_landmark_gram
    virtual void time_gram_kernels(int repeats, double *parent_ms_out, double *mfma_ms_out, double *max_diff_out) = 0;  // lssvm_mi355_problem_time_gram_kernels
    /* exact leave-one-out scores of the fixed-size model over a cost grid (lssvm_reduced.hip) */
    virtual void fit_reduced_loo(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out,
                                 double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out,
                                 lssvm_reduced_loo_info *infos, const double *weights = nullptr) = 0;  // lssvm_mi355_problem_fit_reduced_loo
    virtual void reduced_leverage(uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *V, const double *shift, const double *B_extra, size_t k, double *h_out,
                                  double *f_out) = 0;  // lssvm_mi355_problem_reduced_leverage
    /* `weights` in the five above: N doubles on the host, each finite and >= 0 with a positive sum, for the weighted objective -- or NULL */
    /* both fits with the dense steps on the device (lssvm_dense.hip); `dense`: one record, or num_costs of them, or NULL */
    virtual void fit_reduced_dev(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out,
                                 uint64_t *landmarks_out, lssvm_reduced_info *info, lssvm_dense_info *dense, const double *weights = nullptr) = 0;  // lssvm_mi355_problem_fit_reduced_dev
    virtual void fit_reduced_loo_dev(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out,
                                     double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out,
                                     lssvm_reduced_loo_info *infos, lssvm_dense_info *dense, const double *weights = nullptr) = 0;  // lssvm_mi355_problem_fit_reduced_loo_dev
    virtual void time_leverage_kernel(uint64_t rank, uint64_t slab_rows, size_t k, int repeats, double *gram_ms_out, double *leverage_ms_out) = 0;  // lssvm_mi355_problem_time_leverage_kernel
    /* the leave-one-out scores over a (gamma, cost) grid on this one problem (lssvm_reduced.hip); every output leads with the gamma dimension */
    virtual void fit_reduced_grid(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *gammas, size_t num_gammas,
                                  const double *costs, size_t num_costs, int factor, int product, double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out,
                                  double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_grid_info *infos,
                                  lssvm_dense_info *dense) = 0;  // lssvm_mi355_problem_fit_reduced_grid
    virtual void landmark_acc(const uint64_t *landmarks, uint64_t rank, int product, double *D_out) = 0;  // lssvm_mi355_problem_landmark_acc
    /* the leave-one-out scores of every prefix rank of one fit over a cost grid (lssvm_reduced.hip); every output leads with cost, then checkpoint */
    virtual void fit_reduced_rank_path(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const uint64_t *ranks,
                                       size_t num_ranks, const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out, double *press_out,
                                       uint64_t *loo_errors_out, double *leverage_out, double *fitted_out, double *loo_out, uint64_t *landmarks_out, lssvm_reduced_rank_info *infos,
                                       lssvm_dense_info *dense) = 0;  // lssvm_mi355_problem_fit_reduced_rank_path
    virtual void reduced_leverage_prefix(uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *V, const double *shift, const double *Z, size_t k,
                                         const uint64_t *ranks, size_t num_ranks, double *h_out, double *f_out) = 0;  // lssvm_mi355_problem_reduced_leverage_prefix
    virtual void time_leverage_prefix_kernel(uint64_t rank, uint64_t slab_rows, size_t k, const uint64_t *ranks, size_t num_ranks, int repeats,
                                             double *prefix_ms_out) = 0;  // lssvm_mi355_problem_time_leverage_prefix_kernel
    /* the fixed-size kernel logistic regression by iteratively reweighted least squares (lssvm_logistic.hip) */
    virtual void fit_reduced_logistic(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, int factor, double tol,
                                      uint64_t max_iter, const double *betas0, const double *rhos0, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                                      lssvm_reduced_logistic_info *infos) = 0;  // lssvm_mi355_problem_fit_reduced_logistic
    virtual void reduced_logistic_step(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *betas,
                                       const double *rhos, double *eta_out, double *q_out, double *z_out, double *loss_out,
                                       uint64_t *floored_out) = 0;  // lssvm_mi355_problem_reduced_logistic_step
    /* landmark selection: the pivots of a greedy or randomly pivoted partial Cholesky factorisation (lssvm_select.hip) */
    virtual void select_landmarks(uint64_t rank, int method, uint64_t pool, uint64_t seed, double tol, uint64_t *landmarks_out, double *trace_out, double *residual_out,
                                  lssvm_landmark_select_info *info) = 0;  // lssvm_mi355_problem_select_landmarks
    virtual void cg_begin(const void *y, double eps) = 0;
    virtual void cg_step(uint64_t iterations, int *done_out) = 0;
    virtual void cg_finish(void *alpha_out, double *rho_out, lssvm_cg_info *info) = 0;
    virtual void synchronize() = 0;
    virtual int rebalance(const double *weights, int count) = 0;  // lssvm_mi355_problem_rebalance: 1 if the shares changed
    virtual void fill_info(lssvm_cg_info *info) = 0;
    virtual void ipc_export(void *blob_out, size_t blob_bytes) = 0;
    virtual void ipc_connect(const void *blobs, size_t total_bytes) = 0;
};

/* ------------------------------------------------------------------ one process per GPU without RCCL: HIP IPC + host flags ------------------------------------------------------------------ */
/* What one rank hands to the others (plain bytes; the application moves them, like the RCCL unique id). */
constexpr size_t IPC_BLOB_BYTES = 256;
struct IpcBlob {
    uint32_t magic;
    int32_t rank, world, device;
    uint64_t nvec;
    uint32_t real_size;
    int32_t pid;
    hipIpcMemHandle_t mem;  // this rank's partial K*v vector
    char shm_name[64];      // this rank's flag page (POSIX shared memory)
};
static_assert(sizeof(IpcBlob) <= IPC_BLOB_BYTES, "IpcBlob must fit the published blob size");

/* one rank's flag page: sequence numbers of the implicit matvecs, written by the owner only */
struct IpcFlags {
    std::atomic<uint64_t> ready;     // matvec s: my partial vector is complete in HBM
    std::atomic<uint64_t> consumed;  // matvec s: I have read every peer's partial vector
    std::atomic<uint32_t> abort;     // I gave up (error / timeout): peers stop waiting
};

class IpcPeers {
  public:
    IpcPeers(int rank, int world);
    ~IpcPeers();
    IpcPeers(const IpcPeers &) = delete;
    IpcPeers &operator=(const IpcPeers &) = delete;
    void connect(const IpcBlob *blobs, void *own_vector);
    /* block until every peer's `ready` (which = 0) or `consumed` (which = 1) counter has reached seq */
    void wait_all(int which, uint64_t seq, double timeout_s);

    int rank, world;
    std::string own_name;
    IpcFlags *own = nullptr;
    std::vector<IpcFlags *> flags;  // [world], own included
    std::vector<void *> vectors;    // [world]: the partial K*v vectors, own = the local pointer
    bool connected = false;
};

/* communicators of the devices of ONE process (ncclCommInitAll); cached per device list, destroyed at exit */
struct LocalComms {
    std::vector<int> devices;
    std::vector<ncclComm_t> comms;
    ~LocalComms();
};
std::shared_ptr<LocalComms> local_comms_for(const std::vector<int> &devices);  // lssvm_exchange.hip

struct LeverageArgs;  // what a leave-one-out pass of the fixed-size model works on (lssvm_reduced.hip)
struct PrefixArgs;    // ... and what the pass over every prefix rank works on (lssvm_reduced.hip)
/* what reduced_gram leaves on the device for the device-factored fits instead of releasing it: St as k_reduced_sum's packed 128 x 128 tiles, K_mm rank x rank */
struct ReducedOnDevice {
    DevBuf<double> St, Kmm;
};

/* Solver<T>: the CG driver (csvm.cpp:71-183 / gpu_csvm.hpp:477-654) over the shards that live in THIS process:
 *   - one shard, world 1: single GPU;
 *   - one shard, rank r of a world of processes: one process per GPU (torchrun), exchange = the process communicator (RCCL);
 *   - D shards on D devices: single process, one stream per device driven by the calling thread, exchange = RCCL (ncclCommInitAll,
 *     group calls) or peer kernels over xGMI.  This is the mode behind plssvm::csvm (the reference drives all its devices from one
 *     process too, gpu_csvm.hpp:283-299, :574-593).
 * Every shard runs the identical O(n) kernels on the identical exchanged vector, so all CG scalars are bit-equal on all shards and
 * the host reads the stop criterion from shard 0 only. */
template <typename T>
class Solver final : public ProblemBase {
  public:
    /* `opt`: the options of THIS solve (the caller's lssvm_mi355_options, or a snapshot of the process defaults) */
    Solver(const Options &opt, const lssvm_params &params, const void *X, int mem_kind, size_t num_points, size_t num_features, const std::vector<int> &devices, const lssvm_shard *shard);
    ~Solver() override;

    void get_q(void *q_out, double *QA_cost_out) override;
    void set_weights(const double *weights, size_t num_points) override;
    void matvec(const void *d, void *ret_inout, double add) override;
    void matvec_pair(const void *d0, const void *d1, void *ret0_inout, void *ret1_inout, double add, int *two_vector_out) override;
    void solve_lockstep(const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out, double *rhos_out, lssvm_cg_info *infos_out, uint64_t *passes_out) override;
    /* every cost of a grid from ONE multi-shift CG sequence on this problem's single-vector pass (lssvm_path.hip) */
    void solve_cost_path(const void *y, const double *costs, size_t num_costs, double eps, uint64_t max_iter, bool verify, void *alphas_out, double *rhos_out, lssvm_path_info *infos_out,
                         uint64_t *passes_out) override;
    /* the Nystrom preconditioner of this problem and the reference recipe's CG preconditioned with it (lssvm_precond.hip) */
    void build_preconditioner(uint64_t rank, const uint64_t *landmarks, lssvm_precond_info *info) override;
    void precond_landmarks(uint64_t *out) override;
    void precond_apply(const void *r, void *z_out) override;
    void solve_pcg(const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out, double *rhos_out, lssvm_pcg_info *infos_out) override;
    /* the fixed-size model over m landmarks: [Phi | 1 | Y]^T [Phi | 1 | Y] on the fp64 matrix cores, slab by slab, and the host's solve (lssvm_reduced.hip) */
    void fit_reduced(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                     lssvm_reduced_info *info, const double *weights = nullptr) override;
    void landmark_gram(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *gram_out, const double *weights = nullptr) override;
    void time_gram_kernels(int repeats, double *parent_ms_out, double *mfma_ms_out, double *max_diff_out) override;
    /* leave-one-out with the landmark set held fixed, every cost of a grid: pass 1 is reduced_gram, pass 2 the leverage kernel per slab and cost */
    void fit_reduced_loo(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out,
                         double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out,
                         lssvm_reduced_loo_info *infos, const double *weights = nullptr) override;
    void reduced_leverage(uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *V, const double *shift, const double *B_extra, size_t k, double *h_out,
                          double *f_out) override;
    void time_leverage_kernel(uint64_t rank, uint64_t slab_rows, size_t k, int repeats, double *gram_ms_out, double *leverage_ms_out) override;
    /* fit_reduced_loo at every gamma of a grid: the feature sums behind Phi are formed once per slab and pass and shared by the gammas */
    void fit_reduced_grid(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *gammas, size_t num_gammas,
                          const double *costs, size_t num_costs, int factor, int product, double *betas_out, double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out,
                          double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out, lssvm_reduced_grid_info *infos, lssvm_dense_info *dense) override;
    void landmark_acc(const uint64_t *landmarks, uint64_t rank, int product, double *D_out) override;
    /* every prefix rank of one fit: one Gram pass, the dense steps of `factor` per cost, one prefix leverage pass per cost */
    void fit_reduced_rank_path(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const uint64_t *ranks, size_t num_ranks,
                               const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out, double *press_out, uint64_t *loo_errors_out, double *leverage_out,
                               double *fitted_out, double *loo_out, uint64_t *landmarks_out, lssvm_reduced_rank_info *infos, lssvm_dense_info *dense) override;
    void reduced_leverage_prefix(uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *V, const double *shift, const double *Z, size_t k, const uint64_t *ranks,
                                 size_t num_ranks, double *h_out, double *f_out) override;
    void time_leverage_prefix_kernel(uint64_t rank, uint64_t slab_rows, size_t k, const uint64_t *ranks, size_t num_ranks, int repeats, double *prefix_ms_out) override;
    /* Newton's method on the logistic loss over the landmarks: per pass one walk over the Phi slabs, the step kernel, a weighted Gram pass and the dense steps of `factor`
     * per class (lssvm_logistic.hip) */
    void fit_reduced_logistic(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, int factor, double tol, uint64_t max_iter,
                              const double *betas0, const double *rhos0, double *betas_out, double *rhos_out, uint64_t *landmarks_out, lssvm_reduced_logistic_info *infos) override;
    void reduced_logistic_step(const void *Y, size_t num_rhs, const double *weights, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *betas, const double *rhos,
                               double *eta_out, double *q_out, double *z_out, double *loss_out, uint64_t *floored_out) override;
    /* fit_reduced and fit_reduced_loo with assembly, factorisation, solves and the triangular inverse on the device (lssvm_dense.hip) */
    void fit_reduced_dev(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, double *betas_out, double *rhos_out, uint64_t *landmarks_out,
                         lssvm_reduced_info *info, lssvm_dense_info *dense, const double *weights = nullptr) override;
    void fit_reduced_loo_dev(const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, const double *costs, size_t num_costs, double *betas_out,
                             double *rhos_out, double *leverage_out, double *fitted_out, double *loo_out, double *press_out, uint64_t *loo_errors_out, uint64_t *landmarks_out,
                             lssvm_reduced_loo_info *infos, lssvm_dense_info *dense, const double *weights = nullptr) override;
    /* the pivots of a partial Cholesky factorisation of K over the candidates, one launch pair per step on shard 0's stream (lssvm_select.hip) */
    void select_landmarks(uint64_t rank, int method, uint64_t pool, uint64_t seed, double tol, uint64_t *landmarks_out, double *trace_out, double *residual_out,
                          lssvm_landmark_select_info *info) override;
    void cg_begin(const void *y, double eps) override;
    /* cg_begin for the inner solve of the mixed-precision refinement: A e = r / max|r| from e = 0 -- b, the first residual and delta0 = b^T b come from ONE O(n) kernel
     * over the outer fp64 residual `r_dev` (device 0, complete when the call is made; `absmax_part_dev`: k_absmax's partials of it), no Gram pass.  cg_step follows as
     * after cg_begin; the solution is the device vector x_dev() */
    void cg_begin_from_zero(const double *r_dev, const double *absmax_part_dev, double eps);
    const T *x_dev() const { return shards_[0]->own_.x.p; }
    void cg_step(uint64_t iterations, int *done_out) override;
    int rebalance(const double *weights, int count) override;
    void cg_finish(void *alpha_out, double *rho_out, lssvm_cg_info *info) override;
    void synchronize() override;
    void fill_info(lssvm_cg_info *info) override;
    void ipc_export(void *blob_out, size_t blob_bytes) override;
    void ipc_connect(const void *blobs, size_t total_bytes) override;

    /* for a driver that runs on lanes of shard 0 (the lockstep solve here, the refinement in lssvm_refine.hip) */
    Problem<T> &shard0() { return *shards_[0]; }
    bool lanes_apply() const;  // one unsharded device without an exchange, where the two-vector kernel applies
    void wait_for_deltas();    // the host waits for what shard 0's stream holds: the deltas of the step are in their host words
    /* until the returned object goes: no other solve may begin on this handle, and its weights stay */
    [[nodiscard]] SetOnExit<bool> hold_busy() {
        in_cg_ = true;
        return SetOnExit<bool>(in_cg_, false);
    }

  private:
    enum class Exchange { none, process_rccl, local_rccl, peer, process_peer };
    enum class Vec { d, x, tmp };
    void apply_K(Vec which);  // every shard: Kres_ <- K * v (all rows)
    void exchange();
    void sync_all();
    PackDc<T> pack_with_direction(Problem<T> &p);
    void describe_path(lssvm_cg_info *info);
    void reset_cg(double eps, double y_last);  // cg_begin, cg_begin_from_zero: the host's counters and scalars of a new solve
    void read_delta0(double t0);               // ... and their end: delta0 is read, the handle is between begin and finish
    void solve_in_sequence(const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out, double *rhos_out, lssvm_cg_info *infos_out, uint64_t *passes_out);
    void solve_on_lanes(const T *Y, size_t num_rhs, double eps, uint64_t max_iter, T *alphas_out, double *rhos_out, lssvm_cg_info *infos_out, uint64_t *passes_out);
    Problem<T> &precond_problem(const char *what);                        // the checks every preconditioner entry point shares; shard 0
    void enqueue_precond_apply(const T *r, T *z, double *part_rz) const;  // z = r - Bhat G^-1 Bhat^T r and the partial sums of r.z
    Problem<T> &reduced_problem(const char *what, bool unweighted_only);  // the checks every entry point of the fixed-size model shares; shard 0 (lssvm_reduced.hip)
    /* what fit_reduced and landmark_gram share: the checks, the slabs, St (cols x cols, both triangles) and K_mm (rank x rank) on the host.  `weights` (N doubles on the
     * host, or NULL): St = Pt^T diag(w) Pt; `total_out`: what stands for N in the host's formulas -- the sum of the weights, N without them */
    void reduced_gram(const char *what, const void *Y, size_t num_rhs, uint64_t rank, const uint64_t *landmarks, uint64_t slab_rows, std::vector<uint64_t> &lm_out,
                      std::vector<double> &gram_out, std::vector<double> &kmm_out, lssvm_reduced_info &info, ReducedOnDevice *keep = nullptr, const double *weights = nullptr,
                      double *total_out = nullptr);
    /* pass 2 of fit_reduced_loo, and all of reduced_leverage: the Phi slabs again, the leverage kernel per slab and operand (lssvm_reduced.hip) */
    void leverage_pass(const std::vector<uint64_t> &lm, uint64_t slab_rows, LeverageArgs &args, GridSlabs<T> *grid = nullptr);
    /* pass 2 of fit_reduced_rank_path, and all of reduced_leverage_prefix: the Phi slabs again, the prefix leverage kernel per slab and operand (lssvm_reduced.hip) */
    void prefix_pass(const std::vector<uint64_t> &lm, uint64_t slab_rows, PrefixArgs &args);
    T *vec_of(Problem<T> &p, Vec which) const { return which == Vec::d ? p.own_.d.p : (which == Vec::x ? p.own_.x.p : p.tmp_.p); }

    Options opt_{};
    std::vector<std::unique_ptr<Problem<T>>> shards_;
    Exchange exchange_ = Exchange::none;
    std::shared_ptr<LocalComms> local_comms_;
    std::unique_ptr<IpcPeers> ipc_;  // Exchange::process_peer
    std::unique_ptr<Precond<T>> precond_;  // lssvm_mi355_problem_build_preconditioner (none until then)
    uint64_t xseq_ = 0;              // implicit matvecs exchanged so far
    Event ev_delta_;                 // shard 0's stream: delta of the iteration is on the host
    int world_ = 1;  // shards of the problem in total (all processes)
    int info_shard_ = -1;  // the shard whose tile-kernel times fill_info reports (-1: not chosen yet)

    // CG state (host side)
    double eps_ = 0.0;
    double delta0_ = 0.0, delta_ = 0.0;
    double delta_before_ = 0.0;  // the residuum one iteration before delta_ (0 = none yet): the stop test's forecast, cg_step
    int held_back_ = 0;          // iterations in a row whose next matvec was NOT enqueued ahead of the stop test because of that forecast
    double y_last_ = 0.0;
    uint64_t iter_ = 0;  // iterations done
    bool converged_ = false;
    bool begun_ = false;
    bool in_cg_ = false;  // between cg_begin and cg_finish: the weights may not change
    double setup_ms_ = 0.0, cg_wall_ms_ = 0.0;
};

/* measurement utility (mfma_ceiling.hip): TFLOP/s and held clock of a bare v_mfma_f32_16x16x32_bf16 loop on `device` */
void measure_bf16_mfma_ceiling(int device, int b_from_lds, double settle_ms, double *tflops_out, double *clock_ghz_out, double *nominal_tflops_out);

/* lssvm_mi355_solve_refined_f64 (lssvm_refine.hip); the arguments have been checked */
void solve_refined_f64(const Options &opt, const lssvm_params &params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights,
                       double eps, uint64_t max_iter, double *alphas_out, double *rhos_out, lssvm_cg_info *infos_out, lssvm_refine_info *refine_out, uint64_t *passes_out);

/* the arguments of lssvm_mi355_problem_solve_pcg / lssvm_mi355_solve_pcg_* and of the preconditioner's rank that need no device (lssvm_precond.hip) */
void check_pcg_arguments(const void *Y, size_t num_rhs, double eps, uint64_t max_iter, const void *alphas_out, const double *rhos_out, const lssvm_pcg_info *infos_out);
void check_precond_rank(uint64_t rank, size_t num_points);
/* the caller's `rank` landmarks checked (distinct, < num_points), or the library's own for NULL (lssvm_precond.hip) */
std::vector<uint64_t> resolve_landmarks(const uint64_t *landmarks, size_t rank, size_t num_points);

/* the arguments of lssvm_mi355_problem_fit_reduced / _landmark_gram / lssvm_mi355_fit_reduced_* that need no device (lssvm_reduced.hip); num_points 0: not known yet */
constexpr int REDUCED_MAX_RANK = 1024;
constexpr uint64_t REDUCED_DEFAULT_SLAB_ROWS = 65536;
void check_reduced_arguments(const void *Y, size_t num_rhs, uint64_t rank, uint64_t slab_rows, size_t num_points);
/* the weights of the weighted forms: each finite and >= 0, their sum (in index order: what is returned) finite and > 0; and their `factor`: 0 or 1 */
double check_reduced_weights(const double *weights, size_t num_points);
void check_reduced_factor(int factor);
/* the cost grid of lssvm_mi355_problem_fit_reduced_loo / lssvm_mi355_fit_reduced_loo_*: 1 ... REDUCED_LOO_MAX_COSTS costs, each finite and positive */
constexpr size_t REDUCED_LOO_MAX_COSTS = 64;
void check_reduced_loo_costs(const double *costs, size_t num_costs);
/* what lssvm_mi355_problem_fit_reduced_grid / lssvm_mi355_fit_reduced_grid_* add to those: the gammas (each finite and > 0), at most REDUCED_GRID_MAX_CELLS (gamma, cost)
 * cells, `product` 0 or 1, and a kernel function that has a gamma to vary */
constexpr size_t REDUCED_GRID_MAX_CELLS = 64;
void check_reduced_grid_arguments(const double *gammas, size_t num_gammas, size_t num_costs, int product);
void check_reduced_grid_kernel(int kernel_type);
/* what lssvm_mi355_problem_fit_reduced_rank_path / lssvm_mi355_fit_reduced_rank_path_* add to the cost grid: 1 ... REDUCED_RANK_PATH_MAX_RANKS checkpoints, strictly
 * ascending, each in [1, rank], and at most REDUCED_GRID_MAX_CELLS (cost, checkpoint) cells */
constexpr size_t REDUCED_RANK_PATH_MAX_RANKS = 16;
void check_reduced_rank_list(const uint64_t *ranks, size_t num_ranks, uint64_t rank, size_t num_costs);
/* what lssvm_mi355_problem_fit_reduced_logistic / lssvm_mi355_fit_reduced_logistic_* add to the weighted fit (lssvm_logistic.hip): tol finite and > 0, max_iter >= 1, start
 * values both given or both NULL and finite; and, once N is known (num_points > 0), labels of exactly -1 or +1 (`dtype`: that of Y) */
void check_reduced_logistic_arguments(double tol, uint64_t max_iter, const double *betas0, const double *rhos0, size_t num_rhs, uint64_t rank);
void check_reduced_logistic_labels(const void *Y, int dtype, size_t num_rhs, size_t num_points);

/* the arguments of lssvm_mi355_problem_select_landmarks / lssvm_mi355_select_landmarks_* that need no device (lssvm_select.hip); returns the number of candidates */
constexpr int SELECT_MAX_RANK = 1024;
size_t check_select_arguments(uint64_t rank, int method, uint64_t pool, double tol, const uint64_t *landmarks_out, size_t num_points);

/* the arguments of lssvm_mi355_problem_solve_cost_path / lssvm_mi355_solve_cost_path_* that need no device: checked before one is touched (lssvm_path.hip) */
constexpr size_t PATH_MAX_COSTS = 64;
void check_cost_path_arguments(const void *y, const double *costs, size_t num_costs, double eps, uint64_t max_iter, const void *alphas_out, const double *rhos_out, const lssvm_path_info *infos_out);

/* one-shot helpers used by the C ABI */
template <typename T>
void predict_values(const Options &opt, const lssvm_params &params, const T *sv, size_t nsv, size_t nfeat, const T *alpha, T rho, T *w_inout, int *w_valid, const T *points,
                    size_t npoints, T *out, lssvm_predict_info *info);
/* predict_values for `nvec` weight vectors over the SAME support vectors (a one-vs-all model): alpha [nvec][nsv], rho [nvec], w_inout [nvec][nfeat] (linear kernel),
 * out [npoints][nvec]; column v holds the bits predict_values gives for (alpha[v], rho[v]).  Both point sets are uploaded and prepared once. */
template <typename T>
void predict_values_multi(const Options &opt, const lssvm_params &params, const T *sv, size_t nsv, size_t nfeat, const T *alpha, const T *rho, size_t nvec, T *w_inout, int *w_valid,
                          const T *points, size_t npoints, T *out, lssvm_predict_info *info);
template <typename T>
void calculate_w(const T *sv, size_t nsv, size_t nfeat, const T *alpha, T *w_out);

/* The resident predictor (round 6; lssvm_mi355_predictor_*): a model kept in HBM across predict calls -- csvm::predict_values (csvm.hpp:204-208) uploads and prepares the
 * support vectors on every call, which is the whole cost of a small batch.  create() prepares them once (centring, norms, operand planes, packed records; the linear
 * kernel: w); predict() uploads a batch of points, prepares it alike and runs the product.  What a batch cannot do on the resident form (see Predictor<T>::predict) goes
 * through the one-shot path with the host copies kept here: the result is the same either way. */
struct PredictorBase {
    int dtype = 0;
    virtual ~PredictorBase() = default;
    /* points AND out of mem_kind; out [npoints][the predictor's number of weight vectors].  `multi`: the call is lssvm_mi355_predictor_predict_multi -- the same values, and info->vectors_per_launch
     * reports the largest number of vectors one product launch evaluated; without it (lssvm_mi355_predictor_predict) that field is 0 and a predictor of several
     * vectors refuses the call */
    virtual void predict(const void *points, int mem_kind, size_t npoints, void *out, lssvm_predict_info *info, bool multi) = 0;
};
/* which resident forms a predictor may take: those of _create / _create_multi; FORMS_EVERY (lssvm_mi355_predictor_create_resident): every form on the one-pass kernels,
 * the fp64 one as well; FORMS_PANELS (lssvm_mi355_predictor_create_panels): those, and the models beyond the one-pass kernels on the panel kernels */
constexpr int FORMS_DEFAULT = 0, FORMS_EVERY = 1, FORMS_PANELS = 2;
/* alpha [nvec][nsv], rho [nvec] */
std::unique_ptr<PredictorBase> make_predictor(const Options &opt, const lssvm_params &params, int dtype, const void *sv, size_t nsv, size_t nfeat, const void *alpha, const double *rho,
                                              size_t nvec, int forms = FORMS_DEFAULT);

/* The fixed-size model from a stream of chunks (lssvm_mi355_reduced_stream_*; lssvm_reduced.hip): the landmark rows, K_mm, the running St and one
 * pending slab, kept on device 0 across update calls.  include/plssvm_amd.h has the contract of every call. */
struct ReducedStreamBase {
    virtual ~ReducedStreamBase() = default;
    virtual void update(const void *X, const void *Y, const double *w, size_t n) = 0;
    virtual void solve(const double *costs, size_t num_costs, int factor, double *betas_out, double *rhos_out, lssvm_reduced_loo_info *infos) = 0;
    virtual void loo(const void *X, const void *Y, const double *w, size_t n, double *h_out, double *f_out, double *loo_out) = 0;
    virtual void phi(const void *X, size_t n, double *phi_out) = 0;
    virtual void export_state(double *gram_out, double *kmm_out, uint64_t *num_points_out, uint64_t *fingerprint_out) = 0;
    virtual void merge_state(const double *gram, uint64_t num_points, const uint64_t *fingerprint) = 0;
    virtual void info(lssvm_reduced_stream_info *out, double *centre_out, double *kmm_out) const = 0;
    /* measurement aid (include/plssvm_amd_testing.h): device time of k_cross_product and of k_landmark_product at the same shape, `repeats` runs each after one untimed */
    virtual void time_kernels(const void *X, size_t n, int repeats, double *cross_ms_out, double *landmark_ms_out) = 0;
};
/* what lssvm_mi355_reduced_stream_create_* refuses before a device is touched */
void check_reduced_stream_arguments(const lssvm_params *params, const void *landmark_rows, size_t rank, size_t num_features, size_t num_rhs, uint64_t slab_rows);
std::unique_ptr<ReducedStreamBase> make_reduced_stream(const lssvm_params &params, int dtype, const void *landmark_rows, size_t rank, size_t num_features, size_t num_rhs, bool weighted,
                                                       uint64_t slab_rows);

void check_params(const lssvm_params *params);
/* weighted LS-SVM:`weights` holds num_points entries, each finite and > 0, whose diagonal terms 1/(C w_i) are finite in the real type T */
template <typename T>
void check_weights(const double *weights, size_t num_points, double cost);
int select_device_checked(int device);
/* `num_devices` == 0: automatic (all visible devices, but at least 32 row blocks per device); `devices` may be NULL (0 .. num_devices-1) */
std::vector<int> resolve_devices(const int *devices, int num_devices, size_t num_points);

/* ------------------------------------------------------------------ shared by lssvm_problem.hip and lssvm_predict.hip ------------------------------------------------------------------ */
constexpr double FOLD_MAX_R2 = 200.0;    // folded rbf records (KT_RBFF) only while |c| = R2 / 2 <= 100: 2^c and 2^acc stay far inside the fp32 range
constexpr double PAIR_FOLD_MAX_C = 32.0; // 256-row kernels, rbf: row AND column term folded (K = e_i 2^(x_i.x_j) e_j) only while |c| <= 32: the partial sums then carry at most 2^32 of
                                         // extra scale (RBF_DIRECT_ABOVE = 32 keeps the automatic choice at |c| <= 16)
constexpr int PAIR_MIN_TILES = 64;       // 256-row workgroups from this many row blocks on (a rule on the global shape: every rank decides alike)
constexpr int SPLIT_MAX_FEATURES = 384;  // the bf16x6 kernels exist for 1 ... 6 chunks of 64 features (row panel = 3 planes in registers)
constexpr int F16_MAX_FEATURES = 512;    // the f16x3 kernels exist for 1 ... 8 chunks of 64 features (row panel = 2 planes in registers)
constexpr int F16_LINEAR_MAX_FEATURES = 1 << 20;
constexpr int F16_RBF_MAX_FEATURES = 384;  // ... rbf: 1 ... 6 chunks (three row planes in registers: the shifted planes, see make_planes)
constexpr int F16_RBF_SHIFT = 6;         // rbf: the planes are (2^-6 hi, 2^6 mid, 2^6 hi)
constexpr int F16_TARGET_EXP = 14;       // f16x3, linear / polynomial: the planes carry 2^k x with max |2^k x| in [2^14, 2^15) (f16 overflows at 65504)
constexpr int F16_MAX_SHIFT = 40;        // |k| is clamped here (2^(-2k) must stay a normal float beside gamma)
constexpr float F16_REL2_MAX = 0x1p-44f; // accepted relative representation error of a row, squared: |x - (hi + mid)| <= 2^-22 |x| in the 2-norm
constexpr float F16_ABS_MAX = 0x1p-22f;  // rbf: accepted bound on the ABSOLUTE error of the exponent from the representation, 2 max|rest| max|x|
/* the representability check of make_planes on the statistics of k_split_f16x2: two f16 planes represent the data -- relative error of every row at most 2^-22, or for rbf
 * an absolute bound on the exponent's error, 2 max|rest| max|x| <= F16_ABS_MAX (false for a NaN: an overflowing plane) */
inline bool f16_planes_pass(bool rbf, float rel2, float rest2, float x2) {
    if (rel2 <= F16_REL2_MAX) return true;
    return rbf && std::isfinite(rel2) && 2.0 * std::sqrt(static_cast<double>(rest2) * static_cast<double>(x2)) <= static_cast<double>(F16_ABS_MAX);
}

template <typename T>
T rbf_prescale(const lssvm_params &p, bool fp64_v2);
bool wide_nonlinear_f64(const Options &o, const lssvm_params &p, size_t num_features);
bool wide_nonlinear(const Options &o, const lssvm_params &p, bool rbf_direct, size_t num_features);
bool wide_pair_routed(int plane_mode, int kernel_type, int degree, int nk64);  // the resident fp32 predictor beyond 128 features: one two-vector launch for a pair?
bool panel_pair_routed(int dtype, int plane_mode, int kernel_type, int degree, int panels);  // the resident predictors on the panel kernels: one two-vector launch for a pair?
bool sym_pair_routed(int plane_mode, int kernel_type, int degree, int nk64);   // the fp32 lockstep CG on 129 ... 512 features: one symmetric two-vector launch for a pair of right-hand sides?
template <typename T>
void set_kernel_scalars(TileArgs<T> &a, const lssvm_params &p, bool rbf_direct);
template <typename T>
void set_launch_options(TileArgs<T> &a, const Options &o);
template <typename T>
void column_means(const DeviceMatrix<T> &M, DevBuf<T> &mean, hipStream_t s);
template <typename T>
double max_centred_sqnorm(const DeviceMatrix<T> &M, const DevBuf<T> &mean, hipStream_t s);
template <typename T>
bool rbf_wants_direct_form(const Options &o, const lssvm_params &p, const DeviceMatrix<T> &M, const DeviceMatrix<T> *M2, hipStream_t s, double *r2_out);
void make_planes(const Options &o, const lssvm_params &p, bool rbf_direct, const DeviceMatrix<float> &M, const DeviceMatrix<float> *M2, PlaneSet &out, PlaneSet *out2, hipStream_t s,
                 bool wide_nl = false, bool linear_panels = false, bool f16_known_bad = false);
bool rbf_wants_grid_planes(const Options &o, const lssvm_params &p, size_t num_features, double r2);
float make_grid_planes(const DeviceMatrix<float> &M, double r2_in, PlaneSet &out, float *chg, DevBuf<float> &efac, hipStream_t s, bool wide_nl);
void set_plane_args(TileArgs<float> &a, const lssvm_params &p, const PlaneSet &cols, const PlaneSet &rows, size_t col_rows_alloc, size_t row_rows_alloc);
void enqueue_pack_records(const float *dvec, const float *cc, int ncols_padded, float *dc, int folded, const float *efac, hipStream_t s);
void enqueue_pack_records(const double *dvec, const double *cc, int ncols_padded, double *dc, int folded, const double *efac, hipStream_t s);
/* the records of TWO weight vectors for the rectangular 256-row kernel's NV = 2 instance: (d0 | d1), folded: both times 2^c_j (k_pack_dc2) */
void enqueue_pack_records2(const float *dvec0, const float *dvec1, const float *cc, int ncols_padded, float *dc, int folded, hipStream_t s);
/* ... and for the fp64 v2 kernel's NV = 2 instance: (d0 | d1 | c), 192 reals per 64-column sub-tile (k_pack_dc2_f64, nothing cleared) */
void enqueue_pack_records2(const double *dvec0, const double *dvec1, const double *cc, int ncols_padded, double *dc, hipStream_t s);
void enqueue_planes_fragment_major(const uint16_t *planes, size_t plane_elems, int rows_alloc, int ldx16, int nplanes, uint16_t *frag, hipStream_t s);

}  // namespace lssvm
