/*
 * lssvm_predict.hip -- csvm::predict_values behind the C ABI (reference: src/plssvm/backends/OpenMP/csvm.cpp:188-227,
 * include/plssvm/backends/HIP/predict_kernel.hip.hpp:34-117, gpu_csvm.hpp:656-730): the one-shot call, calculate_w, and the resident predictor.  A rectangular instance
 * of the tile kernels -- rows = the points to predict, columns = the support vectors -- prepared with the helpers of lssvm_problem.hip (declared in lssvm_problem.hip.hpp).
 */
#include "lssvm_problem.hip.hpp"

#include "lssvm_kernels.hip.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace lssvm {

/* ------------------------------------------------------------------ predict path ------------------------------------------------------------------ */
/* What the rectangular 256-row kernel (tile_matvec_f32_pair_rect) needs besides the planes: the row side once more fragment-major (a wave's load instruction reads
 * 1 KiB in one piece), the item list of the whole rectangle in XCD-lane order (xcd_lane_order: the workgroups of an XCD share their column stream in its L2), and the
 * counters of a persistent launch.  Used by the one-shot predict_values and by the resident predictor. */
struct RectSetup {
    DevBuf<uint16_t> frag;
    DevBuf<int2> items;
    DevBuf<unsigned> queue;
};
static void setup_rect_launch(TileArgs<float> &ta, RectSetup &rs, const PlaneSet &planesP, int rows_alloc, int num_ib, int num_jc, hipStream_t s) {
    const size_t plane_elems = static_cast<size_t>(rows_alloc) * planesP.ldx16;
    rs.frag.alloc_zero(static_cast<size_t>(planesP.nplanes) * plane_elems, s);
    enqueue_planes_fragment_major(planesP.buf.p, plane_elems, rows_alloc, planesP.ldx16, planesP.nplanes, rs.frag.p, s);
    const int pairs = num_ib / 2;
    std::vector<std::vector<WorkItem>> by_chunk(static_cast<size_t>(num_jc));
    for (int jc = 0; jc < num_jc; ++jc) {
        by_chunk[static_cast<size_t>(jc)].reserve(static_cast<size_t>(pairs));
        for (int pr = 0; pr < pairs; ++pr) by_chunk[static_cast<size_t>(jc)].push_back({ 2 * pr, jc });
    }
    const std::vector<WorkItem> items = xcd_lane_order(by_chunk);
    rs.items.alloc_zero(items.size(), s);
    LSSVM_HIP_CHECK(hipMemcpyAsync(rs.items.p, items.data(), items.size() * sizeof(WorkItem), hipMemcpyHostToDevice, s));
    LSSVM_HIP_CHECK(hipStreamSynchronize(s));  // `items` goes out of scope
    int cus = 256;
    LSSVM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    ta.items = rs.items.p;
    ta.num_items = static_cast<int>(items.size());
    if (ta.num_items > cus) {
        rs.queue.alloc_zero(512, s);
        ta.queue = rs.queue.p;
        ta.queue_next = rs.queue.p + 256;
        ta.queue_grid = cus;
    }
    ta.Xr16f = rs.frag.p;
    ta.row_pair = 1;
    ta.rect = 1;
}

/* out_p = w . x_p - rho: one pass over the points, HBM bound.  A group of L lanes (a power of two, at most 64) owns a point and reads its row in 16-byte pieces, so
 * that a wave's load instruction covers 1 KiB of consecutive memory wherever a row has at least 16 bytes x L. */
template <typename T>
static void launch_predict_linear(const DeviceMatrix<T> &P, const T *w, T rho, T *out, hipStream_t s, int out_stride = 1) {
    constexpr int V = 16 / static_cast<int>(sizeof(T));  // elements per 16-byte piece
    const int pieces = P.ldx / V;                         // (ldx is a multiple of the k-chunk: 32 floats / 16 doubles)
    int L = 1;
    while (2 * L <= std::min(pieces, 64)) L *= 2;
    const int rows_per_block = 256 / L;
    const dim3 grid(static_cast<unsigned>((P.rows + rows_per_block - 1) / rows_per_block));
    switch (L) {
        case 4: hipLaunchKernelGGL((k_predict_linear_rows<T, 4>), grid, dim3(256), 0, s, P.data.p, P.ldx, P.rows, w, rho, out, out_stride); break;
        case 8: hipLaunchKernelGGL((k_predict_linear_rows<T, 8>), grid, dim3(256), 0, s, P.data.p, P.ldx, P.rows, w, rho, out, out_stride); break;
        case 16: hipLaunchKernelGGL((k_predict_linear_rows<T, 16>), grid, dim3(256), 0, s, P.data.p, P.ldx, P.rows, w, rho, out, out_stride); break;
        case 32: hipLaunchKernelGGL((k_predict_linear_rows<T, 32>), grid, dim3(256), 0, s, P.data.p, P.ldx, P.rows, w, rho, out, out_stride); break;
        default: hipLaunchKernelGGL((k_predict_linear_rows<T, 64>), grid, dim3(256), 0, s, P.data.p, P.ldx, P.rows, w, rho, out, out_stride); break;
    }
}

/* w_v = sum_i alpha_v,i sv_i for `nvec` weight vectors (alpha [nvec][nsv], w_out [nvec][nfeat]): the support vectors are uploaded once, every vector runs the two stages of
 * calculate_w on them */
template <typename T>
static void calculate_w_multi(const T *sv, size_t nsv, size_t nfeat, const T *alpha, size_t nvec, T *w_out) {
    LSSVM_REQUIRE(sv != nullptr && nsv > 0, "The support vectors may not be empty!");                       // csvm.cpp:256
    LSSVM_REQUIRE(nfeat > 0, "Each support vector must at least contain one feature!");                     // csvm.cpp:257
    LSSVM_REQUIRE(alpha != nullptr && w_out != nullptr, "The alpha array may not be empty!");               // csvm.cpp:259
    select_device_checked(0);
    hipStream_t s = nullptr;
    DeviceMatrix<T> S;
    S.upload(sv, LSSVM_MEM_HOST, nsv, nfeat, 0, s);
    DevBuf<T> a, w;
    a.alloc_zero(nvec * nsv, s);
    w.alloc_zero(nvec * nfeat, s);
    LSSVM_HIP_CHECK(hipMemcpyAsync(a.p, alpha, nvec * nsv * sizeof(T), hipMemcpyHostToDevice, s));
    // w[f] = sum_i alpha_i sv[i][f]: partial sums over blocks of 256 support vectors (coalesced across the features), then the blocks in order -- the reference's chain
    // (csvm.cpp:255-280) is one sequential fma chain per feature; 128 threads walking 50 000 rows each took 10 ms where the matrix is read in 10 us
    const int rows_per_block = 256;
    const int nblocks = (S.rows + rows_per_block - 1) / rows_per_block;
    DevBuf<double> part;
    part.alloc_zero(static_cast<size_t>(nblocks) * S.ldx, s);
    for (size_t v = 0; v < nvec; ++v) {
        hipLaunchKernelGGL(k_calculate_w_stage1<T>, dim3(nblocks, (S.ldx + 255) / 256), dim3(256), 0, s, S.data.p, S.ldx, S.rows, rows_per_block, a.p + v * nsv, part.p);
        hipLaunchKernelGGL(k_calculate_w_stage2<T>, dim3((S.dfeat + 255) / 256), dim3(256), 0, s, part.p, nblocks, S.ldx, S.dfeat, w.p + v * nfeat);
    }
    LSSVM_HIP_CHECK(hipGetLastError());
    LSSVM_HIP_CHECK(hipMemcpyAsync(w_out, w.p, nvec * nfeat * sizeof(T), hipMemcpyDeviceToHost, s));
    LSSVM_HIP_CHECK(hipStreamSynchronize(s));
}
template <typename T>
void calculate_w(const T *sv, size_t nsv, size_t nfeat, const T *alpha, T *w_out) {
    calculate_w_multi<T>(sv, nsv, nfeat, alpha, 1, w_out);
}

/* device time of the product launches of a call (what the reference times as "predict", gpu_csvm.hpp:656-730, is the whole call: total_ms): an event pair around each
 * launch, summed when the stream has drained.  `capacity`: the launches to come -- the events must not move once recorded */
struct LaunchTimer {
    std::vector<Event> evs;
    explicit LaunchTimer(size_t capacity) { evs.reserve(2 * capacity); }
    template <typename F>
    void timed(hipStream_t s, F &&launch) {
        evs.emplace_back();
        evs.emplace_back();
        const size_t k = evs.size() - 2;
        evs[k].create(true);
        evs[k + 1].create(true);
        LSSVM_HIP_CHECK(hipEventRecord(evs[k].e, s));
        launch();
        LSSVM_HIP_CHECK(hipEventRecord(evs[k + 1].e, s));
    }
    void sum_into(lssvm_predict_info &info) const {
        double sum = 0.0;
        bool ok = !evs.empty();
        for (size_t k = 0; k + 1 < evs.size(); k += 2) {
            float ms = 0.0f;
            ok = ok && hipEventElapsedTime(&ms, evs[k].e, evs[k + 1].e) == hipSuccess;
            sum += ms;
        }
        if (ok) info.kernel_ms = sum;
    }
};

/* The end of every predict call, linear or not: the values to the caller (to HBM for a batch that came from there), the stream drained, the call's times.  `lap`: see
 * ProductStage::run. */
static constexpr auto no_lap = [](const char *) {};
template <typename T, typename Lap>
static void finish_predict(const LaunchTimer &timer, const DevBuf<T> &o, T *out, int mem_kind, hipStream_t s, double t0, double t_kernel, int per_launch, lssvm_predict_info &info,
                           Lap &&lap) {
    LSSVM_HIP_CHECK(hipGetLastError());
    lap("product, row sums");
    LSSVM_HIP_CHECK(hipMemcpyAsync(out, o.p, o.count * sizeof(T), mem_kind == LSSVM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    LSSVM_HIP_CHECK(hipStreamSynchronize(s));
    lap("values downloaded");
    timer.sum_into(info);
    info.total_ms = now_ms() - t0;
    info.setup_ms = t_kernel - t0;
    info.vectors_per_launch = per_launch;
}

/* ------------------------------------------------------------------ the product stage ------------------------------------------------------------------ */
/* Round 6: from 64 row blocks of points on, on at most 128 features, the RECTANGULAR 256-row kernel (tile_matvec_f32_pair_rect, lssvm_tile_f32_pair.hip.hpp) -- eight
 * waves of a pair of row blocks share one stream of the support vectors' planes, in persistent launches that draw their items from per-XCD counters, like the
 * training matvec's kernel; the 128-row full-square kernels ran this product at 0.49 of the 16-bit peak where the solve's kernel reaches 0.57 (200 000 points x
 * 50 000 support vectors x 128).  The conditions of Problem<float>'s pair_ that every caller shares (split planes are the caller's
 * to check): no run-time integer power, rbf with both exponent terms folded (`rbf_folded` records and |c| = r2 / 2 <= PAIR_FOLD_MAX_C). */
static bool rect_kernel_applies(const Options &opt, const lssvm_params &params, int ldx16, bool rbf_folded, double r2, int num_ib) {
    const bool poly_generic = params.kernel_type == LSSVM_KERNEL_POLYNOMIAL && params.degree != 2 && params.degree != 3;
    const bool rbf_ok = params.kernel_type != LSSVM_KERNEL_RBF || (rbf_folded && r2 <= 2.0 * PAIR_FOLD_MAX_C);
    return ldx16 <= 128 && !poly_generic && rbf_ok && opt.mfma_shape >= 3 && num_ib >= PAIR_MIN_TILES;
}

/* out[p][v] = sum_j alpha_v,j k(sv_j, p) - rho[v] for `nvec` weight vectors: the rectangular instance of the tile kernels behind the one-shot call and both resident
 * predictors.  Rows = the points P (padded to whole pairs of row blocks), columns = the support vectors S, both prepared by the caller.  The stage owns the slabs of
 * partial row sums, the values and the launches' timer; a caller sets the operand-specific launch arguments on what args() returns and calls run() once.
 * `records(v, count) -> const T *`: the column records of the launch group that starts at weight vector v and holds `count` (1 or 2) vectors, NULL for a kernel that
 * reads none.  A caller that packs records on the stream does so inside the callable: args() asks for group 0 -- in front of whatever the caller enqueues next and of the
 * drain that precedes the timed region --, run() for every later group immediately in front of its launch. */
template <typename T>
struct ProductStage {
    const Options &opt;
    const DeviceMatrix<T> &P, &S;
    const bool rect;  // the rectangular 256-row kernel: the caller's decision (rect_kernel_applies) and the caller's setup_rect_launch
    const T *const alpha, *const rho;  // [nvec][S.rows_alloc] in HBM, exact zeros beyond the support vectors; [nvec] on the host
    const int nv, per_launch, num_ib, num_jt;
    const int jc_tiles, num_jc;  // column tiles per work item (product_chunk_tiles, lssvm_geometry.cpp) and the column chunks they make
    const size_t part_plane;
    const hipStream_t s;
    const double t0;    // the caller's start of the call
    LaunchTimer timer;  // around every launch of the kernel that does the product, and nothing else
    DevBuf<T> partial, Kv, o;

    ProductStage(const Options &options, const DeviceMatrix<T> &points, const DeviceMatrix<T> &svs, bool rect256, const T *alphas, const T *rhos, size_t nvec, int vectors_per_launch,
                 hipStream_t stream, double t_begin) :
        opt(options), P(points), S(svs), rect(rect256), alpha(alphas), rho(rhos), nv(static_cast<int>(nvec)), per_launch(vectors_per_launch), num_ib(points.rows_alloc / TILE),
        num_jt(svs.rows_alloc / TILE), jc_tiles(product_chunk_tiles(geometry_options(options), rect256, num_ib, num_jt)), num_jc(num_chunks(num_jt, jc_tiles, 0, 0)), part_plane(static_cast<size_t>(num_jc) * points.rows_alloc), s(stream), t0(t_begin), timer(nvec) {
        partial.alloc_zero(per_launch * part_plane, s);
        Kv.alloc_zero(P.rows_alloc, s);
        o.alloc_zero(static_cast<size_t>(P.rows) * nvec, s);
    }

    /* the launch arguments every caller shares: both sides (`cr` / `cc`: their rbf norms), the slabs, the geometry, the kernel's scalars, and group 0's vector and records */
    template <typename Records>
    TileArgs<T> args(const lssvm_params &params, bool rbf_direct, const T *cr, const T *cc, Records &&records) const {
        TileArgs<T> ta{};
        ta.Xr = P.data.p;
        ta.Xc = S.data.p;
        ta.cr = cr;
        ta.cc = cc;
        ta.dvec = alpha;
        ta.dc = records(0, std::min(per_launch, nv));
        ta.partial = partial.p;
        ta.part_stride = P.rows_alloc;
        ta.ldx = S.ldx;
        ta.kchunks = S.ldx / kchunk_of<T>();
        ta.num_ib = num_ib;
        ta.num_jt = num_jt;
        ta.jc_tiles = jc_tiles;
        ta.ncols_valid = S.rows;
        set_kernel_scalars(ta, params, rbf_direct);
        set_launch_options(ta, opt);
        return ta;
    }

    /* The launch groups in order, each followed by its vectors' row sums, then the end of the call (finish_predict).  `repeat`: extra untimed launches of group 0 in
     * front of the timed one -- the product overwrites its slabs, the result is the same -- (predict_values' measurement aid).  `lap(label)`: called where the set-up,
     * the product and the download end (the resident fp32 form's LSSVM_MI355_DEBUG laps). */
    template <typename Records, typename Lap>
    void run(TileArgs<T> &ta, int kernel_type, bool rbf_direct, Records &&records, T *out, int mem_kind, lssvm_predict_info &info, Lap &&lap, int repeat = 1) {
        const auto launch = [&] { launch_tile_kernel<T>(ta, kernel_type, rbf_direct, num_jc, s); };
        const auto next_counters = [&] {  // (a persistent launch zeroes the OTHER set of counters)
            if (ta.queue != nullptr) std::swap(ta.queue, ta.queue_next);
        };
        LSSVM_HIP_CHECK(hipStreamSynchronize(s));
        lap(rect ? "slabs, 256-row launch set up" : "slabs");
        const double t_kernel = now_ms();
        for (int k = 0; k + 1 < repeat; ++k) {
            launch();
            next_counters();
        }
        for (int v = 0; v < nv; v += per_launch) {
            const int count = std::min(per_launch, nv - v);
            if (v > 0) {  // (group 0: set by args())
                ta.dc = records(v, count);
                ta.dvec = alpha + static_cast<size_t>(v) * S.rows_alloc;
                next_counters();
            }
            ta.nvec = count;
            ta.part_vstride = count == 2 ? static_cast<long>(part_plane) : 0;
            timer.timed(s, launch);
            for (int u = 0; u < count; ++u) {
                hipLaunchKernelGGL(k_reduce_partials<T>, dim3((P.rows_alloc + 255) / 256), dim3(256), 0, s, partial.p + u * part_plane, ta.part_stride, num_jc, 0, P.rows_alloc, Kv.p);
                hipLaunchKernelGGL(k_sub_rho<T>, dim3((P.rows + 255) / 256), dim3(256), 0, s, Kv.p, P.rows, rho[v + u], o.p + (v + u), nv);
            }
        }
        finish_predict(timer, o, out, mem_kind, s, t0, t_kernel, per_launch, info, lap);
    }
};

/* `nvec` weight vectors over the same support vectors: alpha [nvec][nsv], rho [nvec], w_inout [nvec][nfeat], out [npoints][nvec] (nvec = 1: predict_values).  Everything up
 * to the records of the weight vectors is done once; `repeat`: extra untimed launches of the product in front of the timed one (predict_values' measurement aid). */
template <typename T>
static void predict_values_impl(const Options &opt, const lssvm_params &params, const T *sv, size_t nsv, size_t nfeat, const T *alpha, const T *rho, size_t nvec, T *w_inout, int *w_valid,
                                const T *points, size_t npoints, T *out, lssvm_predict_info &info, int repeat) {
    check_params(&params);
    LSSVM_REQUIRE(nvec > 0 && rho != nullptr, "predict_values needs at least one weight vector and its rho");
    LSSVM_REQUIRE(nvec <= static_cast<size_t>(1) << 20, "too many weight vectors");
    LSSVM_REQUIRE(sv != nullptr && nsv > 0, "The support vectors must not be empty!");                       // csvm.cpp:189
    LSSVM_REQUIRE(nfeat > 0, "The support vectors must contain at least one feature!");                      // csvm.cpp:190
    LSSVM_REQUIRE(alpha != nullptr, "The number of support vectors and number of weights must be the same!");  // csvm.cpp:192
    LSSVM_REQUIRE(points != nullptr && npoints > 0, "The data points to predict must not be empty!");        // csvm.cpp:194
    LSSVM_REQUIRE(out != nullptr && w_valid != nullptr, "out / w_valid must not be NULL");
    select_device_checked(0);
    hipStream_t s = nullptr;
    const double t0 = now_ms();
    const int nv = static_cast<int>(nvec);

    if (params.kernel_type == LSSVM_KERNEL_LINEAR) {
        LSSVM_REQUIRE(w_inout != nullptr, "w must have num_features entries for the linear kernel");
        if (!*w_valid) {  // csvm.cpp:204-207
            calculate_w_multi<T>(sv, nsv, nfeat, alpha, nvec, w_inout);
            *w_valid = 1;
        }
        LaunchTimer timer(nvec);
        DeviceMatrix<T> P;
        P.upload(points, LSSVM_MEM_HOST, npoints, nfeat, 0, s);
        DevBuf<T> w, o;
        w.alloc_zero(nvec * static_cast<size_t>(P.ldx), s);  // (zero padded like the points' rows: the kernel reads whole 16-byte pieces)
        o.alloc_zero(npoints * nvec, s);
        LSSVM_HIP_CHECK(hipMemcpy2DAsync(w.p, static_cast<size_t>(P.ldx) * sizeof(T), w_inout, nfeat * sizeof(T), nfeat * sizeof(T), nvec, hipMemcpyHostToDevice, s));
        LSSVM_HIP_CHECK(hipStreamSynchronize(s));
        const double t_kernel = now_ms();
        for (int v = 0; v < nv; ++v) timer.timed(s, [&] { launch_predict_linear<T>(P, w.p + static_cast<size_t>(v) * P.ldx, rho[v], o.p + v, s, nv); });
        finish_predict(timer, o, out, LSSVM_MEM_HOST, s, t0, t_kernel, 1, info, no_lap);
        return;
    }

    // polynomial / rbf: out_p = sum_i alpha_i k(sv_i, p) - rho : a rectangular instance of the tile kernel
    DeviceMatrix<T> S, P;
    S.upload(sv, LSSVM_MEM_HOST, nsv, nfeat, 0, s);
    // (the points padded to whole PAIRS of row blocks: the rectangular 256-row kernel below works on pairs; the padding is zero rows whose sums nobody reads)
    P.upload(points, LSSVM_MEM_HOST, npoints, nfeat, static_cast<size_t>(round_up(static_cast<long>(npoints), 2 * TILE)), s);
    DevBuf<T> cS, cP;
    double rbf_r2 = 0.0;
    bool rbf_direct = rbf_wants_direct_form<T>(opt, params, S, &P, s, &rbf_r2);  // same rule as the training matvec (Problem<T>)
    bool rbf_grid = false;
    if constexpr (std::is_same_v<T, float>) {
        if (rbf_wants_grid_planes(opt, params, nfeat, rbf_r2)) {
            rbf_grid = true;
            rbf_direct = false;
        }
    }
    DevBuf<T> eS, eP;  // grid planes: the folded factors E of the support vectors and of the points
    float grid_sigma = 1.0f;
    int dc_folded = 0;
    if (params.kernel_type == LSSVM_KERNEL_RBF && !rbf_direct) {
        center_columns<T>(S, &P, rbf_prescale<T>(params, v2_eligible_f64(opt, S.ldx) || wide_nonlinear_f64(opt, params, nfeat)), s);
        half_neg_norms<T>(S, cS, s);
        half_neg_norms<T>(P, cP, s);
    }
    bool wide = false;  // rbf / polynomial beyond the one-pass kernels: feature panels inside a tile (full-square instance)
    if constexpr (std::is_same_v<T, float>) {
        wide = wide_nonlinear(opt, params, rbf_direct, nfeat);
    } else {
        wide = wide_nonlinear_f64(opt, params, nfeat);
    }
    const bool v2 = wide || (std::is_same_v<T, float> ? v2_eligible(opt, S.ldx, rbf_direct) : v2_eligible_f64(opt, S.ldx));
    bool poly_prescaled = false;
    if constexpr (std::is_same_v<T, double>) {
        // the fp64 v2 kernel evaluates the polynomial on data that carries sqrt(gamma) (see Problem<T>'s constructor)
        if (v2 && params.kernel_type == LSSVM_KERNEL_POLYNOMIAL && params.gamma > 0.0) {
            const T sc = static_cast<T>(std::sqrt(params.gamma));
            hipLaunchKernelGGL(k_center<T>, dim3((S.dfeat + 255) / 256, S.rows), dim3(256), 0, s, S.data.p, S.ldx, S.dfeat, S.rows, static_cast<const T *>(nullptr), sc);
            hipLaunchKernelGGL(k_center<T>, dim3((P.dfeat + 255) / 256, P.rows), dim3(256), 0, s, P.data.p, P.ldx, P.dfeat, P.rows, static_cast<const T *>(nullptr), sc);
            LSSVM_HIP_CHECK(hipGetLastError());
            poly_prescaled = true;
        }
    }
    // fp32: both sides once more as operand planes (the split kernels, full-square instance: rows = points, columns = support vectors)
    PlaneSet planesS, planesP;
    if constexpr (std::is_same_v<T, float>) {
        if (v2 && rbf_grid) {
            grid_sigma = make_grid_planes(S, rbf_r2, planesS, cS.p, eS, s, wide);
            (void) make_grid_planes(P, rbf_r2, planesP, cP.p, eP, s, wide);  // (the same exponent scale: the same grid and the same sigma)
        } else if (v2) {
            make_planes(opt, params, rbf_direct, S, &P, planesS, &planesP, s, wide);
            if (wide && planesS.mode == 0) throw Error(LSSVM_ERR_INTERNAL, "no operand planes for the wide rbf / polynomial path");
            if (planesS.mode != 0) dc_folded = (params.kernel_type == LSSVM_KERNEL_RBF && opt.rbf_fold != 0 && rbf_r2 <= FOLD_MAX_R2 && !rbf_grid) ? 1 : 0;
        }
    }
    interleave_features<T>(S, s);
    interleave_features<T>(P, s);
    bool rect = false;  // (the rectangular 256-row kernel: here only beside the one-pass split kernels on the norm expansion)
    if constexpr (std::is_same_v<T, float>) {
        rect = v2 && !wide && !rbf_grid && !rbf_direct && planesS.mode != 0 && rect_kernel_applies(opt, params, planesS.ldx16, dc_folded != 0, rbf_r2, P.rows_alloc / TILE);
    }
    // the rectangular 256-row kernel takes the weight vectors two per pass (NV = 2: one evaluation of the Gram tile feeds both), an odd last one alone
    const int per_launch = (rect && nv >= 2) ? 2 : 1;
    DevBuf<T> a, dc;
    a.alloc_zero(nvec * S.rows_alloc, s);  // [nvec][rows_alloc], exact zeros beyond the support vectors
    ProductStage<T> stage(opt, P, S, rect, a.p, rho, nvec, per_launch, s, t0);
    LSSVM_HIP_CHECK(hipMemcpy2DAsync(a.p, static_cast<size_t>(S.rows_alloc) * sizeof(T), alpha, nsv * sizeof(T), nsv * sizeof(T), nvec, hipMemcpyHostToDevice, s));
    // rectangular instance of the tile kernel (full square variant): the v2 kernel when the feature count allows, with the
    // (alpha_j | c_j) records of the support vectors packed for its LDS-DMA -- one buffer, packed anew for every launch group
    const int ncols = stage.num_jt * TILE;
    const bool records = v2 && !(std::is_same_v<T, double> && params.kernel_type == LSSVM_KERNEL_POLYNOMIAL && !poly_prescaled);
    if (records) dc.alloc_zero(static_cast<size_t>(stage.num_jt) * 256, s);
    const auto pack_records = [&](int v, int count) -> const T * {  // the records of the weight vectors v (, v + 1) of the next launch
        if (!records) return nullptr;
        if constexpr (std::is_same_v<T, float>) {
            if (count == 2) {
                enqueue_pack_records2(a.p + static_cast<size_t>(v) * S.rows_alloc, a.p + static_cast<size_t>(v + 1) * S.rows_alloc, cS.p, ncols, dc.p, dc_folded, s);
            } else {
                enqueue_pack_records(a.p + static_cast<size_t>(v) * S.rows_alloc, cS.p, ncols, dc.p, rbf_grid ? 2 : dc_folded, rbf_grid ? eS.p : static_cast<const float *>(nullptr), s);
            }
        } else {
            enqueue_pack_records(a.p + static_cast<size_t>(v) * S.rows_alloc, cS.p, ncols, dc.p, 0, static_cast<const double *>(nullptr), s);
        }
        return dc.p;
    };
    TileArgs<T> ta = stage.args(params, rbf_direct, cP.p, cS.p, pack_records);
    ta.dc_folded = dc_folded;
    if (poly_prescaled) ta.gamma = T(1);
    if constexpr (std::is_same_v<T, float>) {
        if (planesS.mode != 0) set_plane_args(ta, params, planesS, planesP, static_cast<size_t>(S.rows_alloc), static_cast<size_t>(P.rows_alloc));
        if (rbf_grid) {
            ta.gamma = static_cast<T>(1.0 / (static_cast<double>(grid_sigma) * static_cast<double>(grid_sigma)));
            ta.er = eP.p;
            ta.rbf_grid = 1;
        }
    }
    ta.wide_panels = wide ? 1 : 0;
    RectSetup rect_setup;
    if constexpr (std::is_same_v<T, float>) {
        if (rect) setup_rect_launch(ta, rect_setup, planesP, P.rows_alloc, stage.num_ib, stage.num_jc, s);
    }
    stage.run(ta, params.kernel_type, rbf_direct, pack_records, out, LSSVM_MEM_HOST, info, no_lap, repeat);
    info.gram_mode = (planesS.mode != 0 && dc.p != nullptr) ? (rbf_grid ? 3 : planesS.mode) : 0;
    info.rbf_direct = rbf_direct ? 1 : 0;
    info.rbf_exponent_scale = rbf_r2;
    info.f16_row_rel_error = planesS.f16_row_rel_error;
}

/* csvm::predict_values behind the C ABI.  fp32 rbf with rbf_form 0: where the grid planes chosen from the exponent scale do not represent the data, the call runs
 * again on the formula-exact kernel (as Solver's constructor does for the training problem). */
template <typename T>
static void predict_values_retrying(const Options &opt, const lssvm_params &params, const T *sv, size_t nsv, size_t nfeat, const T *alpha, const T *rho, size_t nvec, T *w_inout,
                                    int *w_valid, const T *points, size_t npoints, T *out, lssvm_predict_info &local, int repeat) {
    local = lssvm_predict_info{};
    local.f16_row_rel_error = -1.0;
    try {
        predict_values_impl<T>(opt, params, sv, nsv, nfeat, alpha, rho, nvec, w_inout, w_valid, points, npoints, out, local, repeat);
    } catch (const GridPlanesUnfit &) {
        if (opt.rbf_form != 0) throw;
        Options direct = opt;
        direct.rbf_form = 1;
        local = lssvm_predict_info{};
        local.f16_row_rel_error = -1.0;
        predict_values_impl<T>(direct, params, sv, nsv, nfeat, alpha, rho, nvec, w_inout, w_valid, points, npoints, out, local, repeat);
    }
}
template <typename T>
void predict_values(const Options &opt, const lssvm_params &params, const T *sv, size_t nsv, size_t nfeat, const T *alpha, T rho, T *w_inout, int *w_valid, const T *points,
                    size_t npoints, T *out, lssvm_predict_info *info) {
    // (measurement aid: LSSVM_MI355_PREDICT_REPEAT=k in the environment launches the product kernel k times and times the LAST launch: what the kernel takes once the
    // chip's clocks have settled, beside the first launch after the set-up's idle gaps that a single call measures)
    int repeat = 1;
    if (const char *rep = std::getenv("LSSVM_MI355_PREDICT_REPEAT"); rep != nullptr) repeat = std::min(std::max(std::atoi(rep), 1), 64);
    lssvm_predict_info local{};
    predict_values_retrying<T>(opt, params, sv, nsv, nfeat, alpha, &rho, 1, w_inout, w_valid, points, npoints, out, local, repeat);
    local.vectors_per_launch = 0;  // (vectors_per_launch is predict_values_multi's report)
    if (info != nullptr) *info = local;
}
/* the GridPlanesUnfit retry applies to the whole call: every weight vector runs on the same kernel */
template <typename T>
void predict_values_multi(const Options &opt, const lssvm_params &params, const T *sv, size_t nsv, size_t nfeat, const T *alpha, const T *rho, size_t nvec, T *w_inout, int *w_valid,
                          const T *points, size_t npoints, T *out, lssvm_predict_info *info) {
    lssvm_predict_info local{};
    predict_values_retrying<T>(opt, params, sv, nsv, nfeat, alpha, rho, nvec, w_inout, w_valid, points, npoints, out, local, 1);
    if (info != nullptr) *info = local;
}

template void predict_values<float>(const Options &, const lssvm_params &, const float *, size_t, size_t, const float *, float, float *, int *, const float *, size_t, float *, lssvm_predict_info *);
template void predict_values<double>(const Options &, const lssvm_params &, const double *, size_t, size_t, const double *, double, double *, int *, const double *, size_t, double *, lssvm_predict_info *);
template void predict_values_multi<float>(const Options &, const lssvm_params &, const float *, size_t, size_t, const float *, const float *, size_t, float *, int *, const float *, size_t, float *,
                                          lssvm_predict_info *);
template void predict_values_multi<double>(const Options &, const lssvm_params &, const double *, size_t, size_t, const double *, const double *, size_t, double *, int *, const double *, size_t,
                                           double *, lssvm_predict_info *);
template void calculate_w<float>(const float *, size_t, size_t, const float *, float *);
template void calculate_w<double>(const double *, size_t, size_t, const double *, double *);

/* ------------------------------------------------------------------ the resident predictor ------------------------------------------------------------------ */
/* what every form of a predictor knows of its model: `nvec` weight vectors over the same `nsv` support vectors */
template <typename T>
struct PredictModel {
    Options opt;
    lssvm_params params;
    size_t nsv, nfeat, nvec;
    std::vector<T> rho;
};

/* The resident forms of an rbf / polynomial model, one type per real type: everything of the support vectors' side of the product that does not depend on the batch,
 * held in HBM -- per weight vector the alpha row and the packed column records of its launch group.  prepare(): false = this model has no resident form (nothing is
 * kept); predict(): a batch of points through the product stage, false = this batch needs the one-shot path. */
class ResidentF32 {
  public:
    static constexpr bool declines_batches = true;  // (the one-shot path's inputs stay needed: alpha on the host, the support vectors through fetch_support_vectors)

    bool prepare(const PredictModel<float> &m, const float *sv, const float *alpha, int forms, hipStream_t s) {
        const bool resident = prepare_or_decline(m, sv, alpha, forms, s);
        if (!resident) reset();
        return resident;
    }

    /* the support vectors back on the host, as they came (a resident model keeps no host copy until a batch needs the one-shot path) */
    void fetch_support_vectors(const PredictModel<float> &m, std::vector<float> &sv_host) const {
        select_device_checked(0);
        const float *src = raw_.p != nullptr ? raw_.p : S_.data.p;
        LSSVM_REQUIRE(src != nullptr, "the predictor holds no support vectors");
        sv_host.resize(m.nsv * m.nfeat);
        LSSVM_HIP_CHECK(hipMemcpy2D(sv_host.data(), m.nfeat * sizeof(float), src, static_cast<size_t>(S_.ldx) * sizeof(float), m.nfeat * sizeof(float), m.nsv, hipMemcpyDeviceToHost));
    }

  private:
    /* whatever prepare_or_decline had built before it found the model outside the resident form */
    void reset() {
        for (DevBuf<float> *b : { &S_.data, &mean_, &cS_, &a_, &raw_, &dc_, &dc_folded_, &dc2_ }) b->release();
        planesS_.buf.release();
    }

    /* fp32, rbf / polynomial, a split Gram mode: the support vectors' side of the product, once.  At most 128 features -- or, `every_form`, every width the one-shot
     * call runs on the one-pass split kernels (v2_eligible and not wide_nonlinear: the 128-row full-square kernels with the row panel in registers) -- or,
     * FORMS_PANELS, every width beyond those as well (wide_nonlinear: the panel kernel, planes padded to whole 128-feature panels). */
    bool prepare_or_decline(const PredictModel<float> &m, const float *sv, const float *alpha, int forms, hipStream_t s) {
        const bool beyond128 = round_up(static_cast<long>(m.nfeat), 64) > 128;
        wide_ = wide_nonlinear(m.opt, m.params, false, m.nfeat);
        if ((beyond128 && (forms < FORMS_EVERY || (wide_ && forms < FORMS_PANELS))) || m.opt.gram_mode == 0 || m.opt.tile_kernel == 1) return false;
        if (m.params.kernel_type == LSSVM_KERNEL_RBF && (m.opt.rbf_form == 1 || m.opt.rbf_form == 3)) return false;  // (the direct kernel / the grid planes asked for: the one-shot path has them)
        S_.upload(sv, LSSVM_MEM_HOST, m.nsv, m.nfeat, 0, s);
        if (!wide_ && !v2_eligible(m.opt, S_.ldx, false)) return false;
        const bool rbf = m.params.kernel_type == LSSVM_KERNEL_RBF;
        if (rbf) {
            column_means<float>(S_, mean_, s);
            const double sq = max_centred_sqnorm<float>(S_, mean_, s);
            r2_sv_ = 2.0 * static_cast<double>(static_cast<float>(m.params.gamma)) * 1.4426950408889634 * sq;
            if (!(r2_sv_ <= RBF_DIRECT_ABOVE) && m.opt.rbf_form != 2) return false;  // (beyond the norm expansion's range: grid planes or the direct kernel, one-shot)
            scale_ = rbf_prescale<float>(m.params, false);
            // S_ is centred and scaled in place below: the support vectors as they came stay beside it (the one-shot path's input, should a batch need it)
            raw_.alloc_zero(S_.data.count, s);
            LSSVM_HIP_CHECK(hipMemcpyAsync(raw_.p, S_.data.p, S_.data.count * sizeof(float), hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(k_center<float>, dim3((S_.dfeat + 255) / 256, S_.rows), dim3(256), 0, s, S_.data.p, S_.ldx, S_.dfeat, S_.rows, mean_.p, scale_);
            LSSVM_HIP_CHECK(hipGetLastError());
            half_neg_norms<float>(S_, cS_, s);
        }
        make_planes(m.opt, m.params, false, S_, nullptr, planesS_, nullptr, s, wide_);
        if (planesS_.mode == 0) return false;
        const int num_jt = S_.rows_alloc / TILE;
        const size_t ra = static_cast<size_t>(S_.rows_alloc);
        a_.alloc_zero(m.nvec * ra, s);  // [nvec][rows_alloc], exact zeros beyond the support vectors
        LSSVM_HIP_CHECK(hipMemcpy2DAsync(a_.p, ra * sizeof(float), alpha, m.nsv * sizeof(float), m.nsv * sizeof(float), m.nvec, hipMemcpyHostToDevice, s));
        // The column records of every launch group, once.  Per pair (0,1), (2,3), ... the (alpha0_j | alpha1_j) record of the two-vector kernels -- folded for rbf, the
        // form they exist in; per vector the (alpha_j | c_j) record of the one-vector kernels: for rbf every vector's (the only form an unfolded batch can use: that
        // kernel reads c_j from the record's second half; a batch's OWN exponent scale decides between the forms), otherwise only that of the vector no pair holds
        // (nvec odd; nvec == 1: the single-vector predictor's), and for rbf that vector's folded one-vector record as well.
        const int ncols = num_jt * TILE;
        rec_ = static_cast<size_t>(num_jt) * 256;
        const bool fold = rbf && m.opt.rbf_fold != 0;
        // (beyond 128 features a pair exists only where its launch is dispatched -- wide_pair_routed, panel_pair_routed --; elsewhere every vector keeps the records of a
        // launch of its own)
        const bool pair_routed = wide_ ? panel_pair_routed(LSSVM_DTYPE_F32, planesS_.mode, m.params.kernel_type, m.params.degree, planesS_.ldx16 / 128)
                                       : (planesS_.ldx16 <= 128 || wide_pair_routed(planesS_.mode, m.params.kernel_type, m.params.degree, planesS_.ldx16 / 64));
        const bool pairs = m.nvec >= 2 && (!rbf || fold) && pair_routed;
        folded_first_ = pairs ? m.nvec - 1 : 0;
        dc_.alloc_zero(m.nvec * rec_, s);
        for (size_t v = (rbf || !pairs) ? 0 : m.nvec - m.nvec % 2; v < m.nvec; ++v) enqueue_pack_records(a_.p + v * ra, cS_.p, ncols, dc_.p + v * rec_, 0, static_cast<const float *>(nullptr), s);
        if (fold && (m.nvec % 2 == 1 || !pairs)) {
            dc_folded_.alloc_zero((m.nvec - folded_first_) * rec_, s);
            for (size_t v = folded_first_; v < m.nvec; ++v) enqueue_pack_records(a_.p + v * ra, cS_.p, ncols, dc_folded_.p + (v - folded_first_) * rec_, 1, static_cast<const float *>(nullptr), s);
        }
        if (pairs) {
            dc2_.alloc_zero((m.nvec / 2) * rec_, s);
            for (size_t g = 0; g < m.nvec / 2; ++g) enqueue_pack_records2(a_.p + 2 * g * ra, a_.p + (2 * g + 1) * ra, cS_.p, ncols, dc2_.p + g * rec_, fold ? 1 : 0, s);
        }
        LSSVM_HIP_CHECK(hipGetLastError());
        LSSVM_HIP_CHECK(hipStreamSynchronize(s));
        return true;
    }

  public:
    /* a batch of points against the resident support vectors; false = this batch needs the one-shot path (decided before the product stage allocates anything) */
    bool predict(const PredictModel<float> &m, const float *points, int mem_kind, size_t npoints, float *out, lssvm_predict_info &info) const {
        select_device_checked(0);
        hipStream_t s = nullptr;
        const double t0 = now_ms();
        const char *dbg_env = std::getenv("LSSVM_MI355_DEBUG");
        const bool dbg = dbg_env != nullptr && dbg_env[0] == '1';
        double t_last = t0;
        auto lap = [&](const char *what) {  // LSSVM_MI355_DEBUG=1: where a call's time goes (the stream is drained at every lap, so the laps add up)
            if (!dbg) return;
            (void) hipStreamSynchronize(s);
            const double t = now_ms();
            std::fprintf(stderr, "[plssvm_amd] predictor: %-28s %8.3f ms\n", what, t - t_last);
            t_last = t;
        };
        const bool rbf = m.params.kernel_type == LSSVM_KERNEL_RBF;
        DeviceMatrix<float> P;
        P.upload(points, mem_kind, npoints, m.nfeat, static_cast<size_t>(round_up(static_cast<long>(npoints), 2 * TILE)), s);
        lap(mem_kind == LSSVM_MEM_DEVICE ? "points copied in HBM" : "points uploaded");
        DevBuf<float> cP;
        double r2 = r2_sv_;
        if (rbf) {
            const double sq = max_centred_sqnorm<float>(P, mean_, s);  // (against the SUPPORT VECTORS' means: the centre the resident side was prepared with)
            r2 = std::max(r2, 2.0 * static_cast<double>(static_cast<float>(m.params.gamma)) * 1.4426950408889634 * sq);
            if (!(r2 <= RBF_DIRECT_ABOVE) && m.opt.rbf_form != 2) return false;  // this batch reaches beyond the norm expansion's range
            hipLaunchKernelGGL(k_center<float>, dim3((P.dfeat + 255) / 256, P.rows), dim3(256), 0, s, P.data.p, P.ldx, P.dfeat, P.rows, mean_.p, scale_);
            LSSVM_HIP_CHECK(hipGetLastError());
            half_neg_norms<float>(P, cP, s);
        }
        lap("centred, norms");
        // the batch's planes: the kind and the scale of the support vectors' planes; two f16 planes must represent THIS batch too
        PlaneSet planesP;
        planesP.ldx16 = planesS_.ldx16;
        planesP.nplanes = planesS_.nplanes;
        planesP.mode = planesS_.mode;
        planesP.shift = planesS_.shift;
        planesP.buf.alloc_zero(static_cast<size_t>(planesP.nplanes) * P.rows_alloc * planesP.ldx16, s);
        if (planesS_.mode == 2) {
            DevBuf<unsigned> stats;
            stats.alloc_zero(4, s);
            split_f16_planes(P.data.p, P.ldx, P.dfeat, static_cast<size_t>(P.rows_alloc), planesP.ldx16, std::ldexp(1.0f, planesS_.shift), rbf ? F16_RBF_SHIFT : 0, planesP.buf.p,
                             static_cast<size_t>(P.rows_alloc) * planesP.ldx16, stats.p, s);
            unsigned host[4] = { 0, 0, 0, 0 };
            LSSVM_HIP_CHECK(hipMemcpyAsync(host, stats.p, sizeof(host), hipMemcpyDeviceToHost, s));
            LSSVM_HIP_CHECK(hipStreamSynchronize(s));
            float rel2 = 0.0f, rest2 = 0.0f, x2 = 0.0f;
            std::memcpy(&rel2, &host[0], sizeof(float));
            std::memcpy(&rest2, &host[1], sizeof(float));
            std::memcpy(&x2, &host[2], sizeof(float));
            // the check over BOTH sides, as make_planes runs it for the one-shot call (one set of statistics for the support vectors and the points): the batch's maxima
            // beside the support vectors' -- the batch alone can pass (and the support vectors alone) where the pair does not, e.g. the rbf bound 2 max|rest| max|x| with the
            // rest of one side and the norm of the other.  (std::max keeps a batch's NaN: an overflowing plane)
            rel2 = std::max(rel2, planesS_.f16_rel2);
            rest2 = std::max(rest2, planesS_.f16_rest2);
            x2 = std::max(x2, planesS_.f16_x2);
            const bool ok = f16_planes_pass(rbf, rel2, rest2, x2);
            info.f16_row_rel_error = std::sqrt(static_cast<double>(rel2));
            if (!ok && m.opt.gram_mode != 2) return false;  // the support vectors' planes are f16, the pair needs bf16: one-shot (which splits both sides alike)
        } else {
            split_bf16_planes(P.data.p, P.ldx, P.dfeat, static_cast<size_t>(P.rows_alloc), planesP.ldx16, planesP.buf.p, static_cast<size_t>(P.rows_alloc) * planesP.ldx16, s);
        }
        lap("operand planes");
        const bool folded = rbf && m.opt.rbf_fold != 0 && r2 <= FOLD_MAX_R2;
        // (the rectangular 256-row kernel exists up to 128 features; wider models take the 128-row full-square kernels at every batch size, as in the one-shot call --
        // beyond the one-pass kernels the full-square panel kernel)
        const bool rect = rect_kernel_applies(m.opt, m.params, planesS_.ldx16, folded, r2, P.rows_alloc / TILE);
        // Two weight vectors per product launch wherever a pair record exists in the form this batch needs: the rectangular 256-row kernel under its conditions, the
        // 128-row full-square kernels otherwise (polynomial of any degree, folded rbf).  Unfolded rbf keeps c_j in the record's second half: one vector per launch.
        const int per_launch = (m.nvec >= 2 && dc2_.p != nullptr && (!rbf || folded)) ? 2 : 1;
        ProductStage<float> stage(m.opt, P, S_, rect, a_.p, m.rho.data(), m.nvec, per_launch, s, t0);
        const auto records = [&](int v, int count) -> const float * {
            if (count == 2) return dc2_.p + static_cast<size_t>(v / 2) * rec_;
            if (folded) return dc_folded_.p + (static_cast<size_t>(v) - folded_first_) * rec_;  // (folded and alone: the vector no pair holds -- or, where pairs are not dispatched, every vector)
            return dc_.p + static_cast<size_t>(v) * rec_;
        };
        TileArgs<float> ta = stage.args(m.params, false, cP.p, cS_.p, records);
        ta.dc_folded = folded ? 1 : 0;
        set_plane_args(ta, m.params, planesS_, planesP, static_cast<size_t>(S_.rows_alloc), static_cast<size_t>(P.rows_alloc));
        ta.wide_panels = wide_ ? 1 : 0;
        RectSetup rect_setup;
        if (rect) setup_rect_launch(ta, rect_setup, planesP, P.rows_alloc, stage.num_ib, stage.num_jc, s);
        stage.run(ta, m.params.kernel_type, false, records, out, mem_kind, info, lap);
        info.gram_mode = planesS_.mode;
        info.rbf_direct = 0;
        info.rbf_exponent_scale = r2;
        if (info.f16_row_rel_error < 0.0) info.f16_row_rel_error = planesS_.f16_row_rel_error;
        info.resident = 1;
        return true;
    }

  private:
    DeviceMatrix<float> S_;
    DevBuf<float> mean_, cS_, a_, raw_;
    DevBuf<float> dc_, dc_folded_, dc2_;  // column records: [nvec][rec_] per vector, the folded one of an unpaired last vector, [nvec / 2][rec_] per pair
    size_t rec_ = 0;
    size_t folded_first_ = 0;             // the vector dc_folded_ starts with (the last one; 0 where no pair launch is dispatched and every vector has one)
    PlaneSet planesS_;
    double r2_sv_ = 0.0;
    float scale_ = 1.0f;
    bool wide_ = false;  // beyond the one-pass split kernels: the panel kernel (FORMS_PANELS)
};

/* (lssvm_mi355_predictor_create_resident and _create_panels only: FORMS_EVERY and above) */
class ResidentF64 {
  public:
    static constexpr bool declines_batches = false;

    /* fp64, rbf / polynomial (gamma > 0) on the one-pass v2 kernel (at most 256 padded features, tile_kernel != 1): the support vectors' side of the product, once,
     * prepared as predict_values_impl<double> prepares it -- the same padding, centre, scale and records, so that a batch's values have the one-shot call's bits.  fp64
     * rbf has no direct form and no plane check: this form never declines a batch and keeps no host copy of the support vectors.  FORMS_PANELS: beyond 256 padded
     * features as well (wide_nonlinear_f64: the panel kernel on data padded to whole 64-feature panels, which DeviceMatrix::upload does at these widths). */
    bool prepare(const PredictModel<double> &m, const double *sv, const double *alpha, int forms, hipStream_t s) {
        const bool rbf = m.params.kernel_type == LSSVM_KERNEL_RBF;
        if (forms < FORMS_EVERY || !(rbf || m.params.kernel_type == LSSVM_KERNEL_POLYNOMIAL) || !(m.params.gamma > 0.0)) return false;
        wide_ = forms >= FORMS_PANELS && wide_nonlinear_f64(m.opt, m.params, m.nfeat);
        if (!wide_ && !v2_eligible_f64(m.opt, padded_features<double>(m.nfeat))) return false;
        S_.upload(sv, LSSVM_MEM_HOST, m.nsv, m.nfeat, 0, s);
        const dim3 cgrid((S_.dfeat + 255) / 256, S_.rows);
        if (rbf) {
            scale_ = rbf_prescale<double>(m.params, true);
            column_means<double>(S_, mean_, s);
            hipLaunchKernelGGL(k_center<double>, cgrid, dim3(256), 0, s, S_.data.p, S_.ldx, S_.dfeat, S_.rows, mean_.p, scale_);
            LSSVM_HIP_CHECK(hipGetLastError());
            half_neg_norms<double>(S_, cS_, s);
        } else {  // the polynomial runs on data that carries sqrt(gamma), with gamma = 1 in the launch arguments
            scale_ = std::sqrt(m.params.gamma);
            hipLaunchKernelGGL(k_center<double>, cgrid, dim3(256), 0, s, S_.data.p, S_.ldx, S_.dfeat, S_.rows, static_cast<const double *>(nullptr), scale_);
            LSSVM_HIP_CHECK(hipGetLastError());
        }
        const int num_jt = S_.rows_alloc / TILE;
        const size_t ra = static_cast<size_t>(S_.rows_alloc);
        a_.alloc_zero(m.nvec * ra, s);  // [nvec][rows_alloc], exact zeros beyond the support vectors
        LSSVM_HIP_CHECK(hipMemcpy2DAsync(a_.p, ra * sizeof(double), alpha, m.nsv * sizeof(double), m.nsv * sizeof(double), m.nvec, hipMemcpyHostToDevice, s));
        // The column records of every launch group, once: per pair (0,1), (2,3), ... the (d0_j | d1_j | c_j) record of the two-vector kernel, and the single-vector
        // (d_j | c_j) record of the vector no pair holds (nvec odd; nvec == 1).  Every (kernel function, chunk count) instantiation of the two-vector kernel takes less
        // than two single-vector launches (profiles/predictor_f64.json, launch_level: 0.46 ... 0.58 of two), so every pair is launched as a pair.  The panel kernel:
        // where panel_pair_routed says so; elsewhere every vector keeps the single-vector record of a launch of its own.
        const int ncols = num_jt * TILE;
        rec2_ = static_cast<size_t>(num_jt) * 2 * 192;
        rec1_ = static_cast<size_t>(num_jt) * 256;
        pairs_ = m.nvec >= 2 && (!wide_ || panel_pair_routed(LSSVM_DTYPE_F64, 0, m.params.kernel_type, m.params.degree, S_.ldx / 64));
        single_first_ = pairs_ ? m.nvec - 1 : 0;
        if (m.nvec % 2 == 1 || !pairs_) {
            dc_.alloc_zero((m.nvec - single_first_) * rec1_, s);
            for (size_t v = single_first_; v < m.nvec; ++v) enqueue_pack_records(a_.p + v * ra, cS_.p, ncols, dc_.p + (v - single_first_) * rec1_, 0, static_cast<const double *>(nullptr), s);
        }
        if (pairs_) {
            dc2_.alloc_zero((m.nvec / 2) * rec2_, s);
            for (size_t g = 0; g < m.nvec / 2; ++g) enqueue_pack_records2(a_.p + 2 * g * ra, a_.p + (2 * g + 1) * ra, cS_.p, ncols, dc2_.p + g * rec2_, s);
        }
        LSSVM_HIP_CHECK(hipGetLastError());
        LSSVM_HIP_CHECK(hipStreamSynchronize(s));
        return true;
    }

    /* a batch of points against the resident fp64 support vectors, prepared as predict_values_impl<double> prepares its points */
    bool predict(const PredictModel<double> &m, const double *points, int mem_kind, size_t npoints, double *out, lssvm_predict_info &info) const {
        select_device_checked(0);
        hipStream_t s = nullptr;
        const double t0 = now_ms();
        const bool rbf = m.params.kernel_type == LSSVM_KERNEL_RBF;
        DeviceMatrix<double> P;
        P.upload(points, mem_kind, npoints, m.nfeat, static_cast<size_t>(round_up(static_cast<long>(npoints), 2 * TILE)), s);
        DevBuf<double> cP;
        // (against the SUPPORT VECTORS' means and with their scale: what center_columns(S, &P, ...) does in the one-shot call)
        hipLaunchKernelGGL(k_center<double>, dim3((P.dfeat + 255) / 256, P.rows), dim3(256), 0, s, P.data.p, P.ldx, P.dfeat, P.rows, rbf ? mean_.p : static_cast<const double *>(nullptr), scale_);
        LSSVM_HIP_CHECK(hipGetLastError());
        if (rbf) half_neg_norms<double>(P, cP, s);
        ProductStage<double> stage(m.opt, P, S_, false, a_.p, m.rho.data(), m.nvec, pairs_ ? 2 : 1, s, t0);
        const auto records = [&](int v, int count) -> const double * {
            // (alone: the vector no pair holds -- or, where pairs are not dispatched, every vector)
            return count == 2 ? dc2_.p + static_cast<size_t>(v / 2) * rec2_ : dc_.p + (static_cast<size_t>(v) - single_first_) * rec1_;
        };
        TileArgs<double> ta = stage.args(m.params, false, cP.p, cS_.p, records);
        if (!rbf) ta.gamma = 1.0;
        ta.wide_panels = wide_ ? 1 : 0;
        stage.run(ta, m.params.kernel_type, false, records, out, mem_kind, info, no_lap);
        info.resident = 1;
        return true;
    }

  private:
    DeviceMatrix<double> S_;
    DevBuf<double> mean_, cS_, a_;
    DevBuf<double> dc_, dc2_;  // column records: [num_jt][256] of the vector no pair holds (every vector's where pairs are not dispatched), [nvec / 2][rec2_] per pair
    size_t rec2_ = 0, rec1_ = 0;
    size_t single_first_ = 0;  // the vector dc_ starts with (the last one; 0 where no pair launch is dispatched)
    double scale_ = 1.0;
    bool wide_ = false;   // more than 256 padded features: the panel kernel (FORMS_PANELS)
    bool pairs_ = false;  // two vectors per launch
};

/* `nvec` weight vectors over the same support vectors (lssvm_mi355_predictor_create: one; _create_multi: a one-vs-all model's k).  The linear kernel keeps w per vector;
 * an rbf / polynomial model keeps its real type's resident form where it has one, and the one-shot path's inputs where a batch may need them.
 * `every_form` (lssvm_mi355_predictor_create_resident): fp64 rbf / polynomial models on at most 256 padded features are resident as well (ResidentF64), and so are fp32
 * models of 129 ... 512 features on the one-pass split kernels (ResidentF32); without it such a model goes through the one-shot path, as _create / _create_multi
 * document.  FORMS_PANELS (lssvm_mi355_predictor_create_panels): all of that, and the models beyond the one-pass kernels on the panel kernels -- fp32 rbf / polynomial
 * beyond 512 / 384 features, fp64 beyond 256. */
template <typename T>
class Predictor final : public PredictorBase {
    using Resident = std::conditional_t<std::is_same_v<T, float>, ResidentF32, ResidentF64>;

  public:
    Predictor(const Options &opt, const lssvm_params &params, const T *sv, size_t nsv, size_t nfeat, const T *alpha, const double *rho, size_t nvec, int forms) :
        m_{ opt, params, nsv, nfeat, nvec, {} } {
        dtype = std::is_same_v<T, float> ? LSSVM_DTYPE_F32 : LSSVM_DTYPE_F64;
        check_params(&m_.params);
        LSSVM_REQUIRE(nvec > 0 && rho != nullptr, "a predictor needs at least one weight vector and its rho");
        LSSVM_REQUIRE(nvec <= static_cast<size_t>(1) << 20, "too many weight vectors");
        LSSVM_REQUIRE(sv != nullptr && nsv > 0, "The support vectors must not be empty!");   // csvm.cpp:189
        LSSVM_REQUIRE(nfeat > 0, "The support vectors must contain at least one feature!");  // csvm.cpp:190
        LSSVM_REQUIRE(alpha != nullptr, "The number of support vectors and number of weights must be the same!");
        m_.rho.resize(nvec);
        for (size_t v = 0; v < nvec; ++v) m_.rho[v] = static_cast<T>(rho[v]);
        select_device_checked(0);
        hipStream_t s = nullptr;
        if (params.kernel_type == LSSVM_KERNEL_LINEAR) {
            // the linear kernel predicts through w = sum_i alpha_i sv_i (csvm.cpp:204-213): computed once per vector, resident zero padded like a row of points
            std::vector<T> w_host(nvec * nfeat, T(0));
            calculate_w_multi<T>(sv, nsv, nfeat, alpha, nvec, w_host.data());
            ldw_ = static_cast<size_t>(padded_features<T>(nfeat));
            w_.alloc_zero(nvec * ldw_, s);
            LSSVM_HIP_CHECK(hipMemcpy2DAsync(w_.p, ldw_ * sizeof(T), w_host.data(), nfeat * sizeof(T), nfeat * sizeof(T), nvec, hipMemcpyHostToDevice, s));
            LSSVM_HIP_CHECK(hipStreamSynchronize(s));
            return;
        }
        resident_ = resident_form_.prepare(m_, sv, alpha, forms, s);
        // the one-shot path's inputs: host copies where nothing is resident; a resident model that may decline a batch keeps alpha, leaves its support vectors as they
        // came in HBM and fetches them if a batch ever asks
        if (!resident_ || Resident::declines_batches) alpha_host_.assign(alpha, alpha + nvec * nsv);
        if (!resident_) sv_host_.assign(sv, sv + nsv * nfeat);
    }

    void predict(const void *points_v, int mem_kind, size_t npoints, void *out_v, lssvm_predict_info *info, bool multi) override {
        const T *points = static_cast<const T *>(points_v);
        T *out = static_cast<T *>(out_v);
        LSSVM_REQUIRE(points != nullptr && npoints > 0, "The data points to predict must not be empty!");  // csvm.cpp:194
        LSSVM_REQUIRE(out != nullptr, "out must not be NULL");
        LSSVM_REQUIRE(multi || m_.nvec == 1, "this predictor holds more than one weight vector: use lssvm_mi355_predictor_predict_multi");
        lssvm_predict_info local{};
        local.f16_row_rel_error = -1.0;
        bool done = false;
        if (m_.params.kernel_type == LSSVM_KERNEL_LINEAR) {
            predict_linear(points, mem_kind, npoints, out, local);
            done = true;
        } else if (resident_) {
            done = resident_form_.predict(m_, points, mem_kind, npoints, out, local);
        }
        if (!done) {
            // what the resident form does not cover (outside lssvm_mi355_predictor_create_resident: fp64, and fp32 on more than 128 features; with it: fp64 beyond 256
            // features and fp32 beyond the one-pass split kernels' 512 / 384 -- which lssvm_mi355_predictor_create_panels keeps resident on the panel kernels; under
            // every entry point: a negative polynomial degree beyond the one-pass kernels, gram_mode 0, tile_kernel 1, rbf_form 1 / 3; exponent scales beyond the norm
            // expansion; a batch whose planes fail the f16 check or that lies further from the support vectors' centre than the form chosen for them allows): the
            // one-shot path, same result
            int w_valid = 0;
            std::vector<T> w_tmp(m_.nvec * m_.nfeat);
            if constexpr (Resident::declines_batches) {
                if (sv_host_.empty()) resident_form_.fetch_support_vectors(m_, sv_host_);
            }
            const auto one_shot = [&](const T *pts, T *values) {
                if (multi) {
                    predict_values_multi<T>(m_.opt, m_.params, sv_host_.data(), m_.nsv, m_.nfeat, alpha_host_.data(), m_.rho.data(), m_.nvec, w_tmp.data(), &w_valid, pts, npoints, values, &local);
                } else {
                    predict_values<T>(m_.opt, m_.params, sv_host_.data(), m_.nsv, m_.nfeat, alpha_host_.data(), m_.rho[0], w_tmp.data(), &w_valid, pts, npoints, values, &local);
                }
            };
            if (mem_kind == LSSVM_MEM_DEVICE) {  // (the one-shot entry point takes host buffers: a batch in HBM makes the round trip here -- the rare path)
                select_device_checked(0);
                std::vector<T> points_host(npoints * m_.nfeat), out_host(npoints * m_.nvec);
                LSSVM_HIP_CHECK(hipMemcpy(points_host.data(), points, points_host.size() * sizeof(T), hipMemcpyDeviceToHost));
                one_shot(points_host.data(), out_host.data());
                LSSVM_HIP_CHECK(hipMemcpy(out, out_host.data(), out_host.size() * sizeof(T), hipMemcpyHostToDevice));
            } else {
                one_shot(points, out);
            }
            local.resident = 0;
        }
        if (!multi) local.vectors_per_launch = 0;  // (vectors_per_launch is the multi calls' report)
        if (info != nullptr) *info = local;
    }

  private:
    void predict_linear(const T *points, int mem_kind, size_t npoints, T *out, lssvm_predict_info &info) {
        select_device_checked(0);
        hipStream_t s = nullptr;
        const double t0 = now_ms();
        const int nv = static_cast<int>(m_.nvec);
        LaunchTimer timer(m_.nvec);
        DeviceMatrix<T> P;
        P.upload(points, mem_kind, npoints, m_.nfeat, 0, s);
        DevBuf<T> o;
        o.alloc_zero(npoints * m_.nvec, s);
        LSSVM_HIP_CHECK(hipStreamSynchronize(s));
        const double t_kernel = now_ms();
        for (int v = 0; v < nv; ++v) timer.timed(s, [&] { launch_predict_linear<T>(P, w_.p + static_cast<size_t>(v) * ldw_, m_.rho[static_cast<size_t>(v)], o.p + v, s, nv); });
        finish_predict(timer, o, out, mem_kind, s, t0, t_kernel, 1, info, no_lap);
        info.resident = 1;
    }

    PredictModel<T> m_;
    std::vector<T> sv_host_, alpha_host_;  // the one-shot path's inputs
    DevBuf<T> w_;                          // linear kernel: [nvec][ldw_]
    size_t ldw_ = 0;
    bool resident_ = false;
    Resident resident_form_;
};

std::unique_ptr<PredictorBase> make_predictor(const Options &opt, const lssvm_params &params, int dtype, const void *sv, size_t nsv, size_t nfeat, const void *alpha, const double *rho,
                                              size_t nvec, int forms) {
    if (dtype == LSSVM_DTYPE_F32) return std::make_unique<Predictor<float>>(opt, params, static_cast<const float *>(sv), nsv, nfeat, static_cast<const float *>(alpha), rho, nvec, forms);
    return std::make_unique<Predictor<double>>(opt, params, static_cast<const double *>(sv), nsv, nfeat, static_cast<const double *>(alpha), rho, nvec, forms);
}

}  // namespace lssvm
