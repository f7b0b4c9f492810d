/*
 * lssvm_solver.hip -- Solver<T>: the CG driver over the shards of this process (see lssvm_problem.hip.hpp; the recipe is the reference's
 * src/plssvm/backends/OpenMP/csvm.cpp:71-183, the orchestration replaces include/plssvm/backends/gpu_csvm.hpp:477-654).  The shards themselves (data, planes,
 * work-item geometry, the tile-kernel launches) are lssvm_problem.hip, the exchange of the partial vectors between them lssvm_exchange.hip.  Compiled for gfx950 only.
 */
#include "lssvm_problem.hip.hpp"

#define LSSVM_KERNELS_CG
#include "lssvm_kernels.hip.hpp"

#include <algorithm>
#include <cstdlib>

namespace lssvm {

/* ------------------------------------------------------------------ CgSteps: the O(n) steps of the CG recipe ------------------------------------------------------------------ */
/* launch(weighted, diag): `weighted` a std::bool_constant that names the instantiation, `diag` the argument that goes with it (kernels' DiagArg) */
template <typename T>
template <typename Launch>
void CgSteps<T>::with_diag(Launch &&launch) const {
    if (p_.weighted_) {
        launch(std::true_type{}, static_cast<const double *>(p_.inv_cw_.p));
    } else {
        launch(std::false_type{}, p_.inv_cost_);
    }
    LSSVM_HIP_CHECK(hipGetLastError());
}

template <typename T>
void CgSteps<T>::sum_and_qdot(const State &s, const T *v, int slot_sum, int slot_q) const {
    hipLaunchKernelGGL(k_sum_and_qdot<T>, dim3(RED_BLOCKS), dim3(RED_THREADS), 0, stream(), v, q(), n(), s.part_of(PART_SUMS));
    finish_sums(s, slot_sum, slot_q);
}
template <typename T>
void CgSteps<T>::finish_sums(const State &s, int slot_sum, int slot_q) const {
    hipLaunchKernelGGL(k_finish2, dim3(1), dim3(RED_THREADS), 0, stream(), s.part_of(PART_SUMS), s.sc.p, slot_sum, slot_q);
    LSSVM_HIP_CHECK(hipGetLastError());
}

template <typename T>
void CgSteps<T>::begin(const State &s, const T *y_host) const {
    LSSVM_HIP_CHECK(hipMemcpyAsync(s.y.p, y_host, num_points() * sizeof(T), hipMemcpyHostToDevice, stream()));
    const dim3 gn((n() + 255) / 256), bn(256);
    hipLaunchKernelGGL(k_make_b<T>, gn, bn, 0, stream(), s.y.p, n(), s.b.p);  // csvm.cpp:89-91
    hipLaunchKernelGGL(k_fill<T>, gn, bn, 0, stream(), s.x.p, n(), T(1));     // csvm.cpp:95
    sum_and_qdot(s, s.x.p, SC_SUMX, SC_QX);
}

template <typename T>
void CgSteps<T>::begin_from_zero(const State &s, const double *r_dev, const double *absmax_part_dev) const {
    hipLaunchKernelGGL((k_scale_down<double, T>), dim3(RED_BLOCKS), dim3(RED_THREADS), 0, stream(), r_dev, absmax_part_dev, n(), s.b.p, s.r.p, s.x.p, s.part_of(PART_RR));
    LSSVM_HIP_CHECK(hipGetLastError());
}

template <typename T>
void CgSteps<T>::residual(const State &s, const T *Kv, const T *x, T *r_out, PartSet part) const {
    with_diag([&](auto weighted, auto diag) {
        hipLaunchKernelGGL((k_residual<T, decltype(weighted)::value>), dim3(RED_BLOCKS), dim3(RED_THREADS), 0, stream(), Kv, x, q(), s.b.p, s.sc.p, n(), diag, p_.QA_cost_, r_out, s.part_of(part));
    });
}

template <typename T>
void CgSteps<T>::finish_delta(const State &s, PartSet part, double *host_delta, bool initial) const {
    hipLaunchKernelGGL(k_finish_delta, dim3(1), dim3(RED_THREADS), 0, stream(), s.part_of(part), s.sc.p, host_delta, initial ? 1 : 0);
    LSSVM_HIP_CHECK(hipGetLastError());
}

template <typename T>
void CgSteps<T>::update_d(const State &s, bool initial, const PackDc<T> &pack) const {
    hipLaunchKernelGGL(k_update_d<T>, dim3(RED_BLOCKS), dim3(RED_THREADS), 0, stream(), s.d.p, s.r.p, q(), s.sc.p, n(), initial ? 1 : 0, s.part_of(PART_D), pack);
    LSSVM_HIP_CHECK(hipGetLastError());
}

template <typename T>
void CgSteps<T>::advance(const State &s, const T *Kv, bool refresh, double *sc_alpha) const {
    // (every kernel of the chain reduces its predecessor's partial sums for itself -- finish2_in_block -- so no single-block kernel stands between them)
    with_diag([&](auto weighted, auto diag) {
        hipLaunchKernelGGL((k_Ad_and_dAd<T, decltype(weighted)::value>), dim3(RED_BLOCKS), dim3(RED_THREADS), 0, stream(), Kv, s.d.p, q(), s.part_of(PART_D), s.sc.p, n(), diag, p_.QA_cost_, s.Ad.p,
                           s.part_of(PART_DAD));
    });
    hipLaunchKernelGGL(k_update_x_r<T>, dim3(RED_BLOCKS), dim3(RED_THREADS), 0, stream(), s.x.p, s.r.p, s.d.p, s.Ad.p, s.part_of(PART_DAD), sc_alpha != nullptr ? sc_alpha : s.sc.p, n(), refresh ? 0 : 1, s.part_of(PART_RR));
    LSSVM_HIP_CHECK(hipGetLastError());
    if (refresh) sum_and_qdot(s, s.x.p, SC_SUMX, SC_QX);
}

template <typename T>
void CgSteps<T>::apply_ret(const State &s, const T *Kv, const T *v, double add) const {
    with_diag([&](auto weighted, auto diag) {
        hipLaunchKernelGGL((k_apply_ret<T, decltype(weighted)::value>), dim3((n() + 255) / 256), dim3(256), 0, stream(), Kv, v, q(), s.sc.p, n(), diag, p_.QA_cost_, add, s.Ad.p);
    });
}

template <typename T>
void CgSteps<T>::enqueue_finish(const State &s, T *alpha_out) const {
    sum_and_qdot(s, s.x.p, SC_SUMX, SC_QX);
    LSSVM_HIP_CHECK(hipMemcpyAsync(s.host_sc.p, s.sc.p, SC_COUNT * sizeof(double), hipMemcpyDeviceToHost, stream()));
    if (alpha_out != nullptr) LSSVM_HIP_CHECK(hipMemcpyAsync(alpha_out, s.x.p, static_cast<size_t>(n()) * sizeof(T), hipMemcpyDeviceToHost, stream()));
}
template <typename T>
void CgSteps<T>::read_solution(const State &s, double y_last, T *alpha_out, double *rho_out) const {
    const T sum_x = static_cast<T>(s.host_sc.p[SC_SUMX]);
    const T bias = static_cast<T>(y_last + p_.QA_cost_ * s.host_sc.p[SC_SUMX] - s.host_sc.p[SC_QX]);
    alpha_out[n()] = -sum_x;
    *rho_out = static_cast<double>(-bias);
}
template <typename T>
void CgSteps<T>::finish_now(const State &s, double y_last, T *alpha_out, double *rho_out) const {
    enqueue_finish(s, alpha_out);
    LSSVM_HIP_CHECK(hipStreamSynchronize(stream()));
    read_solution(s, y_last, alpha_out, rho_out);
}

template class CgSteps<float>;
template class CgSteps<double>;

/* ------------------------------------------------------------------ Solver: CG over the shards of this process ------------------------------------------------------------------ */
template <typename T>
Solver<T>::Solver(const Options &opt, const lssvm_params &params, const void *X, int mem_kind, size_t num_points, size_t num_features, const std::vector<int> &devices, const lssvm_shard *shard) :
    opt_(opt) {
    dtype = std::is_same_v<T, float> ? LSSVM_DTYPE_F32 : LSSVM_DTYPE_F64;
    const double t0 = now_ms();
    LSSVM_REQUIRE(!devices.empty() && devices.size() <= static_cast<size_t>(MAX_LOCAL_DEVICES), "invalid number of devices");
    int rank0 = 0;
    world_ = static_cast<int>(devices.size());
    if (shard != nullptr && (shard->world != 1 || shard->rank != 0)) {
        // one process per GPU: this process holds rank `rank` of `world`
        LSSVM_REQUIRE(devices.size() == 1, "a shard descriptor (one process per GPU) and a device list (one process, several GPUs) exclude each other");
        LSSVM_REQUIRE(shard->world >= 1 && shard->rank >= 0 && shard->rank < shard->world, "invalid shard descriptor");
        rank0 = shard->rank;
        world_ = shard->world;
        if (opt_.skip_collective == 0) {
            // exchange 1: RCCL (lssvm_mi355_comm_init first); 2: HIP IPC + peer kernels (lssvm_mi355_problem_ipc_export / _connect after
            // the problem exists); 0: RCCL when this process has a communicator, else IPC
            const bool have_comm = comm().comm != nullptr;
            if (opt_.exchange == 1 || (opt_.exchange == 0 && have_comm)) {
                LSSVM_REQUIRE(have_comm && comm().world == world_ && comm().rank == rank0,
                              "row-block sharding over RCCL requested but lssvm_mi355_comm_init was not called with the same rank/world");
                LSSVM_REQUIRE(comm().device == devices[0], "the communicator was created for another device");
                exchange_ = Exchange::process_rccl;
            } else {
                LSSVM_REQUIRE(world_ <= MAX_LOCAL_DEVICES, "the peer exchange handles at most " + std::to_string(MAX_LOCAL_DEVICES) + " ranks");
                exchange_ = Exchange::process_peer;
            }
        }
    } else if (devices.size() == 1) {
        if (opt_.force_collective != 0 && comm().comm != nullptr && comm().world == 1) exchange_ = Exchange::process_rccl;
    } else {
        std::vector<int> sorted(devices);
        std::sort(sorted.begin(), sorted.end());
        const bool distinct = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
        // (exchange = 1 with a repeated ordinal: RCCL's own ncclCommInitAll refuses the list -- "duplicate GPU detected" -- and its message comes back)
        exchange_ = (opt_.exchange == 1 || (opt_.exchange == 0 && distinct)) ? Exchange::local_rccl : Exchange::peer;
        if (opt_.skip_collective != 0) exchange_ = Exchange::none;
    }
    const auto build_shards = [&] {
        shards_.clear();
        for (size_t r = 0; r < devices.size(); ++r) {
            shards_.push_back(std::make_unique<Problem<T>>(opt_, params, X, mem_kind, num_points, num_features, devices[r], rank0 + static_cast<int>(r), world_));
        }
    };
    try {
        build_shards();
    } catch (const GridPlanesUnfit &) {
        // rbf_form 0 chose the grid planes from the exponent scale, and they do not represent this data: the formula-exact kernel, as before the grid planes existed.
        // Every shard (and every rank: the data is replicated) sees the same planes and comes here alike.  An explicit rbf_form = 3 keeps the error.
        if (opt_.rbf_form != 0) throw;
        opt_.rbf_form = 1;
        build_shards();
    }
    if (exchange_ == Exchange::local_rccl) local_comms_ = local_comms_for(devices);
    if (exchange_ == Exchange::process_peer) {
        Problem<T> &p = *shards_[0];
        p.activate();
        ipc_ = std::make_unique<IpcPeers>(rank0, world_);
        p.Ksum_.alloc_zero(p.nvec_, p.stream());
        p.Kres_ = p.Ksum_.p;
    }
    if (exchange_ == Exchange::peer) {
        for (auto &p : shards_) {
            p->activate();
            for (auto &o : shards_) {
                if (o->device_ == p->device_) continue;
                int can = 0;
                LSSVM_HIP_CHECK(hipDeviceCanAccessPeer(&can, p->device_, o->device_));
                if (can == 0) throw Error(LSSVM_ERR_COMM, "device " + std::to_string(p->device_) + " cannot map the memory of device " + std::to_string(o->device_) + " (use option exchange = 1)");
                const hipError_t e = hipDeviceEnablePeerAccess(o->device_, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) LSSVM_HIP_CHECK(e);
                (void) hipGetLastError();
            }
            p->Ksum_.alloc_zero(p->nvec_, p->stream());
            p->Kres_ = p->Ksum_.p;
        }
    }
    shards_[0]->activate();
    ev_delta_.create(false);
    sync_all();
    setup_ms_ = now_ms() - t0;
}

template <typename T>
Solver<T>::~Solver() {
    for (auto &p : shards_) {
        (void) hipSetDevice(p->device_);
        (void) hipStreamSynchronize(p->stream());
    }
    if (ipc_ && ipc_->connected && xseq_ > 0 && ipc_->own->abort.load() == 0) {
        // the peers read this rank's partial vector through their IPC mapping: it may be freed only after their last read
        try {
            ipc_->wait_all(1, xseq_, 30.0);
        } catch (...) {
        }
    }
}

template <typename T>
void Solver<T>::sync_all() {
    for (auto &p : shards_) {
        p->activate();
        LSSVM_HIP_CHECK(hipStreamSynchronize(p->stream()));
        p->drain_events();
    }
}

template <typename T>
void Solver<T>::apply_K(Vec which) {
    const bool skip = world_ > 1 && opt_.skip_collective != 0;  // testing aid: this rank's share only
    const bool collective = exchange_ != Exchange::none;
    if (exchange_ == Exchange::process_peer && xseq_ > 0 && !skip) {
        // this rank's partial vector is about to be overwritten: every peer must have read the previous one
        ipc_->wait_all(1, xseq_, static_cast<double>(std::max<int64_t>(opt_.ipc_timeout_s, 1)));
    }
    for (auto &p : shards_) {
        p->activate();
        p->enqueue_apply_K_local(vec_of(*p, which), (p->sym_ && collective) || skip);
    }
    if (collective) exchange();
}

template <typename T>
void Solver<T>::get_q(void *q_out, double *QA_cost_out) {
    Problem<T> &p = *shards_[0];
    p.activate();
    if (q_out != nullptr) {
        LSSVM_HIP_CHECK(hipMemcpyAsync(q_out, p.q_.p, static_cast<size_t>(p.n_) * sizeof(T), hipMemcpyDeviceToHost, p.stream()));
        LSSVM_HIP_CHECK(hipStreamSynchronize(p.stream()));
    }
    if (QA_cost_out != nullptr) *QA_cost_out = p.QA_cost_;
}

/* weighted LS-SVM: every shard takes the same diagonal terms and QA_cost (all ranks of a world > 1 are handed the same full vector) */
template <typename T>
void Solver<T>::set_weights(const double *weights, size_t num_points) {
    LSSVM_REQUIRE(!in_cg_, "the weights cannot change between cg_begin and cg_finish");
    if (weights != nullptr) {
        LSSVM_REQUIRE(num_points == shards_[0]->N_, "expected " + std::to_string(shards_[0]->N_) + " weights (one per data point), but got " + std::to_string(num_points) + "!");
        check_weights<T>(weights, num_points, shards_[0]->params_.cost);
    }
    for (auto &p : shards_) p->set_weights(weights);
}

template <typename T>
void Solver<T>::matvec(const void *d, void *ret_inout, double add) {
    LSSVM_REQUIRE(d != nullptr && ret_inout != nullptr, "The d / ret arrays may not be empty!");              // csvm.cpp:284-286
    LSSVM_REQUIRE(add == 1.0 || add == -1.0, "add must either be -1.0 or 1.0, but is " + std::to_string(add) + "!");  // svm_kernel.cpp:28
    const size_t bytes = static_cast<size_t>(shards_[0]->n_) * sizeof(T);
    for (auto &p : shards_) {
        p->activate();
        // tmp_ <- d (zero padded), Ad <- ret
        LSSVM_HIP_CHECK(hipMemcpyAsync(p->tmp_.p, d, bytes, hipMemcpyHostToDevice, p->stream()));
        LSSVM_HIP_CHECK(hipMemcpyAsync(p->own_.Ad.p, ret_inout, bytes, hipMemcpyHostToDevice, p->stream()));
        CgSteps<T>(*p).sum_and_qdot(p->own_, p->tmp_.p, SC_S, SC_QD);
    }
    apply_K(Vec::tmp);
    for (auto &p : shards_) {
        p->activate();
        CgSteps<T>(*p).apply_ret(p->own_, p->Kres_, p->tmp_.p, add);
    }
    Problem<T> &p0 = *shards_[0];
    p0.activate();
    LSSVM_HIP_CHECK(hipMemcpyAsync(ret_inout, p0.own_.Ad.p, bytes, hipMemcpyDeviceToHost, p0.stream()));
    sync_all();
}

/* k_update_d packs the next matvec's records (Problem::pack_for_d) -- except over the IPC exchange: there a rank may clear its partial vector only once every peer
 * has read the previous one, which the host establishes in apply_K, after the direction update. */
template <typename T>
PackDc<T> Solver<T>::pack_with_direction(Problem<T> &p) {
    if (exchange_ == Exchange::process_peer) return PackDc<T>{};
    const bool skip = world_ > 1 && opt_.skip_collective != 0;
    return p.pack_for_d((p.sym_ && exchange_ != Exchange::none) || skip);
}

/* Shares by measured pace (lssvm_mi355_problem_rebalance).  weights == NULL: every shard's tile-kernel time per implicit matvec so far (HIP events) against the area
 * of its share -- one process driving all shards knows them all; one process per GPU gathers them over the library's RCCL communicator, so that every rank
 * computes the same weights (no such channel over HIP IPC: explicit weights only).  Nothing changes where the times lie within 2 % of each other.  Call between
 * cg_step calls. */
template <typename T>
int Solver<T>::rebalance(const double *weights, int count) {
    if (world_ <= 1 || !shards_[0]->sym_) return 0;
    sync_all();
    std::vector<double> w;
    if (weights != nullptr) {
        LSSVM_REQUIRE(count == world_, "one weight per rank");
        for (int k = 0; k < count; ++k) {
            LSSVM_REQUIRE(std::isfinite(weights[k]) && weights[k] > 0.0, "shard weights must be positive and finite");
            w.push_back(weights[k]);
        }
    } else {
        // pace of rank r = area of its share / kernel time per matvec
        std::vector<double> ms(static_cast<size_t>(world_), 0.0);
        for (auto &p : shards_) {
            p->activate();
            p->drain_events();
            // (since the last reshard, and never the cold first matvec of cg_begin: enqueue_apply_K_local does not time launch 0)
            const uint64_t timed = p->matvec_timed_ - p->pace_timed0_;
            ms[static_cast<size_t>(p->rank_)] = timed > 0 ? (p->matvec_ms_ - p->pace_ms0_) / static_cast<double>(timed) : 0.0;
        }
        if (static_cast<int>(shards_.size()) != world_) {  // one process per GPU: every rank contributes its own time
            LSSVM_REQUIRE(exchange_ == Exchange::process_rccl, "measured shares need the RCCL communicator between the processes (give explicit weights over HIP IPC)");
            Problem<T> &p = *shards_[0];
            p.activate();
            DevBuf<double> all;
            all.alloc_zero(static_cast<size_t>(world_), p.stream());
            LSSVM_HIP_CHECK(hipMemcpyAsync(all.p + p.rank_, &ms[static_cast<size_t>(p.rank_)], sizeof(double), hipMemcpyHostToDevice, p.stream()));
            Comm &c = comm();
            nccl_check(c.pAllGather(all.p + p.rank_, all.p, 1, ncclDouble, c.comm, p.stream()), "ncclAllGather");
            LSSVM_HIP_CHECK(hipMemcpyAsync(ms.data(), all.p, sizeof(double) * static_cast<size_t>(world_), hipMemcpyDeviceToHost, p.stream()));
            LSSVM_HIP_CHECK(hipStreamSynchronize(p.stream()));
        }
        double lo = ms[0], hi = ms[0];
        for (const double v : ms) {
            lo = std::min(lo, v);
            hi = std::max(hi, v);
        }
        if (!(lo > 0.0) || hi <= 1.02 * lo) return 0;  // (a rank without a timed matvec, or nothing to gain)
        const int tiles = shards_[0]->num_tiles_;
        double sum = 0.0;
        for (int r = 0; r < world_; ++r) {
            const double b0 = sym_block_boundary(tiles, r, world_, &shards_[0]->opt_.shard_weights), b1 = sym_block_boundary(tiles, r + 1, world_, &shards_[0]->opt_.shard_weights);
            const double area = 0.5 * (b1 * (b1 + 1.0) - b0 * (b0 + 1.0));
            w.push_back(std::max(area, 1.0) / ms[static_cast<size_t>(r)]);
            sum += w.back();
        }
        for (double &v : w) v *= static_cast<double>(world_) / sum;
    }
    for (auto &p : shards_) p->reshard(w);
    opt_.shard_weights = w;
    return 1;
}

template <typename T>
void Solver<T>::reset_cg(double eps, double y_last) {
    eps_ = eps;
    y_last_ = y_last;
    info_shard_ = -1;
    iter_ = 0;
    converged_ = false;
    cg_wall_ms_ = 0.0;
    for (auto &p : shards_) {
        p->matvec_ms_ = p->pace_ms0_ = 0.0;
        p->matvec_launches_ = 0;
        p->matvec_timed_ = p->pace_timed0_ = 0;
    }
}

template <typename T>
void Solver<T>::read_delta0(double t0) {
    Problem<T> &p0 = *shards_[0];
    p0.activate();
    LSSVM_HIP_CHECK(hipMemcpyAsync(p0.own_.host_sc.p, p0.own_.sc.p, SC_COUNT * sizeof(double), hipMemcpyDeviceToHost, p0.stream()));
    sync_all();
    delta0_ = static_cast<double>(static_cast<T>(p0.own_.host_sc.p[SC_DELTA0]));
    delta_ = delta0_;
    delta_before_ = 0.0;
    held_back_ = 0;
    begun_ = true;
    in_cg_ = true;
    cg_wall_ms_ += now_ms() - t0;
}

template <typename T>
void Solver<T>::cg_begin(const void *y, double eps) {
    LSSVM_REQUIRE(y != nullptr, "The right hand side vector must not be empty!");
    LSSVM_REQUIRE(static_cast<T>(eps) > T(0), "The stopping criterion in the CG algorithm must be greater than 0.0, but is " + std::to_string(eps) + "!");  // csvm.cpp:77
    const double t0 = now_ms();
    reset_cg(eps, static_cast<double>(static_cast<const T *>(y)[shards_[0]->N_ - 1]));
    for (auto &p : shards_) {
        p->activate();
        CgSteps<T>(*p).begin(p->own_, static_cast<const T *>(y));
    }
    // r = b - A x   (csvm.cpp:101-104)
    apply_K(Vec::x);
    for (auto &p : shards_) {
        p->activate();
        const CgSteps<T> cg(*p);
        cg.residual(p->own_, p->Kres_, p->own_.x.p, p->own_.r.p, PART_RR);
        cg.finish_delta(p->own_, PART_RR, p->own_.sc.p + SC_COUNT - 1, true);  // (delta0 is read with the scalars: read_delta0)
        cg.update_d(p->own_, true, pack_with_direction(*p));
    }
    read_delta0(t0);
}

/* The inner solve of the mixed-precision refinement begins: cg_begin's statements for b = r / max|r| and x = 0, where r = b - A x is b itself -- no Gram pass. */
template <typename T>
void Solver<T>::cg_begin_from_zero(const double *r_dev, const double *absmax_part_dev, double eps) {
    LSSVM_REQUIRE(r_dev != nullptr && absmax_part_dev != nullptr, "The right hand side vector must not be empty!");
    LSSVM_REQUIRE(static_cast<T>(eps) > T(0), "The stopping criterion in the CG algorithm must be greater than 0.0, but is " + std::to_string(eps) + "!");  // csvm.cpp:77
    LSSVM_REQUIRE(shards_.size() == 1 && world_ == 1, "the inner solve of the refinement runs on one device");
    const double t0 = now_ms();
    reset_cg(eps, 0.0);
    Problem<T> &p = *shards_[0];
    p.activate();
    const CgSteps<T> cg(p);
    cg.begin_from_zero(p.own_, r_dev, absmax_part_dev);
    cg.finish_delta(p.own_, PART_RR, p.own_.sc.p + SC_COUNT - 1, true);
    cg.update_d(p.own_, true, pack_with_direction(p));
    read_delta0(t0);
}

template <typename T>
void Solver<T>::cg_step(uint64_t iterations, int *done_out) {
    LSSVM_REQUIRE(begun_, "cg_step called before cg_begin");
    const double t0 = now_ms();
    // target residuum in the real type, exactly as the reference evaluates "eps * eps * delta0" (csvm.cpp:155)
    const T target = static_cast<T>(eps_) * static_cast<T>(eps_) * static_cast<T>(delta0_);
    Problem<T> &p0 = *shards_[0];
    const auto enqueue_direction_update = [&] {  // d = beta d + r   (csvm.cpp:161-163), and the sums the next matvec needs
        for (auto &p : shards_) {
            p->activate();
            CgSteps<T>(*p).update_d(p->own_, false, pack_with_direction(*p));
        }
    };
    bool matvec_enqueued = false;  // A d of the coming iteration is in the queue already (enqueued ahead of the previous stop test)
    for (uint64_t k = 0; k < iterations && !converged_; ++k) {
        // Ad = A d   (csvm.cpp:131-132)
        if (!matvec_enqueued) apply_K(Vec::d);
        matvec_enqueued = false;
        const bool refresh = iter_ % 50 == 49;
        for (auto &p : shards_) {
            p->activate();
            CgSteps<T>(*p).advance(p->own_, p->Kres_, refresh);
        }
        if (refresh) {  // r = b - A x   (csvm.cpp:140-145)
            apply_K(Vec::x);
            for (auto &p : shards_) {
                p->activate();
                CgSteps<T>(*p).residual(p->own_, p->Kres_, p->own_.x.p, p->own_.r.p, PART_RR);
            }
        }
        for (auto &p : shards_) {
            p->activate();
            // the stop test needs delta on the host: shard 0's kernel stores its 8 bytes straight into mapped host memory (all shards hold the same
            // bits); the others publish into a spare device word
            CgSteps<T>(*p).finish_delta(p->own_, PART_RR, p.get() == &p0 ? p0.own_.host_delta.dev : p->own_.sc.p + SC_COUNT - 1, false);  // csvm.cpp:152-153
        }
        p0.activate();
        LSSVM_HIP_CHECK(hipEventRecord(ev_delta_.e, p0.stream()));
        // Short matvecs (option enqueue_ahead_below_us): waiting for delta here would leave the device idle while the host wakes up and
        // launches the next kernels (about 4 % of a 50 000-point iteration).  So the direction update and the NEXT implicit matvec go
        // into the queue BEFORE the stop test is read: they touch d, K*d and the partial slabs only -- never x or r -- so a solve that
        // turns out to have converged is exactly where the reference stops (csvm.cpp:155-158), at the price of one discarded matvec.
        // The decision must be the same on every rank of a sharded solve (a rank that went ahead has one more collective in its queue than
        // one that did not: a hang at convergence, or every later collective paired one position off), so it is derived from the problem
        // alone -- size, feature count, real type, kernel path, world -- never from this rank's own event timings: an implicit matvec is priced at
        // the full-square rate of its path (one flat 500 TFLOP/s let the fp64 and generic kernels go ahead for matvecs ten times longer
        // than the option says, each converged solve then paying one discarded matvec of that length).  Every input is the same on all ranks.
        const double n_d = static_cast<double>(p0.n_);
        const double matvec_us = 2.0 * n_d * n_d * static_cast<double>(p0.X_.dfeat) / static_cast<double>(world_) / p0.nominal_full_square_rate() * 1e6;
        // Round 6: ... unless this iteration is forecast to be the last.  The discarded matvec is a third of a solve that converges after two iterations (the
        // reference's default epsilon on BASELINE configs[1]: 3.2 ms of CG where 2.4 are needed).  With the residuum falling by rho = delta / delta_before per
        // iteration, the stop test is about to succeed once delta rho^2 <= target -- this iteration or the next: for those (at most four in a row, should the
        // residuum stall there) the host waits for delta before it enqueues anything, as it does for long matvecs.  delta, its predecessor and the target are the
        // same bits on every rank, so every rank decides alike (see above); matvecs shorter than 100 us are not worth a host round trip and always go ahead.
        bool last_iterations = false;
        if (matvec_us >= 100.0 && delta_before_ > 0.0 && delta_ > 0.0 && held_back_ < 4) {
            const double rho = std::min(delta_ / delta_before_, 1.0);
            last_iterations = delta_ * rho * rho <= static_cast<double>(target);
        }
        held_back_ = last_iterations ? held_back_ + 1 : 0;
        const bool ahead = opt_.enqueue_ahead_below_us > 0 && matvec_us < static_cast<double>(opt_.enqueue_ahead_below_us) && k + 1 < iterations
                           && exchange_ != Exchange::process_peer && !last_iterations;
        if (ahead) {
            enqueue_direction_update();
            apply_K(Vec::d);
            p0.activate();
        }
        LSSVM_HIP_CHECK(hipEventSynchronize(ev_delta_.e));
        for (auto &p : shards_) p->drain_events();
        ++iter_;
        delta_before_ = delta_;
        delta_ = static_cast<double>(static_cast<T>(p0.own_.delta_on_host()));
        if (static_cast<T>(delta_) <= target) {  // csvm.cpp:155-158: tested BEFORE the direction update
            converged_ = true;
            if (ahead) sync_all();  // let the discarded work drain
            break;
        }
        if (ahead) {
            matvec_enqueued = true;
        } else {
            enqueue_direction_update();
        }
    }
    cg_wall_ms_ += now_ms() - t0;
    if (done_out != nullptr) *done_out = converged_ ? 1 : 0;
}

template <typename T>
void Solver<T>::cg_finish(void *alpha_out, double *rho_out, lssvm_cg_info *info) {
    LSSVM_REQUIRE(begun_, "cg_finish called before cg_begin");
    LSSVM_REQUIRE(alpha_out != nullptr && rho_out != nullptr, "alpha_out / rho_out must not be NULL");
    in_cg_ = false;
    const double t0 = now_ms();
    Problem<T> &p0 = *shards_[0];
    const bool check = shards_.size() > 1 && exchange_ != Exchange::none;
    for (auto &p : shards_) {
        if (p.get() != &p0 && !check) continue;
        p->activate();
        CgSteps<T>(*p).enqueue_finish(p->own_, p.get() == &p0 ? static_cast<T *>(alpha_out) : nullptr);
    }
    sync_all();
    if (check) {
        // every shard ran the same O(n) kernels on the same exchanged vectors: their scalars must agree to the bit
        for (auto &p : shards_) {
            for (int slot : { static_cast<int>(SC_DELTA), static_cast<int>(SC_SUMX), static_cast<int>(SC_QX) }) {
                if (std::memcmp(&p->own_.host_sc.p[slot], &p0.own_.host_sc.p[slot], sizeof(double)) != 0) {
                    throw Error(LSSVM_ERR_INTERNAL, "the shards of the solve diverged: device " + std::to_string(p->device_) + " holds another CG scalar than device "
                                                        + std::to_string(p0.device_));
                }
            }
        }
    }
    CgSteps<T>(p0).read_solution(p0.own_, y_last_, static_cast<T *>(alpha_out), rho_out);
    cg_wall_ms_ += now_ms() - t0;
    if (info != nullptr) fill_info(info);
}

/* ------------------------------------------------------------------ two vectors per Gram pass: matvec_pair, the lockstep CG ------------------------------------------------------------------ */
template <typename T>
bool Solver<T>::lanes_apply() const {
    return shards_.size() == 1 && world_ == 1 && exchange_ == Exchange::none && shards_[0]->pair_kernel_applies();
}

template <typename T>
void Solver<T>::wait_for_deltas() {
    LSSVM_HIP_CHECK(hipGetLastError());
    LSSVM_HIP_CHECK(hipEventRecord(ev_delta_.e, shards_[0]->stream()));
    LSSVM_HIP_CHECK(hipEventSynchronize(ev_delta_.e));
}

template <typename T>
void Solver<T>::matvec_pair(const void *d0, const void *d1, void *ret0_inout, void *ret1_inout, double add, int *two_vector_out) {
    LSSVM_REQUIRE(d0 != nullptr && d1 != nullptr && ret0_inout != nullptr && ret1_inout != nullptr, "The d / ret arrays may not be empty!");  // csvm.cpp:284-286
    LSSVM_REQUIRE(add == 1.0 || add == -1.0, "add must either be -1.0 or 1.0, but is " + std::to_string(add) + "!");                       // svm_kernel.cpp:28
    LSSVM_REQUIRE(!in_cg_, "matvec_pair cannot run between cg_begin and cg_finish");
    if (two_vector_out != nullptr) *two_vector_out = 0;
    if (!lanes_apply()) {  // two single passes
        matvec(d0, ret0_inout, add);
        matvec(d1, ret1_inout, add);
        return;
    }
    // the statements of matvec() per vector on two lanes (d <- d_u zero padded, Ad <- ret_u), around ONE pass of the two-vector kernel
    Problem<T> &p = *shards_[0];
    const CgSteps<T> cg(p);
    const CgState<T> *lane[2] = { &p.lane(0), &p.lane(1) };
    const void *d[2] = { d0, d1 };
    void *ret[2] = { ret0_inout, ret1_inout };
    const size_t bytes = static_cast<size_t>(p.n_) * sizeof(T);
    for (int u = 0; u < 2; ++u) {
        LSSVM_HIP_CHECK(hipMemcpyAsync(lane[u]->d.p, d[u], bytes, hipMemcpyHostToDevice, p.stream()));
        LSSVM_HIP_CHECK(hipMemcpyAsync(lane[u]->Ad.p, ret[u], bytes, hipMemcpyHostToDevice, p.stream()));
        cg.sum_and_qdot(*lane[u], lane[u]->d.p, SC_S, SC_QD);
    }
    p.enqueue_apply_K_lanes(lane[0]->d.p, lane[0]->Kv.p, lane[1]->d.p, lane[1]->Kv.p, nullptr, nullptr);
    for (int u = 0; u < 2; ++u) {
        cg.apply_ret(*lane[u], lane[u]->Kv.p, lane[u]->d.p, add);
        LSSVM_HIP_CHECK(hipMemcpyAsync(ret[u], lane[u]->Ad.p, bytes, hipMemcpyDeviceToHost, p.stream()));
    }
    sync_all();
    if (two_vector_out != nullptr) *two_vector_out = 1;
}

template <typename T>
void Solver<T>::solve_lockstep(const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out, double *rhos_out, lssvm_cg_info *infos_out, uint64_t *passes_out) {
    LSSVM_REQUIRE(Y != nullptr, "The right hand side vector must not be empty!");
    LSSVM_REQUIRE(num_rhs > 0, "The number of right hand sides must be greater than 0!");
    LSSVM_REQUIRE(static_cast<T>(eps) > T(0), "The stopping criterion in the CG algorithm must be greater than 0.0, but is " + std::to_string(eps) + "!");  // csvm.cpp:77
    LSSVM_REQUIRE(max_iter > 0, "The number of CG iterations must be greater than 0!");                                                                   // csvm.cpp:78
    LSSVM_REQUIRE(alphas_out != nullptr && rhos_out != nullptr, "alpha_out / rho_out must not be NULL");
    LSSVM_REQUIRE(!in_cg_, "solve_lockstep cannot run between cg_begin and cg_finish");
    if (passes_out != nullptr) passes_out[0] = passes_out[1] = 0;
    if (lanes_apply()) {
        solve_on_lanes(static_cast<const T *>(Y), num_rhs, eps, max_iter, static_cast<T *>(alphas_out), rhos_out, infos_out, passes_out);
    } else {
        solve_in_sequence(Y, num_rhs, eps, max_iter, alphas_out, rhos_out, infos_out, passes_out);
    }
}

/* Where no Gram pass can serve two vectors: today's sequence, one right-hand side after the other.  Nothing is enqueued ahead of a stop test (as on the lanes), so a
 * solve takes exactly 1 + it + it / 50 single-vector passes; the bits are those of the one-shot solve either way. */
template <typename T>
void Solver<T>::solve_in_sequence(const void *Y, size_t num_rhs, double eps, uint64_t max_iter, void *alphas_out, double *rhos_out, lssvm_cg_info *infos_out, uint64_t *passes_out) {
    const double t_call = now_ms();
    const size_t N = shards_[0]->N_;
    const SetOnExit<int64_t> restore(opt_.enqueue_ahead_below_us, opt_.enqueue_ahead_below_us);
    const SetOnExit<bool> release(in_cg_, false);  // (a solve that threw between cg_begin and cg_finish does not keep the handle)
    opt_.enqueue_ahead_below_us = 0;
    for (size_t c = 0; c < num_rhs; ++c) {
        cg_begin(static_cast<const T *>(Y) + c * N, eps);
        cg_step(max_iter, nullptr);
        lssvm_cg_info info{};
        cg_finish(static_cast<T *>(alphas_out) + c * N, rhos_out + c, &info);
        info.max_iterations = max_iter;
        info.total_ms = now_ms() - t_call;
        if (passes_out != nullptr) passes_out[1] += info.matvec_launches;
        if (infos_out != nullptr) infos_out[c] = info;
    }
}

/* The recipe of cg_begin / cg_step / cg_finish for every right-hand side, each on a lane of shard 0 with the steps of the single solve on that lane's state -- so every
 * recurrence has the bits of the one-shot solve -- all lanes advancing one iteration per step.  In every step the lanes still active are paired afresh for the
 * implicit matvec: ceil(active / 2) Gram passes, an odd lane taking the single-vector pass.  The host waits for the step's deltas before it enqueues the next step. */
template <typename T>
void Solver<T>::solve_on_lanes(const T *Y, size_t num_rhs, double eps, uint64_t max_iter, T *alphas_out, double *rhos_out, lssvm_cg_info *infos_out, uint64_t *passes_out) {
    const double t_call = now_ms();
    Problem<T> &p = *shards_[0];
    p.activate();
    const CgSteps<T> cg(p);
    const size_t N = p.N_;
    struct State {
        const CgState<T> *lane = nullptr;
        double y_last = 0.0, delta0 = 0.0, delta = 0.0;
        uint64_t matvecs = 0, timed = 0;
        double kernel_ms = 0.0;
        bool converged = false;
    };
    std::vector<State> state(num_rhs);
    for (size_t c = 0; c < num_rhs; ++c) state[c].lane = &p.lane(c);
    std::vector<size_t> active(num_rhs);
    for (size_t c = 0; c < num_rhs; ++c) active[c] = c;
    uint64_t passes[2] = { 0, 0 };

    // one Gram pass per pair of active lanes (`x`: of their x, else of their d) into their K*v; HIP events around every pass, read back after the step's wait
    struct Timed {
        Event a, b;
        size_t lane0 = 0, lane1 = 0;
        bool two = false;
    };
    std::vector<Timed> timers(2 * ((num_rhs + 1) / 2));  // (a step with a residual refresh makes two rounds of passes before its wait)
    for (Timed &t : timers) {
        t.a.create(true);
        t.b.create(true);
    }
    size_t timers_used = 0;
    const auto apply_K = [&](bool x) {
        for (size_t k = 0; k < active.size(); k += 2) {
            State &s0 = state[active[k]];
            State *s1 = k + 1 < active.size() ? &state[active[k + 1]] : nullptr;
            Timed &t = timers[timers_used++];
            t.lane0 = active[k];
            t.two = s1 != nullptr;
            t.lane1 = t.two ? active[k + 1] : 0;
            p.enqueue_apply_K_lanes(x ? s0.lane->x.p : s0.lane->d.p, s0.lane->Kv.p, t.two ? (x ? s1->lane->x.p : s1->lane->d.p) : nullptr, t.two ? s1->lane->Kv.p : nullptr, t.a.e, t.b.e);
            ++passes[t.two ? 0 : 1];
            ++s0.matvecs;
            if (t.two) ++s1->matvecs;
        }
    };
    const auto read_timers = [&] {  // (the stream has been waited for)
        for (size_t k = 0; k < timers_used; ++k) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, timers[k].a.e, timers[k].b.e) != hipSuccess) continue;
            for (int u = 0; u < (timers[k].two ? 2 : 1); ++u) {
                State &s = state[u == 0 ? timers[k].lane0 : timers[k].lane1];
                s.kernel_ms += ms;
                ++s.timed;
            }
        }
        timers_used = 0;
    };

    const SetOnExit<bool> busy = hold_busy();  // (the weights may not change, and no other solve may begin on this handle)
    // ---- cg_begin per lane: b = y - y_last, x = 1, r = b - A x, delta0, d = r ----
    for (size_t c : active) {
        state[c].y_last = static_cast<double>(Y[c * N + N - 1]);
        cg.begin(*state[c].lane, Y + c * N);
    }
    apply_K(true);
    for (size_t c : active) {
        const CgState<T> &l = *state[c].lane;
        cg.residual(l, l.Kv.p, l.x.p, l.r.p, PART_RR);
        cg.finish_delta(l, PART_RR, l.host_delta.dev, true);
        cg.update_d(l, true);  // (the records are packed per pass, for the pair of the step)
    }
    wait_for_deltas();
    read_timers();
    for (size_t c : active) state[c].delta0 = state[c].delta = static_cast<double>(static_cast<T>(state[c].lane->delta_on_host()));

    // ---- cg_step: one iteration of every active lane per step ----
    for (uint64_t iter = 0; !active.empty(); ++iter) {
        const bool refresh = iter % 50 == 49;
        apply_K(false);
        for (size_t c : active) cg.advance(*state[c].lane, state[c].lane->Kv.p, refresh);
        if (refresh) {
            apply_K(true);
            for (size_t c : active) {
                const CgState<T> &l = *state[c].lane;
                cg.residual(l, l.Kv.p, l.x.p, l.r.p, PART_RR);
            }
        }
        for (size_t c : active) cg.finish_delta(*state[c].lane, PART_RR, state[c].lane->host_delta.dev, false);
        wait_for_deltas();
        read_timers();
        // the stop test in the real type, before the direction update (csvm.cpp:155-158); a lane that meets it, or has done max_iter iterations, leaves
        std::vector<size_t> staying;
        for (size_t c : active) {
            State &s = state[c];
            s.delta = static_cast<double>(static_cast<T>(s.lane->delta_on_host()));
            const T target = static_cast<T>(eps) * static_cast<T>(eps) * static_cast<T>(s.delta0);
            s.converged = static_cast<T>(s.delta) <= target;
            if (!s.converged && iter + 1 < max_iter) {
                cg.update_d(*s.lane, false);
                staying.push_back(c);
                continue;
            }
            cg.finish_now(*s.lane, s.y_last, alphas_out + c * N, rhos_out + c);
            if (infos_out != nullptr) {
                // what cg_finish reports for a one-shot solve, with this lane's counters; total_ms: from the start of the call until the lane left
                lssvm_cg_info info{};
                fill_cg_outcome(&info, iter + 1, max_iter, s.delta, s.delta0, static_cast<double>(target), eps, now_ms() - t_call, s.converged);
                describe_path(&info);
                info.matvec_launches = s.matvecs;
                info.matvec_timed = s.timed;
                info.matvec_kernel_ms_total = s.kernel_ms;
                info.matvec_kernel_ms = s.timed > 0 ? s.kernel_ms / static_cast<double>(s.timed) : 0.0;
                infos_out[c] = info;
            }
        }
        active.swap(staying);
    }
    if (passes_out != nullptr) {
        passes_out[0] = passes[0];
        passes_out[1] = passes[1];
    }
}

template <typename T>
void Solver<T>::synchronize() {
    sync_all();
}

template <typename T>
void Solver<T>::fill_info(lssvm_cg_info *info) {
    std::memset(info, 0, sizeof(*info));
    fill_cg_outcome(info, iter_, 0, delta_, delta0_, static_cast<double>(static_cast<T>(eps_) * static_cast<T>(eps_) * static_cast<T>(delta0_)), eps_, cg_wall_ms_, converged_);
    describe_path(info);
}

/* the fields of lssvm_cg_info that describe the problem, its kernel path and the tile-kernel times of the handle's own (single-vector) CG state */
template <typename T>
void Solver<T>::describe_path(lssvm_cg_info *info) {
    const Problem<T> &p0 = *shards_[0];
    info->setup_ms = setup_ms_;
    // the tile kernel of the slowest shard sets the pace of a sharded matvec.  WHICH shard is reported is decided once per cg_begin (the first call that finds timed
    // matvecs) and kept, so that the differences of (matvec_kernel_ms_total, matvec_timed) between two calls always belong to one shard
    if (info_shard_ < 0) {
        double slowest = 0.0;
        for (size_t r = 0; r < shards_.size(); ++r) {
            const double avg = shards_[r]->matvec_timed_ > 0 ? shards_[r]->matvec_ms_ / static_cast<double>(shards_[r]->matvec_timed_) : 0.0;
            if (avg > slowest) {
                slowest = avg;
                info_shard_ = static_cast<int>(r);
            }
        }
    }
    if (info_shard_ >= 0) {
        const Problem<T> &p = *shards_[static_cast<size_t>(info_shard_)];
        info->matvec_timed = p.matvec_timed_;
        info->matvec_kernel_ms_total = p.matvec_ms_;
        info->matvec_kernel_ms = p.matvec_timed_ > 0 ? p.matvec_ms_ / static_cast<double>(p.matvec_timed_) : 0.0;
    }
    info->f16_row_rel_error = p0.f16_row_rel_error_;
    info->matvec_launches = p0.matvec_launches_;
    info->devices_used = world_;
    info->symmetric = p0.sym_ ? 1 : 0;
    info->gram_mode = (p0.planes_.mode != 0 && p0.dc_.p != nullptr) ? (p0.rbf_grid_ ? 3 : p0.planes_.mode) : 0;  // (a split kernel is dispatched only where both exist; 3: rbf on grid planes)
    info->local_devices = static_cast<int32_t>(shards_.size());
    info->rbf_direct = p0.rbf_direct_ ? 1 : 0;
    info->rbf_exponent_scale = p0.rbf_r2_;
    info->tile_launches_per_matvec = static_cast<int32_t>(std::max<size_t>(p0.bands_.size(), 1)) * p0.passes_per_matvec();  // bands x feature panels
    info->persistent_launches = 0;
    if (p0.queue_.p != nullptr) {
        for (const auto &band : p0.bands_) info->persistent_launches += band.item_count > p0.queue_min_items_ ? p0.passes_per_matvec() : 0;
    }
    info->exchange = exchange_ == Exchange::none ? 0 : ((exchange_ == Exchange::peer || exchange_ == Exchange::process_peer) ? 2 : 1);
    // what RCCL itself says about the communicator the partial vectors travel over (a bench line can then prove that N ranks met)
    info->rccl_nranks = 0;
    info->rccl_rank = info->rccl_device = -1;
    ncclComm_t used = exchange_ == Exchange::process_rccl ? comm().comm : (exchange_ == Exchange::local_rccl && local_comms_ ? local_comms_->comms[0] : nullptr);
    if (used != nullptr) {
        int v = 0;
        if (comm().pCommCount(used, &v) == ncclSuccess) info->rccl_nranks = v;
        if (comm().pCommUserRank(used, &v) == ncclSuccess) info->rccl_rank = v;
        if (comm().pCommCuDevice(used, &v) == ncclSuccess) info->rccl_device = v;
    }
}

template class Solver<float>;
template class Solver<double>;

}  // namespace lssvm
