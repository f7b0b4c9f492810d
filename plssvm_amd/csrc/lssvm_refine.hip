/*
 * lssvm_refine.hip -- mixed-precision iterative refinement (lssvm_mi355_solve_refined_f64): the fp64 LS-SVM system solved to the fp64 stop test
 * with the CG iterations run by the fp32 solver on the matrix-core kernels.  Two resident problems over the same points, Solver<double> P64 and Solver<float> P32 on
 * the data rounded to float.  P64 supplies the TRUE residual r = b - A x, one fp64 Gram pass per outer step; P32 solves A e = r / max|r| from e = 0
 * (Solver<float>::cg_begin_from_zero, then cg_step as ever); x + max|r| e is kept if the true residual's norm fell to at most REFINE_ACCEPT_RATIO, else the plain fp64 CG
 * continues from the (x, r) before that step.  Every right-hand side lives on a lane of P64; the outer passes of two right-hand sides that are due together share one
 * pass of the two-vector kernel, which leaves each the bits of its own pass -- so a column of a multi call has the bits of the single call.  No tile kernel is involved
 * beyond being launched; the CG recipe is CgSteps' (lssvm_solver.hip), the kernels launched here are the refinement's own, k_absmax and k_axpy_up.  Compiled for gfx950 only.
 */
#include "lssvm_problem.hip.hpp"

#include "lssvm_kernels.hip.hpp"

#include <algorithm>
#include <cmath>

namespace lssvm {

struct Refiner {
    using Lane = CgState<double>;

    Solver<double> &s64;
    Solver<float> &s32;
    Problem<double> &p;
    const CgSteps<double> cg;
    const bool lanes;  // the right-hand sides advance together on lanes and pair their outer passes; else one after the other on lane 0 with the problem's own pass
    const double eps;
    const uint64_t max_iter;
    const double t_call;
    hipStream_t st;
    int n;
    uint64_t passes[2] = { 0, 0 };

    struct Rhs {
        Lane *lane = nullptr;
        double *Kv = nullptr;  // where a pass leaves K * v for this right-hand side
        double y_last = 0.0, delta0 = 0.0, rr = 0.0, target = 0.0;
        uint64_t outer = 0, inner = 0, f64_it = 0, f64_passes = 0, f32_passes = 0;
        double f64_ms = 0.0, f32_ms = 0.0;
        bool took_over = false, finished = false;
        uint64_t budget_left(uint64_t max_iter) const { return max_iter - std::min(max_iter, inner + f64_it); }
    };
    std::vector<Rhs> rhs;

    Refiner(Solver<double> &a, Solver<float> &b, size_t num_rhs, double eps_, uint64_t max_iter_, double t_call_) :
        s64(a), s32(b), p(a.shard0()), cg(p), lanes(a.lanes_apply()), eps(eps_), max_iter(max_iter_), t_call(t_call_), rhs(num_rhs) {
        p.activate();
        st = cg.stream();
        n = cg.n();
        for (size_t c = 0; c < num_rhs; ++c) {
            rhs[c].lane = &p.lane(lanes ? c : 0);
            rhs[c].Kv = lanes ? rhs[c].lane->Kv.p : cg.Kres();
        }
    }

    /* K * v for the right-hand sides `who`, v = lane vector `which` of each: two per pass of the two-vector kernel on lanes, else the problem's single-vector pass */
    template <typename Which>
    void apply_K(const std::vector<size_t> &who, Which which) {
        LSSVM_REQUIRE(lanes || who.size() == 1, "without lanes the right-hand sides are solved one at a time");
        for (size_t k = 0; k < who.size(); k += 2) {
            Rhs &r0 = rhs[who[k]];
            Rhs *r1 = (lanes && k + 1 < who.size()) ? &rhs[who[k + 1]] : nullptr;
            if (lanes) {
                p.enqueue_apply_K_lanes(which(*r0.lane), r0.Kv, r1 != nullptr ? which(*r1->lane) : nullptr, r1 != nullptr ? r1->Kv : nullptr, nullptr, nullptr);
            } else {
                p.enqueue_apply_K_local(which(*r0.lane), false);  // (into cg.Kres(): `who` is a single right-hand side here)
            }
            ++passes[r1 != nullptr ? 0 : 1];
            ++r0.f64_passes;
            if (r1 != nullptr) ++r1->f64_passes;
        }
    }
    void wait() {
        s64.wait_for_deltas();
        p.drain_events();
    }

    /* step 2: b = y - y_last, x = 1, r = b - A x, delta0, target; the largest |r_i| for the first step */
    void begin(const std::vector<size_t> &who, const double *Y) {
        const double t0 = now_ms();
        const size_t N = cg.num_points();
        const dim3 gr(RED_BLOCKS), br(RED_THREADS);
        for (size_t c : who) {
            rhs[c].y_last = Y[c * N + N - 1];
            cg.begin(*rhs[c].lane, Y + c * N);
        }
        apply_K(who, [](const Lane &l) { return l.x.p; });
        for (size_t c : who) {
            const Rhs &r = rhs[c];
            const Lane &l = *r.lane;
            cg.residual(l, r.Kv, l.x.p, l.r.p, PART_RR);
            cg.finish_delta(l, PART_RR, l.host_delta.dev, true);
            hipLaunchKernelGGL(k_absmax<double>, gr, br, 0, st, l.r.p, n, l.part_of(PART_D));
        }
        wait();
        const double ms = now_ms() - t0;
        for (size_t c : who) {
            Rhs &r = rhs[c];
            r.delta0 = r.rr = r.lane->delta_on_host();
            r.target = eps * eps * r.delta0;
            r.f64_ms += ms;
        }
    }

    /* step 3 for every right-hand side of `who` that is still due, until none is; a rejected step hands its right-hand side to take_over */
    void refine(const std::vector<size_t> &who) {
        const dim3 gr(RED_BLOCKS), br(RED_THREADS);
        const size_t vec_bytes = static_cast<size_t>(n) * sizeof(double), part_bytes = static_cast<size_t>(RED_BLOCKS) * 2 * sizeof(double);
        for (;;) {
            std::vector<size_t> due;
            for (size_t c : who) {
                Rhs &r = rhs[c];
                if (r.finished) continue;
                if (r.rr > r.target && r.budget_left(max_iter) > 0) {
                    due.push_back(c);
                } else {
                    r.finished = true;
                }
            }
            if (due.empty()) return;
            // the inner fp32 solves, one after the other (fp32 has no two-vector symmetric kernel): e lands in l.d as x_try = x + s e
            for (size_t c : due) {
                Rhs &r = rhs[c];
                const Lane &l = *r.lane;
                const double t0 = now_ms();
                const double eps_in = std::min(std::max(0.5 * eps * std::sqrt(r.delta0) / std::sqrt(r.rr), REFINE_INNER_EPS_MIN), REFINE_INNER_EPS_MAX);
                s32.cg_begin_from_zero(l.r.p, l.part_of(PART_D), eps_in);
                s32.cg_step(std::min(REFINE_INNER_CAP, r.budget_left(max_iter)), nullptr);
                s32.synchronize();
                lssvm_cg_info inner{};
                s32.fill_info(&inner);
                r.inner += inner.iterations;
                r.f32_passes += inner.matvec_launches;
                r.f32_ms += now_ms() - t0;
                p.activate();
                hipLaunchKernelGGL((k_axpy_up<double, float>), gr, br, 0, st, l.x.p, s32.x_dev(), l.part_of(PART_D), cg.q(), n, l.d.p, l.part_of(PART_SUMS));
                cg.finish_sums(l, SC_SUMX, SC_QX);
                if (due.size() > 1) LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (the next inner solve overwrites e)
            }
            // the true residuals r_try = b - A x_try (into l.Ad), two right-hand sides per fp64 pass
            const double t0 = now_ms();
            apply_K(due, [](const Lane &l) { return l.d.p; });
            for (size_t c : due) {
                const Rhs &r = rhs[c];
                const Lane &l = *r.lane;
                cg.residual(l, r.Kv, l.d.p, l.Ad.p, PART_DAD);
                cg.finish_delta(l, PART_DAD, l.host_delta.dev, false);
                hipLaunchKernelGGL(k_absmax<double>, gr, br, 0, st, l.Ad.p, n, l.part_of(PART_D));
            }
            wait();
            const double ms = now_ms() - t0;
            for (size_t c : due) {
                Rhs &r = rhs[c];
                const Lane &l = *r.lane;
                const double rr_try = l.delta_on_host();
                ++r.outer;
                r.f64_ms += ms;
                if (std::isfinite(rr_try) && std::sqrt(rr_try) <= REFINE_ACCEPT_RATIO * std::sqrt(r.rr)) {
                    LSSVM_HIP_CHECK(hipMemcpyAsync(l.x.p, l.d.p, vec_bytes, hipMemcpyDeviceToDevice, st));
                    LSSVM_HIP_CHECK(hipMemcpyAsync(l.r.p, l.Ad.p, vec_bytes, hipMemcpyDeviceToDevice, st));
                    LSSVM_HIP_CHECK(hipMemcpyAsync(l.part_of(PART_RR), l.part_of(PART_DAD), part_bytes, hipMemcpyDeviceToDevice, st));
                    r.rr = rr_try;
                } else {
                    r.took_over = true;
                    take_over(r);
                    r.finished = true;
                }
            }
            LSSVM_HIP_CHECK(hipStreamSynchronize(st));  // (the next inner solve reads l.r from the fp32 problem's stream)
        }
    }

    /* step 4: the recipe of cg_step in fp64 from the current (x, r) -- d = r, delta = r^T r (the partial sums of the accepted residual are still in PART_RR) */
    void take_over(Rhs &r) {
        const double t0 = now_ms();
        const Lane &l = *r.lane;
        const std::vector<size_t> me{ static_cast<size_t>(&r - rhs.data()) };
        cg.finish_delta(l, PART_RR, l.host_delta.dev, false);
        cg.update_d(l, true);
        const uint64_t budget = r.budget_left(max_iter);
        for (uint64_t it = 0; it < budget; ++it) {
            const bool refresh = it % 50 == 49;
            apply_K(me, [](const Lane &ln) { return ln.d.p; });
            cg.advance(l, r.Kv, refresh);
            if (refresh) {
                apply_K(me, [](const Lane &ln) { return ln.x.p; });
                cg.residual(l, r.Kv, l.x.p, l.r.p, PART_RR);
            }
            cg.finish_delta(l, PART_RR, l.host_delta.dev, false);
            wait();
            r.rr = l.delta_on_host();
            ++r.f64_it;
            if (r.rr <= r.target) break;  // csvm.cpp:155-158: tested BEFORE the direction update
            cg.update_d(l, false);
        }
        r.f64_ms += now_ms() - t0;
    }

    /* step 5: cg_finish on the lane's x */
    void finish(size_t c, double *alphas_out, double *rhos_out, lssvm_cg_info *infos_out, lssvm_refine_info *refine_out, const lssvm_cg_info &path64, const lssvm_cg_info &path32) {
        const Rhs &r = rhs[c];
        cg.finish_now(*r.lane, r.y_last, alphas_out + c * cg.num_points(), rhos_out + c);
        const double total_ms = now_ms() - t_call;
        if (infos_out != nullptr) {
            lssvm_cg_info info = path64;  // the fp64 problem's description; the Gram mode is the inner solve's
            fill_cg_outcome(&info, r.inner + r.f64_it, max_iter, r.rr, r.delta0, r.target, eps, total_ms, r.rr <= r.target);
            info.setup_ms = path64.setup_ms + path32.setup_ms;
            info.matvec_launches = r.f64_passes + r.f32_passes;
            info.gram_mode = path32.gram_mode;
            info.rbf_direct = path32.rbf_direct;
            info.rbf_exponent_scale = path32.rbf_exponent_scale;
            info.f16_row_rel_error = path32.f16_row_rel_error;
            infos_out[c] = info;
        }
        if (refine_out != nullptr) {
            lssvm_refine_info ri{};
            ri.refined = 1;
            ri.took_over_f64 = r.took_over ? 1 : 0;
            ri.outer_steps = r.outer;
            ri.inner_iterations = r.inner;
            ri.f64_cg_iterations = r.f64_it;
            ri.f64_passes = r.f64_passes;
            ri.f32_passes = r.f32_passes;
            ri.initial_residuum = r.delta0;
            ri.residuum = r.rr;
            ri.target_residuum = r.target;
            ri.f64_ms = r.f64_ms;
            ri.f32_ms = r.f32_ms;
            ri.total_ms = total_ms;
            ri.inner_gram_mode = path32.gram_mode;
            ri.inner_rbf_direct = path32.rbf_direct;
            refine_out[c] = ri;
        }
    }
};

/* the plain fp64 solve on `s64`, as lssvm_mi355_solve_f64 / _solve_weighted_f64 (one right-hand side) or lssvm_mi355_problem_solve_lockstep runs it */
static void solve_plain(Solver<double> &s64, size_t N, const double *Y, size_t num_rhs, double eps, uint64_t max_iter, double *alphas_out, double *rhos_out, lssvm_cg_info *infos_out,
                        lssvm_refine_info *refine_out, uint64_t *passes_out, double t_call) {
    std::vector<lssvm_cg_info> infos(num_rhs);
    uint64_t passes[2] = { 0, 0 };
    if (num_rhs == 1) {
        s64.cg_begin(Y, eps);
        s64.cg_step(max_iter, nullptr);
        s64.cg_finish(alphas_out, rhos_out, &infos[0]);
        infos[0].max_iterations = max_iter;
        passes[1] = infos[0].matvec_launches;
    } else {
        s64.solve_lockstep(Y, num_rhs, eps, max_iter, alphas_out, rhos_out, infos.data(), passes);
    }
    (void) N;
    for (size_t c = 0; c < num_rhs; ++c) {
        if (infos_out != nullptr) infos_out[c] = infos[c];
        if (refine_out != nullptr) {
            lssvm_refine_info ri{};
            ri.f64_cg_iterations = infos[c].iterations;
            ri.f64_passes = infos[c].matvec_launches;
            ri.initial_residuum = infos[c].initial_residuum;
            ri.residuum = infos[c].residuum;
            ri.target_residuum = infos[c].target_residuum;
            ri.total_ms = ri.f64_ms = now_ms() - t_call;
            refine_out[c] = ri;
        }
    }
    if (passes_out != nullptr) {
        passes_out[0] = passes[0];
        passes_out[1] = passes[1];
    }
}

void solve_refined_f64(const Options &opt, const lssvm_params &params, const double *X, size_t num_points, size_t num_features, const double *Y, size_t num_rhs, const double *weights,
                       double eps, uint64_t max_iter, double *alphas_out, double *rhos_out, lssvm_cg_info *infos_out, lssvm_refine_info *refine_out, uint64_t *passes_out) {
    const double t_call = now_ms();
    static const int device0 = 0;
    const std::vector<int> devices = resolve_devices(&device0, 1, num_points);
    // P64, exactly as the one-shot fp64 solve creates it
    Solver<double> s64(opt, params, X, LSSVM_MEM_HOST, num_points, num_features, devices, nullptr);
    if (weights != nullptr) s64.set_weights(weights, num_points);
    // P32 on X rounded to float -- where that rounding leaves the data finite and the options leave an fp32 problem
    std::unique_ptr<Solver<float>> s32;
    std::vector<float> Xf(num_points * num_features);
    bool finite = true;
    for (size_t k = 0; k < Xf.size(); ++k) {
        Xf[k] = static_cast<float>(X[k]);
        finite = finite && std::isfinite(Xf[k]);
    }
    if (finite) {
        try {
            s32 = std::make_unique<Solver<float>>(opt, params, Xf.data(), LSSVM_MEM_HOST, num_points, num_features, devices, nullptr);
            if (weights != nullptr) s32->set_weights(weights, num_points);
        } catch (const Error &e) {
            if (e.status != LSSVM_ERR_INVALID_ARGUMENT && e.status != LSSVM_ERR_INTERNAL) throw;  // (a device or memory error is not an option's doing)
            s32.reset();
        }
    }
    std::vector<float>().swap(Xf);
    if (!s32) {
        solve_plain(s64, num_points, Y, num_rhs, eps, max_iter, alphas_out, rhos_out, infos_out, refine_out, passes_out, t_call);
        return;
    }
    lssvm_cg_info path64{}, path32{};
    s64.fill_info(&path64);
    s32->fill_info(&path32);
    Refiner ref(s64, *s32, num_rhs, eps, max_iter, t_call);
    const SetOnExit<bool> busy = s64.hold_busy();  // between begin and finish no other solve may begin on the fp64 problem, and its weights stay
    std::vector<std::vector<size_t>> groups;
    if (ref.lanes) {
        groups.emplace_back();
        for (size_t c = 0; c < num_rhs; ++c) groups[0].push_back(c);
    } else {
        for (size_t c = 0; c < num_rhs; ++c) groups.push_back({ c });
    }
    for (const auto &who : groups) {
        ref.begin(who, Y);
        ref.refine(who);
        for (size_t c : who) ref.finish(c, alphas_out, rhos_out, infos_out, refine_out, path64, path32);
    }
    if (passes_out != nullptr) {
        passes_out[0] = ref.passes[0];
        passes_out[1] = ref.passes[1];
    }
}

}  // namespace lssvm
