"""GPU (-m gpu): the leave-one-out scores of every prefix rank of one fixed-size fit (lssvm_mi355_problem_fit_reduced_rank_path / _reduced_leverage_prefix,
lssvm_mi355_fit_reduced_rank_path_*, MI355CSVM.fit_reduced_rank_path, svc.fit_reduced_rank_cv).  The yardstick is numpy float64
(tests/reduced_rank_path_model.py); tests/test_reduced_rank_path_host.py shows the model alone to meet the identities the call rests on.

Operator.  reduced_leverage_prefix -- k_reduced_leverage_prefix on the caller's V, shift, Z and checkpoints -- against numpy at N in {255, 777} x rank in {1, 17, 129, 300}
x k in {0, 1, 3} x slab_rows in {256, 0} x both dtypes x the three kernel functions, and once at rank 1 024 (N = 1 100, float64 rbf).  V as in
tests/test_gpu_reduced_loo.py (unit diagonal, 0.1 uniform(0, 1) below it).  The bound is that file's, derived the same way with the contraction length r_q: with
t_ik = sum_j V_kj (phi_ij - shift_j), a_ik = sum_j |V_kj| |phi_ij - shift_j| (V is lower triangular: at most k + 1 <= r_q terms for k < r_q) and E_ik = sum_j |V_kj| dPhi_ij,

    h_i^(q) = sum_{k < r_q} t_ik^2:          2 (r_q + 4) eps64 sum_{k < r_q} |t_ik| a_ik  +  2 sum_{k < r_q} |t_ik| E_ik
    f_ic^(q) = sum_{k < r_q} t_ik Z_ck:      2 (r_q + 4) eps64 sum_{k < r_q} a_ik |Z_ck|  +  sum_{k < r_q} E_ik |Z_ck|

  * t_ik is one chain of at most r_q fused multiply-adds on operands that carry the rounding of their centring (gamma_{r_q + 1} a_ik); in h its square enters twice, in f
    it meets Z_ck once; the r_q terms are summed in a fixed order of at most r_q + 4 additions (four per lane, four across the lanes, one per block before, one for the
    two column waves; |t| <= a): together below 1.5 (r_q + 4) eps64 of the sums above, 2 (r_q + 4) eps64 leaves a small factor;
  * dPhi is the element error of Phi that tests/test_gpu_reduced.py allows (its phi_error, on the same data), through |V|.
The checkpoint lists hit every edge of the kernel: 1; 15, 16, 17 (the MFMA tile); 63, 64, 65 (the column wave); 127, 128, 129 (the column block); 130, 131 (two in one
16-column tile); 299, 300 (the last, partial block; r = m with m no multiple of 16); one checkpoint; sixteen.  Garbage above the diagonal of V changes no bit.

Fit.  reduced_model.FIT_CASES, both dtypes, k in {1, 3}, two costs, both factors, with and without weights, the checkpoints (1, 16, 17, 33, 64): the model takes the
prefixes of ITS full-rank factor with the nu the device reports; h, f, loo, the decision values Phi beta - rho that the returned coefficients give at the training
points (the project's way to judge coefficients, reduced_model.fit_tolerance: beta itself moves with cond(M) times the rounding of the Gram sums, its decision values do
not) and rhos within reduced_loo_model.tolerance with that checkpoint's own cond(M_r + nu I)
and the scale max |reference| (h: at least 1, the size of 1 - h; rho = -(eta - s^T beta) / W: the size of its two terms, (|eta| + |s|^T |beta|) / W -- it is their
difference, and the rounding of a difference is relative to its terms).

Against the existing calls, the bit equalities, the report, the refusals and the surface: see the tests.

Measured on an MI355X (for the record; the assertions are the bounds above): MEASURED below."""

import functools

import numpy as np
import pytest

import pcg_model as pm
import reduced_loo_model as rlm
import reduced_model as rm
import reduced_rank_path_model as rpm
import reduced_weighted_model as rw
import test_gpu_reduced as base
import test_gpu_reduced_loo as loo_base
from plssvm_amd import backend, svc
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.model import Model

pytestmark = pytest.mark.gpu

EPS64 = rm.EPS64
KERNELS, parameter = base.KERNELS, base.parameter
OPERATOR_N, OPERATOR_K, OPERATOR_D = (255, 777), (0, 1, 3), 5
# rank -> the checkpoint lists tried at it
CHECKPOINTS = {
    1: [(1,)],
    17: [(1, 15, 16, 17)],
    129: [(1, 15, 16, 17, 63, 64, 65, 127, 128, 129)],
    300: [(1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 131, 256, 257, 299, 300), (131,)],
    1024: [(1, 128, 129, 513, 896, 1023, 1024)],
}
assert len(CHECKPOINTS[300][0]) == 16

# what one run on an MI355X gave, for the record (the assertions are the bounds of the module docstring, not these figures)
MEASURED = {
    "operator: largest error / bound over all ranks, k, checkpoints and slab sizes": {"float64": "0.10 ... 0.51 (polynomial, N = 777)", "float32": "0.06 ... 0.37", "rank 1024": 0.12},
    "full rank against fit_reduced_loo, largest difference / sum of the operators' bounds": {"h": 0.0, "f": 0.004, "loo": 0.003},
    "leave-one-out accuracy on overlapping blobs at rank 2 / 8 / 32 (greedy landmarks, C = 1)": (0.5183, 0.6583, 0.8100),
}


def operands(rank, k, seed=11):
    V, garbage, B = loo_base.operands(rank, k, seed)
    return V, garbage, np.ascontiguousarray(B.T)  # Z: k x rank


def operator_reference(kernel, X, lms, kw, r, u_h, V, Z, ranks):
    Phi = pm.kernel_matrix(kernel, X, np.asarray(X)[lms.astype(np.int64)], **kw)
    dPhi = base.phi_error(kernel, X, lms, kw, r, u_h)
    shift = Phi.mean(axis=0)
    Pc = Phi - shift[None, :]
    T, A, E = Pc @ V.T, np.abs(Pc) @ np.abs(V).T, dPhi @ np.abs(V).T  # N x m each
    out = []
    for rq in ranks:
        t, a, e, z = T[:, :rq], A[:, :rq], E[:, :rq], Z[:, :rq]
        c = 2.0 * (rq + 4) * EPS64
        h, h_bound = (t * t).sum(axis=1), c * (np.abs(t) * a).sum(axis=1) + 2.0 * (np.abs(t) * e).sum(axis=1)
        f, f_bound = (t @ z.T).T, (c * (a @ np.abs(z).T) + e @ np.abs(z).T).T
        out.append((h, h_bound, f, f_bound))
    return shift, out


def check_operator(prob, kernel, X, lms, kw, r, u_h, k, slab_sizes, lists):
    rank = len(lms)
    V, garbage, Z = operands(rank, k)
    worst = 0.0
    for ranks in lists:
        shift, ref = operator_reference(kernel, X, lms, kw, r, u_h, V, Z, ranks)
        for slab_rows in slab_sizes:
            h, f = prob.reduced_leverage_prefix(V, shift, ranks, Z if k else None, landmarks=lms, slab_rows=slab_rows)
            assert h.shape == (len(ranks), X.shape[0]) and f.shape == (len(ranks), k, X.shape[0]) and np.all(np.isfinite(h)) and np.all(np.isfinite(f))
            for q, (h_ref, h_bound, f_ref, f_bound) in enumerate(ref):
                ratio = float(np.max(np.abs(h[q] - h_ref) / h_bound))
                if k:
                    ratio = max(ratio, float(np.max(np.abs(f[q] - f_ref) / f_bound)))
                assert ratio <= 1.0, (kernel, X.shape, rank, k, slab_rows, ranks[q], ratio)
                worst = max(worst, ratio)
            h2, f2 = prob.reduced_leverage_prefix(garbage, shift, ranks, Z if k else None, landmarks=lms, slab_rows=slab_rows)
            assert np.array_equal(h, h2) and np.array_equal(f, f2), (kernel, rank, k, slab_rows)
        if len(ranks) > 1:  # a checkpoint of a list: the bits of the call with that checkpoint alone; h does not depend on k
            for q in (0, len(ranks) // 2, len(ranks) - 1):
                h1, f1 = prob.reduced_leverage_prefix(V, shift, [ranks[q]], Z if k else None, landmarks=lms, slab_rows=slab_sizes[0])
                hq, fq = prob.reduced_leverage_prefix(V, shift, ranks, Z if k else None, landmarks=lms, slab_rows=slab_sizes[0])
                assert np.array_equal(h1[0], hq[q]) and np.array_equal(f1[0], fq[q]), (kernel, rank, k, ranks[q])
    return worst


@pytest.mark.parametrize("N", OPERATOR_N)
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_operator_against_numpy(dtype, kernel, N):
    X, _ = pm.make_data(N, OPERATOR_D, pm.DATA_SEED, dtype)
    worst = 0.0
    with backend.ResidentProblem(parameter(kernel, rm.rounded_parameters(dtype, **KERNELS[kernel]), 10.0), X) as prob:
        Xy, kw_y, _, r, u_h = base.operator_setup(kernel, dtype, X, prob)
        for rank in (1, 17, 129, 300):
            if rank > N:
                continue
            lms = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
            for k in OPERATOR_K:
                worst = max(worst, check_operator(prob, kernel, Xy, lms, kw_y, r, u_h, k, (256, 0), CHECKPOINTS[rank]))
        h1 = prob.reduced_leverage_prefix(*operands(129, 1)[:1], np.zeros(129), (17, 129), operands(129, 1)[2], landmarks=pm.draw_landmarks(N, 129, pm.LANDMARK_SEED))[0]
        h3 = prob.reduced_leverage_prefix(*operands(129, 3)[:1], np.zeros(129), (17, 129), operands(129, 3)[2], landmarks=pm.draw_landmarks(N, 129, pm.LANDMARK_SEED))[0]
        assert np.array_equal(h1, h3)  # (V of `operands` depends on the rank only)
    print(f"prefix leverage operator {np.dtype(dtype).name} {kernel} N={N}: largest error / bound {worst:.3f}")


def test_operator_at_the_largest_rank():
    N, rank = 1100, rm.MAX_RANK
    X, _ = pm.make_data(N, 3, pm.DATA_SEED, np.float64)
    lms = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
    with backend.ResidentProblem(parameter("rbf", KERNELS["rbf"], 10.0), X) as prob:
        worst = check_operator(prob, "rbf", X, lms, KERNELS["rbf"], 2, EPS64, 3, (256, 0), CHECKPOINTS[1024])
    print(f"prefix leverage operator at rank {rank}: largest error / bound {worst:.3f}")


# ---------------------------------------------------------------- the fit ----------------------------------------------------------------
FIT_RANKS, FIT_COSTS, FIT_RANK = (1, 16, 17, 33, 64), (10.0, 1000.0), 64


@functools.lru_cache(maxsize=None)
def fit_case(name, dtype, k):
    p = rw.fit_case(name, dtype, k)
    for a in (p["X"], p["Y"], p["w"]):
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def stable_loo(name, dtype, k, weighted, cost, r):
    """The leave-one-out values of the fit on landmarks[:r] by the QR route (no normal equations, no nu): the yardstick of e_loo.  Once per case, shared."""
    p = fit_case(name, dtype, k)
    w = p["w"] if weighted else np.ones(p["X"].shape[0])
    out = rw.stable(p["kernel"], p["X"], p["Y"], cost, p["landmarks"][:r], w, held=p["held"], **p["kw"])[2]
    out.setflags(write=False)
    return out


def model_with(p, cost, w, nu, ranks=FIT_RANKS):
    return rpm.RankPathModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], ranks, w=w, nu=nu, held=p["held"], **p["kw"])


def shaped(report, name, s, q):
    return np.atleast_2d(report[name][s][q])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("factor", ["host", "device"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", [c[0] for c in rm.FIT_CASES])
def test_fit_against_the_model(name, dtype, k, factor, weighted):
    p = fit_case(name, dtype, k)
    N = p["X"].shape[0]
    Y = p["Y"] if k > 1 else p["Y"][0]
    w = p["w"] if weighted else None
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 3.0), p["X"]) as prob:  # (the problem's own cost plays no part)
        betas, rhos, used, report = prob.fit_reduced_rank_path(Y, FIT_RANK, FIT_RANKS, FIT_COSTS, landmarks=p["landmarks"], factor=factor, sample_weight=w)
        St = prob.landmark_gram_weighted(Y, FIT_RANK, w, landmarks=p["landmarks"]) if weighted else prob.landmark_gram(Y, FIT_RANK, landmarks=p["landmarks"])
    R, S = len(FIT_RANKS), len(FIT_COSTS)
    assert np.array_equal(used, p["landmarks"]) and np.array_equal(report["costs"], FIT_COSTS) and np.array_equal(report["ranks"], FIT_RANKS)
    assert betas.shape == ((S, R, 3, 64) if k == 3 else (S, R, 64)) and report["leverage"].shape == (S, R, N) and report["loo"].shape == ((S, R, 3, N) if k == 3 else (S, R, N))
    for s, cost in enumerate(FIT_COSTS):
        model = model_with(p, cost, w, report["jitter"][s])
        trace_nu = EPS64 * np.trace(model.M)
        assert any(abs(report["jitter"][s] / (trace_nu * 10.0 ** t) - 1.0) <= 1e-6 for t in range(7)), (report["jitter"][s], trace_nu)
        for q, r in enumerate(FIT_RANKS):
            at = model.at[q]
            e = float(np.max(np.abs(at.loo - stable_loo(name, dtype, k, weighted, cost, r))) / np.max(np.abs(stable_loo(name, dtype, k, weighted, cost, r))))
            b = np.atleast_2d(betas[s][q]) if k == 1 else betas[s][q]
            for what, got, ref in (("h", report["leverage"][s][q], at.h), ("f", shaped(report, "fitted", s, q), at.f), ("loo", shaped(report, "loo", s, q), at.loo),
                                   ("Phi betas - rhos", model.Phi @ b.T - np.atleast_1d(rhos[s][q])[None, :], at.f.T), ("rhos", np.atleast_1d(rhos[s][q]), at.rhos)):
                scale = at.rho_scale if what == "rhos" else max(float(np.max(np.abs(ref))), 1.0 if what == "h" else 0.0)
                tol = rlm.tolerance(at, e, scale)
                diff = float(np.max(np.abs(got - ref)))
                print(f"rank path {name} {np.dtype(dtype).name} k={k} {factor} w={weighted} C={cost:g} r={r} {what}: |device - model| {diff:.2e}, tolerance {tol:.2e} "
                      f"(e_loo {e:.1e}, cond eps64 {at.cond * EPS64:.1e})")
                assert diff <= tol, (name, what, s, r, diff, tol)
            assert np.all(b[:, r:] == 0.0)
            info = report["infos"][s][q]
            assert info["cost"] == cost and info["rank"] == r and info["jitter"] == report["jitter"][s] and info["max_leverage"] == report["leverage"][s][q].max()
            # cond_hint against a host factorisation of the matrix the device factored: M from the device's own Gram sums (the testing aid) and the reported nu
            hint = host_cond_hint(St, model, cost, report["jitter"][s], r)
            assert abs(info["cond_hint"] - hint) <= rlm.tolerance(at, e, hint), (info["cond_hint"], hint, at.cond_hint)
            assert 1.0 <= info["cond_hint"] <= at.cond * (1.0 + 1e-6)
            if weighted:
                zero = p["w"] == 0.0
                assert np.count_nonzero(zero) > 0 and np.all(report["leverage"][s][q][zero] == 0.0)
                assert np.array_equal(shaped(report, "loo", s, q)[:, zero], shaped(report, "fitted", s, q)[:, zero])
    check_report(p["Y"], report, w)


def host_cond_hint(St, model, cost, nu, r):
    """max / min of the squared diagonal of the leading r x r block of numpy's Cholesky factor of M + nu I, M assembled as the library assembles it from the device's
    St = Pt^T diag(w) Pt (S, s and W are its blocks) and K_mm (the model's)."""
    m = model.M.shape[0]
    S, s, W = St[:m, :m], St[m, :m], St[m, m]
    M = S - np.outer(s, s) / W + model.K_mm / cost
    d2 = np.diag(np.linalg.cholesky(0.5 * (M + M.T) + nu * np.eye(m)))[:r] ** 2
    return float(d2.max() / d2.min())


def sequential_press(y, loo, w):
    total = 0.0
    for a, b, c in zip(y.tolist(), loo.tolist(), (np.ones(y.size) if w is None else w).tolist()):
        d = a - b
        total += c * (d * d) if w is not None else d * d
    return total


def check_report(Y, report, w):
    """press, loo_errors and max_leverage as the header defines them, from the arrays of the same report, in row order."""
    Y2 = np.atleast_2d(Y).astype(np.float64)
    S, R = report["leverage"].shape[:2]
    counted = np.ones(Y2.shape[1], dtype=bool) if w is None else w > 0.0
    for s in range(S):
        for q in range(R):
            assert report["max_leverage"][s][q] == report["leverage"][s][q].max()
            loo, press, errors = shaped(report, "loo", s, q), np.atleast_1d(report["press"][s][q]), np.atleast_1d(report["loo_errors"][s][q])
            for c in range(Y2.shape[0]):
                assert press[c] == sequential_press(Y2[c], loo[c], w), (s, q, c)
                assert errors[c] == np.count_nonzero((np.sign(loo[c]) != np.sign(Y2[c])) & counted), (s, q, c)


# ---------------------------------------------------------------- against the existing calls ----------------------------------------------------------------
def operator_bounds(model, p, w, rank):
    """What the two leverage kernels may differ by at the full rank on the SAME Phi, V and z / beta (the bounds of the operators, their dPhi terms gone): of h, of f."""
    W = float(np.sum(w))
    T = model.U.T  # N x m
    A = np.abs(model.Phic) @ np.abs(model.V).T
    c = 2.0 * (rank + 4) * EPS64
    h_bound = w * (c * (np.abs(T) * A).sum(axis=1)) + 4.0 * EPS64 * w * (1.0 / W + (T * T).sum(axis=1))
    betas = model.at[-1].betas
    f_old = c * (np.abs(model.Phic) @ np.abs(betas).T).T
    f_new = c * (A @ np.abs(model.Z).T).T
    return 2.0 * h_bound, f_old + f_new + 4.0 * EPS64 * np.abs(model.at[-1].f)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("factor", ["host", "device"])
@pytest.mark.parametrize("name, dtype", [("rbf_777x5", np.float32), ("poly_777x16", np.float64)])
def test_the_full_rank_checkpoint_against_fit_reduced_loo(name, dtype, factor, weighted):
    p = fit_case(name, dtype, 3)
    N = p["X"].shape[0]
    w = p["w"] if weighted else None
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 3.0), p["X"]) as prob:
        betas, rhos, _, report = prob.fit_reduced_rank_path(p["Y"], FIT_RANK, (17, FIT_RANK), FIT_COSTS, landmarks=p["landmarks"], factor=factor, sample_weight=w)
        b0, r0, _, rep0 = prob.fit_reduced_loo(p["Y"], FIT_RANK, FIT_COSTS, landmarks=p["landmarks"], factor=factor, sample_weight=w)
    for s, cost in enumerate(FIT_COSTS):
        assert report["jitter"][s] == rep0["jitter"][s]
        if factor == "host":  # the very code of the leave-one-out call, then its back substitution on the whole factor
            assert np.array_equal(betas[s][1], b0[s]) and np.array_equal(rhos[s][1], r0[s])
        model = model_with(p, cost, w, report["jitter"][s], (17, FIT_RANK))
        ww = np.ones(N) if w is None else w
        h_bound, f_bound = operator_bounds(model, p, ww, FIT_RANK)
        dh = np.abs(report["leverage"][s][1] - rep0["leverage"][s])
        df = np.abs(report["fitted"][s][1] - rep0["fitted"][s])
        h = rep0["leverage"][s]
        loo_bound = f_bound / (1.0 - h) + np.abs(p["Y"].astype(np.float64) - rep0["fitted"][s]) * h_bound / (1.0 - h) ** 2 + 8.0 * EPS64 * np.abs(rep0["loo"][s])
        dl = np.abs(report["loo"][s][1] - rep0["loo"][s])
        keep = ww > 0.0  # (a row of weight 0 has h = 0 in both calls)
        print(f"full rank vs fit_reduced_loo {name} {factor} w={weighted} C={cost:g}: largest difference / bound of h {float(np.max(dh[keep] / h_bound[keep])):.3f}, "
              f"f {float(np.max(df / f_bound)):.3f}, loo {float(np.max(dl / loo_bound)):.3f}")
        assert np.all(dh <= h_bound) and np.all(df <= f_bound) and np.all(dl <= loo_bound)


@pytest.mark.parametrize("factor", ["host", "device"])
def test_a_prefix_against_fit_reduced_loo_on_the_first_landmarks(factor):
    """r_q < rank: the separate fit takes its own, smaller nu -- the one documented difference.  Within the tolerance plus the jitter term that
    tests/test_reduced_rank_path_host.py pins; the checkpoints whose cond(M_r) <= 1e8 are kept, and there must be some."""
    kept = 0
    for name in ("rbf_777x5", "poly_777x16"):
        p = fit_case(name, np.float64, 1)
        ranks = (7, 16, 33, 64)
        with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 3.0), p["X"]) as prob:
            _, _, _, report = prob.fit_reduced_rank_path(p["Y"][0], FIT_RANK, ranks, FIT_COSTS, landmarks=p["landmarks"], factor=factor)
            for q, r in enumerate(ranks[:-1]):
                _, _, _, rep = prob.fit_reduced_loo(p["Y"][0], r, FIT_COSTS, landmarks=p["landmarks"][:r], factor=factor)
                for s, cost in enumerate(FIT_COSTS):
                    own = rpm.from_scratch(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], r, rep["jitter"][s], held=p["held"], **p["kw"])
                    if own.cond > 1e8:
                        continue
                    kept += 1
                    assert rep["jitter"][s] <= report["jitter"][s]
                    e = float(np.max(np.abs(own.loo - stable_loo(name, np.float64, 1, False, cost, r))) / np.max(np.abs(stable_loo(name, np.float64, 1, False, cost, r))))
                    for what, got, other in (("h", report["leverage"][s][q], rep["leverage"][s]), ("f", report["fitted"][s][q], rep["fitted"][s]), ("loo", report["loo"][s][q], rep["loo"][s])):
                        scale = max(float(np.max(np.abs(other))), 1.0 if what == "h" else 0.0)
                        tol = rlm.tolerance(own, e, scale) + rpm.jitter_bound(own, report["jitter"][s], rep["jitter"][s], scale)
                        diff = float(np.max(np.abs(got - other)))
                        print(f"prefix vs separate fit {name} {factor} C={cost:g} r={r} {what}: {diff:.2e}, tolerance + jitter term {tol:.2e} (cond {own.cond:.1e})")
                        assert diff <= tol, (name, r, what, diff, tol)
    assert kept >= 4, kept


# ---------------------------------------------------------------- bit equality, the problem left as it was, refusals ----------------------------------------------------------------
ARRAYS = ("leverage", "fitted", "loo", "press", "loo_errors", "max_leverage", "cond_hint")


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and all(np.array_equal(a[3][n], b[3][n]) for n in ARRAYS + ("jitter",))


@pytest.mark.parametrize("factor", ["host", "device"])
@pytest.mark.parametrize("name, dtype", [("rbf_777x5", np.float32), ("poly_777x16", np.float64)])
def test_repeats_checkpoints_costs_columns_and_unit_weights_are_bit_equal(name, dtype, factor):
    p = fit_case(name, dtype, 3)
    ranks, costs = (1, 16, 17, 33, 64), FIT_COSTS
    kw = dict(landmarks=p["landmarks"], factor=factor)
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 5.0), p["X"]) as prob:
        for slab_rows in (0, 256):
            full = prob.fit_reduced_rank_path(p["Y"], FIT_RANK, ranks, costs, slab_rows=slab_rows, **kw)
            assert same(full, prob.fit_reduced_rank_path(p["Y"], FIT_RANK, ranks, costs, slab_rows=slab_rows, **kw))
            b3, r3, _, rep3 = full
            for q, r in enumerate(ranks):  # checkpoint q of the list: the bits of the call with [r_q] alone, at the same rank and landmarks
                b, rh, _, rep = prob.fit_reduced_rank_path(p["Y"], FIT_RANK, [r], costs, slab_rows=slab_rows, **kw)
                assert np.array_equal(b[:, 0], b3[:, q]) and np.array_equal(rh[:, 0], r3[:, q]) and np.array_equal(rep["jitter"], rep3["jitter"])
                for n in ARRAYS:
                    assert np.array_equal(rep[n][:, 0], rep3[n][:, q]), (slab_rows, r, n)
            for s, cost in enumerate(costs):  # cost s of the grid: the bits of the one-cost call
                b, rh, _, rep = prob.fit_reduced_rank_path(p["Y"], FIT_RANK, ranks, [cost], slab_rows=slab_rows, **kw)
                assert np.array_equal(b[0], b3[s]) and np.array_equal(rh[0], r3[s]) and rep["jitter"][0] == rep3["jitter"][s]
                for n in ARRAYS:
                    assert np.array_equal(rep[n][0], rep3[n][s]), (slab_rows, s, n)
            for c in range(3):  # column c of the k = 3 call: the bits of the single call; h does not depend on k
                b1, r1, _, rep1 = prob.fit_reduced_rank_path(p["Y"][c], FIT_RANK, ranks, costs, slab_rows=slab_rows, **kw)
                assert np.array_equal(rep1["leverage"], rep3["leverage"]) and np.array_equal(b3[:, :, c], b1) and np.array_equal(r3[:, :, c], r1)
                for n in ("fitted", "loo", "press", "loo_errors"):
                    assert np.array_equal(rep3[n][:, :, c], rep1[n]), (slab_rows, c, n)
        ones = prob.fit_reduced_rank_path(p["Y"], FIT_RANK, ranks, costs, sample_weight=np.ones(p["X"].shape[0]), slab_rows=256, **kw)
        assert same(ones, full)  # weights of 1.0: the bits of weights = None
    one_shot = backend.fit_reduced_rank_path(parameter(p["kernel"], p["kw"], 5.0), p["X"], p["Y"], FIT_RANK, ranks, costs, slab_rows=256, **kw)
    assert same(one_shot, full)


def test_five_right_hand_sides_take_two_launches_and_keep_their_bits():
    """The kernel takes four right-hand sides per launch: column 4 of a k = 5 call comes from the second launch and has the bits of the single call."""
    p = fit_case("rbf_777x5", np.float64, 3)
    rng = np.random.default_rng(5)
    Y = np.vstack([p["Y"], np.where(rng.random((2, 777)) < 0.5, -1.0, 1.0)])
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 5.0), p["X"]) as prob:
        for factor in ("host", "device"):
            b5, r5, _, rep5 = prob.fit_reduced_rank_path(Y, 33, (16, 33), [10.0], landmarks=p["landmarks"][:33], factor=factor)
            for c in (0, 4):
                b1, r1, _, rep1 = prob.fit_reduced_rank_path(Y[c], 33, (16, 33), [10.0], landmarks=p["landmarks"][:33], factor=factor)
                assert np.array_equal(b5[:, :, c], b1) and np.array_equal(r5[:, :, c], r1) and np.array_equal(rep5["leverage"], rep1["leverage"])
                for n in ("fitted", "loo", "press", "loo_errors"):
                    assert np.array_equal(rep5[n][:, :, c], rep1[n]), (factor, c, n)
            check_report(Y, rep5, None)


def test_the_problem_is_left_as_it_was():
    p = fit_case("rbf_777x5", np.float64, 1)
    n = p["X"].shape[0] - 1
    y = p["Y"][0]
    d = np.random.default_rng(3).standard_normal(n)

    def state(prob):
        prob.cg_begin(y, 1e-8)
        prob.cg_step(2000)
        alpha, rho, info = prob.cg_finish()
        return prob.matvec(d, np.zeros(n)), alpha, rho, info["iterations"], prob.precond_landmarks()

    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], p["cost"]), p["X"]) as prob:
        prob.build_preconditioner(landmarks=p["landmarks"][:37])
        before = state(prob)
        for factor in ("host", "device"):
            prob.fit_reduced_rank_path(p["Y"], 64, (8, 64), FIT_COSTS, factor=factor)
        prob.reduced_leverage_prefix(np.eye(16), np.zeros(16), (4, 16), slab_rows=256)
        after = state(prob)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_refusals():
    p = fit_case("rbf_777x5", np.float64, 1)
    N, y = p["X"].shape[0], p["Y"][0]
    prm = parameter(p["kernel"], p["kw"], p["cost"])
    with backend.ResidentProblem(prm, p["X"]) as prob:
        for ranks, message in (([4, 2], "strictly ascending"), ([2, 2], "strictly ascending"), ([0, 2], r"\[1, 8\]"), ([2, 9], r"\[1, 8\]"), ([], "between 1 and 16"),
                               (list(range(1, 18)), "between 1 and 16"), ([1.5], "integers")):
            with pytest.raises(InvalidParameterError, match=message):
                prob.fit_reduced_rank_path(y, 8 if len(ranks) < 17 else 32, ranks, [1.0])
        with pytest.raises(InvalidParameterError, match="at most 64"):
            prob.fit_reduced_rank_path(y, 8, [1, 2, 3, 4, 5], np.arange(1.0, 14.0))
        with pytest.raises(InvalidParameterError, match="checkpoint"):
            prob.reduced_leverage_prefix(np.eye(8), np.zeros(8), [3, 9])
        calls = (lambda: prob.fit_reduced_rank_path(y, 8, [4, 8], [1.0]), lambda: prob.reduced_leverage_prefix(np.eye(8), np.zeros(8), [8]))
        prob.set_weights(np.full(N, 2.0))
        for call in calls:
            with pytest.raises(InvalidParameterError, match="weights"):
                call()
        prob.set_weights(None)
        prob.cg_begin(y, 1e-6)
        for call in calls:
            with pytest.raises(InvalidParameterError, match="between cg_begin and cg_finish"):
                call()
        prob.cg_step(1)
        prob.cg_finish()
        for costs in ([], np.ones(65), [1.0, 0.0], [-1.0], [float("nan")]):
            with pytest.raises(InvalidParameterError, match="cost"):
                prob.fit_reduced_rank_path(y, 8, [8], costs)
        with pytest.raises(InvalidParameterError, match="distinct"):
            prob.fit_reduced_rank_path(y, 3, [3], [1.0], landmarks=[3, 7, 3])
        with pytest.raises(InvalidParameterError, match="index of a data point"):
            prob.fit_reduced_rank_path(y, 2, [2], [1.0], landmarks=[3, N])
        with pytest.raises(InvalidParameterError, match="rank of the reduced model"):
            prob.fit_reduced_rank_path(y, N + 1, [1], [1.0])
        with pytest.raises(InvalidParameterError, match="slab_rows"):
            prob.fit_reduced_rank_path(y, 8, [8], [1.0], slab_rows=100)
        with pytest.raises(InvalidParameterError, match="factor"):
            prob.fit_reduced_rank_path(y, 8, [8], [1.0], factor="gpu")
        for bad in (np.full(N, -1.0), np.zeros(N), np.full(N, np.nan)):
            with pytest.raises(InvalidParameterError, match="weight"):
                prob.fit_reduced_rank_path(y, 8, [8], [1.0], sample_weight=bad)
        _, _, used, report = prob.fit_reduced_rank_path(y, 2, [1, 2], [1.0], landmarks=[0, N - 1])  # (the handle still works)
        assert np.array_equal(used, [0, N - 1]) and np.all(np.isfinite(report["loo"]))
    with backend.ResidentProblem(prm, p["X"], devices=[0, 0]) as shard:  # two shards on the one device
        with pytest.raises(InvalidParameterError, match="one device and one rank"):
            shard.fit_reduced_rank_path(y, 8, [8], [1.0])


# ---------------------------------------------------------------- the surface ----------------------------------------------------------------
SURFACE_COSTS, SURFACE_RANKS = (0.1, 10.0), (16, 64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_csvm_rank_path_models_save_load_and_predict_like_fit_reduced_models(dtype, tmp_path):
    X, labels = rm.blobs(2000, 8, 2, seed=31, dtype=dtype)
    data = DataSet(X, labels.tolist(), real_type=dtype)
    svm = MI355CSVM(kernel_type="rbf", cost=3.0, gamma=1.0 / 8)
    models, report = svm.fit_reduced_rank_path(data, SURFACE_RANKS, SURFACE_COSTS)
    lms = rm.library_landmarks(2000, 64)
    assert len(models) == 2 and len(models[0]) == 2 and report["loo"].shape == (2, 2, 2000) and np.array_equal(report["landmarks"], lms)
    y = data.mapped_labels().astype(np.float64)
    for s, cost in enumerate(SURFACE_COSTS):
        for q, r in enumerate(SURFACE_RANKS):
            model = models[s][q]
            single = MI355CSVM(kernel_type="rbf", cost=cost, gamma=1.0 / 8)
            ref = single.fit_reduced(data, r, landmarks=lms[:r])
            assert model.params.cost == cost and model.alpha.dtype == np.dtype(dtype) and model.num_support_vectors() == r
            assert np.array_equal(model.support_vectors(), ref.support_vectors())
            if r == 64:  # the full rank on the host: the bits of fit_reduced
                assert np.array_equal(model.alpha, ref.alpha) and model.rho == ref.rho
            path = tmp_path / f"rank_path_{s}_{q}.model"
            model.save(str(path))
            loaded = Model.load(str(path), real_type=dtype, label_type=int)
            assert loaded.num_support_vectors() == r
            assert svm.predict(model, data) == svm.predict(loaded, data)
            agree = np.mean(np.asarray(svm.predict(model, data)) == np.asarray(single.predict(ref, data)))
            assert agree >= 0.999 and svm.score(model) >= 0.97  # (well-separated blobs: the jitter of the full rank moves no decision that is not a tie)
            assert report["loo_errors"][s][q] == np.count_nonzero(np.sign(report["loo"][s][q]) != y) and report["loo_accuracy"][s][q] == 1.0 - int(report["loo_errors"][s][q]) / 2000


@pytest.mark.parametrize("classes", [2, 3])
def test_svc_fit_reduced_rank_cv(classes):
    X, labels = rm.blobs(2000, 8, classes, seed=31)
    est = svc.SVC(kernel="rbf", C=3.0, gamma=1.0 / 8)
    scores, clones = svc.fit_reduced_rank_cv(est, X, labels, SURFACE_RANKS, SURFACE_COSTS, landmarks=None)
    assert est._fit is None and scores.shape == (2, 2) and [[c.C for c in row] for row in clones] == [[C, C] for C in SURFACE_COSTS]
    lms = rm.library_landmarks(2000, 64)
    Y = np.where(labels[None, :] == np.arange(classes)[:, None], 1.0, -1.0)
    if classes == 2:
        Y = Y[1:]
    for s, cost in enumerate(SURFACE_COSTS):
        model = rpm.RankPathModel("rbf", X, Y, cost, lms, SURFACE_RANKS, gamma=1.0 / 8)
        for q, r in enumerate(SURFACE_RANKS):
            at = model.at[q]
            tol = rlm.tolerance(at, 0.0, np.max(np.abs(at.loo)))
            if classes == 2:
                clear, predicted = np.abs(at.loo[0]) > tol, (at.loo[0] > 0).astype(int)
            else:
                top = np.sort(at.loo, axis=0)
                clear, predicted = top[-1] - top[-2] > 2 * tol, np.argmax(at.loo, axis=0)
            expected = float(np.mean(predicted == labels))
            print(f"fit_reduced_rank_cv {classes} classes C={cost:g} r={r}: loo accuracy {scores[s][q]:.4f} (numpy {expected:.4f}), points within the tolerance {np.count_nonzero(~clear)}")
            assert np.mean(~clear) <= 0.01 and abs(scores[s][q] - expected) * 2000 <= np.count_nonzero(~clear) + 1e-9
            clone = clones[s][q]
            assert clone.dual_coef_.shape[-1] == r and np.array_equal(clone.support_, lms[:r].astype(np.int32)) and clone.predict(X).shape == (2000,)
            assert np.mean(clone.predict(X) == labels) >= 0.97
    weighted = svc.fit_reduced_rank_cv(svc.SVC(kernel="rbf", gamma=1.0 / 8, class_weight="balanced"), X, labels, SURFACE_RANKS, [1.0], landmarks="greedy", factor="device")
    assert weighted[0].shape == (1, 2) and np.all(weighted[0] >= 0.97)


def test_the_score_rises_with_the_rank_on_overlapping_blobs():
    """Seed, gamma, cost and ranks chosen on the numpy model (reduced_rank_path_model on the greedy pivots of landmark_select_model): its leave-one-out accuracy is
    0.518 at rank 2, 0.658 at rank 8 and 0.810 at rank 32 -- 175 of 600 points between the smallest and the largest rank, no accident."""
    X, labels = rlm.overlapping_blobs(600, 4, 2, seed=41)
    ranks = (2, 8, 32)
    scores, clones = svc.fit_reduced_rank_cv(svc.SVC(kernel="rbf", gamma=0.25), X, labels, ranks, [1.0], landmarks="greedy")
    used = clones[0][-1].support_.astype(np.int64)
    Y = np.where(labels == 1, 1.0, -1.0)[None, :]
    model = rpm.RankPathModel("rbf", X, Y, 1.0, used, ranks, gamma=0.25)
    expected = [1.0 - at.loo_errors[0] / 600 for at in model.at]
    print("loo accuracy over the ranks on overlapping blobs:", scores[0], "numpy on the same landmarks:", expected)
    assert scores[0][0] + 0.2 < scores[0][-1] < 1.0
    assert np.all(np.abs(scores[0] - np.asarray(expected)) <= 2.0 / 600)
