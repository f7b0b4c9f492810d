"""GPU (-m gpu): landmark selection on a resident problem (lssvm_mi355_problem_select_landmarks, lssvm_mi355_select_landmarks_*, and landmarks="greedy" / "rpcholesky"
wherever a landmark list is accepted).  The yardstick is numpy float64: tests/landmark_select_model.py restates the algorithm (and
tests/test_landmark_select_host.py checks that restatement against the closed form), run on the data as the problem holds it (reduced_model.held_data).

(a) Pivots.  The device's pivot sequence equals the model's.  A step may differ only where the model's own margin is below 1e-9 -- greedy: the gap between the best and
    the second-best residual over d0; rpcholesky: the distance of t to the nearer prefix boundary over S -- at most 2 % of a case's steps, never step 0 of a kernel
    other than rbf; the model then continues from the device's pivot.  On the CPU the model's smallest margins over these cases (uniform [-1, 1] data, the kernel
    parameters of kernel_kw, after step 0 for greedy rbf) are 4.1e-8 for greedy (rbf 3.2e-7 polynomial, 2.0e-5 linear) and, for the seed fixed below, 1.5e-7 for
    rpcholesky (1.0e-6 polynomial, 1.4e-6 linear): no step is expected to be excused.  (rbf with gamma = 1 / d leaves gaps of 2e-10 at steps past 240 in 5
    dimensions, where the residuals themselves are below 1e-9 d0; gamma = 4 / d does not decay that far within 300 steps.)  Where the rank is exhausted (linear on
    d features after d steps, polynomial of degree 3 on 5 features after 56) what is left of d is rounding noise around the floor 64 eps64 d0, and the step at which
    the stop test fires may differ by one: that decision's margin is the distance of the pivot's d / d0 from the floor, on the model's own d, excused under the
    same 1e-9 and counted as one excused step (the one a case of exhausted rank is allowed whatever its length).
(b) Values.  residual_out and trace_out against the closed-form Nystrom residual diag(K - K[:, P] K[P, P]^-1 K[P, :]) of the DEVICE's pivots within
    8 max(e_model, cond(K_PP) eps64) d0 -- the bound form of tests/test_gpu_reduced.py; e_model is the model's own deviation from the closed form for the case.
    The trace is a sum of n such entries and is held to n times the bound (the entry bound itself lies below half an ulp of a trace of 700 d0, which no
    double can meet).  Chosen points have exactly 0, points outside the pool NaN.
(c) Edge cases: an exhausted rank, duplicated rows, pool == rank.   (d) Repeats are bit-equal, seeds move rpcholesky only, the problem is left as it was.
(e) Quality on the two data recipes where a rule wins (seed 0, both dtypes); uniform data is reported only.   (f) The surface and every refusal.

Measured on an MI355X (for the record; the assertions are the bounds above): MEASURED below."""

import ctypes as C
import functools

import numpy as np
import pytest

import landmark_select_model as lsm
import pcg_model as pm
import reduced_model as rm
from plssvm_amd import _capi, backend, svc
from plssvm_amd.csvm import MI355CSVM, make_csvm
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter

pytestmark = pytest.mark.gpu

EPS64 = lsm.EPS64
KERNELS = {"rbf": dict(gamma=0.2), "polynomial": dict(gamma=1.0 / 16, coef0=1.0, degree=3), "linear": dict(gamma=1.0)}


def kernel_kw(kernel, d):
    """The kernel parameters of (a) and (b) on d features: a kernel matrix whose residuals stay above 1e-9 d0 for 300 steps, so that the margins mean something."""
    return {"rbf": dict(gamma=4.0 / d), "polynomial": dict(gamma=1.0 / d, coef0=1.0, degree=3), "linear": dict(gamma=1.0)}[kernel]


# N: one to four row blocks of 256; features: past the pivot row's LDS chunk and past 128.  Every N meets every feature count once over the kernels and dtypes.
SHAPES = [(255, 5), (255, 33), (257, 16), (257, 130), (777, 5), (777, 16), (777, 33), (777, 130)]
RANKS = (1, 2, 17, 64, 65, 300)
SEED = 4  # rpcholesky's seed for (a) and (b)
MARGIN, EXCUSED_SHARE = 1e-9, 0.02

# what one run on an MI355X gave, for the record (the assertions are the bounds of the module docstring, not these figures)
MEASURED = {
    "pivots": "no pivot step excused in any case; float32 polynomial 255 x 5 (exact rank 56): the device's stop test fired one step after the model's (57 against 56)",
    "|d - closed form| / entry bound, largest over the float64 cases": "2.7e-15 / 3.3e-14 (257 x 16 rbf, rank 65); rank 300: 1.5e-14 / 1.6e-10",
    "|trace - closed form|, largest over the float64 cases": "9.5e-13 (777 x 16 polynomial, rank 300, n x bound 2.7e-7)",
    "quality (trace ratio to the fixed shuffle | PCG iterations selected / fixed)": {
        "clusters float64": "0.41 | 49 / 86", "clusters float32": "0.41 | 23 / 40", "heavy_rows float64": "0.27 | 36 / 44", "heavy_rows float32": "0.27 | 36 / 43"},
    "uniform 777 x 5 rbf rank 64 (trace | iterations)": {"fixed shuffle": "6.68 | 25", "greedy": "5.90 | 22", "rpcholesky": "5.65 | 24"},
}


def parameter(kernel, kw, cost=100.0):
    return Parameter(kernel_type=kernel, cost=cost, gamma=kw.get("gamma"), coef0=kw.get("coef0", 0.0), degree=kw.get("degree", 3))


def held(kernel, dtype, X, prob):
    """(the data the model is run on, the kernel parameters on it): the data as this problem holds it."""
    kw = rm.rounded_parameters(dtype, **kernel_kw(kernel, X.shape[1]))
    if np.dtype(dtype) == np.float32:
        return rm.held_data(kernel, X, direct=bool(prob.info()["rbf_direct"]), **kw)
    return X, kw


def follow(prob, model_args, rank, method, pool, seed, kernel):
    """One device call compared step by step with the model: ``(device results, the model after the device's pivots, excused steps)``."""
    lmk, trace, residual, info = prob.select_landmarks(rank, method=method, pool=pool, seed=seed)
    sel = lsm.Selection(*model_args[0], method, pool=pool, seed=seed, **model_args[1])
    position = {int(point): i for i, point in enumerate(sel.cand.tolist())}
    excused = []
    floor_rel = 64.0 * EPS64  # (tol = 0)
    for j in range(rank):
        p, margin = sel.propose()
        dev = position[int(lmk[j])] if j < len(lmk) else None
        if p is None or dev is None:
            if p is None and dev is None:
                break
            # the stop test fired on one side only: the margin of that decision is the distance of the pivot's d / d0 from the floor, on the model's own d
            at_stop = abs(float(sel.d[dev if p is None else p]) / sel.d0 - floor_rel)
            assert at_stop < MARGIN and j > 0, (method, pool, rank, j, p, dev, at_stop)
            excused.append(j)
            if p is None:  # the model has nothing left to divide by: the device may take this one step of noise, then it stops too
                assert len(lmk) == j + 1, (method, pool, rank, j, len(lmk))
            break
        elif dev != p:
            assert margin < MARGIN and (j > 0 or kernel == "rbf"), (method, pool, rank, j, p, dev, margin)
            excused.append(j)
        sel.apply(dev)
    assert len(lmk) == info["rank_found"] and sel.rank_found in (len(lmk), len(lmk) - 1 if excused else len(lmk)), (method, pool, rank, len(lmk), sel.rank_found)
    assert len(excused) <= max(EXCUSED_SHARE * rank, 1 if sel.rank_found < rank else 0), (method, pool, rank, excused)
    return (lmk, trace, residual, info), sel, excused


def check_values(kernel, Xh, kwh, N, dev, sel, steps=()):
    """(b) for one call: the final d and the trace at ``steps`` and at the end against the closed form of the device's pivots."""
    lmk, trace, residual, info = dev
    closed, cond = lsm.nystrom_residual(kernel, Xh, sel.cand, lmk, **kwh)
    closed_model, _ = lsm.nystrom_residual(kernel, Xh, sel.cand, sel.landmarks, **kwh)
    e_model = float(np.max(np.abs(sel.d - closed_model)) / sel.d0)
    bound = 8.0 * max(e_model, cond * EPS64) * sel.d0
    err = float(np.max(np.abs(residual[sel.cand] - closed)))
    assert err <= bound, (err, bound)
    outside = np.setdiff1d(np.arange(N), sel.cand)
    assert np.all(np.isnan(residual[outside])) and np.count_nonzero(np.isnan(residual)) == outside.size
    assert np.all(residual[lmk.astype(np.int64)] == 0.0) and np.all(residual[sel.cand] >= 0.0)
    assert np.all(np.diff(np.concatenate([[info["trace0"]], trace])) <= 0.0) and info["trace"] == trace[-1]
    worst = abs(trace[-1] - np.maximum(closed, 0.0).sum())
    assert worst <= sel.n * bound, (worst, sel.n * bound)  # (the trace is the sum of n entries, each within the bound)
    for j in steps:
        at_j, cond_j = lsm.nystrom_residual(kernel, Xh, sel.cand, lmk[:j + 1], **kwh)
        assert abs(trace[j] - np.maximum(at_j, 0.0).sum()) <= sel.n * 8.0 * max(e_model, cond_j * EPS64) * sel.d0, (j,)
    assert info["max_residual"] == residual[sel.cand].max() and info["candidates"] == sel.n
    return err, worst, bound


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pivots_and_values_against_the_model(dtype, kernel, shape):
    N, d = shape
    X, _ = pm.make_data(N, d, pm.DATA_SEED, dtype)
    ranks = [r for r in RANKS if r <= N] + ([N] if N == 255 and kernel == "rbf" else [])
    top = max(ranks)
    report = []
    with backend.ResidentProblem(parameter(kernel, rm.rounded_parameters(dtype, **kernel_kw(kernel, d))), X) as prob:
        Xh, kwh = held(kernel, dtype, X, prob)
        args = ((kernel, Xh), kwh)
        for method in lsm.METHODS:
            pools = [0] + ([300] if N >= 300 else [])
            for pool in pools:
                # every smaller rank is a prefix of the largest one: compared in full once, then as prefixes
                full_rank = min(top, pool) if pool else top
                dev, sel, excused = follow(prob, args, full_rank, method, pool, SEED, kernel)
                err, worst, bound = check_values(kernel, Xh, kwh, N, dev, sel, steps=(0, full_rank // 2))
                report.append(f"{method} pool {pool} rank {full_rank}: found {dev[3]['rank_found']}, excused {excused}, |d - closed| {err:.1e}, |trace - closed| {worst:.1e}, bound {bound:.1e}")
                for rank in ranks:
                    if rank < full_rank:
                        lmk, trace, _, info = prob.select_landmarks(rank, method=method, pool=pool, seed=SEED)
                        found = min(rank, len(dev[0]))
                        assert np.array_equal(lmk, dev[0][:found]) and np.array_equal(trace[:found], dev[1][:found]), (method, pool, rank)
            for rank in ranks:  # pool == rank: every candidate is chosen
                if rank in (17, 65):
                    dev, sel, excused = follow(prob, args, rank, method, rank, SEED, kernel)
                    if dev[3]["rank_found"] == rank:
                        assert sorted(dev[0].tolist()) == sorted(rm.library_landmarks(N, rank).tolist())
    print(f"select {np.dtype(dtype).name} {kernel} {N}x{d}:\n  " + "\n  ".join(report))


# ---------------------------------------------------------------- (c) edge cases ----------------------------------------------------------------
@pytest.mark.parametrize("method", lsm.METHODS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_an_exhausted_rank_stops_the_selection(dtype, method):
    X, _ = pm.make_data(255, 5, pm.DATA_SEED, dtype)
    with backend.ResidentProblem(parameter("linear", KERNELS["linear"]), X) as prob:
        lmk, trace, residual, info = prob.select_landmarks(17, method=method, seed=2)
        raw = np.zeros(17, dtype=np.uint64)
        _capi.check(_capi.select_entry("lssvm_mi355_problem_select_landmarks")(prob._h, 17, _capi.LANDMARK_METHODS[method], 0, 2, 0.0, raw.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, None))
    assert info["rank_found"] == 5 and len(lmk) == 5 and len(set(lmk.tolist())) == 5
    assert np.array_equal(raw[:5], lmk) and np.all(raw[5:] == np.uint64(2 ** 64 - 1))  # (UINT64_MAX from rank_found on; NULL trace / residual / info are allowed)
    assert np.all(trace[5:] == trace[4]) and info["trace"] == trace[4]
    d0 = float((X.astype(np.float64) ** 2).sum(axis=1).max())
    assert info["max_residual"] <= 64 * EPS64 * d0 * 64 and np.all(residual[lmk.astype(np.int64)] == 0.0)


@pytest.mark.parametrize("method", lsm.METHODS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_no_duplicate_of_a_chosen_point_is_chosen(dtype, method):
    X, _ = pm.make_data(300, 5, pm.DATA_SEED, dtype)
    X[200:] = X[:100]
    with backend.ResidentProblem(parameter("rbf", KERNELS["rbf"]), X) as prob:
        lmk, _, residual, info = prob.select_landmarks(150, method=method, seed=5)
    rows = lmk.astype(np.int64)
    originals = np.where(rows >= 200, rows - 200, rows)
    assert info["rank_found"] == 150 and np.unique(originals).size == rows.size
    twins = np.where(rows >= 200, rows - 200, np.where(rows < 100, rows + 200, rows))
    assert np.all(residual[twins] <= 64 * EPS64)  # (the duplicate of a chosen point has no residual left)


# ---------------------------------------------------------------- (d) repeatability ----------------------------------------------------------------
@pytest.mark.parametrize("dtype, kernel", [(np.float64, "rbf"), (np.float32, "polynomial")])
def test_repeats_seeds_and_the_problem_left_as_it_was(dtype, kernel):
    N = 777
    X, y = pm.make_data(N, 16, pm.DATA_SEED, dtype)
    prm = parameter(kernel, KERNELS[kernel])
    v = np.random.default_rng(3).standard_normal(N - 1).astype(dtype)
    with backend.ResidentProblem(prm, X) as prob:
        prob.build_preconditioner(37)
        own = prob.precond_landmarks()
        z0, mv0 = prob.precond_apply(v), prob.matvec(v, np.zeros(N - 1, dtype))
        runs = {(m, s): prob.select_landmarks(64, method=m, seed=s, pool=300) for m in lsm.METHODS for s in (0, 0, 1)}
        for m in lsm.METHODS:
            again = prob.select_landmarks(64, method=m, seed=0, pool=300)
            for a, b in zip(runs[(m, 0)][:3], again[:3]):
                assert np.array_equal(a, b, equal_nan=True)
            assert {k: v_ for k, v_ in runs[(m, 0)][3].items() if k != "select_ms"} == {k: v_ for k, v_ in again[3].items() if k != "select_ms"}
        assert not np.array_equal(runs[("rpcholesky", 0)][0], runs[("rpcholesky", 1)][0])
        for a, b in zip(runs[("greedy", 0)][:3], runs[("greedy", 1)][:3]):
            assert np.array_equal(a, b, equal_nan=True)
        assert np.array_equal(prob.precond_landmarks(), own)  # the preconditioner is kept
        assert np.array_equal(prob.precond_apply(v), z0) and np.array_equal(prob.matvec(v, np.zeros(N - 1, dtype)), mv0)
        resident = prob.select_landmarks(64, method="rpcholesky", seed=7)
    one_shot = backend.select_landmarks(prm, X, 64, method="rpcholesky", seed=7)  # the one-shot entry point: the bits of the resident path
    for a, b in zip(resident[:3], one_shot[:3]):
        assert np.array_equal(a, b, equal_nan=True)


# ---------------------------------------------------------------- (e) quality ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recipe_reference(recipe):
    """(X float64, y, dense Abar, b): float64 numpy, once per recipe, shared, never modified."""
    make, kernel, kw, rank, winner, factor = lsm.RECIPES[recipe]
    X, y = make(0)
    A = pm.reduced_matrix(kernel, X, lsm.RECIPE_COST, **kw)
    b = pm.reduced_rhs(y)
    for a in (X, y, A, b):
        a.setflags(write=False)
    return X, y, A, b


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("recipe", list(lsm.RECIPES))
def test_the_winning_rule_beats_the_fixed_shuffle(recipe, dtype):
    make, kernel, kw, rank, winner, factor = lsm.RECIPES[recipe]
    X64, y64, A, b = recipe_reference(recipe)
    X, y = X64.astype(dtype), y64.astype(dtype)
    eps = pm.GPU_EPS[np.dtype(dtype)]
    A_t = A if np.dtype(dtype) == np.float64 else pm.reduced_matrix(kernel, X, lsm.RECIPE_COST, **kw)  # (the system of the data as rounded to the dtype)
    with backend.ResidentProblem(parameter(kernel, kw, lsm.RECIPE_COST), X) as prob:
        lmk, _, _, info = prob.select_landmarks(rank, method=winner, seed=0)
        prob.build_preconditioner(rank)
        fixed_lm = prob.precond_landmarks()
        _, _, fixed = prob.solve_pcg(y, eps, 5000)
        prob.build_preconditioner(landmarks=lmk)
        alpha, _, selected = prob.solve_pcg(y, eps, 5000)
    trace_selected, trace_fixed = lsm.nystrom_trace(kernel, X, lmk, **kw), lsm.nystrom_trace(kernel, X, fixed_lm, **kw)
    res = pm.true_residual(A_t, b, alpha[:-1])
    print(f"quality {recipe} {np.dtype(dtype).name}: {winner} trace {trace_selected:.4g} against {trace_fixed:.4g} ({trace_selected / trace_fixed:.2f}), "
          f"PCG iterations {selected['iterations']} against {fixed['iterations']}, true residual / eps {res / eps:.3f}")
    assert info["rank_found"] == rank and trace_selected <= factor * trace_fixed
    assert selected["converged"] == 1 and fixed["converged"] == 1 and res <= 2.0 * eps
    assert selected["iterations"] <= fixed["iterations"]


def test_uniform_data_is_a_tie_reported_only():
    X, y = pm.make_data(777, 5, pm.DATA_SEED)
    kw = KERNELS["rbf"]
    rows = []
    with backend.ResidentProblem(parameter("rbf", kw), X) as prob:
        for rule in (None,) + lsm.METHODS:
            prob.build_preconditioner(64, landmarks=rule)
            _, _, info = prob.solve_pcg(y, 1e-8, 5000)
            rows.append(f"{rule or 'fixed shuffle'}: trace {lsm.nystrom_trace('rbf', X, prob.precond_landmarks(), **kw):.4g}, {info['iterations']} iterations")
            assert info["converged"] == 1
    print("uniform 777x5 rbf rank 64 -- " + "; ".join(rows))


# ---------------------------------------------------------------- (f) the surface ----------------------------------------------------------------
def same(a, b):
    if isinstance(a, dict):
        return all(same(a[k], b[k]) for k in a if k not in ("infos", "landmark_ms", "gram_ms", "host_ms", "total_ms", "build_ms", "apply_ms", "leverage_ms"))
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, z) for x, z in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("method", lsm.METHODS)
def test_a_rule_name_gives_the_bits_of_its_indices(method):
    N, rank = 300, 37
    X, y = pm.make_data(N, 16, pm.DATA_SEED, np.float64)
    kw = KERNELS["polynomial"]
    prm = parameter("polynomial", kw, 10.0)
    Y = np.stack([y, -y])
    costs = [1.0, 10.0]
    lmk = backend.select_landmarks(prm, X, rank, method=method)[0]
    assert len(lmk) == rank
    with backend.ResidentProblem(prm, X) as prob:
        assert np.array_equal(prob.select_landmarks(rank, method=method)[0], lmk)
        prob.build_preconditioner(rank, landmarks=method)
        assert np.array_equal(prob.precond_landmarks(), lmk)
        by_name = prob.solve_pcg(y, 1e-8, 2000)
        prob.build_preconditioner(landmarks=lmk)
        assert same(by_name[:2], prob.solve_pcg(y, 1e-8, 2000)[:2])
        assert same(prob.fit_reduced(Y, rank, landmarks=method)[:3], prob.fit_reduced(Y, rank, landmarks=lmk)[:3])
        a, b = prob.fit_reduced_loo(y, rank, costs, landmarks=method), prob.fit_reduced_loo(y, rank, costs, landmarks=lmk)
        assert same(a[:3], b[:3]) and same(a[3], b[3])
    a, b = backend.solve_pcg(prm, X, y, 1e-8, 2000, rank=rank, landmarks=method), backend.solve_pcg(prm, X, y, 1e-8, 2000, landmarks=lmk)
    assert same(a[:2], b[:2]) and a[2]["iterations"] == b[2]["iterations"] and a[2]["rank"] == rank
    assert same(backend.fit_reduced(prm, X, Y, rank, landmarks=method)[:3], backend.fit_reduced(prm, X, Y, rank, landmarks=lmk)[:3])
    a, b = backend.fit_reduced_loo(prm, X, y, rank, costs, landmarks=method), backend.fit_reduced_loo(prm, X, y, rank, costs, landmarks=lmk)
    assert same(a[:3], b[:3]) and same(a[3], b[3])
    # the backend object and the estimator
    data = DataSet(X, [int(v) for v in y])
    named = make_csvm("mi355", solver="pcg", precond_rank=rank, precond_landmarks=method, kernel_type="polynomial", cost=10.0, gamma=kw["gamma"], coef0=kw["coef0"])
    model = named.fit(data, epsilon=1e-8)
    assert named.last_cg_info["rank"] == rank and named.last_cg_info["converged"] == 1
    assert np.array_equal(model.alpha, backend.solve_pcg(prm, X, data.mapped_labels().astype(np.float64), 1e-8, 5000, landmarks=lmk)[0])
    svm = MI355CSVM(kernel_type="polynomial", cost=10.0, gamma=kw["gamma"], coef0=kw["coef0"])
    m_name, m_idx = svm.fit_reduced(data, rank, landmarks=method), svm.fit_reduced(data, rank, landmarks=lmk)
    assert np.array_equal(svm.last_cg_info["landmarks"], lmk) and np.array_equal(m_name.alpha, m_idx.alpha) and m_name.rho == m_idx.rho
    p_name, p_idx = svm.fit_reduced_path(data, rank, costs, landmarks=method), svm.fit_reduced_path(data, rank, costs, landmarks=lmk)
    assert np.array_equal(p_name[1]["landmarks"], lmk) and all(np.array_equal(u.alpha, w.alpha) for u, w in zip(p_name[0], p_idx[0]))
    est = svc.SVC(kernel="poly", C=10.0, gamma=kw["gamma"], coef0=kw["coef0"], degree=3, real_type=np.float64)
    labels = (y > 0).astype(int)
    c_name, c_idx = svc.fit_reduced(est, X, labels, rank, landmarks=method), svc.fit_reduced(est, X, labels, rank, landmarks=lmk)
    assert np.array_equal(c_name.support_, lmk.astype(np.int32)) and np.array_equal(c_name.dual_coef_, c_idx.dual_coef_) and np.array_equal(c_name.intercept_, c_idx.intercept_)
    s_name, s_idx = svc.fit_reduced_cv(est, X, labels, rank, costs, landmarks=method), svc.fit_reduced_cv(est, X, labels, rank, costs, landmarks=lmk)
    assert np.array_equal(s_name[0], s_idx[0]) and np.array_equal(s_name[1][0].support_, lmk.astype(np.int32))
    three = np.arange(N) % 3
    t_name, t_idx = svc.fit_reduced(est, X, three, rank, landmarks=method), svc.fit_reduced(est, X, three, rank, landmarks=lmk)
    assert np.array_equal(t_name.support_, t_idx.support_) and np.array_equal(t_name.dual_coef_, t_idx.dual_coef_)


def test_a_smaller_rank_found_propagates_and_a_missing_class_raises():
    X, y = pm.make_data(255, 5, pm.DATA_SEED, np.float64)
    prm = parameter("linear", KERNELS["linear"], 10.0)
    with backend.ResidentProblem(prm, X) as prob:
        built = prob.build_preconditioner(17, landmarks="greedy")
        assert built["rank"] == 5 and len(prob.precond_landmarks()) == 5
        _, _, info = prob.solve_pcg(y, 1e-8, 100)
        assert info["rank"] == 5 and info["converged"] == 1
        betas, _, used, rinfo = prob.fit_reduced(y, 17, landmarks="rpcholesky")
        assert betas.shape == (5,) and len(used) == 5 and rinfo["rank"] == 5
    svm = make_csvm("mi355", solver="pcg", precond_rank=17, precond_landmarks="greedy", kernel_type="linear", cost=10.0)
    svm.fit(DataSet(X, [int(v) for v in y]), epsilon=1e-8)
    assert svm.last_cg_info["rank"] == 5
    # two classes, the selected landmarks all of one: the existing error of the two-class model file
    rng = np.random.default_rng(1)
    Xc = np.vstack([rng.normal(0.0, 1.0, (250, 4)), 1e-3 * rng.normal(0.0, 1.0, (50, 4)) + 8.0])
    labels = [0] * 250 + [1] * 50
    lmk = backend.select_landmarks(parameter("rbf", dict(gamma=0.5), 10.0), Xc, 1, method="greedy")[0]
    assert lmk.tolist() == [0]
    with pytest.raises(InvalidParameterError, match="hold no point of the class"):
        MI355CSVM(kernel_type="rbf", cost=10.0, gamma=0.5).fit_reduced(DataSet(Xc, labels), 1, landmarks="greedy")


def test_every_refusal():
    N = 300
    X, y = pm.make_data(N, 5, pm.DATA_SEED, np.float64)
    prm = parameter("rbf", KERNELS["rbf"])
    fn = _capi.select_entry("lssvm_mi355_problem_select_landmarks")
    out = np.zeros(8, dtype=np.uint64)
    out_p = out.ctypes.data_as(C.POINTER(C.c_uint64))
    with backend.ResidentProblem(prm, X) as prob:
        for rank, pool in ((0, 0), (N + 1, 0), (1025, 0), (65, 64)):
            with pytest.raises(InvalidParameterError, match="landmarks to select|candidate pool"):
                prob.select_landmarks(rank, pool=pool)
        for rank, pool, match in ((8, 4, "candidate pool"), (8, N + 1, "candidate pool"), (0, 0, "landmarks to select"), (N + 1, 0, "landmarks to select"), (1025, 0, "landmarks to select")):
            with pytest.raises(InvalidParameterError, match=match):  # ... and by the library itself
                _capi.check(fn(prob._h, rank, 1, pool, 0, 0.0, out_p, None, None, None))
        with pytest.raises(InvalidParameterError, match="landmark rule"):
            prob.select_landmarks(8, method="random")
        with pytest.raises(InvalidParameterError, match="landmark rule"):
            _capi.check(fn(prob._h, 8, 3, 0, 0, 0.0, out_p, None, None, None))
        for tol in (-1e-3, float("nan"), float("inf")):
            with pytest.raises(InvalidParameterError, match="tolerance"):
                prob.select_landmarks(8, tol=tol)
            with pytest.raises(InvalidParameterError, match="tolerance"):
                _capi.check(fn(prob._h, 8, 1, 0, 0, tol, out_p, None, None, None))
        with pytest.raises(InvalidParameterError, match="landmarks_out"):
            _capi.check(fn(prob._h, 8, 1, 0, 0, 0.0, None, None, None, None))
        with pytest.raises(InvalidParameterError, match="handle"):
            _capi.check(fn(None, 8, 1, 0, 0, 0.0, out_p, None, None, None))
        prob.set_weights(np.full(N, 2.0))
        with pytest.raises(InvalidParameterError, match="weights"):
            prob.select_landmarks(8)
        prob.set_weights(None)
        prob.cg_begin(y, 1e-6)
        with pytest.raises(InvalidParameterError, match="between cg_begin and cg_finish"):
            prob.select_landmarks(8)
        prob.cg_step(1)
        prob.cg_finish()
        assert len(prob.select_landmarks(8, tol=0.5)[0]) <= 8  # (a large tolerance stops early; the handle works on)
    with backend.ResidentProblem(prm, X, devices=[0, 0]) as shard:  # two shards on the one device
        with pytest.raises(InvalidParameterError, match="one device and one rank"):
            shard.select_landmarks(8)
        with pytest.raises(InvalidParameterError, match="one device and one rank"):
            shard.build_preconditioner(8, landmarks="greedy")
    with pytest.raises(InvalidParameterError, match="precond_landmarks"):
        MI355CSVM(solver="pcg", precond_landmarks="random")
    for bad in (lambda: backend.select_landmarks(prm, X, 8, method="greedy", pool=4), lambda: backend.select_landmarks(prm, X, 0), lambda: backend.select_landmarks(prm, X, 8, tol=-1.0)):
        with pytest.raises(InvalidParameterError):
            bad()
