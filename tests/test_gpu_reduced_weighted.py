"""GPU (-m gpu): the weighted fixed-size LS-SVM and its exact leave-one-out scores (lssvm_mi355_problem_fit_reduced_weighted / _fit_reduced_loo_weighted /
_landmark_gram_weighted and their one-shot forms, MI355CSVM.fit_reduced(sample_weight=), svc.fit_reduced_weighted / fit_reduced_cv_weighted).  The
yardstick is numpy float64 (tests/reduced_weighted_model.py); tests/test_reduced_weighted_host.py shows every input to meet the conditions the bounds below rest on.
Weights: exp(N(0, 1)), about 5 % exact zeros, a few large powers of two.

1. Operator.  landmark_gram_weighted against numpy's Pw^T Pw, Pw = diag(q) Pt, at N in {255, 257, 777} x rank in {1, 15, 16, 17, 64, 65, 130, 300} x k in {1, 3} x slab_rows
   in {256, 0} x both dtypes x the three kernel functions (from rank 130 on there are off-diagonal tiles, where BOTH staged operands are scaled), once at rank 1 024
   (N = 1 100, d = 3) and once at N = 2 305 (two row ranges of 2 048 in one slab: q is indexed past the first).  The bound is that of tests/test_gpu_reduced.py with Pw
   in place of Pt and dPw = q dPt + 2 eps64 |Pw|: the second term covers the rounding of the square root and of the product q_i * p_ij, u each, doubled as the first term
   of that bound is.  Symmetric to the bit.
2. All weights 1.0: every output has the bits of the unweighted entry point, both factors (q = 1, W = N, every product exact).
3. All weights 4.0: the bits of the unweighted call on a problem created with the cost 4 C, press four times the unweighted value (q = 2: powers of two commute with every
   rounding).
4. Fit against the model: decision values at 200 held-out points within 8 max(e_model, cond(M) eps64) max |f| (reduced_model.fit_tolerance on the weighted model).
5. Every point a landmark (weights clipped to >= 0.01): against the weighted dense full solution under the same rule.
6. Integer weights in {0, 1, 2, 3}: against the UNWEIGHTED fit_reduced on the duplicated / removed rows, within the fit tolerance.
7. Leave-one-out: h, f, loo against the weighted model within reduced_loo_model.tolerance, loo against brute-force refits; rows of weight 0 have h == 0.0 and
   loo == fitted to the bit; bit equality across repeats, columns and costs.
8. The surface, and the problem left as it was.

Measured on an MI355X (for the record; the assertions are the bounds above): MEASURED below."""

import functools

import numpy as np
import pytest

import pcg_model as pm
import reduced_loo_model as lm
import reduced_model as rm
import reduced_weighted_model as wm
import test_gpu_reduced as base
from plssvm_amd import backend, svc
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.model import Model

pytestmark = pytest.mark.gpu

EPS64 = rm.EPS64
KERNELS, parameter = base.KERNELS, base.parameter
OPERATOR_N, OPERATOR_RANKS, OPERATOR_D = (255, 257, 777), (1, 15, 16, 17, 64, 65, 130, 300), 5
FACTORS = ("host", "device")

# what one run on an MI355X gave, for the record (the assertions are the bounds of the module docstring, not these figures)
MEASURED = {
    "operator: largest error / bound over all ranks, k and slab sizes": {"float64": (0.009, 0.017), "float32": (0.010, 0.015), "rank 1024": 0.010, "N = 2305": 0.003},
    "fit: (|f_device - f_model|, tolerance), the same on both factors": {
        "rbf_777x5 float64 k=1": (2.3e-07, 9.4e-07), "rbf_777x5 float64 k=3": (2.4e-07, 1.5e-06), "rbf_777x5 float32 k=1": (3.1e-07, 8.9e-07), "rbf_777x5 float32 k=3": (3.1e-07, 1.1e-06),
        "poly_777x16 float64 k=1": (8.9e-11, 2.4e-10), "poly_777x16 float64 k=3": (1.2e-10, 2.9e-10), "poly_777x16 float32 k=1": (1.2e-10, 2.9e-10), "poly_777x16 float32 k=3": (1.7e-10, 3.2e-10)},
    "all landmarks: (|f_device - f_full|, tolerance)": {"float64": (2.0e-08, 1.3e-04), "float32": (3.0e-08, 1.3e-04)},
    "duplication float64: (|weighted - duplicated|, tolerance)": (2.6e-12, 5.6e-11),
    "duplication float32: |weighted - duplicated| (not asserted: the two problems hold differently centred data)": 1.2e-07,
    "loo, k = 3: (|device - model|, tolerance) of h, f, loo": {
        "rank 16 C = 1000 float32": ((2.5e-13, 2.7e-11), (1.5e-12, 5.8e-11), (1.6e-12, 6.5e-11)),
        "rank 130 C = 1000 float64, largest leverage 0.986": ((2.7e-07, 2.5e-04), (4.1e-06, 8.4e-04), (7.6e-06, 1.1e-03))},
    "weights of 1.0 and of 4.0": "bit equal on both factors, as derived",
}


# ---------------------------------------------------------------- 1. the operator ----------------------------------------------------------------
def operator_bound(kernel, X, Y, lms, w, kw, r, u_h):
    P = rm.augmented(kernel, X, Y, lms, **kw)
    dP = np.zeros_like(P)
    dP[:, :len(lms)] = base.phi_error(kernel, X, lms, kw, r, u_h)
    q = np.sqrt(w)[:, None]
    Pw = q * P
    absPw = np.abs(Pw)
    dPw = q * dP + 2.0 * EPS64 * absPw
    return Pw.T @ Pw, 2.0 * P.shape[0] * EPS64 * (absPw.T @ absPw) + dPw.T @ absPw + absPw.T @ dPw


def check_gram(prob, kernel, X, Y, lms, w, kw, r, u_h, slab_sizes):
    rank, k = len(lms), Y.shape[0]
    ref, bound = operator_bound(kernel, X, Y, lms, w, kw, r, u_h)
    worst = 0.0
    for slab_rows in slab_sizes:
        G = prob.landmark_gram_weighted(Y, rank, w, landmarks=lms, slab_rows=slab_rows)
        assert G.shape == (rank + 1 + k, rank + 1 + k) and np.all(np.isfinite(G))
        assert np.array_equal(G, G.T), (rank, k, slab_rows)
        ratio = float(np.max(np.abs(G - ref) / bound))
        assert ratio <= 1.0, (kernel, X.shape, rank, k, slab_rows, ratio)
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("N", OPERATOR_N)
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_operator_against_numpy(dtype, kernel, N):
    X, y = pm.make_data(N, OPERATOR_D, pm.DATA_SEED, dtype)
    rng = np.random.default_rng(7)
    Y3 = np.stack([y, np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(dtype), np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(dtype)])
    w = wm.make_weights(N)
    worst = 0.0
    with backend.ResidentProblem(parameter(kernel, rm.rounded_parameters(dtype, **KERNELS[kernel]), 10.0), X) as prob:
        Xy, kw_y, _, r, u_h = base.operator_setup(kernel, dtype, X, prob)
        for rank in OPERATOR_RANKS:
            if rank > N:
                continue
            lms = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
            for k in (1, 3):
                worst = max(worst, check_gram(prob, kernel, Xy, Y3[:k], lms, w, kw_y, r, u_h, (256, 0)))
    print(f"weighted operator {np.dtype(dtype).name} {kernel} N={N}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("N, rank", [(1100, rm.MAX_RANK), (2305, 17)])
def test_operator_at_the_largest_rank_and_past_one_row_range(N, rank):
    X, y = pm.make_data(N, 3, pm.DATA_SEED, np.float64)
    lms = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
    w = wm.make_weights(N)
    assert np.count_nonzero(w[2048:]) > 0 or N < 2048
    with backend.ResidentProblem(parameter("rbf", KERNELS["rbf"], 10.0), X) as prob:
        worst = check_gram(prob, "rbf", X, y[None, :], lms, w, KERNELS["rbf"], 2, EPS64, (256, 0))
    print(f"weighted operator at N={N}, rank {rank}: largest error / bound {worst:.3f}")


# ---------------------------------------------------------------- 2., 3. weights that must not move a bit ----------------------------------------------------------------
def same_bits(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


LOO_KEYS = ("leverage", "fitted", "loo", "loo_errors", "max_leverage", "jitter")


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("name, dtype, rank", [("rbf_777x5", np.float32, 64), ("poly_777x16", np.float64, 130)])
def test_unit_weights_have_the_bits_of_the_unweighted_entry_points(name, dtype, rank, factor):
    p = rm.fit_case(name, dtype, 3)
    N = p["X"].shape[0]
    ones, costs = np.ones(N), [p["cost"], 100.0 * p["cost"]]
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], p["cost"]), p["X"]) as prob:
        for slab_rows in (0, 256):
            assert np.array_equal(prob.landmark_gram_weighted(p["Y"], rank, ones, slab_rows=slab_rows), prob.landmark_gram(p["Y"], rank, slab_rows=slab_rows))
            assert np.array_equal(prob.landmark_gram_weighted(p["Y"], rank, None, slab_rows=slab_rows), prob.landmark_gram(p["Y"], rank, slab_rows=slab_rows))  # (NULL)
            a = prob.fit_reduced(p["Y"], rank, slab_rows=slab_rows, factor=factor, sample_weight=ones)
            b = prob.fit_reduced(p["Y"], rank, slab_rows=slab_rows, factor=factor)
            assert same_bits(a[:3], b[:3]) and a[3]["jitter"] == b[3]["jitter"], (slab_rows, factor)
            a = prob.fit_reduced_loo(p["Y"], rank, costs, slab_rows=slab_rows, factor=factor, sample_weight=ones)
            b = prob.fit_reduced_loo(p["Y"], rank, costs, slab_rows=slab_rows, factor=factor)
            assert same_bits(a[:3], b[:3]) and same_bits([a[3][key] for key in LOO_KEYS], [b[3][key] for key in LOO_KEYS]), (slab_rows, factor)
            assert np.array_equal(a[3]["press"], b[3]["press"])
    a = backend.fit_reduced(parameter(p["kernel"], p["kw"], p["cost"]), p["X"], p["Y"], rank, factor=factor, sample_weight=ones)  # the one-shot forms
    b = backend.fit_reduced(parameter(p["kernel"], p["kw"], p["cost"]), p["X"], p["Y"], rank, factor=factor)
    assert same_bits(a[:3], b[:3])
    a = backend.fit_reduced_loo(parameter(p["kernel"], p["kw"], p["cost"]), p["X"], p["Y"], rank, costs, factor=factor, sample_weight=ones)
    b = backend.fit_reduced_loo(parameter(p["kernel"], p["kw"], p["cost"]), p["X"], p["Y"], rank, costs, factor=factor)
    assert same_bits(a[:3], b[:3]) and same_bits([a[3][key] for key in LOO_KEYS + ("press",)], [b[3][key] for key in LOO_KEYS + ("press",)])


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("name, dtype, rank", [("rbf_777x5", np.float32, 64), ("poly_777x16", np.float64, 130)])
def test_weights_of_four_are_the_cost_times_four(name, dtype, rank, factor):
    p = rm.fit_case(name, dtype, 3)
    N = p["X"].shape[0]
    four, cost = np.full(N, 4.0), p["cost"]
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], cost), p["X"]) as prob, backend.ResidentProblem(parameter(p["kernel"], p["kw"], 4.0 * cost), p["X"]) as prob4:
        a = prob.fit_reduced(p["Y"], rank, factor=factor, sample_weight=four)
        b = prob4.fit_reduced(p["Y"], rank, factor=factor)
        assert same_bits(a[:3], b[:3]) and a[3]["jitter"] == 4.0 * b[3]["jitter"], factor
        a = prob.fit_reduced_loo(p["Y"], rank, [cost, 25.0 * cost], factor=factor, sample_weight=four)
        b = prob.fit_reduced_loo(p["Y"], rank, [4.0 * cost, 100.0 * cost], factor=factor)
        assert same_bits(a[:3], b[:3]), factor
        for key in ("leverage", "fitted", "loo", "loo_errors", "max_leverage"):
            assert np.array_equal(a[3][key], b[3][key]), (key, factor)
        assert np.array_equal(a[3]["press"], 4.0 * b[3]["press"]) and np.array_equal(a[3]["jitter"], 4.0 * b[3]["jitter"])


# ---------------------------------------------------------------- 4., 5. the fit ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_reference(name, dtype, k):
    """(case, model, e_model): float64 numpy, once per case, shared, never modified."""
    p = wm.fit_case(name, dtype, k)
    model = wm.WeightedReducedModel(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], p["w"], held=p["held"], **p["kw"])
    e = wm.e_model(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], p["w"], p["points"], held=p["held"], **p["kw"])
    for a in (p["X"], p["Y"], p["points"], p["w"], model.betas, model.rhos):
        a.setflags(write=False)
    return p, model, e


def fit_on_device(p, factor):
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], p["cost"]), p["X"]) as prob:
        assert p["held"][0] is p["X"] or prob.info()["rbf_direct"] == 0  # (the yardstick's data is the data this problem holds)
        return prob.fit_reduced(p["Y"] if p["Y"].shape[0] > 1 else p["Y"][0], len(p["landmarks"]), landmarks=p["landmarks"], factor=factor, sample_weight=p["w"])


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", [c[0] for c in rm.FIT_CASES])
def test_fit_against_the_model(name, dtype, k, factor):
    p, model, e = fit_reference(name, dtype, k)
    betas, rhos, used, info = fit_on_device(p, factor)
    assert np.array_equal(used, p["landmarks"]) and info["rank"] == 64 and np.asarray(betas).shape == ((3, 64) if k == 3 else (64,))
    f = model.decision_values(p["points"])
    g = model.decision_values(p["points"], betas, rhos)
    tol = rm.fit_tolerance(model, e, f)
    diff = float(np.max(np.abs(f - g)))
    print(f"weighted fit {name} {np.dtype(dtype).name} k={k} {factor}: |f_device - f_model| {diff:.2e}, tolerance {tol:.2e} (e_model {e:.1e}, cond(M) eps64 {model.cond * EPS64:.1e}), "
          f"jitter {info['jitter']:.2e} (model {model.nu:.2e})")
    assert abs(info["jitter"] / model.nu - 1.0) <= 1e-6  # (no retry on either side)
    assert diff <= tol, (name, diff, tol)


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_point_a_landmark_is_the_weighted_full_solution(dtype, factor):
    p, model, e = fit_reference("rbf_200x4", dtype, 1)
    assert np.min(p["w"]) >= 0.01
    betas, rhos, _, info = fit_on_device(p, factor)
    full = wm.dense_full_solution(p["kernel"], p["X"], p["Y"][0], p["cost"], p["w"], p["points"], held=p["held"], **p["kw"])
    g = model.decision_values(p["points"], betas, rhos)[0]
    tol = rm.fit_tolerance(model, e, full)
    diff = float(np.max(np.abs(full - g)))
    print(f"weighted all landmarks {np.dtype(dtype).name} {factor}: |f_device - f_full| {diff:.2e}, tolerance {tol:.2e}, jitter {info['jitter']:.2e}")
    assert info["rank"] == 200 and diff <= tol


# ---------------------------------------------------------------- 6. duplication and removal ----------------------------------------------------------------
@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_integer_weights_are_duplicated_and_removed_rows(dtype, factor):
    N, d, rank, cost = 255, 5, 16, 10.0
    X, y = pm.make_data(N, d, pm.DATA_SEED, dtype)
    kw = rm.rounded_parameters(dtype, gamma=0.2)
    lms = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
    w = np.random.default_rng(41).integers(0, 4, N)
    w[lms.astype(np.int64)] = np.maximum(w[lms.astype(np.int64)], 1)  # (a landmark must be a row of the expanded set: the unweighted fit takes row indices)
    assert set(np.unique(w).tolist()) == {0, 1, 2, 3}
    points = pm.make_data(rm.HELD_OUT, d, rm.HELD_OUT_SEED, dtype)[0]
    Xd, Yd, first = wm.expand(X, y[None, :], w)
    lms_dup = first[lms.astype(np.int64)].astype(np.uint64)  # the first copies
    prm = parameter("rbf", kw, cost)
    with backend.ResidentProblem(prm, X) as prob:
        direct = bool(prob.info()["rbf_direct"])
        betas, rhos, _, _ = prob.fit_reduced(y, rank, landmarks=lms, factor=factor, sample_weight=w.astype(np.float64))
    with backend.ResidentProblem(prm, Xd) as prob:
        assert bool(prob.info()["rbf_direct"]) == direct
        betas_dup, rhos_dup, _, _ = prob.fit_reduced(Yd[0], rank, landmarks=lms_dup, factor=factor)
    held = rm.held_data("rbf", X, direct=direct, **kw)
    model = wm.WeightedReducedModel("rbf", X, y[None, :], cost, lms, w.astype(np.float64), held=held, **kw)
    e = wm.e_model("rbf", X, y[None, :], cost, lms, w.astype(np.float64), points, held=held, **kw)
    f = model.decision_values(points)
    tol = rm.fit_tolerance(model, e, f)
    g, g_dup = model.decision_values(points, betas, rhos), model.decision_values(points, betas_dup, rhos_dup)
    # a float32 rbf problem centres the data it holds by ITS mean, which the duplicated set moves: both fits are compared with the model of their own held data
    model_dup = rm.ReducedModel("rbf", Xd, Yd, cost, lms_dup, held=rm.held_data("rbf", Xd, direct=direct, **kw), **kw)
    f_dup = model_dup.decision_values(points)
    print(f"duplication {np.dtype(dtype).name} {factor}: |weighted - model| {np.max(np.abs(g - f)):.2e}, |duplicated - its model| {np.max(np.abs(g_dup - f_dup)):.2e}, "
          f"|weighted - duplicated| {np.max(np.abs(g - g_dup)):.2e}, tolerance {tol:.2e}")
    assert np.max(np.abs(g - f)) <= tol and np.max(np.abs(g_dup - f_dup)) <= tol
    if np.dtype(dtype) == np.float64:
        assert np.max(np.abs(g - g_dup)) <= tol


# ---------------------------------------------------------------- 7. leave-one-out ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loo_reference(dtype, k, rank):
    p = wm.loo_case(dtype, k, rank)
    per_cost = []
    for cost in wm.LOO_COSTS:
        model = wm.WeightedLooModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], p["w"], held=p["held"], **p["kw"])
        e = wm.e_loo(model, wm.stable(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], p["w"], held=p["held"], **p["kw"])[2])
        brute = wm.brute_force(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], p["w"], held=p["held"], **p["kw"]) if k == 1 else None
        for a in (model.h, model.f, model.loo):
            a.setflags(write=False)
        per_cost.append((model, e, brute))
    return p, per_cost


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("rank", [16, 130])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_loo_against_the_model_and_brute_force(dtype, rank, k, factor):
    p, per_cost = loo_reference(dtype, k, rank)
    w, Y = p["w"], p["Y"]
    assert np.max(w) == 64.0 and np.count_nonzero(w == 0.0) > 0
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 1.0), p["X"]) as prob:
        assert p["held"][0] is p["X"] or prob.info()["rbf_direct"] == 0
        betas, rhos, used, report = prob.fit_reduced_loo(Y if k > 1 else Y[0], rank, wm.LOO_COSTS, landmarks=p["landmarks"], factor=factor, sample_weight=w)
        again = prob.fit_reduced_loo(Y if k > 1 else Y[0], rank, wm.LOO_COSTS, landmarks=p["landmarks"], factor=factor, sample_weight=w)
        single_cost = [prob.fit_reduced_loo(Y if k > 1 else Y[0], rank, [cost], landmarks=p["landmarks"], factor=factor, sample_weight=w) for cost in wm.LOO_COSTS]
        single_col = [prob.fit_reduced_loo(Y[c], rank, wm.LOO_COSTS, landmarks=p["landmarks"], factor=factor, sample_weight=w) for c in range(k)] if k > 1 else []
    keys = LOO_KEYS + ("press",)
    assert same_bits((betas, rhos), again[:2]) and same_bits([report[key] for key in keys], [again[3][key] for key in keys])  # repeats
    for s, one in enumerate(single_cost):  # a cost has the bits of the one-cost call
        assert np.array_equal(betas[s], one[0][0]) and np.array_equal(rhos[s], one[1][0]) and same_bits([report[key][s] for key in keys], [one[3][key][0] for key in keys]), s
    for c, one in enumerate(single_col):  # column c has the bits of the single-column call; one leverage vector serves all
        assert np.array_equal(betas[:, c], one[0]) and np.array_equal(rhos[:, c], one[1]) and np.array_equal(report["leverage"], one[3]["leverage"])
        assert np.array_equal(report["loo"][:, c], one[3]["loo"]) and np.array_equal(report["fitted"][:, c], one[3]["fitted"]) and np.array_equal(report["press"][:, c], one[3]["press"])
    zero = w == 0.0
    for s, (model, e, brute) in enumerate(per_cost):
        h = report["leverage"][s]
        f, loo = np.atleast_2d(report["fitted"][s]), np.atleast_2d(report["loo"][s])
        assert np.all(h[zero] == 0.0) and np.array_equal(loo[:, zero], f[:, zero])  # to the bit
        assert abs(report["jitter"][s] / model.nu - 1.0) <= 1e-6
        for name, got, ref in (("h", h, model.h), ("f", f, model.f), ("loo", loo, model.loo)):
            tol = lm.tolerance(model, e, np.max(np.abs(ref)))
            diff = float(np.max(np.abs(got - ref)))
            print(f"weighted loo {np.dtype(dtype).name} rank {rank} k={k} {factor} C={wm.LOO_COSTS[s]:g} {name}: |device - model| {diff:.2e}, tolerance {tol:.2e} (max leverage {model.max_leverage:.2f})")
            assert diff <= tol, (name, s, diff, tol)
        if brute is not None:
            tol = lm.tolerance(model, e, np.max(np.abs(brute)))
            assert np.max(np.abs(loo - brute)) <= tol, (s, float(np.max(np.abs(loo - brute))), tol)
        # the sums follow their definitions on the returned arrays
        assert np.allclose(np.atleast_1d(report["press"][s]), wm.press_of(Y, loo, w), rtol=1e-12, atol=0.0)
        assert np.array_equal(np.atleast_1d(report["loo_errors"][s]), wm.errors_of(Y, loo, w)) and report["max_leverage"][s] == h.max()
    # betas and rhos of a cost: the bits of fit_reduced_weighted on a problem created with that cost, same factor
    for s, cost in enumerate(wm.LOO_COSTS):
        with backend.ResidentProblem(parameter(p["kernel"], p["kw"], cost), p["X"]) as prob:
            b1, r1, _, _ = prob.fit_reduced(Y if k > 1 else Y[0], rank, landmarks=p["landmarks"], factor=factor, sample_weight=w)
        assert np.array_equal(betas[s], b1) and np.array_equal(rhos[s], r1), (s, factor)


# ---------------------------------------------------------------- 8. the surface ----------------------------------------------------------------
def imbalanced(classes, dtype=np.float64, N=1200):
    X, labels = lm.overlapping_blobs(N, 6, classes, seed=33, dtype=dtype)
    labels = np.where(np.random.default_rng(8).random(N) < 0.7, 0, labels)
    sw = np.random.default_rng(4).uniform(0.5, 2.0, N)
    sw[::17] = 0.0
    return X, labels, sw


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_csvm_fit_reduced_with_weights_saves_loads_and_predicts(dtype, tmp_path):
    X, labels, sw = imbalanced(2, dtype)
    kw = rm.rounded_parameters(dtype, gamma=1.0 / 6)
    data = DataSet(X, labels.tolist(), real_type=dtype)
    svm = MI355CSVM(kernel_type="rbf", cost=10.0, gamma=1.0 / 6)
    model = svm.fit_reduced(data, 64, sample_weight=sw)
    lms = rm.library_landmarks(X.shape[0], 64)
    assert svm.last_cg_info["iterations"] == 0 and np.array_equal(svm.last_cg_info["landmarks"], lms) and model.num_support_vectors() == 64
    Y = np.where(labels == 1, 1.0, -1.0)[None, :]
    held = rm.held_data("rbf", X, **kw)
    ref = wm.WeightedReducedModel("rbf", X, Y, 10.0, lms, sw, held=held, **kw)
    e = wm.e_model("rbf", X, Y, 10.0, lms, sw, X, held=held, **kw)
    f = ref.decision_values(X)[0]
    tol = rm.fit_tolerance(ref, e, f) + (16 * rm.EPS32 * float(np.max(rm.summand_scale("rbf", ref.X_L, ref.betas, ref.rhos, X, **kw))) if dtype == np.float32 else 0.0)
    unweighted = svm.fit_reduced(data, 64)
    assert not np.array_equal(np.asarray(model.alpha), np.asarray(unweighted.alpha))  # (the weights took part)
    path = tmp_path / "weighted.model"
    model.save(str(path))
    loaded = Model.load(str(path), real_type=dtype, label_type=int)
    clear, expected = np.abs(f) > tol, (f > 0).astype(int)
    assert loaded.num_support_vectors() == 64 and np.mean(~clear) <= 0.01
    for m in (model, loaded):
        assert np.array_equal(np.array(svm.predict(m, data))[clear], expected[clear])
    models, report = svm.fit_reduced_path(data, 64, [10.0], sample_weight=sw)
    assert np.array_equal(np.asarray(models[0].alpha), np.asarray(model.alpha))
    assert report["loo_accuracy"][0] == pytest.approx(np.average(np.sign(report["loo"][0]) == Y[0], weights=sw), abs=1e-12)


@pytest.mark.parametrize("classes", [2, 3])
def test_svc_fit_reduced_weighted_with_balanced_classes(classes):
    X, labels, sw = imbalanced(classes)
    counts = np.array([np.count_nonzero(labels == c) for c in range(classes)], dtype=np.float64)
    multipliers = labels.size / (classes * counts)
    by_hand = sw * multipliers[labels]
    est = svc.SVC(kernel="rbf", C=10.0, gamma=1.0 / 6, class_weight="balanced")
    fitted = svc.fit_reduced_weighted(est, X, labels, 64, sample_weight=sw)
    k = 1 if classes == 2 else classes
    assert est._fit is None and fitted.dual_coef_.shape == (k, 64) and np.allclose(fitted.class_weight_, multipliers)
    # the model built from the hand-computed weights through the backend: the same bits
    Y = np.where(labels[None, :] == np.arange(classes)[:, None], 1.0, -1.0)[(1 if classes == 2 else 0):]
    betas, rhos, used, _ = backend.fit_reduced(est._params().resolved(X.shape[1]), X, Y, 64, sample_weight=by_hand)
    assert np.array_equal(fitted.dual_coef_, betas) and np.array_equal(fitted.intercept_, -rhos) and np.array_equal(fitted.support_, used)
    plain = svc.fit_reduced(svc.SVC(kernel="rbf", C=10.0, gamma=1.0 / 6), X, labels, 64)
    assert not np.array_equal(plain.dual_coef_, fitted.dual_coef_)
    # balanced weights move predictions towards the rare classes
    assert np.mean(fitted.predict(X) != 0) > np.mean(plain.predict(X) != 0)
    scores, clones = svc.fit_reduced_cv_weighted(est, X, labels, 64, [0.1, 10.0], sample_weight=sw)
    assert np.array_equal(clones[1].dual_coef_, fitted.dual_coef_) and all(np.allclose(c.class_weight_, multipliers) for c in clones)
    _, _, _, report = backend.fit_reduced_loo(est._params().resolved(X.shape[1]), X, Y, 64, [0.1, 10.0], sample_weight=by_hand)
    for s in range(2):
        correct = (np.sign(report["loo"][s][0]) == np.sign(Y[0])) if classes == 2 else (np.argmax(report["loo"][s], axis=0) == labels)
        assert scores[s] == pytest.approx(np.average(correct, weights=by_hand), abs=1e-12)
    with pytest.raises(InvalidParameterError, match="class_weight"):  # (the unweighted function stays as it is)
        svc.fit_reduced(est, X, labels, 64)
    for rule in ("greedy", "rpcholesky"):  # the selection rules work as elsewhere and ignore the weights
        chosen = svc.fit_reduced_weighted(est, X, labels, 32, sample_weight=sw, landmarks=rule)
        assert np.array_equal(chosen.support_, svc.fit_reduced(svc.SVC(kernel="rbf", C=10.0, gamma=1.0 / 6), X, labels, 32, landmarks=rule).support_)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_problem_is_left_as_it_was(dtype):
    p, _, _ = fit_reference("rbf_777x5", dtype, 1)
    n = p["X"].shape[0] - 1
    y, w = p["Y"][0], p["w"]
    eps = pm.GPU_EPS[np.dtype(dtype)]
    d = np.random.default_rng(3).standard_normal(n).astype(dtype)

    def state(prob):
        prob.cg_begin(y, eps)
        prob.cg_step(2000)
        alpha, rho, info = prob.cg_finish()
        return prob.matvec(d, np.zeros(n, dtype)), alpha, rho, info["iterations"]

    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], p["cost"]), p["X"]) as prob:
        before = state(prob)
        for factor in FACTORS:
            prob.fit_reduced(p["Y"], 64, factor=factor, sample_weight=w)
            prob.fit_reduced_loo(y, 16, [1.0, 10.0], factor=factor, sample_weight=w)
        prob.landmark_gram_weighted(y, 16, w, slab_rows=256)
        after = state(prob)
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        # the explicit argument is the only source of weights: the problem's own stay untouched, and while they are set the call is refused as the unweighted one is
        positive = np.maximum(w, 0.5)
        prob.set_weights(positive)
        weighted_state = state(prob)
        for call in (lambda: prob.fit_reduced(y, 8, sample_weight=w), lambda: prob.fit_reduced_loo(y, 8, [1.0], sample_weight=w), lambda: prob.landmark_gram_weighted(y, 8, w)):
            with pytest.raises(InvalidParameterError, match="weights"):
                call()
        for a, b in zip(weighted_state, state(prob)):
            assert np.array_equal(a, b)
        assert not np.array_equal(weighted_state[1], before[1])
        prob.set_weights(None)
        prob.cg_begin(y, 1e-6)
        with pytest.raises(InvalidParameterError, match="between cg_begin and cg_finish"):
            prob.fit_reduced(y, 8, sample_weight=w)
        prob.cg_step(1)
        prob.cg_finish()
        with pytest.raises(InvalidParameterError, match="not less than 0.0"):
            prob.fit_reduced(y, 8, sample_weight=-w)
        for a, b in zip(before, state(prob)):
            assert np.array_equal(a, b)
