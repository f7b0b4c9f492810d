"""GPU (-m gpu): exact leave-one-out scores of the fixed-size LS-SVM over a cost grid -- leave-one-out with the landmark set held fixed (lssvm_mi355_problem_fit_reduced_loo /
_reduced_leverage, lssvm_mi355_fit_reduced_loo_*, MI355CSVM.fit_reduced_path, svc.fit_reduced_cv).  The yardstick is numpy float64
(tests/reduced_loo_model.py); tests/test_reduced_loo_host.py shows the model alone to meet the bounds below and every input to meet the conditions they rest on.

Operator.  reduced_leverage -- k_reduced_leverage on the caller's V, shift and extra columns, 1 / N and the mean of y left out -- against numpy at N in {255, 777} x rank in
{1, 16, 64, 65, 129, 300} x k in {0, 1, 3} x slab_rows in {256, 0} x both dtypes x the three kernel functions, and once at rank 1 024 (N = 1 100).  V is lower triangular
with a unit diagonal and 0.1 uniform(0, 1) below it: well conditioned, so the test is about the operator.  With t_ik = sum_j V_kj (phi_ij - shift_j) and
a_ik = sum_j |V_kj| |phi_ij - shift_j| the bound of h_i = sum_k t_ik^2 is derived, not tuned:

    2 (m + 4) eps64 sum_k |t_ik| a_ik  +  2 sum_k |t_ik| sum_j |V_kj| dPhi_ij

  * first term: t_ik is one chain of at most m fused multiply-adds on operands that each carry the rounding of their centring (gamma_{m+1} a_ik), its square enters
    twice, and the m squares are summed in a fixed order of at most m + 4 additions (gamma_{m+4} sum t^2 <= gamma_{m+4} sum |t| a): together below 1.5 (m + 4) eps64 of
    sum |t| a; 2 (m + 4) eps64 leaves a small factor;
  * second term: dPhi is the element error of Phi that test_operator_against_numpy of tests/test_gpu_reduced.py allows (its phi_error, on the same data), through |V|.
The fitted columns f_ic = sum_j (phi_ij - shift_j) B_jc likewise: 2 (m + 4) eps64 sum_j |phi_ij - shift_j| |B_jc| + sum_j dPhi_ij |B_jc|.
Ranks 129 and above cross a column block of V^T: they exercise the triangular skip.  A second call puts nonzero garbage into V's strict upper triangle and must not change
a bit: the blocks above the diagonal are never read, the blocks on it mask.

Fit.  reduced_model.FIT_CASES at the costs (0.1, 10, 1000), k in {1, 3}, both dtypes: h, f and loo within 8 max(e_loo, cond(M) eps64) x the largest |value| of the model's
h, f, loo; betas and rhos of cost s have the bits of fit_reduced on a problem created with that cost; press, loo_errors and max_leverage equal their recomputation from the
returned arrays.  Brute force: at 255 x 5 rbf, rank 16, the device's loo against 255 numpy refits per cost within 8 max(e_loo, cond(M) eps64) max |f|.

Bit equality (repeats; h for k = 1 and k = 3; column c of a k = 3 call against the single call; the costs of a grid against one-cost calls; one-shot against resident), the
problem left as it was, the refusals that need a device, and the surface.

Measured on an MI355X (for the record; the assertions are the bounds above): MEASURED below."""

import functools

import numpy as np
import pytest

import pcg_model as pm
import reduced_loo_model as lm
import reduced_model as rm
import test_gpu_reduced as base
from plssvm_amd import backend, svc
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.model import Model

pytestmark = pytest.mark.gpu

EPS64 = rm.EPS64
KERNELS, parameter = base.KERNELS, base.parameter
OPERATOR_N, OPERATOR_RANKS, OPERATOR_K, OPERATOR_D = (255, 777), (1, 16, 64, 65, 129, 300), (0, 1, 3), 5

# what one run on an MI355X gave, for the record (the assertions are the bounds of the module docstring, not these figures)
MEASURED = {
    "operator: largest error / bound over all ranks, k and slab sizes": {"float64": "0.08 ... 0.40 (polynomial, N = 777)", "float32": "0.04 ... 0.19", "rank 1024": 0.001},
    "fit at C = 1000, k = 3: (|device - model|, tolerance) of h, f, loo": {
        "rbf_777x5 float64": ((4.2e-09, 8.9e-08), (2.9e-08, 2.6e-07), (3.8e-08, 3.2e-07)), "rbf_777x5 float32": ((3.6e-09, 6.0e-08), (2.5e-08, 1.7e-07), (3.4e-08, 2.1e-07)),
        "poly_777x16 float64": ((1.0e-12, 4.1e-11), (1.6e-11, 1.3e-10), (1.8e-11, 1.5e-10)), "poly_777x16 float32": ((1.2e-12, 6.9e-11), (1.3e-11, 2.2e-10), (1.7e-11, 2.6e-10))},
    "brute force, |loo_device - refits| and the tolerance at C = 0.1 / 1 / 100 / 1e4": {
        "float64": ((1.4e-14, 3.2e-13), (4.6e-13, 4.8e-12), (4.0e-12, 3.6e-11), (4.2e-12, 3.8e-11)),
        "float32": ((9.9e-15, 3.2e-13), (2.2e-13, 1.8e-12), (2.0e-12, 1.2e-11), (2.0e-12, 1.2e-11))},
    "leave-one-out accuracy on overlapping blobs at C = 1e-3 / 1 / 1e3": (0.7433, 0.7817, 0.7833),
}


def operands(rank, k, seed=11):
    """V (unit diagonal plus 0.1 uniform below it), the same with garbage above the diagonal, and k extra columns."""
    rng = np.random.default_rng(seed + rank)
    V = np.eye(rank) + 0.1 * np.tril(rng.random((rank, rank)), -1)
    garbage = V + np.triu(1.0 + rng.random((rank, rank)), 1) * 1e3
    return V, garbage, rng.standard_normal((rank, k))


def operator_reference(kernel, X, lms, kw, r, u_h, V, B):
    Phi = pm.kernel_matrix(kernel, X, np.asarray(X)[lms.astype(np.int64)], **kw)
    dPhi = base.phi_error(kernel, X, lms, kw, r, u_h)
    m = len(lms)
    shift = Phi.mean(axis=0)
    Pc = Phi - shift[None, :]
    T, A = Pc @ V.T, np.abs(Pc) @ np.abs(V).T
    h = (T * T).sum(axis=1)
    h_bound = 2.0 * (m + 4) * EPS64 * (np.abs(T) * A).sum(axis=1) + 2.0 * (np.abs(T) * (dPhi @ np.abs(V).T)).sum(axis=1)
    f = (Pc @ B).T
    f_bound = (2.0 * (m + 4) * EPS64 * (np.abs(Pc) @ np.abs(B)) + dPhi @ np.abs(B)).T
    return shift, h, h_bound, f, f_bound


def check_operator(prob, kernel, X, lms, kw, r, u_h, k, slab_sizes):
    rank = len(lms)
    V, garbage, B = operands(rank, k)
    shift, h_ref, h_bound, f_ref, f_bound = operator_reference(kernel, X, lms, kw, r, u_h, V, B)
    worst = 0.0
    for slab_rows in slab_sizes:
        h, f = prob.reduced_leverage(V, shift, B if k else None, landmarks=lms, slab_rows=slab_rows)
        assert h.shape == h_ref.shape and f.shape == f_ref.shape and np.all(np.isfinite(h)) and np.all(np.isfinite(f))
        ratio = float(np.max(np.abs(h - h_ref) / h_bound))
        if k:
            ratio = max(ratio, float(np.max(np.abs(f - f_ref) / f_bound)))
        assert ratio <= 1.0, (kernel, X.shape, rank, k, slab_rows, ratio)
        worst = max(worst, ratio)
        h2, f2 = prob.reduced_leverage(garbage, shift, B if k else None, landmarks=lms, slab_rows=slab_rows)
        assert np.array_equal(h, h2) and np.array_equal(f, f2), (kernel, rank, k, slab_rows)
    return worst


@pytest.mark.parametrize("N", OPERATOR_N)
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_operator_against_numpy(dtype, kernel, N):
    X, _ = pm.make_data(N, OPERATOR_D, pm.DATA_SEED, dtype)
    worst = 0.0
    with backend.ResidentProblem(parameter(kernel, rm.rounded_parameters(dtype, **KERNELS[kernel]), 10.0), X) as prob:
        Xy, kw_y, _, r, u_h = base.operator_setup(kernel, dtype, X, prob)
        for rank in OPERATOR_RANKS:
            if rank > N:
                continue
            lms = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
            for k in OPERATOR_K:
                worst = max(worst, check_operator(prob, kernel, Xy, lms, kw_y, r, u_h, k, (256, 0)))
    print(f"leverage operator {np.dtype(dtype).name} {kernel} N={N}: largest error / bound {worst:.3f}")


def test_operator_at_the_largest_rank():
    N, rank = 1100, rm.MAX_RANK
    X, _ = pm.make_data(N, 3, pm.DATA_SEED, np.float64)
    lms = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
    with backend.ResidentProblem(parameter("rbf", KERNELS["rbf"], 10.0), X) as prob:
        worst = check_operator(prob, "rbf", X, lms, KERNELS["rbf"], 2, EPS64, 3, (256, 0))
    print(f"leverage operator at rank {rank}: largest error / bound {worst:.3f}")


# ---------------------------------------------------------------- the fit ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_reference(name, dtype, k):
    """(case, per cost: (model, e_loo)): float64 numpy, once per case, shared, never modified."""
    p = rm.fit_case(name, dtype, k)
    per_cost = []
    for cost in lm.FIT_COSTS:
        model = lm.LooModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], held=p["held"], **p["kw"])
        e = lm.e_loo(model, lm.stable(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], held=p["held"], **p["kw"])[2])
        for a in (model.h, model.f, model.loo):
            a.setflags(write=False)
        per_cost.append((model, e))
    for a in (p["X"], p["Y"]):
        a.setflags(write=False)
    return p, per_cost


def sequential_press(y, loo):
    total = 0.0
    for a, b in zip(y.tolist(), loo.tolist()):
        d = a - b
        total += d * d
    return total


def check_report_against_its_arrays(Y, report):
    """press, loo_errors and max_leverage as the header defines them, from the arrays of the same report."""
    Y2, loo = np.atleast_2d(Y).astype(np.float64), report["loo"]
    loo = loo[:, None, :] if loo.ndim == 2 else loo
    press, errors = np.atleast_3d(report["press"]).reshape(loo.shape[:2]), np.atleast_3d(report["loo_errors"]).reshape(loo.shape[:2])
    for s in range(loo.shape[0]):
        assert report["max_leverage"][s] == report["leverage"][s].max()
        for c in range(loo.shape[1]):
            assert press[s, c] == sequential_press(Y2[c], loo[s, c]), (s, c)
            assert errors[s, c] == np.count_nonzero(np.sign(loo[s, c]) != np.sign(Y2[c])), (s, c)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", [c[0] for c in rm.FIT_CASES])
def test_fit_against_the_model(name, dtype, k):
    p, per_cost = fit_reference(name, dtype, k)
    Y = p["Y"] if k > 1 else p["Y"][0]
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 3.0), p["X"]) as prob:  # (the problem's own cost plays no part)
        assert p["held"][0] is p["X"] or prob.info()["rbf_direct"] == 0
        betas, rhos, used, report = prob.fit_reduced_loo(Y, 64, lm.FIT_COSTS, landmarks=p["landmarks"])
    assert np.array_equal(used, p["landmarks"]) and np.array_equal(report["costs"], lm.FIT_COSTS)
    assert betas.shape == ((3, 3, 64) if k == 3 else (3, 64)) and report["leverage"].shape == (3, 777) and report["loo"].shape == ((3, 3, 777) if k == 3 else (3, 777))
    for s, (model, e) in enumerate(per_cost):
        for what, got, ref in (("h", report["leverage"][s], model.h), ("f", np.atleast_2d(report["fitted"][s]), model.f), ("loo", np.atleast_2d(report["loo"][s]), model.loo)):
            tol = lm.tolerance(model, e, np.max(np.abs(ref)))
            diff = float(np.max(np.abs(got - ref)))
            print(f"loo fit {name} {np.dtype(dtype).name} k={k} C={lm.FIT_COSTS[s]:g} {what}: |device - model| {diff:.2e}, tolerance {tol:.2e} (e_loo {e:.1e}, cond(M) eps64 {model.cond * EPS64:.1e})")
            assert diff <= tol, (name, what, s, diff, tol)
        assert abs(report["jitter"][s] / model.nu - 1.0) <= 1e-6 and report["infos"][s]["cost"] == lm.FIT_COSTS[s]
        assert np.all(report["leverage"][s] > 1.0 / 777) and np.all(report["leverage"][s] < 1.0)
        # the coefficients of cost s: the bits of fit_reduced on a problem created with that cost
        with backend.ResidentProblem(parameter(p["kernel"], p["kw"], lm.FIT_COSTS[s]), p["X"]) as at_cost:
            b1, r1, _, _ = at_cost.fit_reduced(Y, 64, landmarks=p["landmarks"])
        assert np.array_equal(betas[s], b1) and np.array_equal(rhos[s], r1), (name, s)
    check_report_against_its_arrays(p["Y"], report)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_loo_against_brute_force_refits(dtype):
    p = lm.identity_case("rbf_255x5", dtype)
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 1.0), p["X"]) as prob:
        assert p["held"][0] is p["X"] or prob.info()["rbf_direct"] == 0
        _, _, _, report = prob.fit_reduced_loo(p["Y"][0], 16, lm.IDENTITY_COSTS, landmarks=p["landmarks"])
    for s, cost in enumerate(lm.IDENTITY_COSTS):
        model = lm.LooModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], held=p["held"], **p["kw"])
        e = lm.e_loo(model, lm.stable(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], held=p["held"], **p["kw"])[2])
        brute = lm.brute_force(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], held=p["held"], **p["kw"])[0]
        tol = lm.tolerance(model, e, np.max(np.abs(model.f)))
        diff = float(np.max(np.abs(report["loo"][s] - brute)))
        print(f"brute force {np.dtype(dtype).name} C={cost:g}: |loo_device - refits| {diff:.2e}, tolerance {tol:.2e} (e_loo {e:.1e}, cond(M) {model.cond:.1e})")
        assert diff <= tol, (cost, diff, tol)
    check_report_against_its_arrays(p["Y"], report)


# ---------------------------------------------------------------- bit equality, the problem left as it was, refusals ----------------------------------------------------------------
def same(a, b):
    """betas, rhos, landmarks and every array of the report, to the bit."""
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and all(np.array_equal(a[3][n], b[3][n]) for n in ("leverage", "fitted", "loo", "press", "loo_errors", "max_leverage", "jitter"))


@pytest.mark.parametrize("name, dtype", [("rbf_777x5", np.float32), ("poly_777x16", np.float64)])
def test_repeats_columns_and_costs_are_bit_equal(name, dtype):
    p, _ = fit_reference(name, dtype, 3)
    costs = lm.FIT_COSTS
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 5.0), p["X"]) as prob:
        for slab_rows in (0, 256):
            full = prob.fit_reduced_loo(p["Y"], 64, costs, slab_rows=slab_rows)  # the library's own landmarks
            assert same(full, prob.fit_reduced_loo(p["Y"], 64, costs, slab_rows=slab_rows))
            b3, r3, used, rep3 = full
            for c in range(3):  # column c of the k = 3 call: the bits of the single call; h does not depend on k
                b1, r1, _, rep1 = prob.fit_reduced_loo(p["Y"][c], 64, costs, slab_rows=slab_rows)
                assert np.array_equal(rep1["leverage"], rep3["leverage"]) and np.array_equal(rep1["max_leverage"], rep3["max_leverage"])
                assert np.array_equal(b3[:, c], b1) and np.array_equal(r3[:, c], r1)
                for n in ("fitted", "loo", "press", "loo_errors"):
                    assert np.array_equal(rep3[n][:, c], rep1[n]), (slab_rows, c, n)
            for s, cost in enumerate(costs):  # cost s of the grid: the bits of the one-cost call
                b, r, _, rep = prob.fit_reduced_loo(p["Y"], 64, [cost], slab_rows=slab_rows)
                assert np.array_equal(b[0], b3[s]) and np.array_equal(r[0], r3[s])
                for n in ("leverage", "fitted", "loo", "press", "loo_errors", "max_leverage", "jitter"):
                    assert np.array_equal(rep[n][0], rep3[n][s]), (slab_rows, s, n)
            assert same(full, prob.fit_reduced_loo(p["Y"], 64, costs, landmarks=used, slab_rows=slab_rows))
        assert np.array_equal(used, rm.library_landmarks(p["X"].shape[0], 64))
    one_shot = backend.fit_reduced_loo(parameter(p["kernel"], p["kw"], 5.0), p["X"], p["Y"], 64, costs, slab_rows=256)
    assert same(one_shot, full)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_problem_is_left_as_it_was(dtype):
    p, _ = fit_reference("rbf_777x5", dtype, 1)
    n = p["X"].shape[0] - 1
    y = p["Y"][0]
    eps = pm.GPU_EPS[np.dtype(dtype)]
    d = np.random.default_rng(3).standard_normal(n).astype(dtype)

    def state(prob):
        prob.cg_begin(y, eps)
        prob.cg_step(2000)
        alpha, rho, info = prob.cg_finish()
        a_pcg, rho_pcg, i_pcg = prob.solve_pcg(y, eps, 2000)
        return prob.matvec(d, np.zeros(n, dtype)), alpha, rho, info["iterations"], a_pcg, rho_pcg, i_pcg["iterations"], prob.precond_landmarks()

    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], p["cost"]), p["X"]) as prob:
        prob.build_preconditioner(landmarks=p["landmarks"][:37])
        before = state(prob)
        prob.fit_reduced_loo(p["Y"], 64, lm.FIT_COSTS)
        prob.reduced_leverage(np.eye(16), np.zeros(16), slab_rows=256)
        after = state(prob)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_refusals_on_a_problem():
    p, _ = fit_reference("rbf_777x5", np.float64, 1)
    N, y = p["X"].shape[0], p["Y"][0]
    prm = parameter(p["kernel"], p["kw"], p["cost"])
    with backend.ResidentProblem(prm, p["X"]) as prob:
        calls = (lambda: prob.fit_reduced_loo(y, 8, [1.0]), lambda: prob.reduced_leverage(np.eye(8), np.zeros(8)))
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
                prob.fit_reduced_loo(y, 8, costs)
        with pytest.raises(InvalidParameterError, match="distinct"):
            prob.fit_reduced_loo(y, 3, [1.0], landmarks=[3, 7, 3])
        with pytest.raises(InvalidParameterError, match="index of a data point"):
            prob.fit_reduced_loo(y, 2, [1.0], landmarks=[3, N])
        with pytest.raises(InvalidParameterError, match="rank of the reduced model"):
            prob.fit_reduced_loo(y, N + 1, [1.0])
        with pytest.raises(InvalidParameterError, match="slab_rows"):
            prob.fit_reduced_loo(y, 8, [1.0], slab_rows=100)
        with pytest.raises(InvalidParameterError, match="rows"):
            prob.reduced_leverage(np.eye(8), np.zeros(7))
        _, _, used, report = prob.fit_reduced_loo(y, 2, [1.0], landmarks=[0, N - 1])  # (the last point is allowed, and the handle still works)
        assert np.array_equal(used, [0, N - 1]) and np.all(np.isfinite(report["loo"]))
    with backend.ResidentProblem(prm, p["X"], devices=[0, 0]) as shard:  # two shards on the one device
        for call in (lambda: shard.fit_reduced_loo(y, 8, [1.0]), lambda: shard.reduced_leverage(np.eye(8), np.zeros(8))):
            with pytest.raises(InvalidParameterError, match="one device and one rank"):
                call()
    X2, labels = rm.blobs(200, 4, 2, seed=5)
    with pytest.raises(InvalidParameterError, match="one device"):
        MI355CSVM(num_devices=0, kernel_type="rbf").fit_reduced_path(DataSet(X2, labels.tolist()), 4, [1.0])


# ---------------------------------------------------------------- the surface ----------------------------------------------------------------
SURFACE_COSTS = (0.1, 10.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_csvm_fit_reduced_path_models_save_load_and_predict_like_fit_reduced_models(dtype, tmp_path):
    X, labels = rm.blobs(2000, 8, 2, seed=31, dtype=dtype)
    data = DataSet(X, labels.tolist(), real_type=dtype)
    svm = MI355CSVM(kernel_type="rbf", cost=3.0, gamma=1.0 / 8)
    models, report = svm.fit_reduced_path(data, 64, SURFACE_COSTS)
    assert len(models) == 2 and report["loo"].shape == (2, 2000) and np.array_equal(report["landmarks"], rm.library_landmarks(2000, 64))
    assert [i["iterations"] for i in svm.last_cg_info] == [0, 0]
    for s, (cost, model) in enumerate(zip(SURFACE_COSTS, models)):
        single = MI355CSVM(kernel_type="rbf", cost=cost, gamma=1.0 / 8)
        ref = single.fit_reduced(data, 64)
        assert model.params.cost == cost and model.alpha.dtype == np.dtype(dtype) and np.array_equal(model.alpha, ref.alpha) and model.rho == ref.rho
        assert np.array_equal(model.support_vectors(), ref.support_vectors())
        path = tmp_path / f"reduced_{s}.model"
        model.save(str(path))
        loaded = Model.load(str(path), real_type=dtype, label_type=int)
        assert loaded.num_support_vectors() == 64
        expected = single.predict(ref, data)
        assert svm.predict(model, data) == expected and svm.predict(loaded, data) == expected
        assert svm.score(model) == single.score(ref) >= 0.97
        y = data.mapped_labels().astype(np.float64)
        assert report["loo_errors"][s] == np.count_nonzero(np.sign(report["loo"][s]) != y) and report["loo_accuracy"][s] == 1.0 - int(report["loo_errors"][s]) / 2000


@pytest.mark.parametrize("classes", [2, 3])
def test_svc_fit_reduced_cv(classes):
    X, labels = rm.blobs(2000, 8, classes, seed=31)
    kw = dict(gamma=1.0 / 8)
    lms = rm.library_landmarks(2000, 64)
    Y = np.where(labels[None, :] == np.arange(classes)[:, None], 1.0, -1.0)
    if classes == 2:
        Y = Y[1:]
    est = svc.SVC(kernel="rbf", C=3.0, gamma=1.0 / 8)
    scores, clones = svc.fit_reduced_cv(est, X, labels, 64, SURFACE_COSTS)
    assert est._fit is None and scores.shape == (2,) and [c.C for c in clones] == list(SURFACE_COSTS)
    for s, cost in enumerate(SURFACE_COSTS):
        model = lm.LooModel("rbf", X, Y, cost, lms, **kw)
        e = lm.e_loo(model, lm.stable("rbf", X, Y, cost, lms, **kw)[2])
        tol = lm.tolerance(model, e, np.max(np.abs(model.loo)))
        if classes == 2:
            clear, predicted = np.abs(model.loo[0]) > tol, (model.loo[0] > 0).astype(int)
        else:
            top = np.sort(model.loo, axis=0)
            clear, predicted = top[-1] - top[-2] > 2 * tol, np.argmax(model.loo, axis=0)
        expected = float(np.mean(predicted == labels))
        print(f"fit_reduced_cv {classes} classes C={cost:g}: loo accuracy {scores[s]:.4f} (numpy {expected:.4f}), points within the tolerance {np.count_nonzero(~clear)}")
        assert np.mean(~clear) <= 0.01 and abs(scores[s] - expected) * 2000 <= np.count_nonzero(~clear) + 1e-9
        single = svc.fit_reduced(svc.SVC(kernel="rbf", C=cost, gamma=1.0 / 8), X, labels, 64)
        assert np.array_equal(clones[s].dual_coef_, single.dual_coef_) and np.array_equal(clones[s].support_, single.support_) and np.array_equal(clones[s].intercept_, single.intercept_)
        assert np.array_equal(clones[s].predict(X), single.predict(X))


def test_the_score_moves_with_the_cost_on_overlapping_blobs():
    X, labels = lm.overlapping_blobs(600, 4, 2, seed=41)
    Cs = (1e-3, 1.0, 1e3)
    scores, _ = svc.fit_reduced_cv(svc.SVC(kernel="rbf", gamma=0.25), X, labels, 32, Cs)
    lms = rm.library_landmarks(600, 32)
    Y = np.where(labels == 1, 1.0, -1.0)[None, :]
    expected = [1.0 - lm.LooModel("rbf", X, Y, C, lms, gamma=0.25).loo_errors[0] / 600 for C in Cs]
    print("loo accuracy on overlapping blobs:", scores, "numpy:", expected)
    assert len(set(scores.tolist())) > 1 and np.all(scores < 1.0)
