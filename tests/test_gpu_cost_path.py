"""GPU (-m gpu): the cost path, lssvm_mi355_problem_solve_cost_path / lssvm_mi355_solve_cost_path_* -- every cost of a grid from one multi-shift CG sequence
(DESIGN.md section 10).

The yardstick is numpy float64 (tests/cost_path_model.py): the dense reduced system Abar(1 / C) of every cost, built from the data as the device holds it (rounded to
the problem's dtype).  The inputs are those of tests/test_cost_path_host.py, where the numpy model of the recurrences meets |P (b - Abar x)| <= eps |P b| at every
cost: that is the precondition of the bound asserted here.  Per cost, with x = alpha[:n], z = P^-1 x and the norms of float64 numpy:
  * converged == verified == 1;
  * |P (b - Abar x)| <= 2 eps |P b|: the model's own bound is eps; the factor 2 is for the order of the device's sums and the rounding of the Gram pass, the same
    factor and reasoning as tests/test_gpu_refined.py;
  * |z - z*| / |z*| <= 2 eps kappa_2(P Abar P), the standard residual bound (P Abar P z = P b);
  * alpha[n] = -sum x and rho = -(y_N + (k_NN + 1 / C) sum x - q.x): float64 to 1e-12 of the summands' scale, float32 to 8 epsilon of it;
  * true_residuum (the device's own evaluation) within a factor 4 of numpy's.
Shapes: 130 points = two row blocks with a ragged last one, 700 = six; 20 features = a ragged feature chunk; 700 x 200 float32 = the one-pass split kernels beyond 128
features (two costs per verification pass), 700 x 300 float64 = the feature-panel kernel -- every kernel family runs the path."""

import functools

import numpy as np
import pytest

import cost_path_model as cpm
from plssvm_amd import backend, svc
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter
from test_cost_path_host import COSTS, costs_of, path_inputs

pytestmark = pytest.mark.gpu

KERNELS = ["linear", "polynomial", "rbf"]
CASES = [(N, 20, dtype) for N in (130, 700) for dtype in (np.float64, np.float32)] + [(700, 200, np.float32), (700, 300, np.float64)]
EPS = {np.float64: 1e-9, np.float32: 1e-3}


@functools.lru_cache(maxsize=None)
def dense(N, d, kernel, dtype):
    """(K, q, k_ll, b, y_last, |P b|, kappa per cost) in float64 of the data rounded to dtype: computed once per case, shared, never modified."""
    X, y = path_inputs(N, d)
    K, q, k_ll, b, y_last = cpm.reduced_parts(cpm.kernel_matrix(kernel, X.astype(dtype)), y)
    kappa = cpm.condition_numbers(K, q, k_ll, costs_of(kernel, dtype, d))
    for a in (K, q, b, kappa):
        a.setflags(write=False)
    return K, q, k_ll, b, y_last, float(np.linalg.norm(cpm.apply_P(b))), kappa


@functools.lru_cache(maxsize=None)
def solved(N, d, kernel, dtype):
    """ONE verified path per case on a resident problem: (alphas, rhos, infos, passes, whether the problem has a two-vector pass)."""
    X, y = path_inputs(N, d)
    with backend.ResidentProblem(Parameter(kernel_type=kernel), X.astype(dtype)) as prob:
        alphas, rhos, infos, passes = prob.solve_cost_path(y, costs_of(kernel, dtype, d), EPS[dtype], 2000)
        zero = np.zeros(N - 1, dtype)
        two_vector = prob.matvec_pair(zero, zero, zero, zero)[2]
    alphas.setflags(write=False)
    return alphas, rhos, infos, passes, two_vector


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("N,d,dtype", CASES)
def test_every_cost_meets_the_stop_test_in_the_true_residual(N, d, dtype, kernel):
    K, q, k_ll, b, y_last, norm_b, kappa = dense(N, d, kernel, dtype)
    alphas, rhos, infos, passes, two_vector = solved(N, d, kernel, dtype)
    costs, eps, n = costs_of(kernel, dtype, d), EPS[dtype], N - 1
    assert alphas.dtype == dtype and alphas.shape == (len(costs), N) and np.all(np.isfinite(alphas)) and np.all(np.isfinite(rhos))
    for s, cost in enumerate(costs):
        x = alphas[s, :n].astype(np.float64)
        res = cpm.true_residual_norm(K, q, k_ll, b, cost, x)
        z, z_star = cpm.apply_P_inv(x), cpm.apply_P_inv(cpm.dense_solve(K, q, k_ll, b, cost))
        err = np.linalg.norm(z - z_star) / np.linalg.norm(z_star)
        info = infos[s]
        print(f"  {kernel} {N} x {d} {np.dtype(dtype).name} C {cost:g}: its {info['iterations']}  |P res| / |P b| {res / norm_b:.2e} (<= {2 * eps:.0e})  |z - z*| / |z*| {err:.2e} "
              f"(<= {2 * eps * kappa[s]:.2e})  true_residuum {info['true_residuum']:.3e} (numpy {res * res:.3e})")
        assert info["converged"] == 1 and info["verified"] == 1, info
        assert res <= 2.0 * eps * norm_b, (cost, res / norm_b)
        assert err <= 2.0 * eps * kappa[s], (cost, err, kappa[s])
        # the epilogue of the reduced solution
        sigma = 1.0 / cost
        sx, qx = x.sum(), q @ x
        scale = abs(y_last) + (k_ll + sigma) * np.abs(x).sum() + np.abs(q * x).sum()
        tol = 1e-12 if dtype == np.float64 else 8 * np.finfo(np.float32).eps
        assert abs(float(alphas[s, n]) + sx) <= tol * np.abs(x).sum(), (alphas[s, n], -sx)
        assert abs(float(rhos[s]) + (y_last + (k_ll + sigma) * sx - qx)) <= tol * scale, (float(rhos[s]), -(y_last + (k_ll + sigma) * sx - qx))
        # the report
        assert info["target_residuum"] == pytest.approx(eps * eps * info["initial_residuum"], rel=1e-12)
        assert info["initial_residuum"] == pytest.approx(norm_b * norm_b, rel=1e-12 if dtype == np.float64 else 1e-6)
        assert info["residuum"] <= info["target_residuum"]
        assert res * res / 4.0 <= info["true_residuum"] <= 4.0 * res * res, (info["true_residuum"], res * res)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("N,d,dtype", CASES)
def test_pass_counts_and_freeze_order(N, d, dtype, kernel):
    _, _, infos, passes, two_vector = solved(N, d, kernel, dtype)
    costs = costs_of(kernel, dtype, d)
    its = np.array([info["iterations"] for info in infos])
    assert passes[0] == its.max() == its[int(np.argmax(costs))]  # one Gram pass per iteration of the seed, the largest cost
    assert passes[1] == ((len(costs) + 1) // 2 if two_vector else len(costs))
    assert np.all(np.diff(its[np.argsort(costs)]) >= 0)  # a frozen cost's iterations are non-decreasing in C
    if dtype == np.float64 and d == 20:
        assert two_vector  # (lssvm_mi355_problem_matvec_pair's routing, which the verification shares: the float64 cases of 20 features do have a two-vector pass)


def test_every_kernel_family_ran():
    """700 x 200 float32 runs the one-pass split kernels beyond 128 features, 700 x 300 float64 the feature-panel kernel (one launch per panel for the linear kernel)."""
    X, y = path_inputs(700, 300)
    with backend.ResidentProblem(Parameter(kernel_type="linear"), X) as prob:
        prob.solve_cost_path(y, [1.0], 1e-9, 5, verify=False)
        assert prob.info()["tile_launches_per_matvec"] == 3
    X, y = path_inputs(700, 200)
    with backend.ResidentProblem(Parameter(kernel_type="rbf"), X.astype(np.float32)) as prob:
        _, _, _, passes = prob.solve_cost_path(y, [1.0, 2.0], 1e-30, 5, verify=False)
        assert prob.info()["gram_mode"] in (1, 2) and passes == (5, 0)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exact_properties(dtype, kernel):
    """Bit-equal repeats, permuted and duplicated costs, max_iter; the one-shot entry point gives the resident call's bits."""
    N, d = 130, 20
    X, y = path_inputs(N, d)
    X, eps, costs = X.astype(dtype), EPS[dtype], costs_of(kernel, dtype, d)
    base = solved(N, d, kernel, dtype)
    prm = Parameter(kernel_type=kernel, cost=123.0)  # (the problem's own cost is ignored)
    again = backend.solve_cost_path(prm, X, y, costs, eps, 2000)
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1]) and again[2] == base[2] and again[3] == base[3]
    with backend.ResidentProblem(prm, X) as prob:
        perm = [2, 0, 1] if len(costs) == 3 else [3, 0, 4, 2, 1]
        a, r, infos, _ = prob.solve_cost_path(y, [costs[k] for k in perm], eps, 2000)
        for row, k in enumerate(perm):
            assert np.array_equal(a[row], base[0][k]) and r[row] == base[1][k] and infos[row] == base[2][k]
        a, r, infos, passes = prob.solve_cost_path(y, [costs[0], costs[1], costs[0]], eps, 2000)
        assert np.array_equal(a[0], a[2]) and r[0] == r[2] and infos[0] == infos[2]  # (another grid, another seed: not the bits of `base`)
        # max_iter: unconverged rows with finite values, and no verification asked for
        a, r, infos, passes = prob.solve_cost_path(y, costs, 1e-30, 3, verify=False)
        assert passes == (3, 0) and np.all(np.isfinite(a)) and np.all(np.isfinite(r))
        assert all(i["converged"] == 0 and i["verified"] == 0 and i["iterations"] == 3 and i["true_residuum"] == -1.0 and np.isfinite(i["residuum"]) for i in infos)
        # the problem is left as it was: a solve of the recipe on the same handle has the bits of a fresh one
        prob.cg_begin(y, eps)
        prob.cg_step(2000)
        alpha, rho, _ = prob.cg_finish()
    fresh = backend.solve_system_of_linear_equations(prm, X, y, eps, 2000)
    assert np.array_equal(alpha, fresh[0]) and rho == fresh[1]


def test_rejected_on_a_weighted_problem_and_in_mid_cg():
    X, y = path_inputs(130)
    with backend.ResidentProblem(Parameter(kernel_type="rbf"), X) as prob:
        prob.set_weights(np.full(130, 2.0))
        with pytest.raises(InvalidParameterError, match="weights"):
            prob.solve_cost_path(y, COSTS, 1e-9, 100)
        prob.set_weights(None)
        assert all(i["converged"] == 1 for i in prob.solve_cost_path(y, COSTS, 1e-9, 1000)[2])
        prob.cg_begin(y, 1e-9)
        with pytest.raises(InvalidParameterError, match="between cg_begin and cg_finish"):
            prob.solve_cost_path(y, COSTS, 1e-9, 100)
        prob.cg_step(1)
        with pytest.raises(InvalidParameterError, match="between cg_begin and cg_finish"):
            prob.solve_cost_path(y, COSTS, 1e-9, 100)
        prob.cg_finish()
        assert all(i["converged"] == 1 for i in prob.solve_cost_path(y, COSTS, 1e-9, 1000)[2])


@pytest.mark.parametrize("kernel", KERNELS)
def test_fit_cost_path_models_predict_as_models_fitted_one_by_one(kernel):
    X, y = path_inputs(300)
    Xv, _ = path_inputs(200, seed=8)
    data, points = DataSet(X, y.tolist()), DataSet(Xv)
    models = MI355CSVM(params=Parameter(kernel_type=kernel)).fit_cost_path(data, COSTS, epsilon=1e-9)
    assert [m.params.cost for m in models] == COSTS
    for model, cost in zip(models, COSTS):
        svm = MI355CSVM(params=Parameter(kernel_type=kernel, cost=cost))
        one = svm.fit(data, epsilon=1e-9)
        assert svm.predict(model, points) == svm.predict(one, points) and svm.predict(model, data) == svm.predict(one, data)


@pytest.mark.parametrize("num_classes", [2, 3])
def test_svc_cost_path(num_classes):
    X, y = path_inputs(300)
    Xv, yv = path_inputs(200, seed=8)
    if num_classes == 3:
        y, yv = np.arange(300) % 3, np.arange(200) % 3
    est = svc.SVC(kernel="rbf", tol=1e-9)
    fitted = svc.fit_cost_path(est, X, y, COSTS)
    one_by_one = [svc.SVC(kernel="rbf", C=cost, tol=1e-9).fit(X, y) for cost in COSTS]
    for f, one in zip(fitted, one_by_one):
        assert f.C == one.C and np.array_equal(f.predict(Xv), one.predict(Xv))
    if num_classes == 2:
        scores, _ = svc.cost_path_scores(est, X, y, COSTS, Xv, yv)
        assert scores.tolist() == [one.score(Xv, yv) for one in one_by_one]


def test_one_vs_all_paths_run_on_one_resident_problem(monkeypatch):
    """Three classes: ONE problem is created for the three right-hand sides (the data uploaded and prepared once), no one-shot path runs, and every class's rows are the
    bits of a one-shot path for that class."""
    X, _ = path_inputs(130)
    B = np.stack([np.where(np.arange(130) % 3 == c, 1.0, -1.0) for c in range(3)])
    prm = Parameter(kernel_type="rbf").resolved(20)
    one_shot = [backend.solve_cost_path(prm, X, b, COSTS, 1e-9, 1000) for b in B]
    created = []

    class Counted(backend.ResidentProblem):
        def __init__(self, *args, **kwargs):
            created.append(self)
            super().__init__(*args, **kwargs)

    def one_shot_must_not_run(*args, **kwargs):
        raise AssertionError("a one-shot path per class uploads and prepares the data again")

    monkeypatch.setattr(backend, "ResidentProblem", Counted)
    monkeypatch.setattr(backend, "solve_cost_path", one_shot_must_not_run)
    solved = MI355CSVM(params=prm).solve_cost_paths(prm, X, B, COSTS, 1e-9, 1000)
    assert len(created) == 1 and len(solved) == 3
    for (alphas, rhos, infos), (alphas1, rhos1, infos1, passes1) in zip(solved, one_shot):
        assert np.array_equal(alphas, alphas1) and np.array_equal(rhos, rhos1)
        assert [i["iterations"] for i in infos] == [i["iterations"] for i in infos1] and all(i["verified"] == 1 and i["path_passes"] == passes1 for i in infos)
    fitted = svc.fit_cost_path(svc.SVC(kernel="rbf", tol=1e-9, max_iter=1000), X, np.arange(130) % 3, COSTS)
    assert len(created) == 2  # (one more problem for the whole one-vs-all fit, not one per class)
    for s, f in enumerate(fitted):
        assert np.array_equal(f.dual_coef_, np.stack([c[0][s] for c in solved]))

