"""GPU (-m gpu): the Nystrom preconditioner and PCG on a resident problem (lssvm_mi355_problem_build_preconditioner / _precond_landmarks / _precond_apply / _solve_pcg,
lssvm_mi355_solve_pcg_*).

The yardstick is numpy float64 (tests/pcg_model.py): the dense reduced matrix Abar and the dense P of the same landmarks.  The inputs are pcg_model.GPU_CASES, each shown
solvable in its dtype by tests/test_pcg_host.py: N in {300, 777, 1025} (no multiple of 128, one point past a tile edge), ranks 1 / 37 / 64 / 200 / 32 (rank + 1 on both
sides of 64), fp32 rbf on centred and scaled data (5 and 130 features) and on unscaled data (rbf_form = 1), fp64 rbf, fp64 polynomial on sqrt(gamma)-scaled data, fp32
polynomial, the exact-rank fp64 linear row, and once a landmark set that holds the last point.  eps: 1e-8 in fp64, 1e-4 in fp32.

  * operator: |P z / sigma - r| / |r| of z = precond_apply(r) against the float64 P is at most 8x what the model, run in the problem's dtype, leaves on the same r
    (the margin of 8 covers the order of the device's sums);
  * solve: |b - Abar x| <= 2 eps |b - Abar 1| in float64 (the factor of tests/test_gpu_cost_path.py), alpha_N = -sum x, rho consistent with alpha through the float64
    bias formula (as tests/test_gpu_parity.py: fp32 within 64 eps of the summands' scale, fp64 within 1e-12 of it);
  * it preconditions: at most half the iterations of the lssvm_mi355_cg_* solve of the same problem at the same eps (the model shows >= 4x); exact rank: <= 3;
  * the same call twice, NULL against the library's own landmarks given explicitly, three right-hand sides against three calls: the same bits;
  * every refusal of include/plssvm_amd.h; a plain CG solve after solve_pcg has the bits it had before; MI355CSVM(solver="pcg") on two and three classes.

Measured on an MI355X: the operator's device residual lay between 0.20x and 3.9x the model's (OPERATOR_MEASURED below), the PCG iteration counts within 4 of the model's
(SOLVE_MEASURED); it preconditions: rbf_777x5 float64 CG 156 / PCG 23; poly_777x16 float64 CG 88 / PCG 13; rbf_777x5 float32 CG 92 / PCG 10."""

import functools

import numpy as np
import pytest

import pcg_model as pm
from plssvm_amd import backend, multiclass
from plssvm_amd._capi import Options
from plssvm_amd.csvm import MI355CSVM, make_csvm
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in pm.GPU_CASES]
# what one run on an MI355X gave, for the record (the assertions are the bounds above, not these figures): name -> (device residual, model residual) of the operator
# test, and (PCG iterations on the device, in the model, true residual / eps)
OPERATOR_MEASURED = {
    "f32_rbf5": (4.776e-05, 2.52e-05),
    "f32_rbf130": (5.754e-07, 1.49e-07),
    "f32_rbf_direct": (1.644e-06, 1.974e-06),
    "f64_rbf": (2.155e-09, 3.74e-09),
    "f64_rbf_last": (8.209e-12, 4.121e-11),
    "f64_poly16": (3.703e-11, 9.729e-12),
    "f32_poly": (7.759e-06, 8.116e-06),
    "f64_linear": (3.118e-09, 1.296e-09),
}
SOLVE_MEASURED = {
    "f32_rbf5": (10, 10, 0.892),
    "f32_rbf130": (12, 12, 0.995),
    "f32_rbf_direct": (120, 116, 0.619),
    "f64_rbf": (75, 75, 0.961),
    "f64_rbf_last": (33, 33, 0.406),
    "f64_poly16": (15, 15, 0.278),
    "f32_poly": (14, 14, 0.906),
    "f64_linear": (2, 2, 0.0),
}


def parameter(p):
    return Parameter(kernel_type=p["kernel"], cost=p["cost"], gamma=p["kw"].get("gamma"), coef0=p["kw"].get("coef0", 0.0), degree=p["kw"].get("degree", 3))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, dense Abar, b, the model's preconditioner in the case's dtype): float64 numpy, computed once per case, shared, never modified."""
    p = pm.gpu_case(name)
    A = pm.reduced_matrix(p["kernel"], p["X"], p["cost"], **p["kw"])
    b = pm.reduced_rhs(p["y"])
    pc = pm.Preconditioner(p["kernel"], p["X"], p["cost"], p["landmarks"], dtype=p["dtype"], **p["kw"])
    for a in (A, b, p["X"], p["y"]):
        a.setflags(write=False)
    return p, A, b, pc


def problem(p):
    return backend.ResidentProblem(parameter(p), p["X"], options=Options(**p["options"]) if p["options"] else None)


@functools.lru_cache(maxsize=None)
def solved(name):
    """ONE build, apply and solve per case: (z of a fixed r, r, alpha, rho, info, landmarks read back, build info)."""
    p, A, b, pc = reference(name)
    r = np.random.default_rng(5).standard_normal(A.shape[0]).astype(p["dtype"])
    with problem(p) as prob:
        built = prob.build_preconditioner(landmarks=p["landmarks"])
        lm = prob.precond_landmarks()
        z = prob.precond_apply(r)
        alpha, rho, info = prob.solve_pcg(p["y"], p["eps"], 2000)
    return z, r, alpha, rho, info, lm, built


@pytest.mark.parametrize("name", NAMES)
def test_operator_against_the_dense_preconditioner(name):
    p, A, b, pc = reference(name)
    z, r, _, _, _, lm, built = solved(name)
    assert np.array_equal(lm, p["landmarks"]) and built["rank"] == len(p["landmarks"]) and built["jitter"] > 0.0
    device, model = pc.apply_residual(z, r), pc.apply_residual(pc.apply(r), r)
    print(f"operator {name}: device {device:.3e} model {model:.3e} ratio {device / model:.2f} jitter {built['jitter']:.2e} (model {pc.nu:.2e}) build {built['build_ms']:.1f} ms")
    assert np.all(np.isfinite(z))
    assert device <= 8.0 * model, (name, device, model)


@pytest.mark.parametrize("name", NAMES)
def test_solve_true_residual_and_rho(name):
    p, A, b, pc = reference(name)
    _, _, alpha, rho, info, _, _ = solved(name)
    x = np.asarray(alpha[:-1], dtype=np.float64)
    res = pm.true_residual(A, b, x)
    model_its = pm.solve(A, b, p["eps"], 2000, dtype=p["dtype"], precond=pc)[1]
    print(f"solve {name}: iterations {info['iterations']} (model {model_its}) true residual / eps {res / p['eps']:.3f} passes {info['gram_passes']} apply {info['apply_ms'] * 1e3:.1f} us")
    assert info["converged"] == 1 and info["rank"] == len(p["landmarks"]) and info["residuum"] <= info["target_residuum"]
    assert info["gram_passes"] == 1 + info["iterations"] + info["iterations"] // 50
    assert res <= 2.0 * p["eps"], (name, res)
    eps_t = float(np.finfo(p["dtype"]).eps)
    assert abs(float(alpha[-1]) + x.sum()) <= 4 * eps_t * np.abs(x).sum()
    rho_from_alpha, scale = pm.bias_rho(p["kernel"], p["X"], p["y"], p["cost"], x, **p["kw"])
    bound = 64 * eps_t * scale if p["dtype"] == np.float32 else 1e-12 * scale
    assert abs(float(rho) - rho_from_alpha) <= bound, (float(rho), rho_from_alpha, scale)


@pytest.mark.parametrize("name, dtype, eps", [("rbf_777x5", np.float64, 1e-8), ("poly_777x16", np.float64, 1e-8), ("rbf_777x5", np.float32, 1e-4)])
def test_it_preconditions(name, dtype, eps):
    t = pm.table_problem(name, dtype)
    prm = parameter(t)
    with backend.ResidentProblem(prm, t["X"]) as prob:
        prob.cg_begin(t["y"], eps)
        prob.cg_step(5000)
        _, _, cg = prob.cg_finish()
        prob.build_preconditioner(landmarks=t["landmarks"])
        alpha, _, pcg = prob.solve_pcg(t["y"], eps, 5000)
    print(f"it preconditions {name} {np.dtype(dtype).name}: CG {cg['iterations']} PCG {pcg['iterations']}")
    assert cg["converged"] == 1 and pcg["converged"] == 1
    assert 2 * pcg["iterations"] <= cg["iterations"], (cg["iterations"], pcg["iterations"])
    A = pm.reduced_matrix(t["kernel"], t["X"], t["cost"], **t["kw"])
    assert pm.true_residual(A, pm.reduced_rhs(t["y"]), alpha[:-1]) <= 2 * eps


def test_exact_rank_takes_at_most_three_iterations():
    assert solved("f64_linear")[4]["iterations"] <= 3


@pytest.mark.parametrize("name", ["f32_rbf5", "f64_poly16"])
def test_repeats_own_landmarks_and_several_right_hand_sides_are_bit_equal(name):
    p, A, b, pc = reference(name)
    rank = len(p["landmarks"])
    rng = np.random.default_rng(9)
    Y = np.stack([p["y"], np.where(rng.random(p["y"].size) < 0.5, -1, 1).astype(p["dtype"]), rng.standard_normal(p["y"].size).astype(p["dtype"])])
    r = rng.standard_normal(A.shape[0]).astype(p["dtype"])
    with problem(p) as prob:
        prob.build_preconditioner(rank)  # the library's own choice
        own = prob.precond_landmarks()
        assert len(set(own.tolist())) == rank and own.max() < p["X"].shape[0]
        z0, (a0, rho0, i0) = prob.precond_apply(r), prob.solve_pcg(Y[0], p["eps"], 2000)
        z1, (a1, rho1, i1) = prob.precond_apply(r), prob.solve_pcg(Y[0], p["eps"], 2000)  # the same calls twice
        assert np.array_equal(z0, z1) and np.array_equal(a0, a1) and rho0 == rho1 and i0["iterations"] == i1["iterations"] and i0["residuum"] == i1["residuum"]
        prob.build_preconditioner(landmarks=own)  # ... given explicitly: the same preconditioner
        assert np.array_equal(prob.precond_landmarks(), own)
        z2, (a2, rho2, _) = prob.precond_apply(r), prob.solve_pcg(Y[0], p["eps"], 2000)
        assert np.array_equal(z0, z2) and np.array_equal(a0, a2) and rho0 == rho2
        alphas, rhos, infos = prob.solve_pcg(Y, p["eps"], 2000)  # three right-hand sides in one call: the bits of three calls
        for c in range(3):
            a, rho, info = prob.solve_pcg(Y[c], p["eps"], 2000)
            assert np.array_equal(alphas[c], a) and rhos[c] == rho and infos[c]["iterations"] == info["iterations"]
    with problem(p) as again:  # the same landmarks for the same N, on another handle
        again.build_preconditioner(rank)
        assert np.array_equal(again.precond_landmarks(), own)
    # the one-shot entry point: the bits of the resident path
    a3, rho3, _ = backend.solve_pcg(parameter(p), p["X"], Y[0], p["eps"], 2000, rank=rank, options=Options(**p["options"]) if p["options"] else None)
    assert np.array_equal(a0, a3) and rho0 == rho3


def test_the_problem_is_left_as_it_was():
    p, A, b, pc = reference("f32_rbf130")

    def plain(prob):
        prob.cg_begin(p["y"], p["eps"])
        prob.cg_step(2000)
        return prob.cg_finish()

    with problem(p) as prob:
        a0, rho0, i0 = plain(prob)
        prob.build_preconditioner(landmarks=p["landmarks"])
        prob.solve_pcg(p["y"], p["eps"], 2000)
        a1, rho1, i1 = plain(prob)
        mv0 = prob.matvec(np.ones(A.shape[0], p["dtype"]), np.zeros(A.shape[0], p["dtype"]))
    assert np.array_equal(a0, a1) and rho0 == rho1 and i0["iterations"] == i1["iterations"] and i0["residuum"] == i1["residuum"]
    with problem(p) as fresh:
        assert np.array_equal(mv0, fresh.matvec(np.ones(A.shape[0], p["dtype"]), np.zeros(A.shape[0], p["dtype"])))


def test_every_refusal():
    p, A, b, pc = reference("f64_rbf_last")
    N = p["X"].shape[0]
    y = p["y"]
    with problem(p) as prob:
        for call in (lambda: prob.solve_pcg(y, 1e-6, 10), lambda: prob.precond_apply(np.ones(N - 1)), prob.precond_landmarks):
            with pytest.raises(InvalidParameterError, match="no preconditioner"):
                call()
        for rank in (0, N, 513):
            with pytest.raises(InvalidParameterError, match="rank of the preconditioner"):
                prob.build_preconditioner(rank)
        with pytest.raises(InvalidParameterError, match="distinct"):
            prob.build_preconditioner(landmarks=[3, 7, 3])
        with pytest.raises(InvalidParameterError, match="index of a data point"):
            prob.build_preconditioner(landmarks=[3, N])
        prob.build_preconditioner(landmarks=[0, N - 1])  # (the last point is allowed)
        with pytest.raises(InvalidParameterError, match="stopping criterion"):
            prob.solve_pcg(y, 0.0, 10)
        with pytest.raises(InvalidParameterError, match="CG iterations"):
            prob.solve_pcg(y, 1e-6, 0)
        with pytest.raises(InvalidParameterError, match="right hand side"):
            prob.solve_pcg(y[:-1], 1e-6, 10)
        with pytest.raises(InvalidParameterError, match="Sizes mismatch"):
            prob.precond_apply(np.ones(N))
        # weights set on the problem
        prob.set_weights(np.full(N, 2.0))
        for call in (lambda: prob.solve_pcg(y, 1e-6, 10), lambda: prob.build_preconditioner(4), lambda: prob.precond_apply(np.ones(N - 1))):
            with pytest.raises(InvalidParameterError, match="weights"):
                call()
        prob.set_weights(None)
        # between cg_begin and cg_finish
        prob.cg_begin(y, 1e-6)
        for call in (lambda: prob.solve_pcg(y, 1e-6, 10), lambda: prob.build_preconditioner(4), lambda: prob.precond_apply(np.ones(N - 1))):
            with pytest.raises(InvalidParameterError, match="between cg_begin and cg_finish"):
                call()
        prob.cg_step(1)
        prob.cg_finish()
        # max_iter reached: the iterate comes back, not converged
        _, _, info = prob.solve_pcg(y, 1e-12, 2)
        assert info["converged"] == 0 and info["iterations"] == 2
    # several shards (two on the one device, as tests/test_gpu_parity.py builds them)
    with backend.ResidentProblem(parameter(p), p["X"], devices=[0, 0]) as shard:
        with pytest.raises(InvalidParameterError, match="one device and one rank"):
            shard.build_preconditioner(4)
        with pytest.raises(InvalidParameterError, match="one device and one rank"):
            shard.solve_pcg(y, 1e-6, 10)
    with pytest.raises(InvalidParameterError, match="one device"):
        MI355CSVM(num_devices=0, solver="pcg").solve_system_of_linear_equations(parameter(p), p["X"], y, 1e-6, 10)
    with pytest.raises(InvalidParameterError, match="unweighted"):
        MI355CSVM(solver="pcg").solve_system_of_linear_equations(parameter(p), p["X"], y, 1e-6, 10, sample_weight=np.ones(N))


@pytest.mark.parametrize("classes", [2, 3])
def test_csvm_with_the_pcg_solver_fits_and_predicts(classes):
    rng = np.random.default_rng(11)
    centres = rng.uniform(-1, 1, (classes, 6)) * 2.0
    labels = np.arange(301) % classes
    X = centres[labels] + 0.35 * rng.standard_normal((301, 6))
    if classes == 2:
        data = DataSet(X, [int(v) for v in labels])
        svm, plain = make_csvm("mi355", solver="pcg", precond_rank=37, kernel_type="rbf", cost=10.0), MI355CSVM(kernel_type="rbf", cost=10.0)
        model = svm.fit(data, epsilon=1e-8)
        assert svm.last_cg_info["converged"] == 1 and svm.last_cg_info["rank"] == 37
        assert svm.score(model) >= 0.97
        assert svm.predict(model, data) == plain.predict(plain.fit(data, epsilon=1e-8), data)
    else:
        svm = MI355CSVM(solver="pcg", precond_rank=37, kernel_type="rbf", cost=10.0)
        model = multiclass.fit_one_vs_all(svm, svm.params, X, labels, np.arange(classes), 1e-8)
        assert model.alpha.shape == (3, 301) and all(i["converged"] == 1 and i["rank"] == 37 for i in model.infos)
        assert len({i["build_ms"] for i in model.infos}) == 1  # ONE preconditioner for the three right-hand sides
        A = pm.reduced_matrix("rbf", X, 10.0, gamma=model.params.gamma)
        B = multiclass.one_vs_all_targets(np.arange(classes), labels, X.dtype)
        for c in range(classes):
            assert pm.true_residual(A, pm.reduced_rhs(B[c]), model.alpha[c][:-1]) <= 2e-8
        predicted = multiclass.predict_classes(model.classes, multiclass.decision_values(svm, model, X))
        assert np.mean(predicted == labels) >= 0.97
