"""GPU (-m gpu): the dense SPD toolbox on the device and the device-factored fixed-size fits (lssvm_mi355_dense_*, lssvm_mi355_problem_fit_reduced_dev / _loo_dev,
factor="device" on backend, ResidentProblem, MI355CSVM and svc).  The bounds are the derived ones of tests/dense_model.py (Higham, Accuracy and
Stability, Thm 10.3, 10.4 and sections 14.2 - 14.3); tests/test_dense_host.py shows the numpy yardstick to stay within them on the same inputs.

Toolbox.  The three aids at m in dense_model.sizes(B) x cond in {1e2, 1e10} and on M + nu I of the rbf_777x5 fit case at rank 64; NaN above the diagonal of the input
changes no bit of L.  Status: a planted negative diagonal entry is reported as 1 + its column, the call returns, and the next call is right.  Bit equality of repeats and
of column c of a k = 3 solve with the single-column solve.
Fit.  The checks of test_fit_against_the_model, test_every_point_a_landmark_is_the_full_solution and test_linear_kernel_with_enough_landmarks_is_the_full_solution of
tests/test_gpu_reduced.py and of test_fit_against_the_model and test_device_loo_against_brute_force_refits of tests/test_gpu_reduced_loo.py under THEIR bounds with
factor="device", the bit equalities the header promises, ranks 2 B + 1 and 1 024 against the solve bound, and the default path left as it was."""

import numpy as np
import pytest

import dense_model as dm
import pcg_model as pm
import reduced_loo_model as lm
import reduced_model as rm
import test_gpu_reduced as tr
import test_gpu_reduced_loo as tl
from plssvm_amd import _capi, backend

pytestmark = pytest.mark.gpu

B = _capi.DENSE_BLOCK
EPS64 = dm.EPS64

# what one run on an MI355X gave, for the record (the assertions are the bounds of tests/dense_model.py and of the restated tests, not these figures)
MEASURED = {
    "toolbox, largest ratio to the bounds (factorisation, solve, inverse)": {"cond 1e2": (0.105, 0.037, 0.083), "cond 1e10": (0.054, 0.026, 0.016), "M + nu I of rbf_777x5": (0.022, 0.001, 0.004)},
    "fit: |f_device - f_full| and the tolerance": {"all landmarks float64": (1.26e-09, 3.01e-06), "linear float64, on the range of Phi": (1.48e-13, 2.45e-12)},
    "rank 1024, N = 1100: launches, assemble / factor / solve / invert ms of one cost": (79, 0.008, 2.11, 0.76, 1.21),
    "rank 129: the same": (14, 0.007, 0.285, 0.067, 0.134),
}


def check_toolbox(A, nu, label):
    """The three aids on A + nu I: the three bounds, exact zeros above the diagonals.  Returns the three ratios."""
    m = A.shape[0]
    L, status, _ = dm.device_cholesky(A, nu)
    assert status == 0 and np.all(np.isfinite(L)), (label, status)
    assert np.array_equal(np.triu(L, 1), np.zeros((m, m))), label
    Bm = dm.right_hand_sides(m, 3)
    X, _ = dm.device_solve(L, Bm)
    V, _ = dm.device_invert_lower(L)
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(V)) and np.array_equal(np.triu(V, 1), np.zeros((m, m))), label
    ratios = (dm.factor_ratio(A, nu, L), dm.solve_ratio(A, nu, L, Bm, X), dm.inverse_ratio(L, V)[0])
    assert all(r <= 1.0 for r in ratios), (label, ratios, dm.inverse_ratio(L, V))
    return ratios


@pytest.mark.parametrize("cond", dm.CONDS)
def test_toolbox_against_the_bounds(cond):
    worst = [0.0, 0.0, 0.0]
    for m in dm.sizes(B):
        ratios = check_toolbox(dm.spd_matrix(m, cond), 0.0, (m, cond))
        worst = [max(w, r) for w, r in zip(worst, ratios)]
    print(f"toolbox, cond {cond:g}: factorisation {worst[0]:.3f}, solve {worst[1]:.3f}, inverse {worst[2]:.3f} of the bounds")


def reduced_matrix(G, Kmm, m, N, cost, nu):
    """M + nu I and the right-hand sides of the fit, in numpy, from landmark_gram's output; and the scale of the three roundings of an assembled entry."""
    S, s = G[:m, :m], G[m, :m]
    M = S - np.outer(s, s) / N + Kmm / cost
    scale = np.abs(S) + np.outer(np.abs(s), np.abs(s)) / N + np.abs(Kmm) / cost + nu
    rhs = np.stack([G[m + 1 + c, :m] - s * G[m + 1 + c, m] / N for c in range(G.shape[0] - m - 1)])
    return np.tril(M) + np.tril(M, -1).T, rhs, scale


def test_toolbox_on_the_matrix_of_a_fit():
    p, model, _ = tr.fit_reference("rbf_777x5", np.float64, 1)
    with backend.ResidentProblem(tr.parameter(p["kernel"], p["kw"], p["cost"]), p["X"]) as prob:
        G = prob.landmark_gram(p["Y"][0], 64, landmarks=p["landmarks"])
    XL = p["X"][p["landmarks"].astype(np.int64)]
    M, _, _ = reduced_matrix(G, pm.kernel_matrix(p["kernel"], XL, XL, **p["kw"]), 64, 777, p["cost"], model.nu)
    ratios = check_toolbox(M, model.nu, "rbf_777x5")
    print(f"toolbox on M + nu I of rbf_777x5: factorisation {ratios[0]:.3f}, solve {ratios[1]:.3f}, inverse {ratios[2]:.3f} of the bounds")


@pytest.mark.parametrize("m", [17, 2 * B + 1, 300])
def test_what_stands_above_the_diagonal_is_never_read(m):
    A = dm.spd_matrix(m, 1e2)
    garbage = A.copy()
    garbage[np.triu_indices(m, 1)] = np.nan
    L, status, _ = dm.device_cholesky(A)
    L2, status2, _ = dm.device_cholesky(garbage)
    assert status == status2 == 0 and np.array_equal(L, L2)


@pytest.mark.parametrize("j", [0, B - 1, B, 299])
def test_a_bad_pivot_is_reported_and_the_next_call_is_right(j):
    L, status, _ = dm.device_cholesky(dm.indefinite(300, j))
    assert status == j + 1 and np.all(np.isfinite(L))
    good = dm.spd_matrix(300, 1e2)
    L, status, _ = dm.device_cholesky(good)  # the status word does not outlive the attempt
    assert status == 0 and dm.factor_ratio(good, 0.0, L) <= 1.0


def test_repeats_and_columns_of_the_aids_are_bit_equal():
    m = 2 * B + 1
    A = dm.spd_matrix(m, 1e10)
    L, _, _ = dm.device_cholesky(A)
    assert np.array_equal(L, dm.device_cholesky(A)[0])
    Bm = dm.right_hand_sides(m, 3)
    X = dm.device_solve(L, Bm)[0]
    assert np.array_equal(X, dm.device_solve(L, Bm)[0])
    for c in range(3):
        assert np.array_equal(X[c], dm.device_solve(L, Bm[c])[0][0]), c
    V = dm.device_invert_lower(L)[0]
    assert np.array_equal(V, dm.device_invert_lower(L)[0])


# ---------------------------------------------------------------- the fit ----------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", [c[0] for c in rm.FIT_CASES])
def test_fit_against_the_model(name, dtype, k):
    p, model, e = tr.fit_reference(name, dtype, k)
    betas, rhos, used, info = tr.fit_on_device(p, factor="device")
    host = tr.fit_on_device(p)
    assert np.array_equal(used, p["landmarks"]) and info["rank"] == 64 and info["slabs"] == 1 and info["block"] == B
    assert np.asarray(betas).dtype == np.float64 and np.asarray(betas).shape == ((3, 64) if k == 3 else (64,))
    f = model.decision_values(p["points"])
    g = model.decision_values(p["points"], betas, rhos)
    tol = rm.fit_tolerance(model, e, f)
    diff = float(np.max(np.abs(f - g)))
    print(f"device-factored fit {name} {np.dtype(dtype).name} k={k}: |f_device - f_model| {diff:.2e}, tolerance {tol:.2e}, jitter {info['jitter']:.2e}, "
          f"{info['launches']} launches, assemble / factor / solve {info['assemble_ms']:.3f} / {info['factor_ms']:.3f} / {info['solve_ms']:.3f} ms")
    assert diff <= tol, (name, diff, tol)
    assert info["attempts"] == 1 and info["jitter"] == host[3]["jitter"]  # (no retry on either side: the host path's bits)
    assert info["invert_ms"] == 0.0 and info["launches"] > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_point_a_landmark_is_the_full_solution(dtype):
    p, model, e = tr.fit_reference("rbf_200x4", dtype, 1)
    betas, rhos, _, info = tr.fit_on_device(p, factor="device")
    full = rm.dense_full_solution(p["kernel"], p["X"], p["Y"][0], p["cost"], p["points"], held=p["held"], **p["kw"])
    g = model.decision_values(p["points"], betas, rhos)[0]
    tol = rm.fit_tolerance(model, e, full)
    diff = float(np.max(np.abs(full - g)))
    print(f"device-factored, all landmarks {np.dtype(dtype).name}: |f_device - f_full| {diff:.2e}, tolerance {tol:.2e}, jitter {info['jitter']:.2e}, attempts {info['attempts']}")
    assert info["rank"] == 200 and 1 <= info["attempts"] <= 7 and diff <= tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_linear_kernel_with_enough_landmarks_is_the_full_solution(dtype):
    p, model, e = tr.fit_reference("linear_300x6", dtype, 1)
    betas, rhos, _, info = tr.fit_on_device(p, factor="device")
    full = rm.dense_full_solution(p["kernel"], p["X"], p["Y"][0], p["cost"], p["points"], **p["kw"])
    g = model.decision_values(p["points"], betas, rhos)[0]
    diff = float(np.max(np.abs(full - g)))
    print(f"device-factored, linear {np.dtype(dtype).name}: |f_device - f_full| {diff:.2e}, tolerance {rm.fit_tolerance(model, e, full):.2e}, on the range of Phi "
          f"{rm.range_tolerance(model, e, full):.2e}, attempts {info['attempts']} (numpy {model.retries + 1})")
    assert diff <= rm.fit_tolerance(model, e, full) and diff <= rm.range_tolerance(model, e, full)
    # M is singular by construction: the retry count may differ from the host's, the rule may not
    assert 1 <= info["attempts"] <= 7
    first = model.nu / 10.0 ** model.retries  # eps64 trace(M)
    assert abs(info["jitter"] / (first * 10.0 ** (info["attempts"] - 1)) - 1.0) <= 1e-6


# ---------------------------------------------------------------- leave-one-out ----------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", [c[0] for c in rm.FIT_CASES])
def test_loo_fit_against_the_model(name, dtype, k):
    p, per_cost = tl.fit_reference(name, dtype, k)
    Y = p["Y"] if k > 1 else p["Y"][0]
    with backend.ResidentProblem(tl.parameter(p["kernel"], p["kw"], 3.0), p["X"]) as prob:  # (the problem's own cost plays no part)
        assert p["held"][0] is p["X"] or prob.info()["rbf_direct"] == 0
        betas, rhos, used, report = prob.fit_reduced_loo(Y, 64, lm.FIT_COSTS, landmarks=p["landmarks"], factor="device")
    assert np.array_equal(used, p["landmarks"]) and np.array_equal(report["costs"], lm.FIT_COSTS)
    assert betas.shape == ((3, 3, 64) if k == 3 else (3, 64)) and report["leverage"].shape == (3, 777) and report["loo"].shape == ((3, 3, 777) if k == 3 else (3, 777))
    for s, (model, e) in enumerate(per_cost):
        for what, got, ref in (("h", report["leverage"][s], model.h), ("f", np.atleast_2d(report["fitted"][s]), model.f), ("loo", np.atleast_2d(report["loo"][s]), model.loo)):
            tol = lm.tolerance(model, e, np.max(np.abs(ref)))
            diff = float(np.max(np.abs(got - ref)))
            print(f"device-factored loo fit {name} {np.dtype(dtype).name} k={k} C={lm.FIT_COSTS[s]:g} {what}: |device - model| {diff:.2e}, tolerance {tol:.2e}")
            assert diff <= tol, (name, what, s, diff, tol)
        info = report["infos"][s]
        assert abs(report["jitter"][s] / model.nu - 1.0) <= 1e-6 and info["cost"] == lm.FIT_COSTS[s] and info["attempts"] == 1 and info["block"] == B and info["invert_ms"] > 0.0
        assert np.all(report["leverage"][s] > 1.0 / 777) and np.all(report["leverage"][s] < 1.0)
        # the coefficients of cost s: the bits of the device-factored fit_reduced on a problem created with that cost
        with backend.ResidentProblem(tl.parameter(p["kernel"], p["kw"], lm.FIT_COSTS[s]), p["X"]) as at_cost:
            b1, r1, _, _ = at_cost.fit_reduced(Y, 64, landmarks=p["landmarks"], factor="device")
        assert np.array_equal(betas[s], b1) and np.array_equal(rhos[s], r1), (name, s)
    tl.check_report_against_its_arrays(p["Y"], report)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_loo_against_brute_force_refits(dtype):
    p = lm.identity_case("rbf_255x5", dtype)
    with backend.ResidentProblem(tl.parameter(p["kernel"], p["kw"], 1.0), p["X"]) as prob:
        assert p["held"][0] is p["X"] or prob.info()["rbf_direct"] == 0
        _, _, _, report = prob.fit_reduced_loo(p["Y"][0], 16, lm.IDENTITY_COSTS, landmarks=p["landmarks"], factor="device")
    for s, cost in enumerate(lm.IDENTITY_COSTS):
        model = lm.LooModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], held=p["held"], **p["kw"])
        e = lm.e_loo(model, lm.stable(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], held=p["held"], **p["kw"])[2])
        brute = lm.brute_force(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], held=p["held"], **p["kw"])[0]
        tol = lm.tolerance(model, e, np.max(np.abs(model.f)))
        diff = float(np.max(np.abs(report["loo"][s] - brute)))
        print(f"device-factored brute force {np.dtype(dtype).name} C={cost:g}: |loo_device - refits| {diff:.2e}, tolerance {tol:.2e}")
        assert diff <= tol, (cost, diff, tol)
    tl.check_report_against_its_arrays(p["Y"], report)


def test_loo_repeats_columns_and_costs_are_bit_equal():
    p, _ = tl.fit_reference("rbf_777x5", np.float64, 3)
    costs = lm.FIT_COSTS
    with backend.ResidentProblem(tl.parameter(p["kernel"], p["kw"], 5.0), p["X"]) as prob:
        full = prob.fit_reduced_loo(p["Y"], 64, costs, factor="device")
        assert tl.same(full, prob.fit_reduced_loo(p["Y"], 64, costs, factor="device"))
        b3, r3, _, rep3 = full
        for c in range(3):  # column c of the k = 3 call: the bits of the single call
            b1, r1, _, rep1 = prob.fit_reduced_loo(p["Y"][c], 64, costs, factor="device")
            assert np.array_equal(rep1["leverage"], rep3["leverage"]) and np.array_equal(b3[:, c], b1) and np.array_equal(r3[:, c], r1)
            for n in ("fitted", "loo", "press", "loo_errors"):
                assert np.array_equal(rep3[n][:, c], rep1[n]), (c, n)
        for s, cost in enumerate(costs):  # cost s of the grid: the bits of the one-cost call
            b, r, _, rep = prob.fit_reduced_loo(p["Y"], 64, [cost], factor="device")
            assert np.array_equal(b[0], b3[s]) and np.array_equal(r[0], r3[s])
            for n in ("leverage", "fitted", "loo", "press", "loo_errors", "max_leverage", "jitter"):
                assert np.array_equal(rep[n][0], rep3[n][s]), (s, n)
    one_shot = backend.fit_reduced_loo(tl.parameter(p["kernel"], p["kw"], 5.0), p["X"], p["Y"], 64, costs, factor="device")
    assert tl.same(one_shot, full)


# ---------------------------------------------------------------- past one block and at the cap ----------------------------------------------------------------
@pytest.mark.parametrize("rank", [2 * B + 1, rm.MAX_RANK])
def test_past_one_block_and_at_the_cap(rank):
    N, costs = 1100, [1.0, 100.0]
    X, y = pm.make_data(N, 3, pm.DATA_SEED, np.float64)
    lms = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
    kw = tr.KERNELS["rbf"]
    with backend.ResidentProblem(tr.parameter("rbf", kw, 10.0), X) as prob:
        betas, rhos, _, report = prob.fit_reduced_loo(y, rank, costs, landmarks=lms, factor="device")
        G = prob.landmark_gram(y, rank, landmarks=lms)
    assert np.all(np.isfinite(betas)) and np.all(np.isfinite(rhos)) and np.all(np.isfinite(report["leverage"])) and np.all(np.isfinite(report["loo"]))
    XL = X[lms.astype(np.int64)]
    Kmm = pm.kernel_matrix("rbf", XL, XL, **kw)
    for s, cost in enumerate(costs):
        info = report["infos"][s]
        assert 1 <= info["attempts"] <= 7 and info["rank"] == rank
        nu = info["jitter"]
        M, rhs, scale = reduced_matrix(G, Kmm, rank, N, cost, nu)
        # L only scales the bound (|L||L^T| >= |M + nu I| entry by entry) and comes from numpy alone: where numpy's own factorisation of the numpy-assembled matrix needs
        # it, with a slightly larger shift -- the device factored its own assembly, which differs from this one by roundings
        L = None
        for shift in (nu, 2.0 * nu, 4.0 * nu, 8.0 * nu):
            try:
                L = np.linalg.cholesky(M + shift * np.eye(rank))
                break
            except np.linalg.LinAlgError:
                continue
        assert L is not None, f"numpy could not factor M + nu I at rank {rank}, C={cost:g} with a shift up to 8 nu = {8.0 * nu:.2e}: no independent scale for the bound"
        extra = 4.0 * EPS64 * (np.abs(betas[s])[None, :] @ scale.T)
        ratio = dm.solve_ratio(M, nu, L, rhs, betas[s][None, :], extra=extra)
        print(f"rank {rank}, C={cost:g}: solve residual / bound {ratio:.3f}, attempts {info['attempts']}, jitter {nu:.2e}, {info['launches']} launches, assemble / factor / solve / invert "
              f"{info['assemble_ms']:.3f} / {info['factor_ms']:.3f} / {info['solve_ms']:.3f} / {info['invert_ms']:.3f} ms")
        assert ratio <= 1.0, (rank, cost, ratio)


# ---------------------------------------------------------------- the default is untouched ----------------------------------------------------------------
def test_the_default_is_the_host_path_and_the_problem_is_left_as_it_was():
    p, _, _ = tr.fit_reference("rbf_777x5", np.float64, 1)
    n = p["X"].shape[0] - 1
    d = np.random.default_rng(3).standard_normal(n)
    with backend.ResidentProblem(tr.parameter(p["kernel"], p["kw"], p["cost"]), p["X"]) as prob:
        before = prob.matvec(d, np.zeros(n))
        left_out, named = prob.fit_reduced(p["Y"][0], 64), prob.fit_reduced(p["Y"][0], 64, factor="host")
        assert np.array_equal(left_out[0], named[0]) and left_out[1] == named[1] and "attempts" not in left_out[3] and left_out[3]["jitter"] == named[3]["jitter"]
        loo_out, loo_named = prob.fit_reduced_loo(p["Y"][0], 64, lm.FIT_COSTS), prob.fit_reduced_loo(p["Y"][0], 64, lm.FIT_COSTS, factor="host")
        assert tl.same(loo_out, loo_named) and "attempts" not in loo_out[3]["infos"][0]
        prob.fit_reduced(p["Y"][0], 64, factor="device")
        prob.fit_reduced_loo(p["Y"][0], 64, lm.FIT_COSTS, factor="device")
        assert np.array_equal(before, prob.matvec(d, np.zeros(n)))
        again = prob.fit_reduced(p["Y"][0], 64)  # ... and the host path after a device-factored call: still its bits
        assert np.array_equal(left_out[0], again[0]) and left_out[1] == again[1]
