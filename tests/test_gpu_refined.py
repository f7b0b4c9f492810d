"""GPU (-m gpu): mixed-precision refinement, lssvm_mi355_solve_refined_f64 -- the float64 system solved to the float64 stop test with the CG iterations in float32.

The yardstick is numpy float64 in this file: the reduced system of the CG recipe (b eliminated through the last point),
    A_ij = k(x_i, x_j) + delta_ij / (C w_i) + QA - q_i - q_j,   q_i = k(x_i, x_N),   QA = k(x_N, x_N) + 1 / (C w_N),   b = y[0..n) - y[n],
built densely and solved by numpy.linalg.solve.  What is asserted per solve, with x = alpha[:n] and d0 = |b - A 1|_2:
  * |b - A x|_2 <= 2 eps d0: the device's own (true, float64) residual is within eps d0; the factor 2 covers the different order of the float64 sums, whose effect is
    of order n 2^-53 |A| |x|, far below eps d0 at these sizes;
  * |x - x*|_2 / |x*|_2 <= 2 eps kappa_2(A) d0 / |b|_2, the standard residual bound;
  * alpha[N-1] and rho are the float64 bias formula of x, to 1e-12 of their natural scale;
  * the report: converged, refined, the pass count 1 + outer_steps, 2 <= outer_steps <= 6 at eps = 1e-9 (one step cannot reach 1e-9 with an inner floor of 2^-16; more than
    six means the inner tolerance rule is broken), and inner iterations <= 3 x the plain float64 solve's on the same input (the CPU model shows 1.2 ... 1.8 x).
Shapes: 300 points = three row blocks with a ragged last one, 20 features = a ragged feature chunk, 1500 x 64 = several column tiles per work item."""

import functools

import numpy as np
import pytest

from plssvm_amd import backend
from plssvm_amd.csvm import MI355CSVM, make_csvm
from plssvm_amd.data_set import DataSet
from plssvm_amd.multiclass import one_vs_all_targets
from plssvm_amd.parameter import Parameter

pytestmark = pytest.mark.gpu

KERNELS = {"linear": dict(kernel_type="linear"), "polynomial": dict(kernel_type="polynomial", degree=3, coef0=1.0), "rbf": dict(kernel_type="rbf")}


def param(kernel, d, cost=1.0):
    return Parameter(gamma=1.0 / d, cost=cost, **KERNELS[kernel])


@functools.lru_cache(maxsize=None)
def data(N, d, seed=0):
    """U(-1, 1) points, labels +-1 from a noisy hyperplane."""
    rng = np.random.default_rng(1000 * N + d + seed)
    X = rng.uniform(-1.0, 1.0, size=(N, d))
    y = np.where(X @ rng.standard_normal(d) + 0.3 * rng.standard_normal(N) > 0.0, 1.0, -1.0)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def gram(kernel, X, Z, d):
    g = 1.0 / d
    if kernel == "linear":
        return X @ Z.T
    if kernel == "polynomial":
        return (g * (X @ Z.T) + 1.0) ** 3
    sq = (X * X).sum(1)[:, None] + (Z * Z).sum(1)[None, :] - 2.0 * (X @ Z.T)
    return np.exp(-g * np.maximum(sq, 0.0))


@functools.lru_cache(maxsize=None)
def dense(kernel, N, d, cost, weights_seed=None):
    """(A, q, QA, kappa_2(A), w) of the reduced system in float64 (computed once per case, shared, never modified)."""
    X, _ = data(N, d)
    w = np.ones(N) if weights_seed is None else np.random.default_rng(weights_seed).uniform(0.5, 2.0, size=N)
    K = gram(kernel, X, X, d)
    n = N - 1
    q = K[:n, n].copy()
    QA = K[n, n] + 1.0 / (cost * w[n])
    A = K[:n, :n] + np.diag(1.0 / (cost * w[:n])) + QA - q[:, None] - q[None, :]
    sv = np.linalg.svd(A, compute_uv=False)
    for a in (A, q, w):
        a.setflags(write=False)
    return A, q, QA, sv[0] / sv[-1], w


def check_solution(kernel, N, d, cost, eps, y, alpha, rho, weights_seed=None):
    """The residual bound, the error bound and the bias formula; returns (|b - A x| / d0, relative error of x)."""
    A, q, QA, kappa, _ = dense(kernel, N, d, cost, weights_seed)
    n = N - 1
    b = y[:n] - y[n]
    x = alpha[:n]
    d0 = np.linalg.norm(b - A @ np.ones(n))
    res = np.linalg.norm(b - A @ x)
    x_star = np.linalg.solve(A, b)
    err = np.linalg.norm(x - x_star) / np.linalg.norm(x_star)
    bound = 2.0 * eps * kappa * d0 / np.linalg.norm(b)
    print(f"  {kernel} {N} x {d} C {cost:g} eps {eps:g}: kappa {kappa:.2e}  |b - A x| / d0 {res / d0:.2e} (<= {2 * eps:.0e})  |x - x*| / |x*| {err:.2e} (<= {bound:.2e})")
    assert np.all(np.isfinite(alpha)) and np.isfinite(rho)
    assert res <= 2.0 * eps * d0, (res / d0, eps)
    assert err <= bound, (err, bound)
    sx, qx = x.sum(), q @ x
    scale = abs(y[n]) + abs(QA * sx) + abs(qx)
    assert abs(alpha[n] + sx) <= 1e-12 * np.abs(x).sum(), (alpha[n], -sx)
    assert abs(float(rho) + (y[n] + QA * sx - qx)) <= 1e-12 * scale, (float(rho), -(y[n] + QA * sx - qx))
    return res / d0, err


@functools.lru_cache(maxsize=None)
def plain_iterations(kernel, N, d, cost, eps):
    X, y = data(N, d)
    _, _, info = backend.solve_system_of_linear_equations(param(kernel, d, cost), X, y, eps, N)
    assert info["converged"]
    return int(info["iterations"])


def same_bits(a, b):
    """np.array_equal on the bit patterns (a NaN equals only the same NaN)."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def refined_solve(kernel, N, d, cost, eps, **kw):
    X, y = data(N, d)
    alpha, rho, info, ri = backend.solve_refined(param(kernel, d, cost), X, y, eps, 10 * N, **kw)
    print(f"  refined: outer {ri['outer_steps']} inner {ri['inner_iterations']} f64 cg {ri['f64_cg_iterations']} passes f64 {ri['f64_passes']} f32 {ri['f32_passes']} "
          f"took over {ri['took_over_f64']} residuum {ri['residuum']:.3e} target {ri['target_residuum']:.3e} inner gram mode {ri['inner_gram_mode']}")
    return X, y, alpha, rho, info, ri


def assert_refined_report(info, ri, eps, plain_its, min_outer, max_outer):
    assert info["converged"] == 1 and ri["refined"] == 1 and ri["took_over_f64"] == 0 and ri["f64_cg_iterations"] == 0
    assert ri["f64_passes"] == 1 + ri["outer_steps"]
    assert min_outer <= ri["outer_steps"] <= max_outer, ri["outer_steps"]
    assert ri["inner_iterations"] <= 3 * plain_its, (ri["inner_iterations"], plain_its)
    assert info["iterations"] == ri["inner_iterations"] and info["epsilon"] == eps
    assert ri["residuum"] <= ri["target_residuum"] and info["residuum"] == ri["residuum"] and info["target_residuum"] == ri["target_residuum"]
    assert ri["target_residuum"] == eps * eps * ri["initial_residuum"] and info["initial_residuum"] == ri["initial_residuum"]
    assert info["gram_mode"] == ri["inner_gram_mode"] and info["rbf_direct"] == ri["inner_rbf_direct"]


# ---------------------------------------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("shape", [(300, 20), (1500, 64)])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_meets_the_fp64_stop_test_beyond_the_reach_of_fp32(kernel, shape):
    N, d = shape
    _, y, alpha, rho, info, ri = refined_solve(kernel, N, d, 1.0, 1e-9)
    check_solution(kernel, N, d, 1.0, 1e-9, y, alpha, rho)
    its = plain_iterations(kernel, N, d, 1.0, 1e-9)
    print(f"  plain fp64 CG: {its} iterations")
    assert_refined_report(info, ri, 1e-9, its, 2, 6)


@pytest.mark.parametrize("shape", [(300, 20), (1500, 64)])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_loose_tolerance(kernel, shape):
    N, d = shape
    _, y, alpha, rho, info, ri = refined_solve(kernel, N, d, 1.0, 1e-3)
    check_solution(kernel, N, d, 1.0, 1e-3, y, alpha, rho)
    print(f"  plain fp64 CG: {plain_iterations(kernel, N, d, 1.0, 1e-3)} iterations")
    assert info["converged"] == 1 and ri["refined"] == 1 and ri["outer_steps"] >= 1
    assert ri["residuum"] <= ri["target_residuum"] and ri["f64_passes"] == 1 + ri["outer_steps"] + ri["f64_cg_iterations"] + ri["f64_cg_iterations"] // 50


# ---------------------------------------------------------------------------------------------------------------------------------------------- 3
def test_harder_system():
    """rbf 1500 x 32, C = 100: kappa ~ 5e4 in the CPU model, 2-3 outer steps."""
    _, y, alpha, rho, info, ri = refined_solve("rbf", 1500, 32, 100.0, 1e-8)
    check_solution("rbf", 1500, 32, 100.0, 1e-8, y, alpha, rho)
    its = plain_iterations("rbf", 1500, 32, 100.0, 1e-8)
    print(f"  plain fp64 CG: {its} iterations")
    assert_refined_report(info, ri, 1e-8, its, 2, 6)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4
def test_fp64_cg_takes_over_where_fp32_cannot_see_the_ridge():
    """linear 400 x 8, C = 1e8: 1 / C lies below float32's resolution of the diagonal, the first step does not halve the residual and float64 CG finishes the solve."""
    _, y, alpha, rho, info, ri = refined_solve("linear", 400, 8, 1e8, 1e-6)
    assert ri["refined"] == 1 and ri["took_over_f64"] == 1 and info["converged"] == 1
    check_solution("linear", 400, 8, 1e8, 1e-6, y, alpha, rho)
    its = plain_iterations("linear", 400, 8, 1e8, 1e-6)
    print(f"  plain fp64 CG: {its} iterations")
    assert ri["inner_iterations"] <= 200
    assert 1 <= ri["f64_cg_iterations"] <= 2 * its, (ri["f64_cg_iterations"], its)
    assert ri["residuum"] <= ri["target_residuum"] and info["iterations"] == ri["inner_iterations"] + ri["f64_cg_iterations"]
    assert ri["f64_passes"] == 1 + ri["outer_steps"] + ri["f64_cg_iterations"] + ri["f64_cg_iterations"] // 50


# ---------------------------------------------------------------------------------------------------------------------------------------------- 5
def test_several_right_hand_sides_are_the_single_solves():
    N, d, eps = 1500, 64, 1e-9
    X, _ = data(N, d)
    rng = np.random.default_rng(5)
    labels = np.argmax(X @ rng.standard_normal((d, 3)) + 0.3 * rng.standard_normal((N, 3)), axis=1)
    B = one_vs_all_targets(np.arange(3), labels, np.float64)
    p = param("polynomial", d)
    passes = []
    alphas, rhos, infos, ris = backend.solve_refined(p, X, B, eps, 10 * N, passes_out=passes)
    assert alphas.shape == (3, N) and rhos.shape == (3,) and len(infos) == len(ris) == 3
    print(f"  passes {passes}, outer steps {[r['outer_steps'] for r in ris]}, f64 passes {[r['f64_passes'] for r in ris]}")
    for c in range(3):
        a, rho, info, ri = backend.solve_refined(p, X, B[c], eps, 10 * N)
        assert np.array_equal(alphas[c], a) and rhos[c] == rho, (c, np.count_nonzero(alphas[c] != a))
        assert ris[c]["outer_steps"] == ri["outer_steps"] and ris[c]["inner_iterations"] == ri["inner_iterations"] and ris[c]["residuum"] == ri["residuum"]
        assert infos[c]["converged"] == 1 and ris[c]["refined"] == 1
        check_solution("polynomial", N, d, 1.0, eps, B[c], alphas[c], rhos[c])
    assert passes[0] > 0 and 2 * passes[0] + passes[1] == sum(r["f64_passes"] for r in ris), (passes, [r["f64_passes"] for r in ris])


# ---------------------------------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("kernel", ["polynomial", "rbf"])
def test_weights(kernel):
    N, d, eps = 300, 20, 1e-9
    X, y = data(N, d)
    a1, rho1, _, _ = backend.solve_refined(param(kernel, d), X, y, eps, 10 * N)
    aw, rhow, _, _ = backend.solve_refined(param(kernel, d), X, y, eps, 10 * N, sample_weight=np.ones(N))
    assert np.array_equal(aw, a1) and rhow == rho1, "w == 1 must give the bits of the unweighted call"
    a2, rho2, _, _ = backend.solve_refined(param(kernel, d, 2.0), X, y, eps, 10 * N)
    aw, rhow, _, _ = backend.solve_refined(param(kernel, d), X, y, eps, 10 * N, sample_weight=np.full(N, 2.0))
    assert np.array_equal(aw, a2) and rhow == rho2, "w == 2 must give the bits of the unweighted call at cost 2C"
    w = dense(kernel, N, d, 1.0, 17)[4]
    aw, rhow, info, ri = backend.solve_refined(param(kernel, d), X, y, eps, 10 * N, sample_weight=w)
    assert info["converged"] == 1 and ri["refined"] == 1
    check_solution(kernel, N, d, 1.0, eps, y, aw, rhow, weights_seed=17)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 7
def test_two_identical_calls_are_bit_equal():
    X, y = data(1500, 64)
    first = backend.solve_refined(param("rbf", 64), X, y, 1e-9, 15000)
    second = backend.solve_refined(param("rbf", 64), X, y, 1e-9, 15000)
    assert np.array_equal(first[0], second[0]) and first[1] == second[1]
    for key in ("outer_steps", "inner_iterations", "f64_passes", "f32_passes", "residuum", "initial_residuum"):
        assert first[3][key] == second[3][key], key


@pytest.mark.parametrize("k", [1, 2])
def test_data_beyond_float32_falls_back_to_the_plain_solve(k):
    X, y = data(300, 20)
    X = X.copy()
    X[7, 3] = 1e300
    p = param("linear", 20)
    B = np.stack([y, -y])[:k]
    with np.errstate(all="ignore"):
        alphas, rhos, infos, ris = backend.solve_refined(p, X, B, 1e-6, 300)
        for c in range(k):
            a, rho, info = backend.solve_system_of_linear_equations(p, X, B[c], 1e-6, 300)
            assert ris[c]["refined"] == 0 and ris[c]["outer_steps"] == 0 and ris[c]["inner_iterations"] == 0
            assert same_bits(alphas[c], a) and same_bits(rhos[c], rho)
            assert infos[c]["iterations"] == info["iterations"] and infos[c]["converged"] == info["converged"]
    a, rho, info, ri = backend.solve_refined(p, X, B[0], 1e-6, 300)  # ... and the single right-hand side form of the call
    assert ri["refined"] == 0 and same_bits(a, alphas[0]) and same_bits(rho, rhos[0])


# ---------------------------------------------------------------------------------------------------------------------------------------------- 8
def test_csvm_with_the_refined_solver():
    X, y = data(500, 20)
    p = param("rbf", 20)
    ds = DataSet(X, [int(v) for v in y], real_type=np.float64)
    cg, refined = MI355CSVM(params=p), make_csvm("mi355", params=p, solver="refined")
    assert refined.solver == "refined" and cg.solver == "cg" and refined.last_refine_info is None
    m_cg, m_ref = cg.fit(ds, epsilon=1e-8), refined.fit(ds, epsilon=1e-8)
    assert cg.last_refine_info is None
    assert len(refined.last_refine_info) == 1 and refined.last_refine_info[0]["refined"] == 1 and refined.last_cg_info["converged"] == 1
    assert refined.predict(m_ref, ds) == cg.predict(m_cg, ds)
    # several systems at once: one report per right-hand side
    B = np.stack([y, -y])
    alphas, rhos, infos = refined.solve_systems_of_linear_equations(p, X, B, 1e-8, 500)
    assert [r["refined"] for r in refined.last_refine_info] == [1, 1] and alphas.shape == (2, 500) and len(infos) == 2
    # float32 data: solved as with solver="cg", bit for bit
    ds32 = DataSet(X.astype(np.float32), [int(v) for v in y], real_type=np.float32)
    m32_cg, m32_ref = cg.fit(ds32, epsilon=1e-4), refined.fit(ds32, epsilon=1e-4)
    assert refined.last_refine_info is None
    assert m32_ref.alpha.dtype == np.float32 and np.array_equal(m32_ref.alpha, m32_cg.alpha) and m32_ref.rho == m32_cg.rho
