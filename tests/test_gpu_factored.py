"""GPU: the factored linear-kernel operator K V = X (X^T V) (lssvm_factored.hip) -- matvec_factored against dense float64 under the derived per-entry
bound, the factored lockstep CG against the dense system, the bit equalities of the contract, the declined call and lockstep="factored" through the public objects.  Shapes
sit at the edges of the slab geometry (S = FACTORED_SLAB_ROWS rows: one row, a row count that is no multiple of 4, exactly one slab, a one-row second slab, the fold's
remainder), of the feature panels (1, 17 and 130 features) and of the sixteen-vector group."""

import functools

import numpy as np
import pytest

import pcg_model as pm
from plssvm_amd import _capi, backend, multiclass
from plssvm_amd.csvm import MI355CSVM, make_csvm
from plssvm_amd.data_set import DataSet
from plssvm_amd.parameter import Parameter

pytestmark = pytest.mark.gpu

S = _capi.FACTORED_SLAB_ROWS
DTYPES = [np.float32, np.float64]
COST = 4.0


def parameter(kernel="linear"):
    return Parameter(kernel_type=kernel, cost=COST, gamma=0.5)


@functools.lru_cache(maxsize=None)
def reference(N, d, dtype):
    """(X in dtype, dense float64 H of all N points, dense Abar): computed once per shape, shared, never modified."""
    X = (np.random.default_rng(N + d).uniform(-1, 1, (N, d)) / np.sqrt(d)).astype(dtype)
    H = pm.kernel_matrix("linear", X, X, gamma=1.0)
    A = pm.reduced_matrix("linear", X, COST, gamma=1.0)
    for a in (X, H, A):
        a.setflags(write=False)
    return X, H, A


def entry_bounds(X, H, V, dtype):
    """the bound on |error| of every entry of Abar V, [vector][row].  The factored part is a sum of at most n terms (X^T V) and then one of at most
    ldx terms (X W), both in the real type on data held in it -- linear data is never held scaled, so no representation term: (n + ldx + 6) eps at the FACTORED summand
    scale sum_f |x_if| sum_j |x_jf v_j|.  The rank-one, diagonal and final-rounding terms are those of every other pass (row_bounds of tests/test_gpu_stored.py, linear)."""
    X64, V64 = np.asarray(X, np.float64), V.astype(np.float64)
    n, ldx = X.shape[0] - 1, 32 * -(-X.shape[1] // 32)
    eps = float(np.finfo(dtype).eps)
    aV, aH, aX, Sm = np.abs(V64), np.abs(H), np.abs(X64[:n]), np.abs(V64.sum(1))[:, None]
    factored = (n + ldx + 6) * eps * ((aV @ aX) @ aX.T)
    Eq = (ldx + 2) * eps * (np.abs(X64) @ np.abs(X64).T) + eps * aH
    rest = Sm * Eq[:n, n][None, :] + (aV @ Eq[:n, n])[:, None] + (Eq[n, n] + eps / COST) * Sm + eps * aV / COST
    total = aV @ aH[:n, :n].T + Sm * aH[:n, n][None, :] + (aV @ aH[:n, n])[:, None] + (aH[n, n] + 1 / COST) * Sm + aV / COST
    return factored + rest + eps * total


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,d,nv", [(2, 1, 1), (131, 17, 2), (S + 1, 130, 16), (S + 2, 17, 17), (5 * S + 3, 1, 16), (2 * S + 2, 130, 17)])
def test_matvec_factored_against_dense_float64(N, d, nv, dtype):
    X, H, A = reference(N, d, dtype)
    V = np.random.default_rng(7).standard_normal((nv, N - 1)).astype(dtype)
    with backend.ResidentProblem(parameter(), X) as prob:
        out, ran = prob.matvec_factored(V)
        again, _ = prob.matvec_factored(V)
        alone, _ = prob.matvec_factored(V[-1:])
    assert ran
    ratio = np.abs(out.astype(np.float64) - V.astype(np.float64) @ A.T) / entry_bounds(X, H, V, dtype)
    print(f"factored matvec N={N} d={d} nv={nv} {np.dtype(dtype).name}: largest error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    assert np.array_equal(out, again)           # a repeated call gives the same bits
    assert np.array_equal(out[-1:], alone)      # a column's bits do not depend on the other columns or on its slot


@pytest.mark.parametrize("dtype,eps", [(np.float32, 1e-4), (np.float64, 1e-10)], ids=["f32", "f64"])
@pytest.mark.parametrize("N,d,k,weighted", [(131, 17, 1, False), (S + 2, 130, 3, True), (2 * S + 2, 17, 17, False)])
def test_solve_lockstep_factored_against_the_dense_system(N, d, k, weighted, dtype, eps):
    X, _, _ = reference(N, d, dtype)
    rng = np.random.default_rng(3)
    B = np.where(rng.standard_normal((k, N)) > 0, 1.0, -1.0).astype(dtype)
    w = rng.uniform(0.5, 2.0, N) if weighted else None
    Hn = pm.kernel_matrix("linear", X, X, gamma=1.0) + np.diag(1.0 / (COST * (w if weighted else np.ones(N))))
    A = Hn[:-1, :-1] - Hn[:-1, -1:] - Hn[-1:, :-1] + Hn[-1, -1]
    with backend.ResidentProblem(parameter(), X) as prob:
        if weighted:
            prob.set_weights(w)
        alphas, rhos, infos, passes = prob.solve_lockstep_factored(B, eps, 4 * N)
        one = prob.solve_lockstep_factored(B[-1:], eps, 4 * N)[0]
    assert passes[0] > 0 and passes[1] == passes[2] == 0 and all(i["converged"] == 1 for i in infos)
    for c in range(k):
        assert pm.true_residual(A, pm.reduced_rhs(B[c]), alphas[c][:-1]) <= 2 * eps
    assert np.array_equal(alphas[-1:], one)


def test_on_an_rbf_problem_the_calls_are_the_panels_calls():
    X, _, _ = reference(258, 17, np.float64)
    B = np.where(np.random.default_rng(4).standard_normal((3, 258)) > 0, 1.0, -1.0)
    with backend.ResidentProblem(parameter("rbf"), X) as prob:
        got = prob.solve_lockstep_factored(B, 1e-8, 600)
        want = prob.solve_lockstep(B, 1e-8, 600, panels=True)
        assert not prob.matvec_factored(B[:, :-1])[1]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[3] == (0,) + tuple(want[3])
    assert [(i["iterations"], i["residuum"], i["matvec_launches"]) for i in got[2]] == [(i["iterations"], i["residuum"], i["matvec_launches"]) for i in want[2]]


@pytest.mark.parametrize("classes", [2, 3])
def test_csvm_with_the_factored_lockstep_fits_as_the_default_does(classes):
    rng = np.random.default_rng(11)
    centres = rng.uniform(-1, 1, (classes, 6)) * 2.0
    labels = np.arange(301) % classes
    X = centres[labels] + 0.35 * rng.standard_normal((301, 6))
    svm, plain = make_csvm("mi355", lockstep="factored", kernel_type="linear", cost=10.0), MI355CSVM(kernel_type="linear", cost=10.0)
    if classes == 2:
        data = DataSet(X, [int(v) for v in labels])
        model, ref = svm.fit(data, epsilon=1e-12), plain.fit(data, epsilon=1e-12)
        assert svm.last_cg_info["converged"] == 1
        assert svm.predict(model, data) == plain.predict(ref, data) and svm.score(model) == plain.score(ref)
    else:
        model = multiclass.fit_one_vs_all(svm, svm.params, X, labels, np.arange(classes), 1e-12)
        ref = multiclass.fit_one_vs_all(plain, plain.params, X, labels, np.arange(classes), 1e-12)
        got, want = multiclass.decision_values(svm, model, X), multiclass.decision_values(plain, ref, X)
        assert np.array_equal(got.argmax(1), want.argmax(1)) and np.mean(got.argmax(1) == labels) == np.mean(want.argmax(1) == labels)
    assert svm.last_lockstep_passes[0] > 0
