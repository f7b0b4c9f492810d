"""GPU: the kernel matrix kept in HBM (lssvm_stored.hip) -- matvec_stored against dense float64 under the derived per-row bound, the stored lockstep
CG against dense solves, the bit equalities of the contract, and solver="stored" through the public objects.  Shapes sit at the edges of the 128-tile geometry (N - 1 below,
at and past one tile, three row blocks) and of the sixteen-vector group."""

import functools

import numpy as np
import pytest

import pcg_model as pm
from plssvm_amd import backend, multiclass
from plssvm_amd.csvm import MI355CSVM, make_csvm
from plssvm_amd.data_set import DataSet
from plssvm_amd.parameter import Parameter

pytestmark = pytest.mark.gpu

KERNELS = {  # (gamma and coef0 are exact in float32: the reference evaluates the parameters the problem holds)
    "linear": dict(kernel="linear", kw=dict(gamma=1.0)),
    "poly3": dict(kernel="polynomial", kw=dict(gamma=0.25, coef0=1.0, degree=3)),
    "polym2": dict(kernel="polynomial", kw=dict(gamma=0.125, coef0=1.5, degree=-2)),
    "rbf": dict(kernel="rbf", kw=dict(gamma=0.5)),
}
# a sparse cross: (points N, features, vectors, kernel function)
CASES = [(2, 1, 1, "rbf"), (129, 17, 2, "poly3"), (130, 130, 16, "rbf"), (258, 17, 17, "linear"), (386, 1, 16, "polym2"), (386, 130, 17, "rbf"), (258, 130, 2, "poly3")]
DTYPES = [np.float32, np.float64]
COST = 4.0


def parameter(kernel):
    k = KERNELS[kernel]
    return Parameter(kernel_type=k["kernel"], cost=COST, gamma=k["kw"]["gamma"], coef0=k["kw"].get("coef0", 0.0), degree=k["kw"].get("degree", 3))


@functools.lru_cache(maxsize=None)
def reference(N, d, kernel, dtype):
    """(X in dtype, dense float64 H of all N points, dense Abar): computed once per shape, shared, never modified."""
    X = (np.random.default_rng(N + d).uniform(-1, 1, (N, d)) / np.sqrt(d)).astype(dtype)
    k = KERNELS[kernel]
    H = pm.kernel_matrix(k["kernel"], X, X, **k["kw"])
    A = pm.reduced_matrix(k["kernel"], X, COST, **k["kw"])
    for a in (X, H, A):
        a.setflags(write=False)
    return X, H, A


def entry_errors(X64, H, kernel, ldx, unit, representation):
    """|error| of every kernel value whose sum over the features runs in arithmetic of precision `unit` on data held to `representation` (relative, per component)."""
    k, kw = KERNELS[kernel]["kernel"], KERNELS[kernel]["kw"]
    if k == "rbf":  # the norm terms of the centred data, carried through gamma k
        Xc = X64 - X64.mean(0)
        nrm = (Xc * Xc).sum(1)
        terms = nrm[:, None] + nrm[None, :] + 2.0 * np.abs(Xc) @ np.abs(Xc).T
        return kw["gamma"] * H * ((ldx + 4) * unit + 2 * representation) * terms + 4 * unit * H
    P = np.abs(X64) @ np.abs(X64).T  # the dot products, carried through |deg| gamma |k / base|
    if k == "linear":
        return ((ldx + 2) * unit + representation) * P
    deg = kw["degree"]
    base = kw["gamma"] * (X64 @ X64.T) + kw["coef0"]
    return abs(deg) * kw["gamma"] * np.abs(H / base) * ((ldx + 2) * unit + representation) * P + (abs(deg) + 4) * unit * np.abs(H)


def row_bounds(X, H, V, kernel, dtype):
    """the bound on |error| of every entry of Abar V, [vector][row]."""
    X64, V64 = np.asarray(X, np.float64), V.astype(np.float64)
    n, ldx = X.shape[0] - 1, 32 * -(-X.shape[1] // 32)
    eps, eps64 = float(np.finfo(dtype).eps), float(np.finfo(np.float64).eps)
    aV, aH, S = np.abs(V64), np.abs(H), np.abs(V64.sum(1))[:, None]
    # the stored part: fp64 evaluation of data held in the real type, one rounding on the store, a sum of n terms in the real type
    E = entry_errors(X64, H, kernel, ldx, eps64, eps)
    stored = aV @ E[:n, :n].T + (eps / 2 + n * eps) * (aV @ aH[:n, :n].T)
    # the rank-one and diagonal terms, as every other pass has them: q and QA_cost evaluated and held in the real type, the row's result rounded once
    Eq = entry_errors(X64, H, kernel, ldx, eps, 0.0) + eps * aH
    rest = S * Eq[:n, n][None, :] + (aV @ Eq[:n, n])[:, None] + (Eq[n, n] + eps / COST) * S + eps * aV / COST
    total = aV @ aH[:n, :n].T + S * aH[:n, n][None, :] + (aV @ aH[:n, n])[:, None] + (aH[n, n] + 1 / COST) * S + aV / COST
    return stored + rest + eps * total


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,d,nv,kernel", CASES)
def test_matvec_stored_against_dense_float64(N, d, nv, kernel, dtype):
    X, H, A = reference(N, d, kernel, dtype)
    V = np.random.default_rng(7).standard_normal((nv, N - 1)).astype(dtype)
    with backend.ResidentProblem(parameter(kernel), X) as prob:
        stored, nbytes, _ = prob.store_gram()
        out, ran = prob.matvec_stored(V)
        again, _ = prob.matvec_stored(V)
        alone, _ = prob.matvec_stored(V[-1:])
    assert stored and ran and nbytes >= (N - 1) ** 2 // 2 * np.dtype(dtype).itemsize
    ratio = np.abs(out.astype(np.float64) - V.astype(np.float64) @ A.T) / row_bounds(X, H, V, kernel, dtype)
    print(f"stored matvec N={N} d={d} nv={nv} {kernel} {np.dtype(dtype).name}: largest error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    assert np.array_equal(out, again)           # a repeated call gives the same bits
    assert np.array_equal(out[-1:], alone)      # a column's bits do not depend on the other columns or on its slot


@pytest.mark.parametrize("dtype,eps", [(np.float32, 1e-4), (np.float64, 1e-10)], ids=["f32", "f64"])
@pytest.mark.parametrize("N,d,k,kernel,weighted", [(130, 17, 1, "rbf", False), (258, 130, 3, "poly3", True), (386, 17, 17, "rbf", False)])
def test_solve_lockstep_stored_against_dense_solves(N, d, k, kernel, weighted, dtype, eps):
    X, _, _ = reference(N, d, kernel, dtype)
    rng = np.random.default_rng(3)
    B = np.where(rng.standard_normal((k, N)) > 0, 1.0, -1.0).astype(dtype)
    w = rng.uniform(0.5, 2.0, N) if weighted else None
    kk = KERNELS[kernel]
    Hn = pm.kernel_matrix(kk["kernel"], X, X, **kk["kw"]) + np.diag(1.0 / (COST * (w if weighted else np.ones(N))))
    A = Hn[:-1, :-1] - Hn[:-1, -1:] - Hn[-1:, :-1] + Hn[-1, -1]
    with backend.ResidentProblem(parameter(kernel), X) as prob:
        assert prob.store_gram()[0]
        if weighted:
            prob.set_weights(w)  # (after store_gram: the stored matrix survives it)
        alphas, rhos, infos, passes = prob.solve_lockstep_stored(B, eps, 4 * N)
        one = prob.solve_lockstep_stored(B[-1:], eps, 4 * N)[0]
    assert passes[0] > 0 and passes[1] == passes[2] == 0 and all(i["converged"] == 1 for i in infos)
    for c in range(k):
        assert pm.true_residual(A, pm.reduced_rhs(B[c]), alphas[c][:-1]) <= 2 * eps
    assert np.array_equal(alphas[-1:], one)


@pytest.mark.parametrize("how", ["dropped", "declined"])
def test_without_a_stored_matrix_the_calls_are_the_panels_calls(how):
    X, _, _ = reference(258, 17, "rbf", np.float64)
    B = np.where(np.random.default_rng(4).standard_normal((3, 258)) > 0, 1.0, -1.0)
    with backend.ResidentProblem(parameter("rbf"), X) as prob:
        if how == "dropped":
            assert prob.store_gram()[0]
            prob.drop_gram()
        else:
            assert prob.store_gram(max_bytes=1) == (False, 0, 0.0)
        got = prob.solve_lockstep_stored(B, 1e-8, 600)
        want = prob.solve_lockstep(B, 1e-8, 600, panels=True)
        assert not prob.matvec_stored(B[:, :-1])[1]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[3] == (0,) + tuple(want[3])
    assert [(i["iterations"], i["residuum"], i["matvec_launches"]) for i in got[2]] == [(i["iterations"], i["residuum"], i["matvec_launches"]) for i in want[2]]


@pytest.mark.parametrize("classes", [2, 3])
def test_csvm_with_the_stored_solver_fits_as_cg_does(classes):
    rng = np.random.default_rng(11)
    centres = rng.uniform(-1, 1, (classes, 6)) * 2.0
    labels = np.arange(301) % classes
    X = centres[labels] + 0.35 * rng.standard_normal((301, 6))
    svm, plain = make_csvm("mi355", solver="stored", kernel_type="rbf", cost=10.0), MI355CSVM(kernel_type="rbf", cost=10.0)
    if classes == 2:
        data = DataSet(X, [int(v) for v in labels])
        model = svm.fit(data, epsilon=1e-12)
        assert svm.last_cg_info["converged"] == 1 and svm.score(model) >= 0.97
        assert svm.predict(model, data) == plain.predict(plain.fit(data, epsilon=1e-12), data)
    else:
        model = multiclass.fit_one_vs_all(svm, svm.params, X, labels, np.arange(classes), 1e-12)
        ref = multiclass.fit_one_vs_all(plain, plain.params, X, labels, np.arange(classes), 1e-12)
        # two solves of one system to a relative residual of 1e-12 each: with cond(Abar) <= (N + 1 / C) C ~ 3e3 the solutions, and with them the decision values
        # (sums of 301 kernel values <= 1 times alpha), agree to ~1e-8 of |alpha| ~ 10; 1e-6 leaves two orders of room and is far below any decision margin
        assert np.allclose(multiclass.decision_values(svm, model, X), multiclass.decision_values(plain, ref, X), rtol=0, atol=1e-6)
    assert svm.last_lockstep_passes[0] > 0
