"""GPU (-m gpu): the block lockstep CG -- lssvm_mi355_problem_matvec_block / _solve_lockstep_block, ``MI355CSVM(lockstep="block")`` -- and the sixteen-vector symmetric
kernel behind it (tile_matvec_f64_blk_sym, plssvm_amd/csrc/lssvm_tile_f64_blk_sym.hip.hpp).

matvec_block: against numpy in ``np.longdouble`` on the float64 data -- ret = Abar V with Abar_ij = k_ij + delta_ij / C + QA - q_i - q_j, the system of n = points - 1 rows
-- in units u_iv = eps64 * sum_j |v_jv k_ij|.  e_old is the largest error of the single-vector ``matvec`` on the same case (the terms beside K v are common to both),
e_new that of the block call; asserted: e_new <= e_old + (L + 3).  L, the additions in the longest chain of one value, from the sum order the kernel defines, with T
column tiles of 128:
  row product: one MFMA (four columns) per addition over the work item's sub-tiles, 32 T over all chunks together, then one addition per chunk slab (at most T chunks);
  mirror: one MFMA (four rows) per addition over a wave's 32 rows (8), the four waves (2), then the row blocks' records in fold order (k_reduce_colslab: at most
  T records over its groups, 15 additions of the groups' sums, one into K v), and the row sums on top (1).
L = 32 T + T + 8 + 2 + T + 15 + 1 + 1.  A wrong index, a dropped tile or a swapped operand is an error of 1 / eps64 units.
solve_lockstep_block: against the dense float64 reduced system (the construction of tests/test_gpu_refined.py), the true relative residual within the factor 2 of
tests/test_gpu_cost_path.py.  Bits: repeats, a vector alone against its place in a block, a right-hand side alone against its column, every declined case against
``solve_lockstep(..., panels=True)``."""

import functools

import numpy as np
import pytest

from plssvm_amd import backend
from plssvm_amd._capi import Options
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.parameter import KernelFunctionType, Parameter

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
FORMS = {"rbf": ("rbf", 3, 0.0), "poly5": ("polynomial", 5, 0.5), "poly2": ("polynomial", 2, 0.0), "poly3": ("polynomial", 3, -0.25)}

# (form, n rows of the system, features, vectors, options)
CASES = ([(f, n, 17, 3, {}) for f, n in zip(("rbf", "poly5", "poly2", "poly3", "rbf"), (1, 63, 64, 65, 128))]    # one row block: only the diagonal, no mirror
         + [(f, n, 20, 5, {}) for f, n in (("poly3", 129), ("rbf", 200), ("poly5", 200))]                       # the first mirrored tile, a padded row block
         + [(f, 300, 33, 16, {}) for f in FORMS]                                                                # mirror sums from two row blocks plus the own row sums
         + [(f, 777, 24, 7, {"j_chunk_tiles": 1}) for f in ("rbf", "poly2")]                                    # several column chunks
         + [(f, 300, d, 4, {}) for f, d in zip(("rbf", "poly5", "poly3", "poly2", "rbf"), (1, 16, 17, 130, 256))]  # 1, 1, 2, 9 (padded: 10) and 16 chunks
         + [("rbf", 300, 40, k, {}) for k in (1, 2, 15, 17, 33)]                                                # vector groups
         + [("poly3", 6100, 8, 2, {"colslab_band_mb": 1})])                                                     # 48 row blocks, 1.1 MiB of records: two bands


@functools.lru_cache(maxsize=None)
def points(n, d):
    X = np.random.default_rng(100 * n + d).uniform(-1.0, 1.0, size=(n + 1, d))
    X.setflags(write=False)
    return X


def kernel_rows(prm, X, Z, dt):
    X, Z = X.astype(dt), Z.astype(dt)
    G = X @ Z.T
    if prm.kernel_type == KernelFunctionType.RBF:
        return np.exp(-dt(prm.gamma) * ((X * X).sum(axis=1)[:, None] + (Z * Z).sum(axis=1)[None, :] - 2 * G))
    return (dt(prm.gamma) * G + dt(prm.coef0)) ** int(prm.degree)


def reference(prm, X, V, rows):
    """(Abar V, units u_iv) at `rows` of the system, in longdouble"""
    n = X.shape[0] - 1
    K = kernel_rows(prm, X[rows], X, LD)  # [rows, n + 1]
    qall = kernel_rows(prm, X[n:], X, LD)[0]
    q, QA, Vl = qall[:n], qall[n] + 1 / LD(prm.cost), V.astype(LD)
    S, QV = Vl.sum(axis=1), Vl @ q
    want = K[:, :n] @ Vl.T + Vl[:, rows].T / LD(prm.cost) + (QA * S - QV)[None, :] - q[rows, None] * S[None, :]
    return want, EPS64 * (np.abs(K[:, :n]) @ np.abs(Vl).T)


@pytest.mark.parametrize("form, n, d, k, opts", CASES, ids=lambda c: str(c))
def test_matvec_block_against_longdouble(form, n, d, k, opts):
    kernel, degree, coef0 = FORMS[form]
    prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=coef0, cost=2.0)
    X = points(n, d)
    V = np.random.default_rng(7 + k).standard_normal((k, n))
    rows = np.arange(n) if n <= 1000 else np.unique(np.concatenate([np.arange(0, n, 97), np.arange(128 * 34 - 3, 128 * 34 + 3), [n - 1]]))  # (the band edge: row block 34 of 48)
    want, unit = reference(prm, X, V, rows)
    T = -(-n // 128)
    L = 32 * T + T + 8 + 2 + T + 15 + 1 + 1
    with backend.ResidentProblem(prm, X, options=Options(**opts)) as prob:
        got, block = prob.matvec_block(V, np.zeros_like(V))
        again, _ = prob.matvec_block(V, np.zeros_like(V))
        old = np.stack([prob.matvec(V[v], np.zeros(n)) for v in range(k)])
    e_new, e_old = float(np.max(np.abs(got[:, rows].T - want) / unit)), float(np.max(np.abs(old[:, rows].T - want) / unit))
    print(f"{form} n={n} d={d} k={k} {opts}: e_new {e_new:.2f}, e_old {e_old:.2f} units, e_new - e_old {e_new - e_old:.2f}, L = {L}")
    assert block and got.shape == (k, n) and np.all(np.isfinite(got))
    assert np.array_equal(got, again)  # a repeat has the same bits
    assert e_new <= e_old + (L + 3), (e_new, e_old, L)


def test_a_vector_alone_has_the_bits_of_its_place_in_a_block():
    prm, X = Parameter(kernel_type="rbf", gamma=1.0 / 40, cost=2.0), points(300, 40)
    V = np.random.default_rng(5).standard_normal((17, 300))
    with backend.ResidentProblem(prm, X) as prob:
        got, _ = prob.matvec_block(V, np.zeros_like(V))
        for v in (0, 5, 15, 16):  # slots 0, 5, 15 of the first group, slot 0 of the second
            assert np.array_equal(prob.matvec_block(V[v:v + 1], np.zeros((1, 300)))[0][0], got[v]), v


SOLVES = {"rbf": (Parameter(kernel_type="rbf", gamma=0.2, cost=100.0), 5), "polynomial": (Parameter(kernel_type="polynomial", degree=3, gamma=1.0 / 16, coef0=1.0, cost=1.0), 16)}


@functools.lru_cache(maxsize=None)
def dense(kernel):
    """(A, X) of the reduced system of 777 points in float64: computed once per kernel, shared, never modified"""
    prm, d = SOLVES[kernel]
    X = points(776, d)
    K = kernel_rows(prm, X, X, np.float64)
    n = 776
    q = K[:n, n]
    A = K[:n, :n] + np.eye(n) / prm.cost + (K[n, n] + 1.0 / prm.cost) - q[:, None] - q[None, :]
    A.setflags(write=False)
    return A, X


@pytest.mark.parametrize("kernel", list(SOLVES))
@pytest.mark.parametrize("k", [1, 3, 17])
def test_solve_lockstep_block_against_dense_solves(kernel, k):
    A, X = dense(kernel)
    n, eps = 776, 1e-8
    Y = np.where(np.random.default_rng(k).standard_normal((k, 777)) > 0.0, 1.0, -1.0)
    with backend.ResidentProblem(SOLVES[kernel][0], X) as prob:
        alphas, rhos, infos, passes = prob.solve_lockstep_block(Y, eps, 2000)
        alone = {c: prob.solve_lockstep_block(Y[c:c + 1], eps, 2000) for c in sorted({0, k - 1})}
    for c in range(k):
        b = Y[c, :n] - Y[c, n]
        res, d0 = np.linalg.norm(b - A @ alphas[c, :n]), np.linalg.norm(b - A @ np.ones(n))
        print(f"  {kernel} rhs {c} of {k}: {infos[c]['iterations']} iterations, |b - A x| / d0 {res / d0:.2e} (<= {2 * eps:.0e})")
        assert infos[c]["converged"] == 1 and res <= 2.0 * eps * d0, (c, res / d0, infos[c])
    m = max(info["iterations"] for info in infos)
    if k <= 16:
        assert list(passes) == [1 + m + m // 50, 0, 0], (passes, m)
    assert passes[0] > 0 and passes[1] == passes[2] == 0
    for c, (a1, r1, i1, _) in alone.items():  # column c has the bits of the call with that right-hand side alone
        assert np.array_equal(a1[0], alphas[c]) and r1[0] == rhos[c] and i1[0]["iterations"] == infos[c]["iterations"], c


@pytest.mark.parametrize("case", ["fp32", "linear", "300_features", "tile_kernel_1", "symmetric_0", "negative_degree"])
def test_a_declined_case_is_solve_lockstep_panels(case):
    dt = np.float32 if case == "fp32" else np.float64
    d = 300 if case == "300_features" else 12
    X = np.random.default_rng(3).uniform(0.5, 1.5, size=(400, d)).astype(dt)  # (a negative power needs bases away from 0)
    Y = np.where(np.random.default_rng(4).standard_normal((3, 400)) > 0.0, 1.0, -1.0).astype(dt)
    prm = {"linear": Parameter(kernel_type="linear"), "negative_degree": Parameter(kernel_type="polynomial", degree=-1, gamma=1.0 / d, coef0=1.0)}.get(case, Parameter(kernel_type="rbf", gamma=1.0 / d))
    opts = {"tile_kernel_1": {"tile_kernel": 1}, "symmetric_0": {"symmetric": 0}}.get(case, {})
    eps = 1e-3 if dt == np.float32 else 1e-8
    with backend.ResidentProblem(prm, X, options=Options(**opts)) as prob:
        a0, r0, i0, p0 = prob.solve_lockstep(Y, eps, 500, panels=True)
        a1, r1, i1, p1 = prob.solve_lockstep_block(Y, eps, 500)
        V = np.ascontiguousarray(Y[:, :399])
        mv, block = prob.matvec_block(V, np.zeros_like(V))
        assert not block and np.array_equal(mv[2], prob.matvec(V[2], np.zeros(399, dt)))
    kept = ("iterations", "converged", "residuum", "initial_residuum", "target_residuum", "matvec_launches", "symmetric", "gram_mode")
    assert np.array_equal(a0, a1) and np.array_equal(r0, r1)
    assert [{n: i[n] for n in kept} for i in i0] == [{n: i[n] for n in kept} for i in i1]
    assert p1[0] == 0 and tuple(p1[1:]) == tuple(p0), (p0, p1)


def test_csvm_lockstep_block_reaches_the_block_passes():
    prm = Parameter(kernel_type="rbf", gamma=0.2, cost=10.0)
    X = points(599, 5)
    Y = np.where(np.arange(600)[None, :] % 5 == np.arange(5)[:, None], 1.0, -1.0)  # a 5-class one-vs-all target
    plain, blk = MI355CSVM(), MI355CSVM(lockstep="block")
    a0, r0, i0 = plain.solve_systems_of_linear_equations(prm, X, Y, 1e-8, 1000)
    a1, r1, i1 = blk.solve_systems_of_linear_equations(prm, X, Y, 1e-8, 1000)
    assert plain.last_lockstep_passes[0] == 0 and plain.last_lockstep_passes[1] > 0  # the default keeps its pair passes
    with backend.ResidentProblem(prm, X) as prob:
        assert plain.last_lockstep_passes[1:] == prob.solve_lockstep(Y, 1e-8, 1000, panels=True)[3]
    m = max(i["iterations"] for i in i1)
    assert blk.last_lockstep_passes == (1 + m + m // 50, 0, 0), blk.last_lockstep_passes
    assert all(i["converged"] == 1 for i in i1) and a1.shape == a0.shape and r1.shape == r0.shape
