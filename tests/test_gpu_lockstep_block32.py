"""GPU (-m gpu): the fp32 block lockstep CG -- lssvm_mi355_problem_matvec_block32 / _solve_lockstep_block32, ``MI355CSVM(lockstep="block32")`` -- and the sixteen-vector
symmetric fp32 kernel behind it (tile_matvec_f32_blk_sym, plssvm_amd/csrc/lssvm_tile_f32_blk_sym.hip.hpp).

matvec_block(..., block32=True): against numpy in ``np.longdouble`` on the float32 data -- ret = Abar V, the system of tests/test_gpu_lockstep_block.py -- in units
u_iv = eps32 * sum_j |v_jv k_ij|.  e_old is the largest error of the single-vector ``matvec`` on the same case (both evaluate every kernel value by the same plane
products, so the difference is the summation's share), e_new that of the block call; asserted: e_new <= e_old + (L + 3).  L, the additions in the longest chain of one
value, from the sum order the kernel defines, an fp32 MFMA counted as four additions (the rule of tests/test_gpu_predictor_block32.py), with T column tiles of 128:
  row product: 32 MFMAs (of four columns) per tile over the work item's tiles, 128 T over all chunks together, then one addition per chunk slab (at most T chunks);
  mirror: 8 MFMAs (of four rows) over a wave's 32 rows (32), the column's factor (rbf: 1), the four waves (2), then the row blocks' records in fold order
  (k_reduce_colslab: at most T records over its eight groups, 7 additions of the groups' sums, one into K v), and the row sums on top (1).
L = 128 T + T + 32 + 1 + 2 + T + 7 + 1 + 1 = 130 T + 44.  A wrong index, a dropped sub-tile or a swapped operand is an error of 1 / eps32 units.
Measured on an MI355X over the 31 cases: e_new - e_old at most 1.28 (rbf, 128 rows: 2.20 against 0.92), e_new at most 31.04 where e_old is 31.04 (poly2, 64 rows).  (The two-band shape, 6 100 points with colslab_band_mb = 1, is
ONE band in fp32 -- 1 128 records of 512 bytes; two bands need more than 2 048 records, i.e. 65 row blocks: the 8 300-point case with colslab_band_mb = 1 has them, on the
second geometry.)
solve_lockstep_block(..., block32=True): against the dense float64 reduced system, the true relative residual within the factor 2 of tests/test_gpu_cost_path.py, with
the existing ``solve_lockstep`` held to the same bound.  Bits: repeats, a vector alone against its place in a block, a right-hand side alone against its column, every
declined case against ``solve_lockstep(..., panels=True)``, an fp64 problem against the ``_block`` calls."""

import functools

import numpy as np
import pytest

from plssvm_amd import backend
from plssvm_amd._capi import Options
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.parameter import KernelFunctionType, Parameter

pytestmark = pytest.mark.gpu

LD = np.longdouble
F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
FORMS = {"rbf": ("rbf", 3, 0.0), "poly5": ("polynomial", 5, 0.5), "poly2": ("polynomial", 2, 0.0), "poly3": ("polynomial", 3, -0.25)}
BF = {"gram_mode": 1}  # bf16x6 planes (the default at these widths: f16x3)

# (form, n rows of the system, features, vectors, options)
CASES = ([(f, n, 17, 3, o) for f, n, o in zip(("rbf", "poly5", "poly2", "poly3", "rbf"), (1, 63, 64, 65, 128), ({}, BF, {}, BF, {}))]      # one row block: only the diagonal, no mirror
         + [("poly3", 129, 20, 5, {}), ("rbf", 200, 20, 5, BF)]                                                                         # the first mirrored tile, a padded row block
         + [(f, 300, 33, 16, o) for f in FORMS for o in ({}, BF)]                                                                        # mirror sums from two row blocks, every form x plane kind
         + [("rbf", 777, 24, 7, {"j_chunk_tiles": 1}), ("poly2", 777, 24, 7, {"j_chunk_tiles": 1, **BF})]                                # several column chunks
         + [(f, 300, d, 4, o) for f, d, o in zip(("rbf", "poly5", "poly3", "poly2", "rbf", "poly3"), (1, 32, 33, 64, 65, 128), ({}, BF, {}, {}, BF, {}))]  # k32 step, chunk edge, both NK64
         + [("rbf", 300, 40, k, {}) for k in (1, 2, 15, 17, 33)]                                                                         # vector groups
         + [("poly3", 6100, 8, 2, {"colslab_band_mb": 1})]                                                                               # 48 row blocks
         + [("rbf", 8299, 8, 3, {}), ("poly2", 8299, 8, 3, {"colslab_band_mb": 1, **BF})])                                               # 65 row blocks: the 256-row form; two bands


@functools.lru_cache(maxsize=None)
def points(n, d):
    X = np.random.default_rng(100 * n + d).uniform(-1.0, 1.0, size=(n + 1, d)).astype(F32)
    X.setflags(write=False)
    return X


def kernel_rows(prm, X, Z, dt):
    X, Z = X.astype(dt), Z.astype(dt)
    G = X @ Z.T
    if prm.kernel_type == KernelFunctionType.RBF:
        return np.exp(-dt(prm.gamma) * ((X * X).sum(axis=1)[:, None] + (Z * Z).sum(axis=1)[None, :] - 2 * G))
    return (dt(prm.gamma) * G + dt(prm.coef0)) ** int(prm.degree)


def reference(prm, X, V, rows):
    """(Abar V, units u_iv) at `rows` of the system, in longdouble on the float32 data"""
    n = X.shape[0] - 1
    K = kernel_rows(prm, X[rows], X, LD)  # [rows, n + 1]
    qall = kernel_rows(prm, X[n:], X, LD)[0]
    q, QA, Vl = qall[:n], qall[n] + 1 / LD(prm.cost), V.astype(LD)
    S, QV = Vl.sum(axis=1), Vl @ q
    want = K[:, :n] @ Vl.T + Vl[:, rows].T / LD(prm.cost) + (QA * S - QV)[None, :] - q[rows, None] * S[None, :]
    return want, EPS32 * (np.abs(K[:, :n]) @ np.abs(Vl).T)


@pytest.mark.parametrize("form, n, d, k, opts", CASES, ids=lambda c: str(c))
def test_matvec_block32_against_longdouble(form, n, d, k, opts):
    kernel, degree, coef0 = FORMS[form]
    prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=coef0, cost=2.0)
    X = points(n, d)
    V = np.random.default_rng(7 + k).standard_normal((k, n)).astype(F32)
    edges = [128 * 34, 128 * 46] if n > 8000 else [128 * 34]  # row-block edges (8 299 rows: 46 is the band edge of the two-band case, and a block-pair edge)
    rows = np.arange(n) if n <= 1000 else np.unique(np.concatenate([np.arange(0, n, 97)] + [np.arange(e - 3, e + 3) for e in edges] + [[n - 1]]))
    want, unit = reference(prm, X, V, rows)
    T = -(-n // 128)
    L = 130 * T + 44
    zero = np.zeros(n, F32)
    with backend.ResidentProblem(prm, X, options=Options(**opts)) as prob:
        old = np.stack([prob.matvec(V[v], zero) for v in range(k)])
        got, block = prob.matvec_block(V, np.zeros_like(V), block32=True)
        again, _ = prob.matvec_block(V, np.zeros_like(V), block32=True)
        assert np.array_equal(prob.matvec(V[0], zero), old[0])  # the problem's own pass (on 65 row blocks: its 256-row geometry) keeps its bits behind a block pass
    e_new, e_old = float(np.max(np.abs(got[:, rows].T - want) / unit)), float(np.max(np.abs(old[:, rows].T - want) / unit))
    print(f"{form} n={n} d={d} k={k} {opts}: e_new {e_new:.2f}, e_old {e_old:.2f} units, e_new - e_old {e_new - e_old:.2f}, L = {L}")
    assert block and got.shape == (k, n) and np.all(np.isfinite(got))
    assert np.array_equal(got, again)  # a repeat has the same bits
    assert e_new <= e_old + (L + 3), (e_new, e_old, L)


def test_a_vector_alone_has_the_bits_of_its_place_in_a_block():
    prm, X = Parameter(kernel_type="rbf", gamma=1.0 / 40, cost=2.0), points(300, 40)
    V = np.random.default_rng(5).standard_normal((17, 300)).astype(F32)
    with backend.ResidentProblem(prm, X) as prob:
        got, _ = prob.matvec_block(V, np.zeros_like(V), block32=True)
        for v in (0, 5, 15, 16):  # slots 0, 5, 15 of the first group, slot 0 of the second
            assert np.array_equal(prob.matvec_block(V[v:v + 1], np.zeros((1, 300), F32), block32=True)[0][0], got[v]), v


SOLVES = {"rbf": (Parameter(kernel_type="rbf", gamma=0.2, cost=100.0), 5), "polynomial": (Parameter(kernel_type="polynomial", degree=3, gamma=1.0 / 16, coef0=1.0, cost=1.0), 16)}


@functools.lru_cache(maxsize=None)
def dense(kernel):
    """(A, X) of the reduced system of 777 points, float64 on the float32 data: computed once per kernel, shared, never modified"""
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
def test_solve_lockstep_block32_against_dense_solves(kernel, k):
    A, X = dense(kernel)
    n, eps = 776, 1e-3  # (the eps of the fp32 cases of tests/test_gpu_lockstep.py)
    Y = np.where(np.random.default_rng(k).standard_normal((k, 777)) > 0.0, 1.0, -1.0).astype(F32)
    with backend.ResidentProblem(SOLVES[kernel][0], X) as prob:
        ref_alphas, _, ref_infos, _ = prob.solve_lockstep(Y, eps, 2000)
        alphas, rhos, infos, passes = prob.solve_lockstep_block(Y, eps, 2000, block32=True)
        alone = {c: prob.solve_lockstep_block(Y[c:c + 1], eps, 2000, block32=True) for c in sorted({0, k - 1})}
    for name, al, inf in (("solve_lockstep", ref_alphas, ref_infos), ("block32", alphas, infos)):  # (a bound the data cannot meet shows on the existing path first)
        for c in range(k):
            b = Y[c, :n].astype(np.float64) - float(Y[c, n])
            res, d0 = np.linalg.norm(b - A @ al[c, :n].astype(np.float64)), np.linalg.norm(b - A @ np.ones(n))
            print(f"  {kernel} {name} rhs {c} of {k}: {inf[c]['iterations']} iterations, |b - A x| / d0 {res / d0:.2e} (<= {2 * eps:.0e})")
            assert inf[c]["converged"] == 1 and res <= 2.0 * eps * d0, (name, c, res / d0, inf[c])
    m = max(info["iterations"] for info in infos)
    if k <= 16:
        assert list(passes) == [1 + m + m // 50, 0, 0], (passes, m)
    assert passes[0] > 0 and passes[1] == passes[2] == 0
    for c, (a1, r1, i1, _) in alone.items():  # column c has the bits of the call with that right-hand side alone
        assert np.array_equal(a1[0], alphas[c]) and r1[0] == rhos[c] and i1[0]["iterations"] == infos[c]["iterations"], c


@pytest.mark.parametrize("case", ["linear", "200_features", "tile_kernel_1", "symmetric_0", "negative_degree", "gram_mode_0", "fp64"])
def test_a_declined_case_is_solve_lockstep_panels(case):
    dt = np.float64 if case == "fp64" else F32
    d = 200 if case == "200_features" else 12
    X = np.random.default_rng(3).uniform(0.5, 1.5, size=(400, d)).astype(dt)  # (a negative power needs bases away from 0)
    Y = np.where(np.random.default_rng(4).standard_normal((3, 400)) > 0.0, 1.0, -1.0).astype(dt)
    prm = {"linear": Parameter(kernel_type="linear"), "negative_degree": Parameter(kernel_type="polynomial", degree=-1, gamma=1.0 / d, coef0=1.0)}.get(case, Parameter(kernel_type="rbf", gamma=1.0 / d))
    opts = {"tile_kernel_1": {"tile_kernel": 1}, "symmetric_0": {"symmetric": 0}, "gram_mode_0": {"gram_mode": 0}}.get(case, {})
    eps = 1e-8 if case == "fp64" else 1e-3
    V = np.ascontiguousarray(Y[:, :399])
    with backend.ResidentProblem(prm, X, options=Options(**opts)) as prob:
        # fp32 where the kernel does not apply: the _panels calls; fp64: the _block calls
        a0, r0, i0, p0 = prob.solve_lockstep_block(Y, eps, 500) if case == "fp64" else prob.solve_lockstep(Y, eps, 500, panels=True)
        a1, r1, i1, p1 = prob.solve_lockstep_block(Y, eps, 500, block32=True)
        mv, block = prob.matvec_block(V, np.zeros_like(V), block32=True)
        if case == "fp64":
            mv0, block0 = prob.matvec_block(V, np.zeros_like(V))
            assert block and block0 and np.array_equal(mv, mv0)
        else:
            assert not block and np.array_equal(mv[2], prob.matvec(V[2], np.zeros(399, dt)))
    kept = ("iterations", "converged", "residuum", "initial_residuum", "target_residuum", "matvec_launches", "symmetric", "gram_mode")
    assert np.array_equal(a0, a1) and np.array_equal(r0, r1)
    assert [{n: i[n] for n in kept} for i in i0] == [{n: i[n] for n in kept} for i in i1]
    assert tuple(p1) == tuple(p0) if case == "fp64" else (p1[0] == 0 and tuple(p1[1:]) == tuple(p0)), (p0, p1)


def test_csvm_lockstep_block32_reaches_the_block_passes():
    prm = Parameter(kernel_type="rbf", gamma=0.2, cost=10.0)
    X = points(599, 5)
    Y = np.where(np.arange(600)[None, :] % 5 == np.arange(5)[:, None], 1.0, -1.0).astype(F32)  # a 5-class one-vs-all target
    plain, blk = MI355CSVM(), MI355CSVM(lockstep="block32")
    a0, r0, i0 = plain.solve_systems_of_linear_equations(prm, X, Y, 1e-3, 1000)
    a1, r1, i1 = blk.solve_systems_of_linear_equations(prm, X, Y, 1e-3, 1000)
    assert plain.last_lockstep_passes[0] == 0  # the default object never reaches the block passes
    m = max(i["iterations"] for i in i1)
    assert blk.last_lockstep_passes == (1 + m + m // 50, 0, 0), blk.last_lockstep_passes
    assert all(i["converged"] == 1 for i in i1) and a1.shape == a0.shape and r1.shape == r0.shape
