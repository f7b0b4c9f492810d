"""GPU (-m gpu): two right-hand sides per symmetric Gram pass in fp32 on 129 ... 512 features -- lssvm_mi355_problem_matvec_pair and the lockstep CG
lssvm_mi355_problem_solve_lockstep on the symmetric one-pass 128-row split kernels (tile_launch_f32v2ws.hip: polynomial forms and rbf with folded records, f16x3 and
bf16x6 planes).

What is asserted, and why (the contract of the fp64 pair kernel, tests/test_gpu_lockstep.py):
  * a two-vector pass against two single-vector passes on the same handle: EXACT equality, whatever the partner vector is.  The kernel value of an element is computed
    once; each vector then runs the fma chains, the butterflies, the column's factor (folded rbf) and the slab reductions of the single-vector kernel in the same order
    on planes of its own.  A unit vector beside the zero vector isolates one row of mirrored column sums and shows anything of one vector that leaks into the other.
  * a lockstep solve against fresh one-shot solves per right-hand side: exact equality of alpha, rho, iterations, residuum, target and `converged`; the counters of
    the pairing (a lane takes part in 1 + it + it // 50 matvecs, a step of `active` lanes costs ceil(active / 2) Gram passes).
  * where the pair kernel does not apply in fp32 (full square, the native kernels, unfolded rbf, the panel kernels, the linear kernel) two single passes run:
    two_vector == 0, passes == (0, sum of the launches), the same bits.
"""

import functools

import numpy as np
import pytest

from plssvm_amd import _capi, backend
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.datagen import make_blobs_multiclass
from plssvm_amd.multiclass import one_vs_all_targets
from plssvm_amd.parameter import Parameter
from plssvm_amd.svc import SVC

pytestmark = pytest.mark.gpu

DT = np.float32
KERNELS = {"linear": ("linear", 3), "poly4": ("polynomial", 4), "poly2": ("polynomial", 2), "poly3": ("polynomial", 3), "rbf": ("rbf", 3)}


def param(kernel, d, cost=1.0):
    name, degree = KERNELS[kernel]
    return Parameter(kernel_type=name, degree=degree, gamma=1.0 / d, coef0=0.5, cost=cost)


def vector_pairs(n, rng):
    """(name, d0, d1): two random normal vectors; a unit vector on a row of the LAST row block beside the zero vector, both ways; (v, v)."""
    v, w = rng.standard_normal(n).astype(DT), rng.standard_normal(n).astype(DT)
    e = np.zeros(n, dtype=DT)
    e[max(n - 4, 0)] = 1.0
    zero = np.zeros(n, dtype=DT)
    return [("random", v, w), ("unit, zero", e, zero), ("zero, unit", zero, e), ("same", v, v)]


def assert_pair_equals_singles(prob, n, rng, two_vector, what):
    for name, d0, d1 in vector_pairs(n, rng):
        for add in (1.0, -1.0):
            r0, r1 = rng.standard_normal(n).astype(DT), rng.standard_normal(n).astype(DT)
            want0, want1 = prob.matvec(d0, r0, add), prob.matvec(d1, r1, add)
            got0, got1, two = prob.matvec_pair(d0, d1, r0, r1, add)
            differ = np.count_nonzero(got0 != want0), np.count_nonzero(got1 != want1)
            if differ != (0, 0) or two != two_vector:
                print(f"{what}, pair '{name}', add {add:+.0f}: two_vector {two}, {differ[0]} / {differ[1]} of {n} entries differ from the single passes")
            assert two == two_vector, (what, name)
            assert np.array_equal(got0, want0) and np.array_equal(got1, want1), (what, name, add, differ)
            assert np.all(np.isfinite(got0)) and np.all(np.isfinite(got1)), (what, name)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 1
# 100: one row block (diagonal tile only, no column record flushed); 130: two blocks, ragged; 300: several blocks; 647 with j_chunk_tiles = 1: many one-tile work items
SHAPES = [(100, 0), (130, 0), (300, 0), (647, 1)]
# 129: three chunks, 63 padded features; then every chunk count up to eight (448, 512: the polynomial forms on f16x3 planes only -- rbf holds three row planes, bf16x6 too)
FEATURES = [129, 192, 256, 320, 384, 448, 512]
PLANES = {"f16x3": None, "bf16x6": dict(gram_mode=1)}


# (beyond 384 features rbf and the bf16x6 planes run the panel kernel: test_where_the_pair_kernel_does_not_apply)
CASES = [(planes, kernel, features) for planes in PLANES for kernel in ("poly4", "poly2", "poly3", "rbf") for features in FEATURES
         if features <= 384 or (planes == "f16x3" and kernel != "rbf")]


@pytest.mark.parametrize("planes,kernel,features", CASES)
def test_pair_pass_is_the_single_pass(planes, kernel, features):
    rng = np.random.default_rng(2000 + features)
    for points, jct in SHAPES:
        X = rng.uniform(-1, 1, size=(points, features)).astype(DT)
        with backend.ResidentProblem(param(kernel, features), X, options=_capi.Options(j_chunk_tiles=jct, **(PLANES[planes] or {}))) as prob:
            assert_pair_equals_singles(prob, points - 1, rng, True, f"{planes} {kernel} {points} x {features} j_chunk_tiles {jct}")


@pytest.mark.parametrize("kernel", ["poly3", "rbf"])
def test_pair_pass_with_weights(kernel):
    rng = np.random.default_rng(7)
    X = rng.uniform(-1, 1, size=(300, 192)).astype(DT)
    with backend.ResidentProblem(param(kernel, 192), X) as prob:
        prob.set_weights(rng.uniform(0.25, 4.0, size=300))
        assert_pair_equals_singles(prob, 299, rng, True, f"{kernel} weighted")
        prob.set_weights(None)
        assert_pair_equals_singles(prob, 299, rng, True, f"{kernel} weights taken back")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 2
COST, POINTS, D = 100.0, 700, 192
EPS = 1e-3        # (as the fp32 cases of tests/test_gpu_lockstep.py)
EPS_TIGHT = 1e-5  # with max_iter = 60: columns that run past the residual refresh of iteration 50


@functools.lru_cache(maxsize=None)
def lockstep_case():
    """make_blobs_multiclass(700, 192, 5, seed=7) and seven right-hand sides whose solves take different numbers of iterations (as tests/test_gpu_lockstep.py builds them)."""
    X, y = make_blobs_multiclass(POINTS, D, 5, seed=7, dtype=DT)
    ova = one_vs_all_targets(np.arange(5), y, np.float64)
    rng = np.random.default_rng(3)
    unit = np.zeros(POINTS)
    unit[5] = 1.0
    B = np.stack([ova[0], ova[1], rng.choice([-1.0, 1.0], size=POINTS), rng.standard_normal(POINTS), unit, np.ones(POINTS), 1e6 * ova[2]]).astype(DT)
    B.setflags(write=False)
    return X, B, np.random.default_rng(5).uniform(0.25, 4.0, size=POINTS)


@functools.lru_cache(maxsize=None)
def one_shot(kernel, weighted, eps, max_iter):
    """The reference side: a fresh one-shot solve per right-hand side (computed once, shared by the tests)."""
    X, B, w = lockstep_case()
    return [backend.solve_system_of_linear_equations(param(kernel, D, COST), X, b, eps, max_iter, sample_weight=w if weighted else None) for b in B]


def assert_lockstep_equals_one_shot(kernel, weighted, eps, max_iter, ks=(1, 2, 3, 7)):
    X, B, w = lockstep_case()
    want = one_shot(kernel, weighted, eps, max_iter)
    its = [info["iterations"] for _, _, info in want]
    print(f"{kernel} float32 weighted {weighted} eps {eps} max_iter {max_iter}: one-shot iterations {its}")
    assert len(set(its)) > 1, "the right-hand sides must leave the lockstep at different steps"
    with backend.ResidentProblem(param(kernel, D, COST), X) as prob:
        if weighted:
            prob.set_weights(w)
        for k in ks:
            alphas, rhos, infos, passes = prob.solve_lockstep(B[:k], eps, max_iter)
            assert alphas.shape == (k, POINTS) and alphas.dtype == DT and rhos.shape == (k,) and len(infos) == k
            launches = [info["matvec_launches"] for info in infos]
            print(f"  k = {k}: iterations {[info['iterations'] for info in infos]}, passes {passes}")
            for c in range(k):
                a, rho, info = want[c]
                assert infos[c]["iterations"] == info["iterations"] and infos[c]["converged"] == info["converged"], (k, c, infos[c], info)
                assert np.array_equal(alphas[c], a) and rhos[c] == rho, (k, c, np.count_nonzero(alphas[c] != a), rhos[c], rho)
                assert infos[c]["residuum"] == info["residuum"] and infos[c]["target_residuum"] == info["target_residuum"] and infos[c]["max_iterations"] == max_iter
                assert launches[c] == 1 + its[c] + its[c] // 50, (k, c, launches[c], its[c])
            assert 2 * passes[0] + passes[1] == sum(launches), (k, passes, launches)
            # a step of `active` lanes costs ceil(active / 2) Gram passes, floor(active / 2) of them two-vector passes
            steps = sum(-(-sum(1 for m in launches if m > t) // 2) for t in range(max(launches)))
            assert passes[0] + passes[1] == steps, (k, passes, steps)
            assert passes[0] == sum(sum(1 for m in launches if m > t) // 2 for t in range(max(launches))) and (passes[0] > 0 or k == 1)
    return its


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kernel", ["poly3", "rbf"])
def test_lockstep_solves_are_the_one_shot_solves(kernel, weighted):
    assert_lockstep_equals_one_shot(kernel, weighted, EPS, POINTS)


@pytest.mark.parametrize("kernel", ["poly3", "rbf"])
def test_lockstep_with_the_residual_refresh_inside(kernel):
    """eps tight, max_iter = 60: at least one column of the ONE-SHOT solves runs past iteration 50, so the refresh pass K x lies inside the lockstep."""
    its = assert_lockstep_equals_one_shot(kernel, False, EPS_TIGHT, 60)
    assert max(its) > 50, "a residual refresh (iteration 50) must lie inside the lockstep"


# ---------------------------------------------------------------------------------------------------------------------------------------------- 3
NOT_APPLICABLE = {
    "symmetric = 0": (dict(symmetric=0), D, ("poly3", "rbf")),
    "tile_kernel = 1": (dict(tile_kernel=1), D, ("poly3", "rbf")),
    "gram_mode = 0": (dict(gram_mode=0), D, ("poly3", "rbf")),
    "rbf_fold = 0": (dict(rbf_fold=0), D, ("rbf",)),
    "600 features": (None, 600, ("poly3", "rbf")),
    "linear": (None, D, ("linear",)),
}


@pytest.mark.parametrize("case", list(NOT_APPLICABLE))
def test_where_the_pair_kernel_does_not_apply(case):
    """Two single passes: two_vector == 0 and the same bits; the lockstep solve is the sequence of solves, passes == (0, sum(launches))."""
    options, features, kernels = NOT_APPLICABLE[case]
    rng = np.random.default_rng(11)
    X = rng.uniform(-1, 1, size=(300, features)).astype(DT)
    B = np.stack([rng.choice([-1.0, 1.0], size=300), rng.standard_normal(300), np.ones(300)]).astype(DT)
    for kernel in kernels:
        with backend.ResidentProblem(param(kernel, features), X, options=_capi.Options(**options) if options else None) as prob:
            assert_pair_equals_singles(prob, 299, rng, False, f"{kernel} {case}")
            alphas, rhos, infos, passes = prob.solve_lockstep(B, EPS, 300)
            launches = [info["matvec_launches"] for info in infos]
            print(f"{kernel} {case}: iterations {[info['iterations'] for info in infos]}, passes {passes}")
            assert passes == (0, sum(launches)), (kernel, case, passes, launches)
            for c in range(3):
                prob.cg_begin(B[c], EPS)
                prob.cg_step(300)
                a, rho, info = prob.cg_finish()
                assert np.array_equal(alphas[c], a) and rhos[c] == rho and infos[c]["iterations"] == info["iterations"], (kernel, case, c)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4
def test_the_handle_after_a_lockstep_solve():
    X, B, _ = lockstep_case()
    want = one_shot("rbf", False, EPS, POINTS)
    rng = np.random.default_rng(13)
    d, r = rng.standard_normal(POINTS - 1).astype(DT), rng.standard_normal(POINTS - 1).astype(DT)
    with backend.ResidentProblem(param("rbf", D, COST), X) as fresh:
        mv = fresh.matvec(d, r)
    with backend.ResidentProblem(param("rbf", D, COST), X) as prob:
        prob.solve_lockstep(B[:3], EPS, POINTS)
        assert np.array_equal(prob.matvec(d, r), mv)
        for c in (3, 0):
            prob.cg_begin(B[c], EPS)
            prob.cg_step(POINTS)
            a, rho, info = prob.cg_finish()
            assert np.array_equal(a, want[c][0]) and rho == want[c][1] and info["iterations"] == want[c][2]["iterations"]
        alphas, rhos, infos, passes = prob.solve_lockstep(B[:2], EPS, POINTS)  # ... and lockstep again after the single solves
        assert passes[0] > 0
        for c in range(2):
            assert np.array_equal(alphas[c], want[c][0]) and rhos[c] == want[c][1]
        assert np.array_equal(prob.matvec(d, r), mv)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 5
@functools.lru_cache(maxsize=None)
def five_classes():
    X, y = make_blobs_multiclass(1000, D, 5, seed=11, dtype=DT)
    return X, y, one_vs_all_targets(np.arange(5), y, DT)


def test_csvm_solves_five_classes_in_lockstep():
    """MI355CSVM.solve_systems_of_linear_equations, float32, 5 classes, 1000 x 192: the per-class one-shot solves, bit for bit, from two-vector passes."""
    X, _, B = five_classes()
    p = Parameter(kernel_type="rbf", gamma=1.0 / D, cost=1.0)
    alphas, rhos, infos = MI355CSVM(params=p).solve_systems_of_linear_equations(p, X, B, EPS, 1000)
    for c in range(5):
        a, rho, info = backend.solve_system_of_linear_equations(p, X, B[c], EPS, 1000)
        assert infos[c]["iterations"] == info["iterations"] and infos[c]["max_iterations"] == 1000
        assert np.array_equal(alphas[c], a) and rhos[c] == rho
    with backend.ResidentProblem(p, X) as prob:  # (the path the class takes: what it costs in passes)
        _, _, infos2, passes = prob.solve_lockstep(B, EPS, 1000)
    launches = [info["matvec_launches"] for info in infos2]
    print(f"five classes: launches {launches}, passes {passes}")
    assert passes[0] > 0 and 2 * passes[0] + passes[1] == sum(launches)
    assert passes[0] == sum(sum(1 for m in launches if m > t) // 2 for t in range(max(launches)))


def test_svc_fits_five_classes_with_the_one_shot_solves():
    X, y, B = five_classes()
    clf = SVC(kernel="rbf", C=1.0, gamma=1.0 / D, tol=EPS, real_type=DT).fit(X, y)
    p = Parameter(kernel_type="rbf", gamma=1.0 / D, cost=1.0)
    for c in range(5):
        a, rho, _ = backend.solve_system_of_linear_equations(p, X, B[c], EPS, 1000)
        assert np.array_equal(clf.dual_coef_[c], a), (c, np.count_nonzero(clf.dual_coef_[c] != a))
