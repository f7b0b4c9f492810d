"""GPU (-m gpu): two right-hand sides per symmetric Gram pass in fp64 -- lssvm_mi355_problem_matvec_pair and the lockstep CG lssvm_mi355_problem_solve_lockstep.

What is asserted, and why:
  * a two-vector pass against two single-vector passes on the same handle: EXACT equality, whatever the partner vector is.  The kernel value of an element is computed
    once; each vector then runs the fma chains, the butterflies and the slab reductions of the single-vector kernel in the same order on planes of its own, so there is
    nothing to tolerate -- and nothing of one vector may show in the other (unit vector beside the zero vector).
  * a lockstep solve against fresh one-shot solves per right-hand side: exact equality of alpha, rho, the iteration count and `converged` -- every lane runs the O(n)
    kernels of the single solve on the bits the pair pass gives it.  The right-hand sides are chosen so that their iteration counts differ (lanes leave at different
    steps, the pairing changes) and reach past the residual refresh of iteration 50.
  * the counters: a lane takes part in exactly 1 + it + it / 50 matvecs (nothing is enqueued ahead of a stop test), a step of `active` lanes costs
    ceil(active / 2) Gram passes, and every matvec of a lane is one half of a two-vector pass or a single pass.  Where the pair kernel does not apply (fp32) the
    right-hand sides are solved one after the other: no two-vector pass, and as many single passes as matvecs -- the ceil(active / 2) count belongs to the pairing
    and cannot hold there beside passes[0] == 0.
"""

import functools

import numpy as np
import pytest

from plssvm_amd import _capi, backend
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.datagen import make_blobs_multiclass
from plssvm_amd.exceptions import PlssvmError
from plssvm_amd.multiclass import one_vs_all_targets
from plssvm_amd.parameter import Parameter
from plssvm_amd.svc import SVC

pytestmark = pytest.mark.gpu

KERNELS = {"linear": ("linear", 3), "poly2": ("polynomial", 2), "poly3": ("polynomial", 3), "poly4": ("polynomial", 4), "rbf": ("rbf", 3)}


def param(kernel, d, cost=1.0):
    name, degree = KERNELS[kernel]
    return Parameter(kernel_type=name, degree=degree, gamma=1.0 / d, coef0=0.5, cost=cost)


def vector_pairs(n, rng, dt):
    """(name, d0, d1): two random normal vectors; a unit vector on a row of block 1 (the last block of a one-block problem) beside the zero vector, both ways; (v, v)."""
    v, w = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
    e = np.zeros(n, dtype=dt)
    e[min(128 + 3, n - 1)] = 1.0
    zero = np.zeros(n, dtype=dt)
    return [("random", v, w), ("unit, zero", e, zero), ("zero, unit", zero, e), ("same", v, v)]


def assert_pair_equals_singles(prob, n, rng, two_vector, what):
    dt = prob.dtype
    for name, d0, d1 in vector_pairs(n, rng, dt):
        for add in (1.0, -1.0):
            r0, r1 = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
            want0, want1 = prob.matvec(d0, r0, add), prob.matvec(d1, r1, add)
            got0, got1, two = prob.matvec_pair(d0, d1, r0, r1, add)
            differ = np.count_nonzero(got0 != want0), np.count_nonzero(got1 != want1)
            if differ != (0, 0) or two != two_vector:
                print(f"{what}, pair '{name}', add {add:+.0f}: two_vector {two}, {differ[0]} / {differ[1]} of {n} entries differ from the single passes")
            assert two == two_vector, (what, name)
            assert np.array_equal(got0, want0) and np.array_equal(got1, want1), (what, name, add, differ)
            if name == "same":
                s0, s1, _ = prob.matvec_pair(d0, d1, r0, r0, add)
                assert np.array_equal(s0, s1), (what, "both halves of (v, v)")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 1
# 100: one row block (diagonal tile only, no column record flushed); 130: two blocks, ragged; 300: several blocks; 647: the default column chunks and j_chunk_tiles = 1
# (many chunks per row block, one-tile work items)
SHAPES = [(100, 0), (130, 0), (300, 0), (647, 0), (647, 1)]
# 5: one chunk (two steps per sub-tile, only the checked hand-over runs); 17: two; 64: four chunks, two workgroups per CU; 72: five, one workgroup per CU; 200: padded to the
# next instantiated chunk count (14); 256: sixteen
FEATURES = [5, 17, 64, 72, 200, 256]


@pytest.mark.parametrize("features", FEATURES)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_pair_pass_is_the_single_pass(kernel, features):
    rng = np.random.default_rng(1000 + features)
    for points, jct in SHAPES:
        X = rng.uniform(-1, 1, size=(points, features))
        with backend.ResidentProblem(param(kernel, features), X, options=_capi.Options(j_chunk_tiles=jct)) as prob:
            assert_pair_equals_singles(prob, points - 1, rng, True, f"{kernel} {points} x {features} j_chunk_tiles {jct}")


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_pair_pass_with_weights(kernel):
    rng = np.random.default_rng(7)
    X = rng.uniform(-1, 1, size=(300, 17))
    with backend.ResidentProblem(param(kernel, 17), X) as prob:
        prob.set_weights(rng.uniform(0.25, 4.0, size=300))
        assert_pair_equals_singles(prob, 299, rng, True, f"{kernel} weighted")
        prob.set_weights(None)
        assert_pair_equals_singles(prob, 299, rng, True, f"{kernel} weights taken back")


@pytest.mark.parametrize("case", ["symmetric = 0", "fp32", "300 features", "tile_kernel = 1"])
def test_pair_call_where_the_pair_kernel_does_not_apply(case):
    """Two single passes: two_vector == 0 and, of course, the same bits."""
    rng = np.random.default_rng(11)
    features = 300 if case == "300 features" else 40
    X = rng.uniform(-1, 1, size=(300, features)).astype(np.float32 if case == "fp32" else np.float64)
    options = {"symmetric = 0": _capi.Options(symmetric=0), "tile_kernel = 1": _capi.Options(tile_kernel=1)}.get(case)
    for kernel in ("linear", "poly3", "rbf"):
        with backend.ResidentProblem(param(kernel, features), X, options=options) as prob:
            assert_pair_equals_singles(prob, 299, rng, False, f"{kernel} {case}")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 2
EPS, COST, POINTS = 1e-8, 100.0, 700
EPS_F32 = 1e-3  # (fp32 cannot reach 1e-8: the residual refresh of iteration 50 puts the true residual back)


@functools.lru_cache(maxsize=None)
def lockstep_case(dt):
    """make_blobs_multiclass(700, 20, 5, seed=7) and seven right-hand sides whose solves take different numbers of iterations."""
    X, y = make_blobs_multiclass(POINTS, 20, 5, seed=7, dtype=dt)
    ova = one_vs_all_targets(np.arange(5), y, np.float64)
    rng = np.random.default_rng(3)
    unit = np.zeros(POINTS)
    unit[5] = 1.0
    B = np.stack([ova[0], ova[1], rng.choice([-1.0, 1.0], size=POINTS), rng.standard_normal(POINTS), unit, np.ones(POINTS), 1e6 * ova[2]]).astype(dt)
    B.setflags(write=False)
    return X, B, np.random.default_rng(5).uniform(0.25, 4.0, size=POINTS)


@functools.lru_cache(maxsize=None)
def one_shot(kernel, dt, weighted, max_iter):
    """The reference side: a fresh one-shot solve per right-hand side (computed once, shared by the tests)."""
    X, B, w = lockstep_case(dt)
    eps = EPS if dt == np.float64 else EPS_F32
    return [backend.solve_system_of_linear_equations(param(kernel, 20, COST), X, b, eps, max_iter, sample_weight=w if weighted else None) for b in B]


def assert_lockstep_equals_one_shot(kernel, dt, weighted, max_iter, two_vector):
    X, B, w = lockstep_case(dt)
    eps = EPS if dt == np.float64 else EPS_F32
    want = one_shot(kernel, dt, weighted, max_iter)
    its = [info["iterations"] for _, _, info in want]
    print(f"{kernel} {np.dtype(dt).name} weighted {weighted} max_iter {max_iter}: one-shot iterations {its}")
    assert len(set(its)) > 1 or max_iter == 30, "the right-hand sides must leave the lockstep at different steps"
    with backend.ResidentProblem(param(kernel, 20, COST), X) as prob:
        if weighted:
            prob.set_weights(w)
        for k in (1, 2, 3, 7):
            alphas, rhos, infos, passes = prob.solve_lockstep(B[:k], eps, max_iter)
            assert alphas.shape == (k, POINTS) and alphas.dtype == dt and rhos.shape == (k,) and len(infos) == k
            launches = [info["matvec_launches"] for info in infos]
            print(f"  k = {k}: iterations {[info['iterations'] for info in infos]}, passes {passes}")
            for c in range(k):
                a, rho, info = want[c]
                assert infos[c]["iterations"] == info["iterations"] and infos[c]["converged"] == info["converged"], (k, c, infos[c], info)
                assert np.array_equal(alphas[c], a) and rhos[c] == rho, (k, c, np.count_nonzero(alphas[c] != a), rhos[c], rho)
                assert infos[c]["residuum"] == info["residuum"] and infos[c]["target_residuum"] == info["target_residuum"] and infos[c]["max_iterations"] == max_iter
                assert launches[c] == 1 + its[c] + its[c] // 50, (k, c, launches[c], its[c])
            assert 2 * passes[0] + passes[1] == sum(launches), (k, passes, launches)
            if two_vector:  # a step of `active` lanes costs ceil(active / 2) Gram passes, floor(active / 2) of them two-vector passes
                steps = sum(-(-sum(1 for m in launches if m > t) // 2) for t in range(max(launches)))
                assert passes[0] + passes[1] == steps, (k, passes, steps)
                assert passes[0] == sum(sum(1 for m in launches if m > t) // 2 for t in range(max(launches))) and (passes[0] > 0 or k == 1)
            else:  # no pair kernel: every matvec of every right-hand side is a single-vector pass of its own (with passes[0] == 0 the two sums above can only agree for k = 1)
                assert passes == (0, sum(launches)), (k, passes, launches)
    return its


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kernel", ["poly3", "rbf", "linear"])
def test_lockstep_solves_are_the_one_shot_solves(kernel, weighted):
    its = assert_lockstep_equals_one_shot(kernel, np.float64, weighted, POINTS, True)
    if kernel != "linear" and not weighted:
        assert max(its) > 50, "a residual refresh (iteration 50) must lie inside the lockstep"


@pytest.mark.parametrize("kernel", ["poly3", "rbf"])
def test_lockstep_stops_every_lane_at_max_iter(kernel):
    its = assert_lockstep_equals_one_shot(kernel, np.float64, False, 30, True)
    assert its == [30] * 7 and not any(info["converged"] for _, _, info in one_shot(kernel, np.float64, False, 30))


@pytest.mark.parametrize("kernel", ["poly3", "rbf", "linear"])
def test_lockstep_in_fp32_is_the_sequence_of_solves(kernel):
    assert_lockstep_equals_one_shot(kernel, np.float32, False, POINTS, False)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 3
def test_the_handle_after_a_lockstep_solve():
    X, B, _ = lockstep_case(np.float64)
    want = one_shot("rbf", np.float64, False, POINTS)
    with backend.ResidentProblem(param("rbf", 20, COST), X) as prob:
        prob.solve_lockstep(B[:3], EPS, POINTS)
        for c in (3, 0):
            prob.cg_begin(B[c], EPS)
            with pytest.raises(PlssvmError):  # between cg_begin and cg_finish
                prob.solve_lockstep(B[:2], EPS, POINTS)
            with pytest.raises(PlssvmError):
                prob.matvec_pair(B[0][:-1], B[1][:-1], B[0][:-1], B[1][:-1])
            prob.cg_step(POINTS)
            a, rho, info = prob.cg_finish()
            assert np.array_equal(a, want[c][0]) and rho == want[c][1] and info["iterations"] == want[c][2]["iterations"]
        alphas, rhos, infos, _ = prob.solve_lockstep(B[:2], EPS, POINTS)  # ... and lockstep again after the single solves
        for c in range(2):
            assert np.array_equal(alphas[c], want[c][0]) and rhos[c] == want[c][1]


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4
def test_csvm_solves_five_classes_in_lockstep():
    """MI355CSVM.solve_systems_of_linear_equations, fp64, 5 classes, 3000 x 32: the per-class one-shot solves, bit for bit."""
    X, y = make_blobs_multiclass(3000, 32, 5, seed=7, dtype=np.float64)
    B = one_vs_all_targets(np.arange(5), y, np.float64)
    p = Parameter(kernel_type="rbf", gamma=1.0 / 32, cost=1.0)
    alphas, rhos, infos = MI355CSVM(params=p).solve_systems_of_linear_equations(p, X, B, 1e-8, 3000)
    for c in range(5):
        a, rho, info = backend.solve_system_of_linear_equations(p, X, B[c], 1e-8, 3000)
        assert infos[c]["iterations"] == info["iterations"] and infos[c]["max_iterations"] == 3000
        assert np.array_equal(alphas[c], a) and rhos[c] == rho


def test_svc_predicts_what_the_one_shot_solves_predict():
    X, y = make_blobs_multiclass(2000, 32, 5, seed=11, dtype=np.float64)
    Xt, yt, Xh = X[:1000], y[:1000], X[1000:]
    clf = SVC(kernel="rbf", C=1.0, gamma=1.0 / 32, tol=1e-6, real_type=np.float64).fit(Xt, yt)
    p = Parameter(kernel_type="rbf", gamma=1.0 / 32, cost=1.0)
    B = one_vs_all_targets(np.arange(5), yt, np.float64)
    values = np.empty((1000, 5))
    for c in range(5):
        a, rho, _ = backend.solve_system_of_linear_equations(p, Xt, B[c], 1e-6, 1000)
        assert np.array_equal(clf.dual_coef_[c], a)
        values[:, c], _ = backend.predict_values(p, Xt, a, float(rho), None, Xh)
    assert np.array_equal(clf.predict(Xh), np.argmax(values, axis=1))
