"""GPU (-m gpu): two right-hand sides per symmetric Gram pass BEYOND the one-pass kernels -- lssvm_mi355_problem_matvec_pair_panels and the lockstep CG
lssvm_mi355_problem_solve_lockstep_panels on the symmetric two-vector panel kernels (tile_launch_f32xv2s.hip: polynomial forms and rbf with folded records on f16x3 and
bf16x6 planes; tile_launch_f64xv2s.hip: rbf and the polynomial forms).

What is asserted (the contract of tests/test_gpu_lockstep_f32_wide.py, whose shape this file has):
  * a two-vector pass against two single-vector passes on the same handle: EXACT equality, whatever the partner vector is;
  * a two-vector pass against the dense float64 product, within the bound tests/cross_check.py has for the single-vector panel kernels: 16 eps (fp32) / 256 eps (fp64) of
    each row's summands;
  * a lockstep solve against fresh one-shot solves per right-hand side: exact equality, and the counters of the pairing;
  * where the panel pair kernels do not apply, and through the entry points WITHOUT `panels`: two single passes, two_vector == 0, the same bits.
"""

import functools

import numpy as np
import pytest

from plssvm_amd import _capi, backend
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.datagen import make_blobs_multiclass
from plssvm_amd.multiclass import one_vs_all_targets
from plssvm_amd.parameter import Parameter

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
KERNELS = {"linear": ("linear", 3), "poly4": ("polynomial", 4), "poly2": ("polynomial", 2), "poly3": ("polynomial", 3), "rbf": ("rbf", 3)}
PLANES = {"f16x3": (F32, {}), "bf16x6": (F32, dict(gram_mode=1)), "fp64": (F64, {})}


def param(kernel, d, cost=1.0):
    name, degree = KERNELS[kernel]
    return Parameter(kernel_type=name, degree=degree, gamma=1.0 / d, coef0=0.5, cost=cost)


def vector_pairs(n, rng, dt):
    """(name, d0, d1): two random normal vectors; a unit vector on a row of the LAST row block beside the zero vector, both ways; (v, v)."""
    v, w = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
    e = np.zeros(n, dtype=dt)
    e[max(n - 4, 0)] = 1.0
    zero = np.zeros(n, dtype=dt)
    return [("random", v, w), ("unit, zero", e, zero), ("zero, unit", zero, e), ("same", v, v)]


def assert_pair_equals_singles(prob, n, rng, two_vector, what, panels=True):
    dt = prob.dtype
    for name, d0, d1 in vector_pairs(n, rng, dt):
        for add in (1.0, -1.0):
            r0, r1 = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
            want0, want1 = prob.matvec(d0, r0, add), prob.matvec(d1, r1, add)
            got0, got1, two = prob.matvec_pair(d0, d1, r0, r1, add, panels=panels)
            differ = np.count_nonzero(got0 != want0), np.count_nonzero(got1 != want1)
            if differ != (0, 0) or two != two_vector:
                print(f"{what}, pair '{name}', add {add:+.0f}: two_vector {two}, {differ[0]} / {differ[1]} of {n} entries differ from the single passes")
            assert two == two_vector, (what, name)
            assert np.array_equal(got0, want0) and np.array_equal(got1, want1), (what, name, add, differ)
            assert np.all(np.isfinite(got0)) and np.all(np.isfinite(got1)), (what, name)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 1
# 100: one row block (diagonal tile only, nothing flushed); 130: two blocks, ragged; 300: several blocks; 647 with j_chunk_tiles = 1: many one-tile work items
SHAPES = [(100, 0), (130, 0), (300, 0), (647, 1)]
POLY = ("poly4", "poly2", "poly3")
# f16x3: 513 = five 128-feature panels, 127 padded columns (rbf: 385 = four); 784 = seven.  bf16x6: 385, 640.  fp64: 257 = five 64-feature panels, 63 padded; 784 = thirteen
CASES = ([("f16x3", k, f) for k in POLY for f in (513, 640, 784)] + [("f16x3", "rbf", f) for f in (385, 640, 784)]
         + [("bf16x6", k, f) for k in POLY + ("rbf",) for f in (385, 640)] + [("fp64", k, f) for k in ("rbf",) + POLY for f in (257, 320, 784)])


@pytest.mark.parametrize("planes,kernel,features", CASES)
def test_pair_pass_is_the_single_pass(planes, kernel, features):
    dt, options = PLANES[planes]
    rng = np.random.default_rng(3000 + features)
    for points, jct in SHAPES:
        X = rng.uniform(-1, 1, size=(points, features)).astype(dt)
        with backend.ResidentProblem(param(kernel, features), X, options=_capi.Options(j_chunk_tiles=jct, **options)) as prob:
            assert_pair_equals_singles(prob, points - 1, rng, True, f"{planes} {kernel} {points} x {features} j_chunk_tiles {jct}")


@pytest.mark.parametrize("planes,kernel,features", [("f16x3", "rbf", 640), ("fp64", "poly3", 320)])
def test_pair_pass_with_weights(planes, kernel, features):
    dt, options = PLANES[planes]
    rng = np.random.default_rng(7)
    X = rng.uniform(-1, 1, size=(300, features)).astype(dt)
    with backend.ResidentProblem(param(kernel, features), X, options=_capi.Options(**options)) as prob:
        prob.set_weights(rng.uniform(0.25, 4.0, size=300))
        assert_pair_equals_singles(prob, 299, rng, True, f"{planes} {kernel} weighted")
        prob.set_weights(None)
        assert_pair_equals_singles(prob, 299, rng, True, f"{planes} {kernel} weights taken back")


# ---------------------------------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("planes,kernel,features", [("f16x3", "rbf", 640), ("bf16x6", "poly3", 385), ("fp64", "rbf", 257), ("fp64", "poly4", 320)])
def test_pair_pass_against_float64(planes, kernel, features):
    """Both vectors' Abar d = K d + d / C + (QA_cost S - q.d) 1 - S q against dense numpy float64, on the scale of each row's summands."""
    dt, options = PLANES[planes]
    N, n = 130, 129
    rng = np.random.default_rng(17)
    X = rng.uniform(-1, 1, size=(N, features)).astype(dt)
    p = param(kernel, features)
    Xa = X.astype(F64)
    G = Xa @ Xa.T
    if kernel == "rbf":
        sq = np.einsum("ij,ij->i", Xa, Xa)
        Ka = np.exp(-p.gamma * np.maximum(sq[:, None] + sq[None, :] - 2.0 * G, 0.0))
    else:
        Ka = (p.gamma * G + p.coef0) ** KERNELS[kernel][1]
    K, q, QA = Ka[:n, :n], Ka[:n, n], Ka[n, n] + 1.0
    d = [rng.uniform(-1, 1, n).astype(dt) for _ in range(2)]
    with backend.ResidentProblem(p, X, options=_capi.Options(**options)) as prob:
        got0, got1, two = prob.matvec_pair(d[0], d[1], np.zeros(n, dt), np.zeros(n, dt), 1.0, panels=True)
    assert two
    bound = 256.0 if dt == F64 else 16.0
    for u, got in enumerate((got0, got1)):
        v = d[u].astype(F64)
        S = float(v.sum())
        truth = K @ v + v + (QA * S - float(q @ v)) - S * q
        scale = np.abs(K) @ np.abs(v) + np.abs(v) + abs(QA * S) + abs(float(q @ v)) + np.abs(S * q)
        err = float(np.max(np.abs(got.astype(F64) - truth) / scale)) / float(np.finfo(dt).eps)
        print(f"{planes} {kernel} {N} x {features}, vector {u}: {err:.2f} eps of the row's summands (bound {bound:.0f})")
        assert np.all(np.isfinite(got)) and err < bound, (planes, kernel, u, err)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 3
COST, POINTS = 100.0, 700
LOCKSTEP = {"f32 rbf": (F32, "rbf", 640, 1e-7), "f32 poly3": (F32, "poly3", 640, 1e-8), "f64 rbf": (F64, "rbf", 320, 1e-10)}  # eps tight: with max_iter = 60 columns run past the refresh of iteration 50


@functools.lru_cache(maxsize=None)
def lockstep_case(dt, features):
    """make_blobs_multiclass(700, features, 5, seed=7) and the seven right-hand sides of tests/test_gpu_lockstep_f32_wide.py (solves of different lengths)."""
    X, y = make_blobs_multiclass(POINTS, features, 5, seed=7, dtype=dt)
    ova = one_vs_all_targets(np.arange(5), y, np.float64)
    rng = np.random.default_rng(3)
    unit = np.zeros(POINTS)
    unit[5] = 1.0
    B = np.stack([ova[0], ova[1], rng.choice([-1.0, 1.0], size=POINTS), rng.standard_normal(POINTS), unit, np.ones(POINTS), 1e6 * ova[2]]).astype(dt)
    B.setflags(write=False)
    return X, B


@pytest.mark.parametrize("case", list(LOCKSTEP))
def test_lockstep_solves_are_the_one_shot_solves(case, max_iter=60):
    dt, kernel, features, eps = LOCKSTEP[case]
    X, B = lockstep_case(dt, features)
    p = param(kernel, features, COST)
    want = [backend.solve_system_of_linear_equations(p, X, b, eps, max_iter) for b in B]
    its = [info["iterations"] for _, _, info in want]
    print(f"{case} eps {eps} max_iter {max_iter}: one-shot iterations {its}")
    assert len(set(its)) > 1 and max(its) > 50, "the right-hand sides must leave the lockstep at different steps, one of them past the residual refresh of iteration 50"
    with backend.ResidentProblem(p, X) as prob:
        for k in (1, 2, 3, 7):
            alphas, rhos, infos, passes = prob.solve_lockstep(B[:k], eps, max_iter, panels=True)
            launches = [info["matvec_launches"] for info in infos]
            print(f"  k = {k}: iterations {[info['iterations'] for info in infos]}, passes {passes}")
            for c in range(k):
                a, rho, info = want[c]
                assert infos[c]["iterations"] == info["iterations"] and infos[c]["converged"] == info["converged"], (k, c, infos[c], info)
                assert np.array_equal(alphas[c], a) and rhos[c] == rho, (k, c, np.count_nonzero(alphas[c] != a), rhos[c], rho)
                assert infos[c]["residuum"] == info["residuum"] and infos[c]["target_residuum"] == info["target_residuum"]
                assert launches[c] == 1 + its[c] + its[c] // 50, (k, c, launches[c], its[c])
            # a step of `active` lanes costs ceil(active / 2) Gram passes, floor(active / 2) of them two-vector passes
            active = [sum(1 for m in launches if m > t) for t in range(max(launches))]
            assert passes == (sum(a // 2 for a in active), sum(a % 2 for a in active)), (k, passes, launches)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4
NOT_APPLICABLE = {
    "symmetric = 0": (dict(symmetric=0), ("poly3", "rbf")),
    "tile_kernel = 1": (dict(tile_kernel=1), ("poly3", "rbf")),
    "gram_mode = 0": (dict(gram_mode=0), ("poly3", "rbf")),
    "rbf_fold = 0": (dict(rbf_fold=0), ("rbf",)),
    "linear": ({}, ("linear",)),
}


@pytest.mark.parametrize("case", list(NOT_APPLICABLE))
def test_where_the_panel_pair_kernels_do_not_apply(case):
    """640 features through the panels entry points: two single passes, two_vector == 0 and the same bits; the lockstep solve is the sequence of solves."""
    options, kernels = NOT_APPLICABLE[case]
    rng = np.random.default_rng(11)
    X = rng.uniform(-1, 1, size=(300, 640)).astype(F32)
    B = np.stack([rng.choice([-1.0, 1.0], size=300), rng.standard_normal(300), np.ones(300)]).astype(F32)
    for kernel in kernels:
        with backend.ResidentProblem(param(kernel, 640), X, options=_capi.Options(**options)) as prob:
            assert_pair_equals_singles(prob, 299, rng, False, f"{kernel} {case}")
            alphas, rhos, infos, passes = prob.solve_lockstep(B, 1e-3, 300, panels=True)
            launches = [info["matvec_launches"] for info in infos]
            assert passes == (0, sum(launches)), (kernel, case, passes, launches)
            for c in range(3):
                prob.cg_begin(B[c], 1e-3)
                prob.cg_step(300)
                a, rho, info = prob.cg_finish()
                assert np.array_equal(alphas[c], a) and rhos[c] == rho and infos[c]["iterations"] == info["iterations"], (kernel, case, c)


def test_the_entry_point_without_panels_keeps_its_routing():
    rng = np.random.default_rng(12)
    X = rng.uniform(-1, 1, size=(300, 640)).astype(F32)
    with backend.ResidentProblem(param("rbf", 640), X) as prob:
        assert_pair_equals_singles(prob, 299, rng, False, "rbf 640 without panels", panels=False)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 5
def test_csvm_solves_five_classes_of_784_features():
    """MI355CSVM.solve_systems_of_linear_equations, float32 rbf, 5 classes, 700 x 784: the per-class one-shot solves, bit for bit."""
    X, y = make_blobs_multiclass(700, 784, 5, seed=11, dtype=F32)
    B = one_vs_all_targets(np.arange(5), y, F32)
    p = Parameter(kernel_type="rbf", gamma=1.0 / 784, cost=1.0)
    alphas, rhos, infos = MI355CSVM(params=p).solve_systems_of_linear_equations(p, X, B, 1e-3, 700)
    for c in range(5):
        a, rho, info = backend.solve_system_of_linear_equations(p, X, B[c], 1e-3, 700)
        assert infos[c]["iterations"] == info["iterations"] and np.array_equal(alphas[c], a) and rhos[c] == rho, c
