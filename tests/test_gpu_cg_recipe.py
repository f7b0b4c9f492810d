"""GPU (-m gpu): one CG recipe behind cg_begin / cg_step / cg_finish and the lockstep lanes -- how a solve is cut into cg_step calls does not show in the bits.

The single solve, the lanes of solve_lockstep and the fp64 CG of the refinement run the same O(n) steps (CgSteps, lssvm_solver.hip); what differs between two ways of
stepping through a solve is only WHEN the host enqueues: cg_step(60) puts the direction update and the next implicit matvec into the queue ahead of every stop test but
the last, sixty calls of cg_step(1) never do, calls of cg_step(7) mix both.  None of that touches x or r, so alpha, rho, the residuum and the iteration count are asserted
EQUAL, exactly, across the three patterns -- and in fp64 equal to solve_lockstep of the same right-hand side, alone (the single-vector pass on a lane) and as the first
of two (one half of a two-vector pass), stopped by max_iter at the same iteration.

Cases: the 700 x 20 case of test_gpu_lockstep.py (six row blocks; 60 iterations at eps = 1e-30, so the residual refresh of iteration 50 lies inside and the stop test
never fires) and 130 x 17 (two row blocks, the second ragged; 12 iterations), rbf and polynomial degree 3, fp32 and fp64, with and without weights.
"""

import functools

import numpy as np
import pytest

from plssvm_amd import backend
from plssvm_amd.datagen import make_blobs_multiclass
from plssvm_amd.multiclass import one_vs_all_targets
from plssvm_amd.parameter import Parameter

pytestmark = pytest.mark.gpu

KERNELS = {"poly3": "polynomial", "rbf": "rbf"}
COST, EPS = 100.0, 1e-30
# (points, features, iterations, the three ways to cut them into cg_step calls)
CASES = {
    "700x20": (700, 20, 60, ([60], [1] * 60, [7] * 8 + [4])),
    "130x17": (130, 17, 12, ([12], [1] * 12, [5, 5, 2])),
}


@functools.lru_cache(maxsize=None)
def case_data(points, features, dt):
    X, y = make_blobs_multiclass(points, features, 5, seed=7, dtype=dt)
    B = one_vs_all_targets(np.arange(5), y, np.float64)[:2].astype(dt)
    w = np.random.default_rng(5).uniform(0.25, 4.0, size=points)
    for a in (X, B, w):
        a.setflags(write=False)
    return X, B, w


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("case", list(CASES))
def test_the_cut_into_cg_step_calls_does_not_show_in_the_bits(case, kernel, dt, weighted):
    points, features, iterations, patterns = CASES[case]
    X, B, w = case_data(points, features, dt)
    p = Parameter(kernel_type=KERNELS[kernel], degree=3, gamma=1.0 / features, coef0=0.5, cost=COST)
    with backend.ResidentProblem(p, X) as prob:
        if weighted:
            prob.set_weights(w)
        runs = []
        for steps in patterns:
            assert sum(steps) == iterations
            prob.cg_begin(B[0], EPS)
            for k in steps:
                assert not prob.cg_step(k), "the stop test must not fire"
            alpha, rho, info = prob.cg_finish()
            print(f"{case} {kernel} {np.dtype(dt).name} weighted {weighted}, {len(steps)} cg_step calls: iterations {info['iterations']} residuum {info['residuum']!r} "
                  f"rho {rho!r} matvecs {info['matvec_launches']}")
            runs.append((alpha, rho, info["residuum"], info["iterations"]))
        if dt == np.float64:  # the lanes: alone on a single-vector pass, and as one half of two-vector passes
            for k in (1, 2):
                alphas, rhos, infos, passes = prob.solve_lockstep(B[:k], EPS, iterations)
                print(f"  solve_lockstep k = {k}: iterations {infos[0]['iterations']} residuum {infos[0]['residuum']!r} rho {rhos[0]!r} passes {passes}")
                assert (passes[0] > 0) == (k == 2), passes
                runs.append((alphas[0], rhos[0], infos[0]["residuum"], infos[0]["iterations"]))
    alpha, rho, residuum, its = runs[0]
    assert its == iterations and np.all(np.isfinite(alpha)) and np.isfinite(rho) and residuum > 0.0
    for other in runs[1:]:
        assert np.array_equal(other[0], alpha), np.count_nonzero(other[0] != alpha)
        assert other[1] == rho and other[2] == residuum and other[3] == iterations, (other[1:], (rho, residuum, iterations))
