"""GPU (-m gpu): the lanes' Gram pass over MORE THAN ONE row-block band (Options(colslab_band_mb=1)).

The problem's own pass and the lanes' pass (one or two vectors) run one walk over the bands: per band the tile kernel and, per vector, the fold of the band's mirrored
column sums; after the bands the row slabs per vector.  The shapes are the smallest with two bands at a 1 MiB slab -- a record is 128 reals, so more than
1 MiB / (128 * sizeof(real)) block pairs: fp64 46 row blocks (46 * 45 / 2 = 1035 > 1024), fp32 65 (2080 > 2048; 192 features: the 256-row workgroups are off and the
two-vector symmetric split kernel applies).  Three right-hand sides in lockstep give one two-vector pass and one single-vector lane pass per step.

What is asserted: both kinds of pass ran, every matvec took at least two tile launches, and every column is EXACTLY the one-shot solve of that right-hand side with the
same options (whose Gram passes are the problem's own) -- alpha, rho, the residuum and the iteration count.  Nothing is tolerated: per vector the lanes' pass runs the
operations of the single-vector pass in the same order.
"""

import numpy as np
import pytest

from plssvm_amd import _capi, backend
from plssvm_amd.datagen import make_blobs_multiclass
from plssvm_amd.multiclass import one_vs_all_targets
from plssvm_amd.parameter import Parameter

pytestmark = pytest.mark.gpu

KERNELS = {"poly3": "polynomial", "rbf": "rbf"}
EPS, MAX_ITER, RHS = 1e-30, 6, 3  # (no stop before max_iter: a handful of Gram passes per case)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("dt, points, features", [(np.float64, 5900, 20), (np.float32, 8400, 192)])
def test_lockstep_over_two_bands_is_the_one_shot_solve(dt, points, features, kernel):
    X, labels = make_blobs_multiclass(points, features, RHS, seed=7, dtype=dt)
    B = one_vs_all_targets(np.arange(RHS), labels, np.float64).astype(dt)
    p = Parameter(kernel_type=KERNELS[kernel], degree=3, gamma=1.0 / features, coef0=0.5, cost=1.0)
    options = _capi.Options(colslab_band_mb=1)
    with backend.ResidentProblem(p, X, options=options) as prob:
        alphas, rhos, infos, passes = prob.solve_lockstep(B, EPS, MAX_ITER)
    print(f"{np.dtype(dt).name} {kernel} {points} x {features}: passes {passes}, tile launches per matvec {[i['tile_launches_per_matvec'] for i in infos]}, "
          f"iterations {[i['iterations'] for i in infos]}")
    assert passes[0] > 0 and passes[1] > 0, passes
    for c in range(RHS):
        assert infos[c]["tile_launches_per_matvec"] >= 2, infos[c]
        alpha, rho, info = backend.solve_system_of_linear_equations(p, X, B[c], EPS, MAX_ITER, options=options)
        differ = np.count_nonzero(alphas[c] != alpha)
        print(f"  column {c}: {differ} of {points} entries differ, rho {rhos[c]!r} / {rho!r}, residuum {infos[c]['residuum']!r} / {info['residuum']!r}")
        assert np.array_equal(alphas[c], alpha), (c, differ)
        assert rhos[c] == rho and infos[c]["residuum"] == info["residuum"] and infos[c]["iterations"] == info["iterations"], (c, infos[c], info)
