"""CPU: the numpy model of the (gamma, cost) grid of the fixed-size LS-SVM (tests/reduced_grid_model.py), the bound of the norm expansion the
matrix-core path takes, and the refusals of the entry points, which all happen before a device is touched.

  * a cell of the grid IS the sibling model at that (gamma, C): to the bit where the data is held as given, and at the problem's own gamma on the held data;
  * a cell's leave-one-out values against N brute-force refits (unweighted and weighted), under reduced_loo_model.tolerance;
  * the norm expansion n_i + n_l - 2 a . b against the direct sum of squares, and the dot products, within reduced_grid_model.expansion_bound on the data of
    reduced_model.FIT_CASES and on every shape tests/test_gpu_reduced_grid.py uses -- in float64 numpy, whose own pairwise sums obey the same bound: the reference alone
    is inside the bound the device is held to;
  * the refusals, through the Python layer and through the C entry points themselves."""

import ctypes as C

import numpy as np
import pytest

import pcg_model as pm
import reduced_grid_model as gm
import reduced_loo_model as lm
import reduced_model as rm
import reduced_weighted_model as wm
from plssvm_amd import _capi, backend
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter

GAMMAS = (0.05, 0.2, 0.8)
COSTS = (1.0, 100.0)


def test_padded_features():
    assert [gm.padded_features(d, np.float32) for d in (5, 16, 33, 130)] == [32, 32, 64, 192]
    assert [gm.padded_features(d, np.float64) for d in (5, 16, 33, 130)] == [16, 16, 48, 160]


@pytest.mark.parametrize("name", [c[0] for c in lm.IDENTITY_CASES])
def test_a_cell_is_the_sibling_model_at_that_gamma_and_cost(name):
    p = lm.identity_case(name, np.float64)
    gammas = (p["kw"]["gamma"], 0.37)
    grid = gm.GridModel(p["kernel"], p["X"], p["Y"], p["landmarks"], gammas, COSTS, p["kw"], with_e=False)
    for g, gamma in enumerate(gammas):
        for s, cost in enumerate(COSTS):
            ref = lm.LooModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], **dict(p["kw"], gamma=gamma))
            cell = grid.cells[g][s]
            for a, b in ((cell.h, ref.h), (cell.f, ref.f), (cell.loo, ref.loo), (cell.betas, ref.betas), (cell.rhos, ref.rhos)):
                assert np.array_equal(a, b), (name, g, s)


def test_on_held_float32_data_the_own_gamma_is_the_sibling_model_and_another_gamma_is_scaled():
    p = lm.identity_case("rbf_255x5", np.float32)
    own = p["kw"]["gamma"]
    X_held, kws = gm.held_for_grid("rbf", p["X"], p["kw"], (own, 4.0 * own))
    assert X_held is p["held"][0] or np.array_equal(X_held, p["held"][0])
    assert kws[0]["gamma"] == p["held"][1]["gamma"] and kws[1]["gamma"] == pytest.approx(4.0 * kws[0]["gamma"], rel=4 * gm.EPS64)
    grid = gm.GridModel("rbf", p["X"], p["Y"], p["landmarks"], (own,), (10.0,), p["kw"], with_e=False)
    ref = lm.LooModel("rbf", p["X"], p["Y"], 10.0, p["landmarks"], held=p["held"], **p["kw"])
    assert np.array_equal(grid.cells[0][0].loo, ref.loo) and np.array_equal(grid.cells[0][0].h, ref.h)


@pytest.mark.parametrize("weighted", [False, True])
def test_cells_against_brute_force_refits(weighted):
    p = wm.loo_case(np.float64) if weighted else lm.identity_case("rbf_255x5", np.float64)
    w = p["w"] if weighted else None
    gammas, costs = (0.1, 0.4), (1.0, 100.0)
    grid = gm.GridModel(p["kernel"], p["X"], p["Y"], p["landmarks"], gammas, costs, p["kw"], w=w)
    X_held, kws = grid.held
    for g in range(len(gammas)):
        for s, cost in enumerate(costs):
            cell, e = grid.cells[g][s], grid.e[g][s]
            if weighted:
                brute = wm.brute_force(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], w, held=(X_held, kws[g]), **kws[g])
            else:
                brute = lm.brute_force(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], held=(X_held, kws[g]), **kws[g])
            tol = lm.tolerance(cell, e, np.max(np.abs(cell.f)))
            diff = float(np.max(np.abs(cell.loo - brute)))
            print(f"grid cell gamma={gammas[g]:g} C={cost:g} weighted={weighted}: |loo - refits| {diff:.2e}, tolerance {tol:.2e}")
            assert diff <= tol, (g, s, diff, tol)


def check_expansion(kernel, X_held, lms, ldx):
    direct, expanded = gm.direct_sums(kernel, X_held, lms), gm.expanded_sums(kernel, X_held, lms)
    bound = gm.expansion_bound(kernel, X_held, lms, ldx)
    assert np.all(np.abs(expanded - direct) <= bound)
    if kernel == "rbf":
        assert np.all(expanded >= 0.0) and np.all(expanded[np.asarray(lms, dtype=np.int64), np.arange(len(lms))] == 0.0)
    return float(np.max(np.abs(expanded - direct) / np.where(bound > 0.0, bound, 1.0)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("row", rm.FIT_CASES, ids=[c[0] for c in rm.FIT_CASES])
def test_norm_expansion_stays_within_its_bound_on_the_fit_cases(row, dtype):
    p = rm.case(row, dtype)
    X_held, _ = p["held"]
    worst = check_expansion(p["kernel"], X_held, p["landmarks"], gm.padded_features(X_held.shape[1], dtype))
    print(f"norm expansion {p['name']} {np.dtype(dtype).name}: largest |expanded - direct| / bound {worst:.3f}")


@pytest.mark.parametrize("d", [5, 16, 33, 130])
@pytest.mark.parametrize("N", [255, 777])
@pytest.mark.parametrize("kernel", ["rbf", "polynomial"])
def test_the_gpu_file_s_shapes_keep_the_reference_inside_the_bound(kernel, N, d):
    for dtype in (np.float64, np.float32):
        X, _ = pm.make_data(N, d, pm.DATA_SEED, dtype)
        kw = rm.rounded_parameters(dtype, **({"gamma": 1.0 / d} if kernel == "rbf" else {"gamma": 1.0 / d, "coef0": 1.0, "degree": 3}))
        X_held, _ = rm.held_data(kernel, X, **kw)
        for rank in (1, 17, min(300, N)):
            check_expansion(kernel, X_held, pm.draw_landmarks(N, rank, pm.LANDMARK_SEED), gm.padded_features(d, dtype))


def test_values_error_is_the_derivative_of_the_kernel_value():
    D = np.linspace(0.1, 3.0, 7)
    for kernel, kw in (("rbf", dict(gamma=0.3)), ("polynomial", dict(gamma=0.5, coef0=1.0, degree=3)), ("polynomial", dict(gamma=0.5, coef0=1.0, degree=-2))):
        h = 1e-6
        slope = np.abs(gm.kernel_values(kernel, D + h, kw) - gm.kernel_values(kernel, D - h, kw)) / (2 * h)
        assert np.allclose(gm.values_error(kernel, D, np.ones_like(D), kw), slope, rtol=1e-6)


# ---------------------------------------------------------------- the refusals: no device is touched ----------------------------------------------------------------
def test_python_layer_refuses_before_any_library_call():
    X, y = pm.make_data(40, 3, pm.DATA_SEED, np.float64)
    rbf = Parameter(kernel_type="rbf", gamma=0.5)
    for gammas, costs, match in (([], [1.0], "gamma"), ([0.0], [1.0], "gamma"), ([-1.0], [1.0], "gamma"), ([float("nan")], [1.0], "gamma"), ([float("inf")], [1.0], "gamma"),
                                 (np.full(9, 0.5), np.ones(8), "cells"), (np.full(65, 0.5), [1.0], "cells"), ([0.5], [], "cost"), ([0.5], [0.0], "cost")):
        with pytest.raises(InvalidParameterError, match=match):
            backend.fit_reduced_grid(rbf, X, y, 4, gammas, costs)
    with pytest.raises(InvalidParameterError, match="product"):
        backend.fit_reduced_grid(rbf, X, y, 4, [0.5], [1.0], product="fast")
    with pytest.raises(InvalidParameterError, match="factor"):
        backend.fit_reduced_grid(rbf, X, y, 4, [0.5], [1.0], factor="gpu")
    with pytest.raises(InvalidParameterError, match="linear kernel has no gamma"):
        backend.fit_reduced_grid(Parameter(kernel_type="linear"), X, y, 4, [0.5], [1.0])
    with pytest.raises(InvalidParameterError, match="rank of the reduced model"):
        backend.fit_reduced_grid(rbf, X, y, 41, [0.5], [1.0])
    with pytest.raises(InvalidParameterError, match="weight"):
        backend.fit_reduced_grid(rbf, X, y, 4, [0.5], [1.0], sample_weight=-np.ones(40))


def raw_one_shot(kernel_type=2, gammas=(0.5,), costs=(1.0,), factor=0, product=1, rank=4, slab_rows=0, weights=None, null_gammas=False, null_betas=False, num_rhs=1):
    """lssvm_mi355_fit_reduced_grid_f64 itself on 40 x 3 points: the status the LIBRARY gives (the Python layer's own checks are not in the way)."""
    X, y = pm.make_data(40, 3, pm.DATA_SEED, np.float64)
    ps = _capi.LssvmParams(kernel_type, 3, 0.5, 0.0, 1.0)
    g, c = np.ascontiguousarray(gammas, dtype=np.float64), np.ascontiguousarray(costs, dtype=np.float64)
    G, S = g.size, c.size
    betas, rhos = np.zeros((max(G, 1), max(S, 1), 1, rank)), np.zeros((max(G, 1), max(S, 1), 1))
    dp = C.POINTER(C.c_double)
    fn = _capi.reduced_grid_entry("lssvm_mi355_fit_reduced_grid_f64")
    return fn(C.byref(ps), _capi.ptr(X), 40, 3, _capi.ptr(y), num_rhs, _capi.weights_ptr(weights), rank, None, slab_rows, None if null_gammas else g.ctypes.data_as(dp), G,
              c.ctypes.data_as(dp), S, factor, product, None if null_betas else betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp), None, None, None, None, None, None, None, None, None)


def test_library_refuses_without_a_device():
    for kw, match in ((dict(gammas=()), "at least 1 gamma"), (dict(null_gammas=True), "gammas must not be NULL"), (dict(gammas=(0.5, 0.0)), "gamma 1"), (dict(gammas=(-2.0,)), "gamma 0"),
                      (dict(gammas=(float("nan"),)), "gamma 0"), (dict(gammas=(float("inf"),)), "gamma 0"), (dict(gammas=np.full(9, 0.5), costs=np.ones(8)), r"at most 64 \(gamma, cost\) cells"),
                      (dict(gammas=np.full(65, 0.5)), "cells"), (dict(product=2), "product"), (dict(product=-1), "product"), (dict(factor=2), "factor"),
                      (dict(kernel_type=0), "linear kernel has no gamma"), (dict(costs=()), "cost"), (dict(costs=(0.0,)), "cost"), (dict(rank=0), "rank of the reduced model"),
                      (dict(rank=41), "rank of the reduced model"), (dict(slab_rows=100), "slab_rows"), (dict(num_rhs=0), "right hand sides"), (dict(null_betas=True), "betas_out"),
                      (dict(weights=np.full(40, -1.0)), "weight")):
        with pytest.raises(InvalidParameterError, match=match):
            _capi.check(raw_one_shot(**kw))
    # the resident form: a NULL handle, and the grid's own checks ahead of the handle's use
    dp = C.POINTER(C.c_double)
    one = np.ones(1)
    fn = _capi.reduced_grid_entry("lssvm_mi355_problem_fit_reduced_grid")
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(fn(None, _capi.ptr(one), 1, None, 1, None, 0, one.ctypes.data_as(dp), 1, one.ctypes.data_as(dp), 1, 0, 1, one.ctypes.data_as(dp), one.ctypes.data_as(dp),
                       None, None, None, None, None, None, None, None))
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(_capi.reduced_grid_entry("lssvm_mi355_problem_landmark_acc")(None, None, 1, 1, one.ctypes.data_as(dp)))
    assert C.sizeof(_capi.LssvmReducedGridInfo) == 80  # (static_assert in capi.hip)
