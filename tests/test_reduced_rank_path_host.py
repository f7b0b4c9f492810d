"""CPU, numpy only: the algebra behind the rank path of the fixed-size LS-SVM on tests/reduced_rank_path_model.py -- the prefixes of ONE full-rank
factor are the fits on landmarks[:r] (the nesting identity), their leave-one-out values are those of 255 refits, and the one documented difference to separate fits, the
jitter of the full rank, moves the results by no more than a bound computed here.  The device is checked against the same model in tests/test_gpu_reduced_rank_path.py."""

import ctypes as C

import numpy as np
import pytest

import reduced_loo_model as rlm
import reduced_rank_path_model as rpm
import reduced_weighted_model as rw
from plssvm_amd import _capi

CASES = [row[0] for row in rlm.IDENTITY_CASES]


def _stable_e(p, cost, r, scratch):
    """e_loo of the fit on landmarks[:r]: its normal equations against the QR route of reduced_weighted_model.stable (which takes no nu)."""
    loo_s = rw.stable(p["kernel"], p["X"], p["Y"], cost, p["landmarks"][:r], p["w"], held=p["held"], **p["kw"])[2]
    return float(np.max(np.abs(scratch.loo - loo_s)) / np.max(np.abs(loo_s)))


@pytest.mark.parametrize("cost", rpm.NESTING_COSTS)
@pytest.mark.parametrize("name", CASES)
def test_the_prefixes_of_one_factor_are_the_fits_on_the_first_landmarks(name, cost):
    """The nesting identity: with the SAME nu, prefix r of the rank-40 factor and a from-scratch fit on landmarks[:r] are the same numbers up to rounding."""
    p = rpm.nesting_case(name, k=2)
    assert np.count_nonzero(p["w"] == 0.0) >= 3 and p["w"].max() <= 2.0
    model = rpm.RankPathModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], rpm.NESTING_PREFIXES, w=p["w"], held=p["held"], **p["kw"])
    for q, r in enumerate(rpm.NESTING_PREFIXES):
        a = model.at[q]
        b = rpm.from_scratch(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], r, model.nu, w=p["w"], held=p["held"], **p["kw"])
        e = _stable_e(p, cost, r, b)
        for what, x, y in (("h", a.h, b.h), ("f", a.f, b.f), ("loo", a.loo, b.loo), ("betas", a.betas[:, :r], b.betas), ("rhos", a.rhos, b.rhos)):
            scale = a.rho_scale if what == "rhos" else max(float(np.max(np.abs(y))), 1.0 if what == "h" else 0.0)  # (rho: the size of the terms it is the difference of)
            tol = rlm.tolerance(b, e, scale)
            diff = float(np.max(np.abs(x - y)))
            print(f"{name} C={cost} r={r} {what}: |prefix - scratch| {diff:.1e}, tolerance {tol:.1e} (cond {b.cond:.1e}, e_loo {e:.1e})")
            assert diff <= tol, (what, r, diff, tol)
        assert np.all(a.betas[:, r:] == 0.0)
        assert np.all(a.h[p["w"] == 0.0] == 0.0) and np.array_equal(a.loo[:, p["w"] == 0.0], a.f[:, p["w"] == 0.0])
        np.testing.assert_allclose(a.cond, b.cond, rtol=1e-6)
        assert 1.0 <= a.cond_hint <= a.cond * (1.0 + 1e-9)  # the hint is a lower bound of the condition number


@pytest.mark.parametrize("cost", rpm.NESTING_COSTS)
def test_the_prefix_leave_one_out_values_are_those_of_refits(cost):
    """255 refits per (cost, prefix) -- the same model with w_i set to 0, on landmarks[:r] -- against the prefix's identity y - (y - f) / (1 - h)."""
    p = rpm.nesting_case("rbf_255x5")
    prefixes = (7, 40)
    model = rpm.RankPathModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], prefixes, w=p["w"], held=p["held"], **p["kw"])
    for q, r in enumerate(prefixes):
        brute = rw.brute_force(p["kernel"], p["X"], p["Y"], cost, p["landmarks"][:r], p["w"], held=p["held"], **p["kw"])
        e = _stable_e(p, cost, r, model.at[q])
        tol = rlm.tolerance(model.at[q], e, np.max(np.abs(brute)))
        diff = float(np.max(np.abs(model.at[q].loo - brute)))
        print(f"C={cost} r={r}: |loo - refits| {diff:.1e}, tolerance {tol:.1e} (cond {model.at[q].cond:.1e}, e_loo {e:.1e}, largest leverage {model.at[q].max_leverage:.2f})")
        assert diff <= tol


def test_the_jitter_of_the_full_rank_moves_a_prefix_by_no_more_than_its_bound():
    """The one documented difference to separate fits: prefix r takes nu_m = eps64 trace(M) over all 40 landmarks where a fit on landmarks[:r] takes its own, smaller
    nu_r.  The results move by no more than 8 cond(M_r) (nu_m - nu_r) / |M_r| x scale (reduced_rank_path_model.jitter_bound).  Only the cases where that says something
    (cond <= 1e8) are kept; there must be some."""
    kept = 0
    for name in CASES:
        p = rpm.nesting_case(name, k=2)
        for cost in rpm.NESTING_COSTS:
            model = rpm.RankPathModel(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], rpm.NESTING_PREFIXES, w=p["w"], held=p["held"], **p["kw"])
            assert model.retries == 0
            for q, r in enumerate(rpm.NESTING_PREFIXES):
                own = rpm.from_scratch(p["kernel"], p["X"], p["Y"], cost, p["landmarks"], r, None, w=p["w"], held=p["held"], **p["kw"])
                assert own.nu <= model.nu
                if r == rpm.NESTING_RANK:
                    assert own.nu == pytest.approx(model.nu, rel=1e-12)
                if own.cond > 1e8 or r == rpm.NESTING_RANK:
                    continue
                kept += 1
                a = model.at[q]
                for what, x, y in (("h", a.h, own.h), ("f", a.f, own.f), ("loo", a.loo, own.loo)):
                    scale = max(float(np.max(np.abs(y))), 1.0 if what == "h" else 0.0)
                    bound = rpm.jitter_bound(own, model.nu, own.nu, scale)
                    diff = float(np.max(np.abs(x - y)))
                    print(f"{name} C={cost} r={r} {what}: moved by {diff:.1e}, bound {bound:.1e} (cond {own.cond:.1e}, nu_m - nu_r {model.nu - own.nu:.1e})")
                    assert diff <= bound, (name, cost, r, what, diff, bound)
    assert kept >= 6, kept


def test_entry_points_are_declared_exported_and_bound():
    for name in ("lssvm_mi355_problem_fit_reduced_rank_path", "lssvm_mi355_fit_reduced_rank_path_f32", "lssvm_mi355_fit_reduced_rank_path_f64",
                 "lssvm_mi355_problem_reduced_leverage_prefix", "lssvm_mi355_problem_time_leverage_prefix_kernel"):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib, name)
        assert _capi.reduced_rank_path_entry(name).restype is C.c_int
    assert C.sizeof(_capi.LssvmReducedRankInfo) == 72


@pytest.mark.parametrize("ranks, costs, message", [
    ((4, 2), (1.0,), "strictly ascending"), ((2, 2), (1.0,), "strictly ascending"), ((0, 2), (1.0,), r"\[1, 8\]"), ((2, 9), (1.0,), r"\[1, 8\]"),
    ((), (1.0,), "between 1 and 16"), (tuple(range(1, 18)), (1.0,), "between 1 and 16"), ((1, 2, 3, 4, 5), tuple(float(c) for c in range(1, 14)), "at most 64"),
])
def test_a_bad_rank_list_is_refused_before_a_device_is_touched(ranks, costs, message):
    """The C entry point itself (not the checks of backend.py): LSSVM_ERR_INVALID_ARGUMENT on a machine with or without a device."""
    from plssvm_amd.exceptions import InvalidParameterError

    N, d, rank, k = 20, 3, 8 if len(ranks) < 17 else 20, 1
    if len(ranks) == 17:
        message = "between 1 and 16"
    X, Y = np.ones((N, d)), np.ones((k, N))
    ps = _capi.LssvmParams(2, 3, 0.5, 0.0, 1.0)
    r, c = np.asarray(ranks, dtype=np.uint64), np.asarray(costs, dtype=np.float64)
    R, S = r.size, c.size
    betas, rhos = np.zeros((S, max(R, 1), k, rank)), np.zeros((S, max(R, 1), k))
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    fn = _capi.reduced_rank_path_entry("lssvm_mi355_fit_reduced_rank_path_f64")
    for factor in (0, 1):
        with pytest.raises(InvalidParameterError, match=message):
            _capi.check(fn(C.byref(ps), _capi.ptr(X), N, d, _capi.ptr(Y), k, None, rank, None, 0, r.ctypes.data_as(up), R, c.ctypes.data_as(dp), S, factor, betas.ctypes.data_as(dp),
                           rhos.ctypes.data_as(dp), None, None, None, None, None, None, None, None, None))
