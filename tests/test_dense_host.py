"""CPU: the yardstick of the dense SPD toolbox (tests/dense_model.py) and every refusal of the device-factored fixed-size fits that needs no device.

1. The numpy yardstick -- numpy.linalg.cholesky, row-wise substitution, a row-wise forward-substitution inverse -- stays within the three derived bounds of
   dense_model at every size and condition the GPU test uses, with nu = 0, and factors every matrix without jitter.  MEASURED records the largest ratios.
2. The indefinite inputs of the GPU status test fail a restated unblocked Cholesky exactly at the planted column.
3. factor="gpu" is refused by every Python entry point before any library call; the three testing aids refuse m = 0, m = 1025 and NULL pointers, and the six new public
   entry points refuse what their host forms refuse -- all LSSVM_ERR_INVALID_ARGUMENT, without a device."""

import ctypes as C

import numpy as np
import pytest

import dense_model as dm
from plssvm_amd import _capi, backend, svc
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter

B = _capi.DENSE_BLOCK

# the largest ratio of the NUMPY YARDSTICK (numpy.linalg.cholesky, row-wise substitution, the row-wise inverse) to the bounds over dense_model.sizes(64) x cond in
# {1e2, 1e10}, as one run of this file printed them (the assertions are the bounds, not these figures).  They are the yardstick's, not the device's: the device's 0.105 / 0.037 /
# 0.083 stand in tests/test_gpu_dense.py.  Both inverses are forward substitutions L v_j = e_j per column and meet the RIGHT residual bound; the
# figures differ because the orders of the sums differ (blocks and MFMA chains there, numpy's dot products here)
MEASURED = {"factorisation": (0.105, 0.043), "solve (k = 3)": (0.035, 0.038), "inverse, the smaller of the two residual ratios": (0.021, 0.021)}  # (cond 1e2, cond 1e10)


def test_block_width_is_one_the_toolbox_supports():
    assert B in (64, 128) and dm.MAX_RANK == _capi.REDUCED_MAX_RANK


@pytest.mark.parametrize("cond", dm.CONDS)
def test_numpy_yardstick_stays_within_the_bounds(cond):
    worst = [0.0, 0.0, 0.0]
    for m in dm.sizes(B):
        A = dm.spd_matrix(m, cond)
        assert np.array_equal(A, A.T)
        L = np.linalg.cholesky(A)  # (raises where it needs jitter: it never does)
        X = dm.reference_solve(L, dm.right_hand_sides(m, 3))
        V = dm.reference_inverse(L)
        ratios = (dm.factor_ratio(A, 0.0, L), dm.solve_ratio(A, 0.0, L, dm.right_hand_sides(m, 3), X), dm.inverse_ratio(L, V)[0])
        assert all(r <= 1.0 for r in ratios), (m, cond, ratios)
        assert np.array_equal(np.triu(V, 1), np.zeros_like(V))
        worst = [max(w, r) for w, r in zip(worst, ratios)]
    print(f"numpy yardstick, cond {cond:g}: factorisation {worst[0]:.3f}, solve {worst[1]:.3f}, inverse {worst[2]:.3f} of the bounds")


@pytest.mark.parametrize("j", [0, B - 1, B, 299])
def test_indefinite_inputs_fail_at_the_planted_column(j):
    A = dm.indefinite(300, j)
    assert dm.unblocked_cholesky_failure(A) == j + 1
    assert dm.unblocked_cholesky_failure(dm.spd_matrix(300, 1e2)) == 0
    if j > 0:  # the leading block is well conditioned: its factor exists and the pivot is -1 - sum l^2
        lead = np.linalg.cholesky(A[:j, :j])
        row = np.linalg.solve(lead, A[j, :j])
        assert -1.0 - row @ row < -1.0 and np.linalg.cond(A[:j, :j]) <= 1e2 * (1 + 1e-8)


def test_an_unknown_factor_is_refused_before_any_library_call():
    X = np.random.default_rng(0).standard_normal((40, 3))
    y = np.where(np.arange(40) % 2 == 0, 1.0, -1.0)
    labels = (np.arange(40) % 2).tolist()
    prm = Parameter(kernel_type="rbf", gamma=0.5)
    est = svc.SVC(kernel="rbf", gamma=0.5)
    data = DataSet(X, labels)
    # (a handle is never needed: the keyword is checked first.  ResidentProblem and MI355CSVM themselves need a device, so their methods are called on bare objects)
    bare, bare_svm = object.__new__(backend.ResidentProblem), object.__new__(MI355CSVM)
    calls = [lambda f: backend.fit_reduced(prm, X, y, 4, factor=f), lambda f: backend.fit_reduced_loo(prm, X, y, 4, [1.0], factor=f),
             lambda f: backend.ResidentProblem.fit_reduced(bare, y, 4, factor=f), lambda f: backend.ResidentProblem.fit_reduced_loo(bare, y, 4, [1.0], factor=f),
             lambda f: MI355CSVM.fit_reduced(bare_svm, data, 4, factor=f), lambda f: MI355CSVM.fit_reduced_path(bare_svm, data, 4, [1.0], factor=f),
             lambda f: svc.fit_reduced(est, X, np.asarray(labels), 4, factor=f), lambda f: svc.fit_reduced_cv(est, X, np.asarray(labels), 4, [1.0], factor=f)]
    for call in calls:
        for bad in ("gpu", "Device", None, 1):
            with pytest.raises(InvalidParameterError, match="factor must be"):
                call(bad)


def test_the_testing_aids_refuse_without_a_device():
    dp = C.POINTER(C.c_double)
    a = np.eye(4)
    out = np.zeros((4, 4))
    status = C.c_uint64(0)
    p = lambda x: x.ctypes.data_as(dp)  # noqa: E731
    chol, solve, inv = (_capi.dense_entry(f"lssvm_mi355_dense_{n}") for n in ("cholesky", "solve", "invert_lower"))
    for m in (0, 1025):
        for call in (lambda: chol(p(a), m, 0.0, p(out), C.byref(status), None), lambda: solve(p(a), m, p(a), 1, p(out), None), lambda: inv(p(a), m, p(out), None)):
            with pytest.raises(InvalidParameterError, match=r"m must lie in \[1, 1024\]"):
                _capi.check(call())
    null = dp()
    for call in (lambda: chol(null, 4, 0.0, p(out), C.byref(status), None), lambda: chol(p(a), 4, 0.0, null, C.byref(status), None), lambda: chol(p(a), 4, 0.0, p(out), None, None),
                 lambda: solve(null, 4, p(a), 1, p(out), None), lambda: solve(p(a), 4, null, 1, p(out), None), lambda: solve(p(a), 4, p(a), 1, null, None),
                 lambda: inv(null, 4, p(out), None), lambda: inv(p(a), 4, null, None)):
        with pytest.raises(InvalidParameterError, match="must not be NULL"):
            _capi.check(call())
    with pytest.raises(InvalidParameterError, match="k must lie"):
        _capi.check(solve(p(a), 4, p(a), 0, p(out), None))


@pytest.mark.parametrize("suffix, dtype", [("f32", np.float32), ("f64", np.float64)])
def test_the_device_entry_points_refuse_what_their_host_forms_refuse(suffix, dtype):
    N, d, m = 32, 3, 4
    X = np.random.default_rng(1).standard_normal((N, d)).astype(dtype)
    Y = np.ones((1, N), dtype=dtype)
    ps = _capi.LssvmParams(2, 3, 0.5, 0.0, 1.0)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    betas, rhos, costs = np.zeros((1, m)), np.zeros(1), np.ones(1)
    bp, rp, cp = betas.ctypes.data_as(dp), rhos.ctypes.data_as(dp), costs.ctypes.data_as(dp)
    dup = (C.c_uint64 * 3)(1, 2, 1)

    def fit(form, Y=Y, num_rhs=1, rank=m, lm=None, slab_rows=0, bp=bp, X=X):
        fn = _capi.reduced_entry(f"lssvm_mi355_fit_reduced{form}_{suffix}")
        tail = (None,) if form else ()
        return fn(C.byref(ps), _capi.ptr(X) if X is not None else None, N, d, _capi.ptr(Y) if Y is not None else None, num_rhs, rank, lm, slab_rows, bp, rp, None, None, None, *tail)

    def loo(form, Y=Y, num_rhs=1, rank=m, lm=None, slab_rows=0, bp=bp, cp=cp, num_costs=1):
        fn = _capi.reduced_loo_entry(f"lssvm_mi355_fit_reduced_loo{form}_{suffix}")
        tail = (None,) if form else ()
        return fn(C.byref(ps), _capi.ptr(X), N, d, _capi.ptr(Y) if Y is not None else None, num_rhs, rank, lm, slab_rows, cp, num_costs, bp, rp, None, None, None, None, None, None, None, None, *tail)

    bad = [dict(Y=None), dict(num_rhs=0), dict(rank=0), dict(rank=1025), dict(rank=N + 1), dict(slab_rows=100), dict(bp=None), dict(rank=3, lm=dup)]
    for kw in bad:
        for call in (fit, loo):
            texts = []
            for form in ("", "_dev"):
                with pytest.raises(InvalidParameterError) as err:
                    _capi.check(call(form, **kw))
                texts.append(str(err.value))
            assert texts[0] == texts[1], (kw, texts)  # the refusal of the host form, word for word
    for kw in (dict(cp=None), dict(num_costs=0), dict(num_costs=65)):
        texts = []
        for form in ("", "_dev"):
            with pytest.raises(InvalidParameterError, match="cost") as err:
                _capi.check(loo(form, **kw))
            texts.append(str(err.value))
        assert texts[0] == texts[1]
    with pytest.raises(InvalidParameterError, match="data must not be empty"):
        _capi.check(fit("_dev", X=None))
    for name in ("lssvm_mi355_problem_fit_reduced_dev", "lssvm_mi355_problem_fit_reduced_loo_dev"):
        entry = _capi.reduced_loo_entry if "loo" in name else _capi.reduced_entry
        args = (None, _capi.ptr(Y), 1, m, None, 0) + ((cp, 1) if "loo" in name else ()) + (bp, rp) + ((None,) * 7 if "loo" in name else (None, None)) + (None,)
        with pytest.raises(InvalidParameterError, match="handle"):
            _capi.check(entry(name)(*args))
