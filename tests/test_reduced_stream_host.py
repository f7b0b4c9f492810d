"""CPU: the numpy model of the fixed-size LS-SVM from a stream of chunks (tests/reduced_stream_model.py), the bound of the centred norm expansion
the new kernel takes, and the refusals of the entry points that happen before a device is touched.

  * the chunks' states add up to the state of the whole (within N eps64 |Pt|^T |Pt|: another order of the same sums);
  * a merge of shard states gives the fit on the concatenation: decision values at held-out points within reduced_model.fit_tolerance of the weighted sibling model;
  * k-fold refits from "total minus own fold" states against brute-force refits (the sibling model with the fold's rows at weight 0) within reduced_model.fit_tolerance;
  * landmarks that are NOT rows of the data: the model on the rows alone is the sibling model with the landmark rows appended at weight 0;
  * n_i + n_l - 2 a . b on the CENTRED rows against the direct sum of squares, and the dot products, within reduced_grid_model.expansion_bound with ldx = d rounded up to
    16, on the fit cases and on every shape tests/test_gpu_reduced_stream.py uses;
  * the refusals, through the C entry points themselves: without a device every one of them must be LSSVM_ERR_INVALID_ARGUMENT, never LSSVM_ERR_NO_DEVICE."""

import ctypes as C

import numpy as np
import pytest

import pcg_model as pm
import reduced_model as rm
import reduced_stream_model as sm
import reduced_weighted_model as wm
from plssvm_amd import _capi, backend
from plssvm_amd.exceptions import BackendError, InvalidParameterError
from plssvm_amd.parameter import Parameter

EPS64 = rm.EPS64
CUTS = (1, 127, 129, 520)


def staged(p):
    """(the rows as a stream stages them, the landmark rows likewise, the centre)"""
    XL = p["X"][p["landmarks"].astype(np.int64)]
    centre = sm.centre_of(p["kernel"], XL)
    return sm.held(p["X"], centre), sm.held(XL, centre), centre


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", ["rbf_777x5", "poly_777x16"])
def test_chunk_states_add_up_to_the_whole(name, weighted):
    p = rm.fit_case(name, np.float64, 3)
    Xh, XLh, _ = staged(p)
    N = Xh.shape[0]
    w = wm.make_weights(N, large=(64.0,)) if weighted else None
    whole = sm.state(p["kernel"], Xh, p["Y"], XLh, w, **p["kw"])
    total, at = np.zeros_like(whole), 0
    for n in CUTS:
        total += sm.state(p["kernel"], Xh[at:at + n], p["Y"][:, at:at + n], XLh, None if w is None else w[at:at + n], **p["kw"])
        at += n
    assert at == N
    P = np.abs(sm.augmented(p["kernel"], Xh, p["Y"], XLh, **p["kw"]))
    scale = P.T @ ((np.ones(N) if w is None else w)[:, None] * P)
    assert np.all(np.abs(total - whole) <= 2.0 * N * EPS64 * scale)
    m = XLh.shape[0]
    assert whole[m, m] == (N if w is None else pytest.approx(w.sum(), rel=1e-14))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", ["rbf_777x5", "poly_777x16"])
def test_merged_shard_states_give_the_fit_on_the_concatenation(name, weighted):
    p = rm.fit_case(name, np.float64, 3)
    Xh, XLh, centre = staged(p)
    N, k = Xh.shape[0], 3
    w = wm.make_weights(N, large=(64.0,)) if weighted else np.ones(N)
    held = (Xh, p["kw"])
    model = wm.WeightedReducedModel(p["kernel"], Xh, p["Y"], p["cost"], p["landmarks"], w, held=held, **p["kw"])
    points = sm.held(p["points"], centre)
    e = wm.e_model(p["kernel"], Xh, p["Y"], p["cost"], p["landmarks"], w, points, held=held, **p["kw"])
    K_mm = sm.phi(p["kernel"], XLh, XLh, **p["kw"])
    for shards in (2, 3):
        edges = np.linspace(0, N, shards + 1).astype(int)
        merged = sum(sm.state(p["kernel"], Xh[a:b], p["Y"][:, a:b], XLh, w[a:b], **p["kw"]) for a, b in zip(edges[:-1], edges[1:]))
        betas, rhos, nu, _ = sm.solve_state(merged, K_mm, k, p["cost"])
        f = model.decision_values(points)
        g = sm.decision_values(p["kernel"], XLh, betas, rhos, points, **p["kw"])
        tol = rm.fit_tolerance(model, e, f)
        diff = float(np.max(np.abs(f - g)))
        print(f"merge of {shards} shard states {name} weighted={weighted}: |f_merged - f_model| {diff:.2e}, tolerance {tol:.2e}")
        assert diff <= tol and abs(nu / model.nu - 1.0) <= 1e-6


@pytest.mark.parametrize("name", ["rbf_777x5", "poly_777x16"])
def test_k_fold_refits_from_total_minus_own_fold(name):
    p = rm.fit_case(name, np.float64, 1)
    Xh, XLh, centre = staged(p)
    N = Xh.shape[0]
    held = (Xh, p["kw"])
    points = sm.held(p["points"], centre)
    K_mm = sm.phi(p["kernel"], XLh, XLh, **p["kw"])
    folds = np.arange(N) % 5
    states = [sm.state(p["kernel"], Xh[folds == v], p["Y"][:, folds == v], XLh, **p["kw"]) for v in range(5)]
    total = sum(states)
    for v in range(5):
        keep = (folds != v).astype(np.float64)  # the brute-force refit: the fold's rows at weight 0 (the landmark set held fixed, as a stream holds it)
        model = wm.WeightedReducedModel(p["kernel"], Xh, p["Y"], p["cost"], p["landmarks"], keep, held=held, **p["kw"])
        e = wm.e_model(p["kernel"], Xh, p["Y"], p["cost"], p["landmarks"], keep, points, held=held, **p["kw"])
        betas, rhos, _, _ = sm.solve_state(total - states[v], K_mm, 1, p["cost"])
        f = model.decision_values(points)
        g = sm.decision_values(p["kernel"], XLh, betas, rhos, points, **p["kw"])
        tol = rm.fit_tolerance(model, e, f)
        diff = float(np.max(np.abs(f - g)))
        print(f"fold {v} of {name}: |f_total_minus_fold - f_refit| {diff:.2e}, tolerance {tol:.2e}")
        assert diff <= tol, (v, diff, tol)


def test_landmarks_that_are_no_rows_of_the_data():
    p = rm.fit_case("rbf_777x5", np.float64, 3)
    XL = pm.make_data(64, 5, 77, np.float64)[0]
    centre = sm.centre_of("rbf", XL)
    Xh, XLh = sm.held(p["X"], centre), sm.held(XL, centre)
    X2, Y2, w2, lms = sm.with_landmark_rows(Xh, p["Y"], None, XLh)
    model = wm.WeightedReducedModel("rbf", X2, Y2, p["cost"], lms, w2, **p["kw"])
    betas, rhos, nu, _ = sm.solve_state(sm.state("rbf", Xh, p["Y"], XLh, **p["kw"]), sm.phi("rbf", XLh, XLh, **p["kw"]), 3, p["cost"])
    points = sm.held(p["points"], centre)
    e = wm.e_model("rbf", X2, Y2, p["cost"], lms, w2, points, **p["kw"])
    f, g = model.decision_values(points), sm.decision_values("rbf", XLh, betas, rhos, points, **p["kw"])
    assert float(np.max(np.abs(f - g))) <= rm.fit_tolerance(model, e, f)


def check_expansion(kernel, Xh, XLh):
    direct, bound = sm.direct_and_bound(kernel, Xh, XLh, sm.padded_features(Xh.shape[1]))
    expanded = sm.expanded_sums(kernel, Xh, XLh)
    assert np.all(np.abs(expanded - direct) <= bound)
    if kernel == "rbf":
        assert np.all(expanded >= 0.0)
    return float(np.max(np.abs(expanded - direct) / np.where(bound > 0.0, bound, 1.0)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["rbf_777x5", "poly_777x16"])
def test_centred_expansion_stays_within_its_bound_on_the_fit_cases(name, dtype):
    p = rm.fit_case(name, dtype, 1)
    Xh, XLh, _ = staged(p)
    print(f"centred expansion {name} {np.dtype(dtype).name}: largest |expanded - direct| / bound {check_expansion(p['kernel'], Xh, XLh):.3f}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kernel", ["rbf", "polynomial", "linear"])
def test_centred_expansion_stays_within_its_bound_on_the_operator_shapes(kernel, dtype):
    worst = 0.0
    for d in (1, 5, 16, 17, 33, 130):
        X = pm.make_data(257, d, pm.DATA_SEED, dtype)[0]
        for rank in (1, 17, 129):
            XL = X[pm.draw_landmarks(257, rank, pm.LANDMARK_SEED).astype(np.int64)]
            centre = sm.centre_of(kernel, XL)
            worst = max(worst, check_expansion(kernel, sm.held(X, centre), sm.held(XL, centre)))
    print(f"centred expansion {kernel} {np.dtype(dtype).name}: largest |expanded - direct| / bound {worst:.3f}")


def test_centre_is_the_landmarks_mean_for_rbf_and_zero_otherwise():
    XL = pm.make_data(37, 5, 3, np.float32)[0]
    assert np.allclose(sm.centre_of("rbf", XL), XL.astype(np.float64).mean(axis=0), rtol=1e-14, atol=0.0)
    assert np.all(sm.centre_of("polynomial", XL) == 0.0) and np.all(sm.centre_of("linear", XL) == 0.0)


# ---------------------------------------------------------------- the refusals that need no device ----------------------------------------------------------------
def create(dtype, ps, XL, rank, d, k, weighted=0, slab_rows=0):
    h = C.c_void_p(None)
    fn = _capi.reduced_stream_entry(f"lssvm_mi355_reduced_stream_create_{_capi.suffix_of(dtype)}")
    status = fn(C.byref(h), None if ps is None else C.byref(ps), None if XL is None else _capi.ptr(XL), rank, d, k, weighted, slab_rows, None)
    assert not h  # (nothing was created)
    return status


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_create_refuses_bad_arguments_before_a_device_is_touched(dtype):
    XL = np.ones((4, 3), dtype=dtype)
    rbf = _capi.LssvmParams(2, 3, 0.5, 0.0, 1.0)
    bad = [
        (None, XL, 4, 3, 1, 0, 0, "params"),
        (rbf, None, 4, 3, 1, 0, 0, "landmark rows"),
        (rbf, XL, 0, 3, 1, 0, 0, "rank"),
        (rbf, XL, 1025, 3, 1, 0, 0, "rank"),
        (rbf, XL, 4, 3, 0, 0, 0, "right hand sides"),
        (rbf, XL, 4, 3, 1, 0, 100, "slab_rows"),
        (rbf, XL, 4, 3, 1, 0, 257, "slab_rows"),
        (rbf, XL, 4, 0, 1, 0, 0, "feature"),
        (_capi.LssvmParams(2, 3, 0.0, 0.0, 1.0), XL, 4, 3, 1, 0, 0, "gamma"),
        (_capi.LssvmParams(2, 3, -1.0, 0.0, 1.0), XL, 4, 3, 1, 0, 0, "gamma"),
        (_capi.LssvmParams(2, 3, float("nan"), 0.0, 1.0), XL, 4, 3, 1, 0, 0, "gamma"),
        (_capi.LssvmParams(1, 3, float("inf"), 0.0, 1.0), XL, 4, 3, 1, 0, 0, "gamma"),
        (_capi.LssvmParams(7, 3, 0.5, 0.0, 1.0), XL, 4, 3, 1, 0, 0, "kernel function"),
    ]
    for ps, rows, rank, d, k, weighted, slab_rows, what in bad:
        with pytest.raises(InvalidParameterError, match=what):
            _capi.check(create(dtype, ps, rows, rank, d, k, weighted, slab_rows))
    # the cost is ignored (0 is refused everywhere else), and a linear kernel has no gamma to check: valid arguments reach the device -- and without one fail LOUDLY
    if _capi.device_count() == 0:
        for ps in (_capi.LssvmParams(2, 3, 0.5, 0.0, 0.0), _capi.LssvmParams(0, 3, -1.0, 0.0, 1.0)):
            assert create(dtype, ps, XL, 4, 3, 1, 1, 512) == -2  # LSSVM_ERR_NO_DEVICE
    with pytest.raises(InvalidParameterError, match="out"):
        fn = _capi.reduced_stream_entry(f"lssvm_mi355_reduced_stream_create_{_capi.suffix_of(dtype)}")
        _capi.check(fn(None, C.byref(rbf), _capi.ptr(XL), 4, 3, 1, 0, 0, None))


def test_every_call_refuses_a_null_handle():
    X, y, out = np.ones((4, 3)), np.ones(4), np.zeros(64)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    words = np.zeros(_capi.REDUCED_STREAM_FINGERPRINT_WORDS, dtype=np.uint64)
    n = C.c_uint64(0)
    calls = {
        "update": (None, _capi.ptr(X), _capi.ptr(y), None, 4),
        "solve": (None, out.ctypes.data_as(dp), 1, 0, out.ctypes.data_as(dp), out.ctypes.data_as(dp), None),
        "loo": (None, _capi.ptr(X), _capi.ptr(y), None, 4, out.ctypes.data_as(dp), out.ctypes.data_as(dp), out.ctypes.data_as(dp)),
        "export_state": (None, out.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(n), words.ctypes.data_as(up)),
        "merge_state": (None, out.ctypes.data_as(dp), 4, words.ctypes.data_as(up)),
        "info": (None, None, None, None),
        "phi": (None, _capi.ptr(X), 4, out.ctypes.data_as(dp)),
    }
    for name, args in calls.items():
        with pytest.raises(InvalidParameterError, match="handle"):
            _capi.check(_capi.reduced_stream_entry(f"lssvm_mi355_reduced_stream_{name}")(*args))
    assert _capi.reduced_stream_entry("lssvm_mi355_reduced_stream_destroy")(None) == 0  # (as free(NULL))


def test_python_layer_refuses_what_it_can_see_and_fails_loudly_without_a_device():
    XL = np.ones((4, 3))
    with pytest.raises(InvalidParameterError, match="slab_rows"):
        backend.ReducedStream(Parameter(kernel_type="rbf"), XL, slab_rows=100)
    with pytest.raises(InvalidParameterError, match="right hand sides"):
        backend.ReducedStream(Parameter(kernel_type="rbf"), XL, num_rhs=0)
    with pytest.raises(InvalidParameterError, match="rank"):
        backend.ReducedStream(Parameter(kernel_type="rbf"), np.ones((1025, 2)))
    with pytest.raises(InvalidParameterError, match="gamma"):
        backend.ReducedStream(Parameter(kernel_type="rbf", gamma=float("inf")), XL)
    if _capi.device_count() == 0:
        with pytest.raises(BackendError, match="no HIP capable devices"):
            backend.ReducedStream(Parameter(kernel_type="rbf"), XL)
