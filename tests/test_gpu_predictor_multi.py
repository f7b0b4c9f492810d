"""GPU (-m gpu): the resident predictor of a one-vs-all model -- lssvm_mi355_predictor_create_multi / _predict_multi, k weight vectors over one set of support vectors
kept in HBM -- and the 128-row full-square split kernels with two weight vectors per pass.

What is asserted, and why:
  * every column against the SINGLE-VECTOR resident predictor of that (alpha_v, rho_v) with the same options: EXACT equality, on every path (rectangular 256-row kernel
    with two vectors per pass, 128-row kernels with two vectors per pass, one vector per launch, linear, the one-shot fallback).  Per vector the multi call performs the
    single call's operations in the same order; there is nothing to tolerate.
  * against predict_values_multi: exact equality for rbf (the resident form prepares the batch as the one-shot call does) and for every fallback; for the polynomial
    kernel 16 eps_fp32 of the summand scale sum_j |alpha_v,j| max |gamma x.s + coef0|^degree -- the planes' power-of-two scale comes from the support vectors alone in
    the resident form and from both sides in the one-shot call, the documented difference of the single-vector predictor (tests/test_gpu_round6.py,
    test_resident_predictor_equals_the_one_shot_predict_values, whose bar and scale these are).
  * against a float64 numpy evaluation on sampled rows: the same bar.
  * lssvm_predict_info: resident, and vectors_per_launch = 2 wherever a pair record serves the batch (polynomial of any degree, folded rbf; below and above the 64 row
    blocks of the rectangular kernel), 1 for the linear kernel and for rbf on unfolded records.
"""

import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from plssvm_amd import _capi, backend, multiclass
from plssvm_amd._capi import Options
from plssvm_amd.datagen import make_blobs_multiclass, make_blobs_pm1
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter
from plssvm_amd.svc import SVC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = float(np.finfo(np.float32).eps)
NSV, POOL = 3001, 9000
# 1, 100, 300 points; 7 936 = 62 row blocks (the 128-row kernels); 7 937 and 9 000 points are padded to 64 and 72 row blocks (the rectangular 256-row kernel)
BATCHES = (1, 100, 300, 7936, 7937, 9000)
COEF0 = 0.5


@functools.lru_cache(maxsize=None)
def data(d, dt):
    X, _ = make_blobs_pm1(NSV + POOL, d, seed=23, dtype=dt)
    return X[:NSV], X[NSV:]


@functools.lru_cache(maxsize=None)
def max_abs_gram(d, dt):
    """(max |gamma x.s + coef0|, max |x.s|) over the pool and the support vectors, in float64"""
    sv, pool = data(d, dt)
    G = pool.astype(np.float64) @ sv.astype(np.float64).T
    return float(np.max(np.abs(G / d + COEF0))), float(np.max(np.abs(G)))


def weights(k, dt, seed=17):
    rng = np.random.default_rng(seed + k)
    return rng.standard_normal((k, NSV)).astype(dt), (0.125 + 0.25 * np.arange(k)).astype(np.float64)


def summand_scale(kernel, degree, d, alpha_v):
    """sum_j |alpha_v,j| max |k(x, s_j)|: the scale of tests/test_gpu_round6.py::test_resident_predictor_equals_the_one_shot_predict_values"""
    s = float(np.abs(alpha_v.astype(np.float64)).sum())
    if kernel == "rbf":
        return s
    base, gram = max_abs_gram(d, alpha_v.dtype.type)
    return s * (base ** degree if kernel == "polynomial" else gram)


def float64_values(kernel, degree, d, sv, alpha, rho, pts):
    P, S = pts.astype(np.float64), sv.astype(np.float64)
    G = P @ S.T
    if kernel == "rbf":
        sq = np.sum(P * P, axis=1)[:, None] + np.sum(S * S, axis=1)[None, :] - 2.0 * G
        K = np.exp(-(1.0 / d) * np.maximum(sq, 0.0))
    elif kernel == "polynomial":
        K = (G / d + COEF0) ** degree
    else:
        K = G
    return K @ alpha.astype(np.float64).T - np.asarray(rho, dtype=np.float64)[None, :]


def check_model(kernel, degree, k, d, dt, opts, expect_vectors_per_launch, batches=BATCHES):
    """the multi predictor against k single-vector predictors, predict_values_multi and float64 on every batch size"""
    sv, pool = data(d, dt)
    alpha, rho = weights(k, dt)
    prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=COEF0)
    eps = float(np.finfo(dt).eps)
    scales = np.array([summand_scale(kernel, degree, d, alpha[v]) for v in range(k)])
    singles = [backend.Predictor(prm, sv, alpha[v], float(rho[v]), options=Options(**opts)) for v in range(k)]
    try:
        with backend.Predictor(prm, sv, alpha, rho, options=Options(**opts)) as pred:
            for npts in batches:
                pts = pool[:npts]
                info = {}
                got = pred.predict(pts, info_out=info)
                assert got.shape == (npts, k) and got.dtype == dt
                assert info["resident"] == 1, (npts, info)
                assert info["vectors_per_launch"] == expect_vectors_per_launch, (npts, info)
                assert info["kernel_ms"] > 0 and info["total_ms"] >= info["kernel_ms"]
                for v in range(k):
                    single = {}
                    want = singles[v].predict(pts, info_out=single)
                    differ = np.flatnonzero(got[:, v] != want)
                    assert differ.size == 0, (npts, v, differ.size, got[differ[0], v], want[differ[0]])
                    assert single["resident"] == 1 and single["vectors_per_launch"] == 0 and single["gram_mode"] == info["gram_mode"], (single, info)
                multi = {}
                one, _ = backend.predict_values_multi(prm, sv, alpha, rho.astype(dt), None, pts, options=Options(**opts), info_out=multi)
                err = np.max(np.abs(got.astype(np.float64) - one), axis=0) / (eps * scales)
                sample = np.unique(np.concatenate([np.arange(0, npts, 257), [0, npts // 2, npts - 1]]))
                err64 = np.max(np.abs(got[sample] - float64_values(kernel, degree, d, sv, alpha, rho, pts[sample])), axis=0) / (eps * scales)
                print(f"{kernel} degree {degree} k={k} d={d} {opts} {npts} points: vectors_per_launch {info['vectors_per_launch']} (one-shot {multi['vectors_per_launch']}), against "
                      f"predict_values_multi {err.max():.2f} eps, against float64 {err64.max():.2f} eps of the summand scale")
                if kernel == "polynomial":
                    assert np.all(err <= 16), (npts, err)
                else:
                    assert np.array_equal(got, one), (npts, err)
                assert np.all(err64 <= 16), (npts, err64)
            again = pred.predict(pool[:batches[-1]])
            assert np.array_equal(again, got)  # (a second call: the resident records are read, never written)
    finally:
        for s in singles:
            s.close()


# ------------------------------------------------------------------------------------------------------------ bit-identity, launch plan, both references
@pytest.mark.parametrize("gram_mode", [3, 1], ids=["f16x3", "bf16x6"])
@pytest.mark.parametrize("d", [48, 64, 100, 128])
@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 2), ("polynomial", 3), ("polynomial", 5)])
def test_columns_equal_the_single_vector_predictor(kernel, degree, k, d, gram_mode):
    """Two weight vectors per product launch at every batch size: below 64 row blocks on the 128-row full-square kernels (NV = 2 of s6w_body), from 64 row blocks on on the
    rectangular 256-row kernel -- which has no run-time integer power, so degree 5 stays on the 128-row two-vector kernel there too.  An odd last vector runs alone."""
    check_model(kernel, degree, k, d, np.float32, {"gram_mode": gram_mode}, expect_vectors_per_launch=2)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("d", [48, 128])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_linear_kernel_holds_one_w_per_vector(k, d, dt):
    check_model("linear", 3, k, d, dt, {}, expect_vectors_per_launch=1)


@pytest.mark.parametrize("npts", [300, 8000])
@pytest.mark.parametrize("k", [2, 3])
def test_unfolded_rbf_records_run_one_vector_per_launch(k, npts):
    """Options(rbf_form=2) at an exponent scale above 200: the records keep c_j in their second half (KT_RBF), which leaves no room for a second vector."""
    d = 64
    sv, pool = data(d, np.float32)
    pts = pool[:npts]
    alpha, rho = weights(k, np.float32)
    mean = sv.astype(np.float64).mean(axis=0)
    sq = max(float(np.max(np.sum((M.astype(np.float64) - mean) ** 2, axis=1))) for M in (sv, pts))
    gamma = float(np.float32(400.0 / (2.0 * 1.4426950408889634 * sq)))
    prm = Parameter(kernel_type="rbf", gamma=gamma)
    info, multi = {}, {}
    with backend.Predictor(prm, sv, alpha, rho, options=Options(rbf_form=2)) as pred:
        got = pred.predict(pts, info_out=info)
    assert info["resident"] == 1 and info["rbf_exponent_scale"] > 200 and info["vectors_per_launch"] == 1, info
    for v in range(k):
        with backend.Predictor(prm, sv, alpha[v], float(rho[v]), options=Options(rbf_form=2)) as single:
            assert np.array_equal(got[:, v], single.predict(pts))
    one, _ = backend.predict_values_multi(prm, sv, alpha, rho.astype(np.float32), None, pts, options=Options(rbf_form=2), info_out=multi)
    assert np.array_equal(got, one)


@pytest.mark.parametrize("k", [2, 3])
def test_folded_rbf_between_the_two_fold_limits_runs_two_vectors_on_the_128_row_kernel(k):
    """An exponent scale in (64, 200]: folded records, but beyond the rectangular kernel's range -- 8 000 points still take two vectors per pass, on the 128-row kernel."""
    d = 64
    sv, pool = data(d, np.float32)
    pts = pool[:8000]
    alpha, rho = weights(k, np.float32)
    mean = sv.astype(np.float64).mean(axis=0)
    sq = max(float(np.max(np.sum((M.astype(np.float64) - mean) ** 2, axis=1))) for M in (sv, pts))
    prm = Parameter(kernel_type="rbf", gamma=float(np.float32(128.0 / (2.0 * 1.4426950408889634 * sq))))
    info = {}
    with backend.Predictor(prm, sv, alpha, rho, options=Options(rbf_form=2)) as pred:
        got = pred.predict(pts, info_out=info)
    assert info["resident"] == 1 and 64 < info["rbf_exponent_scale"] <= 200 and info["vectors_per_launch"] == 2, info
    for v in range(k):
        with backend.Predictor(prm, sv, alpha[v], float(rho[v]), options=Options(rbf_form=2)) as single:
            assert np.array_equal(got[:, v], single.predict(pts))
    one, _ = backend.predict_values_multi(prm, sv, alpha, rho.astype(np.float32), None, pts, options=Options(rbf_form=2))
    assert np.array_equal(got, one)


# ------------------------------------------------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize("case", ["fp64_rbf", "192_features", "far_batch"])
def test_what_the_resident_form_does_not_cover_equals_predict_values_multi(case):
    k = 3
    dt = np.float64 if case == "fp64_rbf" else np.float32
    d = 192 if case == "192_features" else 64
    X, _ = make_blobs_pm1(2000 + 9000, d, seed=29, dtype=dt)
    sv, pts = X[:2000], X[2000:]
    alpha = np.random.default_rng(19).standard_normal((k, 2000)).astype(dt)
    rho = 0.125 + 0.25 * np.arange(k)
    prm = Parameter(kernel_type="rbf", gamma=1.0 / d)
    batch = (pts * 12.0).astype(dt) if case == "far_batch" else pts
    with backend.Predictor(prm, sv, alpha, rho) as pred:
        if case == "far_batch":
            near = {}
            pred.predict(pts, info_out=near)
            assert near["resident"] == 1 and near["vectors_per_launch"] == 2, near
        info, one = {}, {}
        got = pred.predict(batch, info_out=info)
        want, _ = backend.predict_values_multi(prm, sv, alpha, rho.astype(dt), None, batch, info_out=one)
        assert info["resident"] == 0, info
        assert np.array_equal(got, want)
        assert info["gram_mode"] == one["gram_mode"] and info["vectors_per_launch"] == one["vectors_per_launch"], (info, one)
        assert np.array_equal(pred.predict(batch), got)
        for v in range(k):
            with backend.Predictor(prm, sv, alpha[v], float(rho[v])) as single:
                assert np.array_equal(got[:, v], single.predict(batch))


# ------------------------------------------------------------------------------------------------------------ handle rules
@pytest.mark.parametrize("kernel", ["rbf", "polynomial", "linear"])
def test_a_multi_handle_of_one_vector_equals_create(kernel):
    sv, pool = data(100, np.float32)
    alpha, rho = weights(1, np.float32)
    prm = Parameter(kernel_type=kernel, degree=3, gamma=1.0 / 100, coef0=COEF0)
    with backend.Predictor(prm, sv, alpha, rho) as multi, backend.Predictor(prm, sv, alpha[0], float(rho[0])) as single:
        for npts in (100, 9000):
            a, b = {}, {}
            got, want = multi.predict(pool[:npts], info_out=a), single.predict(pool[:npts], info_out=b)
            assert got.shape == (npts, 1) and np.array_equal(got[:, 0], want)
            assert a["resident"] == b["resident"] == 1 and a["vectors_per_launch"] == 1 and b["vectors_per_launch"] == 0
        # the single-vector entry point serves a one-vector handle of create_multi, and predict_multi a handle of create
        want = single.predict(pool[:100])
        out = np.zeros(100, np.float32)
        _capi.check(_capi.lib.lssvm_mi355_predictor_predict(multi._h, _capi.ptr(pool[:100]), C.c_int(_capi.LSSVM_MEM_HOST), C.c_size_t(100), _capi.ptr(out), None))
        assert np.array_equal(out, want)
        out2 = np.zeros((100, 1), np.float32)
        _capi.check(_capi.predictor_multi_entry("lssvm_mi355_predictor_predict_multi")(single._h, _capi.ptr(pool[:100]), _capi.LSSVM_MEM_HOST, 100, _capi.ptr(out2), None))
        assert np.array_equal(out2[:, 0], want)


def test_the_single_vector_entry_point_refuses_a_handle_of_three_vectors():
    sv, pool = data(64, np.float32)
    alpha, rho = weights(3, np.float32)
    with backend.Predictor(Parameter(kernel_type="rbf", gamma=1.0 / 64), sv, alpha, rho) as pred:
        out = np.zeros(100 * 3, np.float32)
        with pytest.raises(InvalidParameterError, match="more than one weight vector"):
            _capi.check(_capi.lib.lssvm_mi355_predictor_predict(pred._h, _capi.ptr(pool[:100]), C.c_int(_capi.LSSVM_MEM_HOST), C.c_size_t(100), _capi.ptr(out), None))
        assert np.all(out == 0)
        assert pred.predict(pool[:100]).shape == (100, 3)  # (the handle is as good as before)


# ------------------------------------------------------------------------------------------------------------ batch and values in HBM
def test_batch_and_values_in_hbm():
    """predict_multi with LSSVM_MEM_DEVICE: torch tensors on device 0 in, [npoints][k] out -- the bits of the call from host buffers, on the resident paths, for fp64 (the
    one-shot path inside the predictor) and for a batch the resident form declines.  In a process of its own, as tests/test_gpu_interop.py runs torch."""
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests')
import torch
from plssvm_amd import backend
from plssvm_amd.parameter import Parameter
from plssvm_amd.datagen import make_blobs_pm1
rng = np.random.default_rng(5)
k = 3
for kernel, dt in (('rbf', np.float32), ('linear', np.float32), ('polynomial', np.float32), ('rbf', np.float64)):
    X, _ = make_blobs_pm1(2500 + 9000, 96, seed=3, dtype=dt)
    sv, pts = X[:2500], X[2500:]
    alpha = rng.standard_normal((k, 2500)).astype(dt)
    with backend.Predictor(Parameter(kernel_type=kernel, degree=2, gamma=1.0 / 96, coef0=1.0), sv, alpha, np.array([0.25, 0.5, -1.0])) as pred:
        for batch in (pts, pts[:77], (pts * 12.0).astype(dt)):
            info_h, info_d = {}, {}
            want = pred.predict(batch, info_out=info_h)
            Pd = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
            Od = torch.full((batch.shape[0], k), float('nan'), dtype=Pd.dtype, device='cuda')
            torch.cuda.synchronize()
            pred.predict_device(Pd.data_ptr(), batch.shape[0], Od.data_ptr(), info_out=info_d)
            got = Od.cpu().numpy()
            assert np.array_equal(got, want), (kernel, dt, batch.shape, float(np.max(np.abs(got - want))))
            assert info_d['resident'] == info_h['resident'] and info_d['vectors_per_launch'] == info_h['vectors_per_launch'], (kernel, dt, info_d, info_h)
            assert np.array_equal(Pd.cpu().numpy(), batch)  # the caller's tensor is read only
print('OK')
""" % (ROOT, ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------------------ what residency is for
@pytest.mark.parametrize("kernel", ["rbf", "polynomial"])
@pytest.mark.parametrize("npts", [100, 4096])
def test_the_resident_call_takes_less_time_than_the_one_shot_call(kernel, npts):
    """k = 4: the support vectors are not uploaded and prepared again, and no record is packed per launch (the best of three calls each: now and then one call of a
    long-lived process takes tens of milliseconds longer than its kernels -- the form and the reason of the single-vector predictor's assertion)."""
    sv, pool = data(100, np.float32)
    alpha, rho = weights(4, np.float32)
    prm = Parameter(kernel_type=kernel, degree=3, gamma=1.0 / 100, coef0=COEF0)
    pts = pool[:npts]
    with backend.Predictor(prm, sv, alpha, rho) as pred:
        pred.predict(pts)
        t_res, t_one = [], []
        for _ in range(3):
            a, b = {}, {}
            pred.predict(pts, info_out=a)
            backend.predict_values_multi(prm, sv, alpha, rho.astype(np.float32), None, pts, info_out=b)
            assert a["resident"] == 1
            t_res.append(a["total_ms"])
            t_one.append(b["total_ms"])
    print(f"{kernel} {npts} points, k = 4: resident {min(t_res):.3f} ms, one-shot {min(t_one):.3f} ms")
    assert min(t_res) < min(t_one), (t_res, t_one)


# ------------------------------------------------------------------------------------------------------------ SVC
@pytest.mark.parametrize("kernel", ["rbf", "poly", "linear"])
@pytest.mark.parametrize("k, seed", [(3, 11), (5, 7)])
def test_svc_keeps_its_model_resident(k, seed, kernel):
    """A multi-class SVC: the labels of predict_classes over predict_values_multi, from a predictor that the second predict reuses and that a set_option on the backend
    object or a refit replaces."""
    X, y = make_blobs_multiclass(3000 + 4000, 32, k, seed=seed, dtype=np.float64)
    Xt, yt, Xh = X[:3000], y[:3000], X[3000:]
    clf = SVC(kernel=kernel, C=1.0, gamma=1.0 / 32, tol=1e-3, real_type=np.float32).fit(Xt, yt)  # (float32: the resident form)
    m = clf._model
    assert not hasattr(m, "_predictor")
    predicted = clf.predict(Xh)
    first = m._predictor["predictor"]
    assert first.num_vectors == k
    values, _ = backend.predict_values_multi(m.params, m.support_vectors, m.alpha, m.rho, None, Xh.astype(m.support_vectors.dtype))
    assert np.array_equal(predicted, multiclass.predict_classes(clf.classes_, values))
    assert np.array_equal(clf.predict(Xh), predicted) and m._predictor["predictor"] is first  # reused
    assert clf.decision_function(Xh[:50]).shape == (50, k) and m._predictor["predictor"] is first
    assert clf.score(Xh, predicted) == 1.0 and m._predictor["predictor"] is first
    clf._svm.set_option("gram_mode", 1)  # a changed option of the backend object: a new predictor, the old one closed
    assert np.array_equal(clf.predict(Xh), predicted)
    second = m._predictor["predictor"]
    assert second is not first and not first._h and second._h
    clf.fit(Xt, yt)  # a refit: a new model, and with it a new predictor
    assert clf._model is not m and not hasattr(clf._model, "_predictor")
    assert np.array_equal(clf.predict(Xh), predicted)
    assert clf._model._predictor["predictor"] is not second
