"""GPU (-m gpu): the resident predictor for models beyond the one-pass kernels -- ``backend.Predictor(..., panels=True)`` (``lssvm_mi355_predictor_create_panels``) on
float32 rbf / polynomial models of more than 512 / 384 features and float64 models of more than 256 -- and the two-vector instantiations of the panel kernels behind it
(plssvm_amd/csrc/tile_launch_f32xv2.hip, tile_launch_f64xv2.hip).

What is asserted, and why:
  * every column against the SINGLE-VECTOR panels predictor of that (alpha_v, rho_v) with the same options: EXACT equality.  NV = 2 keeps each vector's chain of operations
    identical to NV = 1; there is nothing to tolerate.
  * float64, and float32 rbf, against predict_values_multi: EXACT equality (the resident form pads, centres, scales, splits and chunks as the one-shot call does).
  * float32 polynomial against predict_values_multi, and every float32 model against a float64 numpy evaluation: 16 eps_fp32 of the summand scale
    sum_j |alpha_v,j| max |gamma x.s + coef0|^degree -- bar and scale of tests/test_gpu_predictor_multi.py and tests/test_gpu_predictor_f32_wide.py.  Not exact, because the
    planes' power-of-two scale comes from the support vectors alone in the resident form and from both sides in the one-shot call.  The one-shot call's own distance to
    float64 is printed beside it.
  * lssvm_predict_info: resident, gram_mode, and vectors_per_launch = 2 for k >= 2 wherever the library's routing function (panel_pair_routed, lssvm_problem.hip)
    dispatches the pair launch -- every instantiation --, 1 for k = 1 and for float32 rbf on unfolded records (rbf_fold = 0).
  * what the form declines has resident == 0 and the one-shot call's bits and info.

300 support vectors are three column tiles, the last one ragged; the batches are 1, 100 and 300 points."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from plssvm_amd import backend
from plssvm_amd._capi import Options
from plssvm_amd.csvm import make_csvm
from plssvm_amd.data_set import DataSet
from plssvm_amd.datagen import make_blobs_multiclass, make_blobs_pm1
from plssvm_amd.parameter import KernelFunctionType, Parameter
from plssvm_amd.svc import SVC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = float(np.finfo(np.float32).eps)
COEF0 = 0.5
NSV, POOL = 300, 300
BATCHES = (1, 100, 300)
BAR = 16.0  # eps_fp32 of the summand scale
F32, F64 = np.float32, np.float64
NOT_TIMES = ("rbf_exponent_scale", "f16_row_rel_error", "gram_mode", "rbf_direct", "resident", "vectors_per_launch")  # lssvm_predict_info apart from the times


def pair_routed(dtype, prm, opts):
    """the library's panel_pair_routed (lssvm_problem.hip) names no instantiation: every pair that HAS a pair record runs as one launch -- float64, the polynomial kernel,
    float32 rbf on folded records"""
    return not (dtype == F32 and is_rbf(prm) and opts.get("rbf_fold", 1) == 0)


@functools.lru_cache(maxsize=None)
def data(d, dtype=F32, nsv=NSV, pool=POOL, seed=23):
    X, _ = make_blobs_pm1(nsv + pool, d, seed=seed, dtype=dtype)
    return X[:nsv], X[nsv:]


@functools.lru_cache(maxsize=None)
def two_populations(d, nsv=NSV, pool=POOL):
    """entries ~1e+4 and ~1e-4, eight decades apart (tests/test_gpu_predictor_f32_wide.py): fails the f16 check by itself"""
    rng = np.random.default_rng(11)
    X = rng.standard_normal((nsv + pool, d)).astype(np.float32)
    big = np.arange(nsv + pool) % 2 == 0
    X[big] *= np.float32(1e4)
    X[~big] *= np.float32(1e-4)
    return X[:nsv], X[nsv:]


def weights(k, nsv, dtype=F32, seed=17):
    """the k-vector models are the first k rows of one matrix, so that the single-vector predictors serve every k"""
    rng = np.random.default_rng(seed + 3)
    return rng.standard_normal((5, nsv)).astype(dtype)[:k], (0.125 + 0.25 * np.arange(5))[:k].astype(np.float64)


def is_rbf(prm):
    return prm.kernel_type == KernelFunctionType.RBF


def reference(prm, sv, alpha, rho, pts):
    """(float64 values, per-vector summand scale sum_j |alpha_v,j| max |k|)"""
    P, S = pts.astype(np.float64), sv.astype(np.float64)
    G = P @ S.T
    gamma = float(sv.dtype.type(prm.gamma))
    if is_rbf(prm):
        sq = np.sum(P * P, axis=1)[:, None] + np.sum(S * S, axis=1)[None, :] - 2.0 * G
        K, peak = np.exp(-gamma * np.maximum(sq, 0.0)), 1.0
    else:
        base = gamma * G + float(prm.coef0)
        K, peak = base ** int(prm.degree), float(np.max(np.abs(base))) ** int(prm.degree)
    scales = np.abs(alpha.astype(np.float64)).sum(axis=1) * peak
    return K @ alpha.astype(np.float64).T - np.asarray(rho, dtype=np.float64)[None, :], scales


def check_model(prm, sv, pool, opts=None, ks=(1, 2, 3), batches=BATCHES, gram_mode=None):
    """the panels predictor of k vectors on every batch: info, the single-vector panels predictors' bits, predict_values_multi, float64, a second call"""
    opts = opts or {}
    dtype = sv.dtype.type
    f32 = dtype == F32
    exact = (not f32) or is_rbf(prm)
    d = sv.shape[1]
    kmax = max(ks)
    alpha_all, rho_all = weights(kmax, sv.shape[0], dtype)
    singles = [backend.Predictor(prm, sv, alpha_all[v], float(rho_all[v]), options=Options(**opts), panels=True) for v in range(kmax)]
    refs, want_single = {}, {}
    try:
        f64_all, scales = reference(prm, sv, alpha_all, rho_all, pool[:max(batches)])
        for npts in batches:
            pts = pool[:npts]
            multi = {}
            one, _ = backend.predict_values_multi(prm, sv, alpha_all, rho_all.astype(dtype), None, pts, options=Options(**opts), info_out=multi)
            refs[npts] = (one, multi, f64_all[:npts])
            for v in range(kmax):
                single = {}
                want_single[(npts, v)] = (singles[v].predict(pts, info_out=single), single)
        for k in ks:
            with backend.Predictor(prm, sv, alpha_all[:k], rho_all[:k], options=Options(**opts), panels=True) as pred:
                for npts in batches:
                    pts = pool[:npts]
                    info = {}
                    got = pred.predict(pts, info_out=info)
                    one, multi, f64 = refs[npts]
                    assert got.shape == (npts, k) and got.dtype == dtype
                    assert info["resident"] == 1, (k, npts, info)
                    assert info["gram_mode"] == (gram_mode if gram_mode is not None else multi["gram_mode"]), (k, npts, info, multi)
                    assert info["vectors_per_launch"] == (2 if k >= 2 and pair_routed(dtype, prm, opts) else 1), (k, npts, info)
                    assert info["kernel_ms"] > 0 and info["total_ms"] >= info["kernel_ms"]
                    for v in range(k):
                        want, single = want_single[(npts, v)]
                        differ = np.flatnonzero(got[:, v] != want)
                        assert differ.size == 0, (k, npts, v, differ.size, got[differ[0], v], want[differ[0]])
                        assert single["resident"] == 1 and single["vectors_per_launch"] == 0 and single["gram_mode"] == info["gram_mode"], (single, info)
                    assert np.all(np.isfinite(got))
                    err = np.max(np.abs(got.astype(np.float64) - one[:, :k]), axis=0) / (EPS32 * scales[:k])
                    err64 = np.max(np.abs(got - f64[:, :k]), axis=0) / (EPS32 * scales[:k])
                    one64 = np.max(np.abs(one[:, :k] - f64[:, :k]), axis=0) / (EPS32 * scales[:k])
                    print(f"{np.dtype(dtype).name} {prm.kernel_type} degree {prm.degree} k={k} d={d} nsv={sv.shape[0]} {opts} {npts} points: gram_mode {info['gram_mode']}, "
                          f"vectors_per_launch {info['vectors_per_launch']} (one-shot {multi['vectors_per_launch']}), against predict_values_multi {err.max():.2f} eps, against float64 "
                          f"{err64.max():.2f} eps, the one-shot call against float64 {one64.max():.2f} eps_fp32 of the summand scale")
                    if exact:
                        assert np.array_equal(got, one[:, :k]), (k, npts, err)
                    else:
                        assert np.all(err <= BAR), (k, npts, err)
                    if f32:
                        assert np.all(err64 <= BAR), (k, npts, err64, one64)
                    assert np.array_equal(pred.predict(pts), got)  # (a second call: the resident records are read, never written)
    finally:
        for s in singles:
            s.close()


def params(kernel, degree, d, coef0=COEF0, gamma=None):
    return Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d if gamma is None else gamma, coef0=coef0)


def kid(kernel, degree):
    return kernel if kernel == "rbf" else f"poly{degree}"


# ------------------------------------------------------------------------------------------------------------ 1. every edge of the panel walk
F32_CASES = [(d, "polynomial", g) for d in (576, 784, 1100) for g in (2, 3, 5)] + [(d, "rbf", 3) for d in (448, 784)]


@pytest.mark.parametrize("d, kernel, degree", F32_CASES, ids=[f"{d}-{kid(k, g)}" for d, k, g in F32_CASES])
def test_f32_f16x3_every_panel_count(d, kernel, degree):
    """576 -> 5 panels of 128 features, 784 -> 7, 1 100 -> 9 (ragged features); rbf: 448 -> 4, the fewest the panel kernel meets, and 784"""
    sv, pool = data(d)
    check_model(params(kernel, degree, d), sv, pool, gram_mode=2)


@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 3)], ids=["rbf", "poly3"])
@pytest.mark.parametrize("d", [448, 784])
def test_f32_bf16x6_planes(d, kernel, degree):
    sv, pool = data(d)
    check_model(params(kernel, degree, d), sv, pool, opts={"gram_mode": 1}, gram_mode=1)


F64_CASES = [(d, k, g) for d in (257, 300, 784) for k, g in (("rbf", 3), ("polynomial", 2), ("polynomial", 3), ("polynomial", 5))]


@pytest.mark.parametrize("d, kernel, degree", F64_CASES, ids=[f"{d}-{kid(k, g)}" for d, k, g in F64_CASES])
def test_f64_every_panel_count(d, kernel, degree):
    """257 -> 5 panels of 64 features (the fewest), 300 -> 5, 784 -> 13"""
    sv, pool = data(d, F64)
    check_model(params(kernel, degree, d), sv, pool)


@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 3)], ids=["rbf", "poly3"])
@pytest.mark.parametrize("dtype, d", [(F32, 784), (F64, 300)], ids=["f32-784", "f64-300"])
def test_row_slabs_reduced_over_three_column_chunks(dtype, d, kernel, degree):
    """j_chunk_tiles = 1: every column tile is a chunk of its own, the row slabs of both vectors are reduced over three of them"""
    sv, pool = data(d, dtype)
    check_model(params(kernel, degree, d), sv, pool, opts={"j_chunk_tiles": 1}, ks=(1, 3))


@pytest.mark.parametrize("d", [448, 784])
def test_f32_unfolded_rbf_records_run_one_vector_per_launch(d):
    """rbf_fold = 0: the records keep c_j in their second half, which leaves no room for a second vector -- the single-vector panel kernel on the resident data"""
    sv, pool = data(d)
    check_model(params("rbf", 3, d), sv, pool, opts={"rbf_fold": 0}, ks=(1, 3), gram_mode=2)


# ------------------------------------------------------------------------------------------------------------ 2. ragged column side
@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 3)], ids=["rbf", "poly3"])
@pytest.mark.parametrize("nsv", [1, 127, 129])
@pytest.mark.parametrize("dtype, d", [(F32, 576), (F64, 300)], ids=["f32-576", "f64-300"])
def test_ragged_column_side(dtype, d, nsv, kernel, degree):
    sv, pool = data(d, dtype)
    check_model(params(kernel, degree, d), sv[:nsv], pool, ks=(3,), batches=(300,))


# ------------------------------------------------------------------------------------------------------------ 3. automatic chunking
@pytest.mark.parametrize("dtype, d, kernel", [(F32, 576, "polynomial"), (F32, 448, "rbf"), (F64, 300, "rbf")], ids=["f32-576-poly3", "f32-448-rbf", "f64-300-rbf"])
def test_automatic_chunking_3001_support_vectors_9000_points_five_vectors(dtype, d, kernel):
    """24 column tiles x 72 row blocks: the column chunks the geometry chooses by itself; two pairs and an odd vector"""
    sv, pool = data(d, dtype, 3001, 9000, seed=29)
    check_model(params(kernel, 3, d), sv, pool, ks=(5,), batches=(9000,))


# ------------------------------------------------------------------------------------------------------------ 4. what the form declines
def declined(prm, sv, alpha, rho, batch, opts, pred):
    info, one = {}, {}
    got = pred.predict(batch, info_out=info)
    want, _ = backend.predict_values_multi(prm, sv, alpha, rho.astype(sv.dtype), None, batch, options=Options(**opts), info_out=one)
    assert info["resident"] == 0, info
    assert np.array_equal(got, want), float(np.max(np.abs(got - want)))
    for key in NOT_TIMES:
        assert info[key] == one[key] or (key == "f16_row_rel_error" and np.isnan(info[key]) and np.isnan(one[key])), (key, info, one)


DECLINED = [("f32_negative_degree", F32, "polynomial", -1, 576, {}), ("f64_negative_degree", F64, "polynomial", -1, 300, {}),
            ("f32_gram_mode_0", F32, "polynomial", 3, 576, {"gram_mode": 0}), ("f32_gram_mode_0_rbf", F32, "rbf", 3, 448, {"gram_mode": 0}),
            ("f32_tile_kernel_1", F32, "rbf", 3, 448, {"tile_kernel": 1}), ("f64_tile_kernel_1", F64, "rbf", 3, 300, {"tile_kernel": 1}),
            ("f32_rbf_form_1", F32, "rbf", 3, 448, {"rbf_form": 1}), ("f32_rbf_form_3", F32, "rbf", 3, 448, {"rbf_form": 3}),
            ("f32_exponent_scale_beyond_the_norm_expansion", F32, "rbf", 3, 448, {})]


@pytest.mark.parametrize("case, dtype, kernel, degree, d, opts", DECLINED, ids=[c[0] for c in DECLINED])
def test_models_the_form_declines_equal_predict_values_multi(case, dtype, kernel, degree, d, opts):
    sv, pool = data(d, dtype)
    alpha, rho = weights(3, NSV, dtype)
    prm = params(kernel, degree, d)
    if degree < 0:  # (positive data, coef0 = 0: no base near zero)
        sv, pool = np.abs(sv) + dtype(0.25), np.abs(pool) + dtype(0.25)
        prm = params(kernel, degree, d, coef0=0.0)
    if case.endswith("norm_expansion"):  # exponent scale 2 gamma log2(e) max |x - mean|^2 = 100 > 32: beyond the automatic choice of the norm expansion
        mean = sv.astype(np.float64).mean(axis=0)
        sq = float(np.max(np.sum((sv.astype(np.float64) - mean) ** 2, axis=1)))
        prm = Parameter(kernel_type="rbf", gamma=float(np.float32(100.0 / (2.0 * 1.4426950408889634 * sq))))
    with backend.Predictor(prm, sv, alpha, rho, options=Options(**opts), panels=True) as pred:
        declined(prm, sv, alpha, rho, pool, opts, pred)


@pytest.mark.parametrize("case", ["far_batch", "f16_check"])
def test_batches_the_form_declines_after_a_resident_call_on_the_same_handle(case):
    """The handle keeps no host copy of its support vectors: the declined batch brings them back from HBM (fetch_support_vectors)."""
    alpha, rho = weights(3, NSV)
    if case == "far_batch":  # further from the support vectors' centre than the norm expansion allows
        d = 448
        sv, pool = data(d)
        prm, batch = params("rbf", 3, d), (pool * 12.0).astype(np.float32)
    else:  # a batch that two f16 planes do not represent, beside support vectors that pass
        d = 576
        sv, pool = data(d)
        prm, batch = params("polynomial", 3, d), two_populations(d)[1]
    with backend.Predictor(prm, sv, alpha, rho, panels=True) as pred:
        near = {}
        first = pred.predict(pool, info_out=near)
        assert near["resident"] == 1 and near["vectors_per_launch"] == 2 and near["gram_mode"] == 2, near
        declined(prm, sv, alpha, rho, batch, {}, pred)
        again = {}
        assert np.array_equal(pred.predict(pool, info_out=again), first) and again["resident"] == 1  # (the handle is as good as before)


# ------------------------------------------------------------------------------------------------------------ 5. beside the old entry points
@pytest.mark.parametrize("dtype, kernel, d", [(F32, "polynomial", 576), (F32, "rbf", 448), (F64, "rbf", 300)], ids=["f32-poly3-576", "f32-rbf-448", "f64-rbf-300"])
def test_every_form_handles_keep_declining_these_widths(dtype, kernel, d):
    sv, pool = data(d, dtype)
    alpha, rho = weights(3, NSV, dtype)
    prm = params(kernel, 3, d)
    with backend.Predictor(prm, sv, alpha, rho, panels=True) as wide, backend.Predictor(prm, sv, alpha, rho, every_form=True) as old:
        a, b = {}, {}
        want, got = wide.predict(pool, info_out=a), old.predict(pool, info_out=b)
        assert a["resident"] == 1 and a["vectors_per_launch"] == 2 and b["resident"] == 0 and b["vectors_per_launch"] == 1, (a, b)
        if dtype == F64 or kernel == "rbf":
            assert np.array_equal(got, want)
        else:
            _, scales = reference(prm, sv, alpha, rho, pool)
            assert np.all(np.max(np.abs(got.astype(np.float64) - want), axis=0) <= BAR * EPS32 * scales)


# ------------------------------------------------------------------------------------------------------------ 6. narrow models through the new handle
@pytest.mark.parametrize("kernel", ["rbf", "polynomial", "linear"])
@pytest.mark.parametrize("dtype, d", [(F32, 64), (F32, 192), (F64, 100)], ids=["f32-64", "f32-192", "f64-100"])
def test_a_model_that_is_not_panel_wide_behaves_as_on_an_every_form_handle(dtype, d, kernel):
    sv, pool = data(d, dtype)
    prm = params(kernel, 3, d)
    for k in (1, 3):
        alpha, rho = weights(k, NSV, dtype)
        with backend.Predictor(prm, sv, alpha, rho, panels=True) as new, backend.Predictor(prm, sv, alpha, rho, every_form=True) as old:
            for npts in BATCHES:
                a, b = {}, {}
                got, want = new.predict(pool[:npts], info_out=a), old.predict(pool[:npts], info_out=b)
                assert np.array_equal(got, want), (k, npts)
                assert {key: a[key] for key in NOT_TIMES} == {key: b[key] for key in NOT_TIMES}, (k, npts, a, b)


# ------------------------------------------------------------------------------------------------------------ 7. batch and values in HBM
def test_batch_and_values_in_hbm():
    """predict_multi with LSSVM_MEM_DEVICE on panel-wide models, k = 3: the bits and the info of the call from host buffers.  In a process of its own, as
    tests/test_gpu_predictor_multi.py runs torch."""
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests')
import torch
from plssvm_amd import backend
from plssvm_amd.parameter import Parameter
from plssvm_amd.datagen import make_blobs_pm1
rng = np.random.default_rng(5)
k = 3
for dtype, kernel, d in ((np.float32, 'rbf', 448), (np.float32, 'polynomial', 576), (np.float64, 'rbf', 300)):
    X, _ = make_blobs_pm1(300 + 300, d, seed=3, dtype=dtype)
    sv, pts = X[:300], X[300:]
    alpha = rng.standard_normal((k, 300)).astype(dtype)
    with backend.Predictor(Parameter(kernel_type=kernel, degree=3, gamma=1.0 / d, coef0=0.5), sv, alpha, np.array([0.25, 0.5, -1.0]), panels=True) as pred:
        for batch in (pts, pts[:77]):
            info_h, info_d = {}, {}
            want = pred.predict(batch, info_out=info_h)
            Pd = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
            Od = torch.full((batch.shape[0], k), float('nan'), dtype=Pd.dtype, device='cuda')
            torch.cuda.synchronize()
            pred.predict_device(Pd.data_ptr(), batch.shape[0], Od.data_ptr(), info_out=info_d)
            got = Od.cpu().numpy()
            assert np.array_equal(got, want), (kernel, batch.shape, float(np.max(np.abs(got - want))))
            assert info_h['resident'] == 1 and info_h['vectors_per_launch'] == 2, info_h
            for key in ('resident', 'vectors_per_launch', 'gram_mode', 'rbf_direct', 'rbf_exponent_scale', 'f16_row_rel_error'):
                assert info_d[key] == info_h[key], (kernel, key, info_d, info_h)
            assert np.array_equal(Pd.cpu().numpy(), batch)  # the caller's tensor is read only
print('OK')
""" % (ROOT, ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------------------ 8. through the public objects
@pytest.mark.parametrize("real_type, d", [(F32, 576), (F64, 300)], ids=["f32-576", "f64-300"])
def test_svc_decision_function_of_three_classes_on_a_panel_wide_model(real_type, d):
    X, y = make_blobs_multiclass(400 + 300, d, 3, seed=11, dtype=np.float64)
    Xt, yt, Xh = X[:400], y[:400], X[400:]
    clf = SVC(kernel="rbf", C=1.0, gamma=1.0 / d, tol=1e-3, real_type=real_type).fit(Xt, yt)
    m = clf._model
    got = clf.decision_function(Xh)
    assert got.dtype == real_type and got.shape == (300, 3)
    info = {}
    with backend.Predictor(m.params, m.support_vectors, m.alpha, m.rho, panels=True) as pred:
        want = pred.predict(Xh.astype(real_type), info_out=info)
    assert info["resident"] == 1 and info["vectors_per_launch"] == 2, info
    assert np.array_equal(got, want)
    m._predictor["predictor"].predict(Xh.astype(real_type), info_out=info)
    assert info["resident"] == 1 and info["vectors_per_launch"] == 2, info


def test_csvm_predict_keeps_a_binary_576_feature_float32_model_resident():
    X, y = make_blobs_pm1(400, 576, seed=41, dtype=np.float32)
    ds = DataSet(X, [int(v) for v in y], real_type=np.float32)
    svm = make_csvm("mi355", params=Parameter(kernel_type="rbf"))
    model = svm.fit(ds, epsilon=1e-4, max_iter=100)
    labels = svm.predict(model, ds)
    assert svm.last_predict_phases["resident"] == 1, svm.last_predict_phases
    assert list(svm.predict(model, ds)) == list(labels) and svm.last_predict_phases["resident"] == 1
