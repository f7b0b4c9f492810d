"""GPU (-m gpu): the resident fp32 predictor beyond 128 features -- ``backend.Predictor(..., every_form=True)`` on float32 rbf / polynomial models of 129 ... 512 features --
and the wide two-vector instantiations of the 128-row full-square split kernels behind it (plssvm_amd/csrc/tile_launch_f32v2w.hip).

What is asserted, and why:
  * every column against the SINGLE-VECTOR every_form predictor of that (alpha_v, rho_v) with the same options: EXACT equality.  NV = 2 keeps each vector's chain of
    operations identical to NV = 1; there is nothing to tolerate.
  * rbf against predict_values_multi: EXACT equality (the resident form centres, scales, splits and chunks the batch as the one-shot call does).
  * polynomial against predict_values_multi, and sampled rows of every kernel against a float64 numpy evaluation: 16 eps_fp32 of the summand scale
    sum_j |alpha_v,j| max |gamma x.s + coef0|^degree -- bar and scale of tests/test_gpu_predictor_multi.py.  Not exact, because the planes' power-of-two scale comes from
    the support vectors alone in the resident form and from both sides in the one-shot call.  The one-shot call's own distance to float64 is printed beside it.
  * lssvm_predict_info: resident, gram_mode, and vectors_per_launch = 2 for k >= 2 wherever the library's routing function (wide_pair_routed, lssvm_problem.hip)
    dispatches the pair launch -- every instantiation --, 1 for k = 1 and for rbf on unfolded records.
  * what the form declines has resident == 0 and the one-shot call's bits.

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
KERNELS = [("rbf", 3), ("polynomial", 2), ("polynomial", 3), ("polynomial", 5)]
KERNEL_IDS = ["rbf", "poly2", "poly3", "poly5"]
BAR = 16.0  # eps_fp32 of the summand scale


def pair_routed(gram_mode, kernel, d):
    """the library's wide_pair_routed (lssvm_problem.hip): which (plane kind, kernel function, 64-feature chunks) run a pair of vectors as one launch -- all of them"""
    return True


@functools.lru_cache(maxsize=None)
def data(d, nsv=NSV, pool=POOL, seed=23):
    X, _ = make_blobs_pm1(nsv + pool, d, seed=seed, dtype=np.float32)
    return X[:nsv], X[nsv:]


@functools.lru_cache(maxsize=None)
def two_populations(d, nsv=NSV, pool=POOL):
    """entries ~1e+4 and ~1e-4, eight decades apart (tests/test_gpu_parity.py, test_f16_planes_prescale_check_and_fallback): fails the f16 check by itself"""
    rng = np.random.default_rng(11)
    X = rng.standard_normal((nsv + pool, d)).astype(np.float32)
    big = np.arange(nsv + pool) % 2 == 0
    X[big] *= np.float32(1e4)
    X[~big] *= np.float32(1e-4)
    return X[:nsv], X[nsv:]


def weights(k, nsv, seed=17):
    """as weights() of tests/test_gpu_predictor_multi.py; the k-vector models are the first k rows of one matrix, so that the single-vector predictors serve every k"""
    rng = np.random.default_rng(seed + 3)
    return rng.standard_normal((3, nsv)).astype(np.float32)[:k], (0.125 + 0.25 * np.arange(3))[:k].astype(np.float64)


def is_rbf(prm):
    return prm.kernel_type == KernelFunctionType.RBF


def float64_kernel(prm, sv, pts):
    P, S = pts.astype(np.float64), sv.astype(np.float64)
    G = P @ S.T
    gamma = float(np.float32(prm.gamma))
    if is_rbf(prm):
        sq = np.sum(P * P, axis=1)[:, None] + np.sum(S * S, axis=1)[None, :] - 2.0 * G
        return np.exp(-gamma * np.maximum(sq, 0.0)), None
    base = gamma * G + float(prm.coef0)
    return base ** int(prm.degree), base


def reference(prm, sv, alpha, rho, pts):
    """(float64 values, per-vector summand scale sum_j |alpha_v,j| max |k|)"""
    K, base = float64_kernel(prm, sv, pts)
    peak = 1.0 if base is None else float(np.max(np.abs(base))) ** int(prm.degree)
    scales = np.abs(alpha.astype(np.float64)).sum(axis=1) * peak
    return K @ alpha.astype(np.float64).T - np.asarray(rho, dtype=np.float64)[None, :], scales


def check_model(prm, sv, pool, opts=None, ks=(1, 2, 3), batches=BATCHES, gram_mode=None):
    """the every_form predictor of k vectors on every batch: info, the single-vector every_form predictors' bits, predict_values_multi, float64, a second call"""
    opts = opts or {}
    rbf = is_rbf(prm)
    d = sv.shape[1]
    alpha3, rho3 = weights(3, sv.shape[0])
    kmax = max(ks)
    singles = [backend.Predictor(prm, sv, alpha3[v], float(rho3[v]), options=Options(**opts), every_form=True) for v in range(kmax)]
    # the one-shot call and float64 once per batch, for all three vectors (a k-vector model's one-shot columns are its first k: every vector has a launch of its own there)
    refs = {}
    try:
        want_single = {}
        for npts in batches:
            pts = pool[:npts]
            multi = {}
            one, _ = backend.predict_values_multi(prm, sv, alpha3[:kmax], rho3[:kmax].astype(np.float32), None, pts, options=Options(**opts), info_out=multi)
            f64, scales = reference(prm, sv, alpha3[:kmax], rho3[:kmax], pool)
            refs[npts] = (one, multi, f64[:npts], scales)
            for v in range(kmax):
                single = {}
                want_single[(npts, v)] = (singles[v].predict(pts, info_out=single), single)
        for k in ks:
            alpha, rho = alpha3[:k], rho3[:k]
            with backend.Predictor(prm, sv, alpha, rho, options=Options(**opts), every_form=True) as pred:
                for npts in batches:
                    pts = pool[:npts]
                    info = {}
                    got = pred.predict(pts, info_out=info)
                    one, multi, f64, scales = refs[npts]
                    assert got.shape == (npts, k) and got.dtype == np.float32
                    assert info["resident"] == 1, (k, npts, info)
                    if gram_mode is not None:
                        assert info["gram_mode"] == gram_mode, (k, npts, info)
                    pair = pair_routed(info["gram_mode"], prm.kernel_type, d)
                    assert info["vectors_per_launch"] == (2 if k >= 2 and pair else 1), (k, npts, info)
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
                    print(f"{prm.kernel_type} degree {prm.degree} k={k} d={d} nsv={sv.shape[0]} {opts} {npts} points: gram_mode {info['gram_mode']}, vectors_per_launch "
                          f"{info['vectors_per_launch']} (one-shot {multi['vectors_per_launch']}), against predict_values_multi {err.max():.2f} eps, against float64 {err64.max():.2f} eps, "
                          f"the one-shot call against float64 {one64.max():.2f} eps of the summand scale")
                    if rbf:
                        assert np.array_equal(got, one[:, :k]), (k, npts, err)
                        assert multi["gram_mode"] == info["gram_mode"], (multi, info)
                    else:
                        assert np.all(err <= BAR), (k, npts, err)
                    assert np.all(err64 <= BAR), (k, npts, err64, one64)
                    assert np.array_equal(pred.predict(pts), got)  # (a second call: the resident records are read, never written)
    finally:
        for s in singles:
            s.close()


def params(kernel, degree, d, coef0=COEF0, gamma=None):
    return Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d if gamma is None else gamma, coef0=coef0)


# ------------------------------------------------------------------------------------------------------------ 1. every chunk count
# (rbf holds three row planes: up to 384 features; beyond, the feature-panel kernel runs and the form declines -- test_models_the_form_declines_equal_predict_values_multi)
CHUNK_CASES = [(d, kernel, degree) for d in (130, 192, 256, 320, 384, 448, 500, 512) for kernel, degree in KERNELS if kernel != "rbf" or d <= 384]


@pytest.mark.parametrize("d, kernel, degree", CHUNK_CASES, ids=[f"{d}-{k if k == 'rbf' else 'poly' + str(g)}" for d, k, g in CHUNK_CASES])
def test_every_chunk_count(d, kernel, degree):
    """Three (130: ragged features) to eight 64-feature chunks on the default planes (f16x3 on this data); k = 1, 2, 3 on 1, 100 and 300 points."""
    sv, pool = data(d)
    check_model(params(kernel, degree, d), sv, pool, gram_mode=2)


@pytest.mark.parametrize("kernel, degree", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("d", [192, 384])
def test_row_slabs_reduced_over_three_column_chunks(d, kernel, degree):
    """j_chunk_tiles = 1: every column tile is a chunk of its own, the row slabs of both vectors are reduced over three of them"""
    sv, pool = data(d)
    check_model(params(kernel, degree, d), sv, pool, opts={"j_chunk_tiles": 1}, ks=(1, 3), gram_mode=2)


# ------------------------------------------------------------------------------------------------------------ 2. bf16x6 planes
@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 3)], ids=["rbf", "poly3"])
@pytest.mark.parametrize("d", [192, 384])
def test_bf16x6_planes(d, kernel, degree):
    sv, pool = data(d)
    check_model(params(kernel, degree, d), sv, pool, opts={"gram_mode": 1}, ks=(3,), gram_mode=1)


@pytest.mark.parametrize("kernel, opts", [("polynomial", {}), ("polynomial", {"gram_mode": 1}), ("rbf", {"gram_mode": 1})], ids=["poly3-by-the-check", "poly3-bf16x6", "rbf-bf16x6"])
def test_bf16x6_planes_for_support_vectors_of_two_populations_eight_decades_apart(kernel, opts):
    """Data that fails the f16 check by itself: with the default Gram mode the support vectors' planes become bf16x6 at set-up (polynomial; for rbf, whose check accepts
    an absolute bound on the exponent, bf16x6 is asked for).  gamma = 1 / (d 1e8): the effect of 1 / d on unit-variance data, as in the test this data comes from."""
    d = 192
    sv, pool = two_populations(d)
    check_model(params(kernel, 3, d, gamma=1.0 / (d * 1e8)), sv, pool, opts=opts, ks=(3,), gram_mode=1)


# ------------------------------------------------------------------------------------------------------------ 3. ragged column side
@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 3)], ids=["rbf", "poly3"])
@pytest.mark.parametrize("nsv", [1, 127, 129])
def test_ragged_column_side(nsv, kernel, degree):
    d = 192
    sv, pool = data(d)
    check_model(params(kernel, degree, d), sv[:nsv], pool, ks=(3,), batches=(300,), gram_mode=2)


# ------------------------------------------------------------------------------------------------------------ 4. negative degree
def test_negative_degree_padded_columns_contribute_zero_to_both_vectors():
    """degree -1, coef0 = 0, positive data: a padded column's kernel value is 0^-1 = inf, which the kernel must replace by zero for BOTH vectors (150 support vectors:
    106 padded columns in the second tile)."""
    d, nsv = 192, 150
    sv, pool = data(d)
    sv, pool = np.abs(sv[:nsv]) + np.float32(0.25), np.abs(pool) + np.float32(0.25)
    prm = params("polynomial", -1, d, coef0=0.0)
    alpha, rho = weights(3, nsv)
    f64, scales = reference(prm, sv, alpha, rho, pool)
    singles = [backend.Predictor(prm, sv, alpha[v], float(rho[v]), every_form=True) for v in range(3)]
    try:
        with backend.Predictor(prm, sv, alpha, rho, every_form=True) as pred:
            for npts in BATCHES:
                info = {}
                got = pred.predict(pool[:npts], info_out=info)
                assert info["resident"] == 1 and info["vectors_per_launch"] == 2, info
                assert np.all(np.isfinite(got)), got[~np.isfinite(got)][:4]
                for v in range(3):
                    assert np.array_equal(got[:, v], singles[v].predict(pool[:npts])), (npts, v)
                err64 = np.max(np.abs(got - f64[:npts]), axis=0) / (EPS32 * scales)
                print(f"polynomial degree -1 d={d} nsv={nsv} {npts} points: against float64 {err64.max():.2f} eps of the summand scale")
    finally:
        for s in singles:
            s.close()


# ------------------------------------------------------------------------------------------------------------ 5. unfolded rbf
@pytest.mark.parametrize("k", [2, 3])
def test_unfolded_rbf_records_run_one_vector_per_launch(k):
    """Options(rbf_form=2) at an exponent scale above 200 (the batch's scale of tests/test_gpu_predictor_multi.py): the records keep c_j in their second half, which
    leaves no room for a second vector -- the existing single-vector wide instantiations, one launch per vector."""
    d = 192
    sv, pool = data(d)
    alpha, rho = weights(k, NSV)
    mean = sv.astype(np.float64).mean(axis=0)
    sq = max(float(np.max(np.sum((M.astype(np.float64) - mean) ** 2, axis=1))) for M in (sv, pool))
    prm = Parameter(kernel_type="rbf", gamma=float(np.float32(400.0 / (2.0 * 1.4426950408889634 * sq))))
    info, multi = {}, {}
    with backend.Predictor(prm, sv, alpha, rho, options=Options(rbf_form=2), every_form=True) as pred:
        got = pred.predict(pool, info_out=info)
    assert info["resident"] == 1 and info["rbf_exponent_scale"] > 200 and info["vectors_per_launch"] == 1, info
    for v in range(k):
        with backend.Predictor(prm, sv, alpha[v], float(rho[v]), options=Options(rbf_form=2), every_form=True) as single:
            assert np.array_equal(got[:, v], single.predict(pool))
    one, _ = backend.predict_values_multi(prm, sv, alpha, rho.astype(np.float32), None, pool, options=Options(rbf_form=2), info_out=multi)
    assert np.array_equal(got, one)


# ------------------------------------------------------------------------------------------------------------ 6. 64 row blocks and more
@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 3)], ids=["rbf", "poly3"])
def test_64_row_blocks_stay_on_the_128_row_kernels(kernel, degree):
    """7 937 points are padded to 64 row blocks, where a model of at most 128 features moves to the rectangular 256-row kernel: that kernel exists up to 128 features
    only, a 192-feature model must stay on the 128-row full-square kernels -- the values of the single-vector predictors and (rbf) of the one-shot call, which does."""
    d = 192
    sv, pool = data(d, NSV, 7937, seed=29)
    check_model(params(kernel, degree, d), sv, pool, ks=(3,), batches=(7937,), gram_mode=2)


# ------------------------------------------------------------------------------------------------------------ 7. what the form declines
def declined(prm, sv, alpha, rho, batch, opts, pred):
    info, one = {}, {}
    got = pred.predict(batch, info_out=info)
    want, _ = backend.predict_values_multi(prm, sv, alpha, rho.astype(np.float32), None, batch, options=Options(**opts), info_out=one)
    assert info["resident"] == 0, info
    assert np.array_equal(got, want), float(np.max(np.abs(got - want)))
    assert info["gram_mode"] == one["gram_mode"] and info["vectors_per_launch"] == one["vectors_per_launch"], (info, one)


@pytest.mark.parametrize("case, kernel, d, opts", [("poly_576", "polynomial", 576, {}), ("rbf_448", "rbf", 448, {}), ("gram_mode_0", "rbf", 192, {"gram_mode": 0}),
                                                  ("gram_mode_0_poly", "polynomial", 192, {"gram_mode": 0}), ("tile_kernel_1", "rbf", 192, {"tile_kernel": 1})],
                         ids=lambda v: v if isinstance(v, str) and "_" in v else None)
def test_models_the_form_declines_equal_predict_values_multi(case, kernel, d, opts):
    sv, pool = data(d)
    alpha, rho = weights(3, NSV)
    prm = params(kernel, 3, d)
    with backend.Predictor(prm, sv, alpha, rho, options=Options(**opts), every_form=True) as pred:
        declined(prm, sv, alpha, rho, pool, opts, pred)


@pytest.mark.parametrize("case", ["far_batch", "f16_check"])
def test_batches_the_form_declines_after_a_resident_call_on_the_same_handle(case):
    """The handle keeps no host copy of its support vectors: the declined batch brings them back from HBM, rows 192 floats apart (fetch_support_vectors)."""
    d = 192
    sv, pool = data(d)
    alpha, rho = weights(3, NSV)
    if case == "far_batch":  # further from the support vectors' centre than the norm expansion allows
        prm, batch = params("rbf", 3, d), (pool * 12.0).astype(np.float32)
    else:  # a batch that two f16 planes do not represent, beside support vectors that pass
        prm, batch = params("polynomial", 3, d), two_populations(d)[1]
    with backend.Predictor(prm, sv, alpha, rho, every_form=True) as pred:
        near = {}
        first = pred.predict(pool, info_out=near)
        assert near["resident"] == 1 and near["vectors_per_launch"] == 2 and near["gram_mode"] == 2, near
        declined(prm, sv, alpha, rho, batch, {}, pred)
        again = {}
        assert np.array_equal(pred.predict(pool, info_out=again), first) and again["resident"] == 1  # (the handle is as good as before)


# ------------------------------------------------------------------------------------------------------------ 8. the old entry points beside it
@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 3)], ids=["rbf", "poly3"])
def test_default_handles_keep_their_routing_at_192_features(kernel, degree):
    d = 192
    sv, pool = data(d)
    alpha, rho = weights(3, NSV)
    prm = params(kernel, degree, d)
    with backend.Predictor(prm, sv, alpha, rho, every_form=True) as wide, backend.Predictor(prm, sv, alpha, rho) as multi, backend.Predictor(prm, sv, alpha[0], float(rho[0])) as single:
        a, b, c = {}, {}, {}
        want = wide.predict(pool, info_out=a)
        got_multi, got_single = multi.predict(pool, info_out=b), single.predict(pool, info_out=c)
        assert a["resident"] == 1 and b["resident"] == 0 and c["resident"] == 0, (a, b, c)
        if kernel == "rbf":
            assert np.array_equal(got_multi, want) and np.array_equal(got_single, want[:, 0])
        else:
            _, scales = reference(prm, sv, alpha, rho, pool)
            assert np.all(np.max(np.abs(got_multi.astype(np.float64) - want), axis=0) <= BAR * EPS32 * scales)


# ------------------------------------------------------------------------------------------------------------ 9. through the public objects
def test_svc_decision_function_of_three_float32_classes_on_192_features():
    X, y = make_blobs_multiclass(400 + 300, 192, 3, seed=11, dtype=np.float64)
    Xt, yt, Xh = X[:400], y[:400], X[400:]
    clf = SVC(kernel="rbf", C=1.0, gamma=1.0 / 192, tol=1e-3, real_type=np.float32).fit(Xt, yt)
    m = clf._model
    got = clf.decision_function(Xh)
    assert got.dtype == np.float32 and got.shape == (300, 3)
    info = {}
    with backend.Predictor(m.params, m.support_vectors, m.alpha, m.rho, every_form=True) as pred:
        want = pred.predict(Xh.astype(np.float32), info_out=info)
    assert info["resident"] == 1 and info["vectors_per_launch"] == 2, info
    assert np.array_equal(got, want)
    m._predictor["predictor"].predict(Xh.astype(np.float32), info_out=info)
    assert info["resident"] == 1 and info["vectors_per_launch"] == 2, info


def test_csvm_predict_keeps_a_binary_192_feature_float32_model_resident():
    X, y = make_blobs_pm1(400, 192, seed=41, dtype=np.float32)
    ds = DataSet(X, [int(v) for v in y], real_type=np.float32)
    svm = make_csvm("mi355", params=Parameter(kernel_type="rbf"))
    model = svm.fit(ds, epsilon=1e-4, max_iter=100)
    labels = svm.predict(model, ds)
    assert svm.last_predict_phases["resident"] == 1, svm.last_predict_phases
    assert list(svm.predict(model, ds)) == list(labels) and svm.last_predict_phases["resident"] == 1


# ------------------------------------------------------------------------------------------------------------ 10. batch and values in HBM
def test_batch_and_values_in_hbm():
    """predict_multi with LSSVM_MEM_DEVICE at 192 features, k = 3: the bits and the info of the call from host buffers.  In a process of its own, as
    tests/test_gpu_predictor_multi.py runs torch."""
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests')
import torch
from plssvm_amd import backend
from plssvm_amd.parameter import Parameter
from plssvm_amd.datagen import make_blobs_pm1
rng = np.random.default_rng(5)
k, d = 3, 192
X, _ = make_blobs_pm1(300 + 300, d, seed=3, dtype=np.float32)
sv, pts = X[:300], X[300:]
alpha = rng.standard_normal((k, 300)).astype(np.float32)
for kernel in ('rbf', 'polynomial'):
    with backend.Predictor(Parameter(kernel_type=kernel, degree=3, gamma=1.0 / d, coef0=0.5), sv, alpha, np.array([0.25, 0.5, -1.0]), every_form=True) as pred:
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
