"""GPU (-m gpu): the resident fp64 predictor -- lssvm_mi355_predictor_create_resident, ``backend.Predictor(..., every_form=True)`` -- and the full-square instance of the
two-vector fp64 tile kernel (tile_matvec_f64_v2<KT, NKC, false, 2>) behind it.

What is asserted, and why: EXACT equality everywhere.  The resident form pads, centres, scales and chunks as lssvm_mi355_predict_values_f64 does, and in the two-vector
kernel each vector's fma chains, butterfly and slab order are those of a single-vector launch, so every value has the bits of the one-shot call for that
(alpha_v, rho_v) whatever its partner in the launch is.  There is nothing to tolerate, and a value that differs in its last bit is a defect."""

import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from plssvm_amd import _capi, backend, multiclass
from plssvm_amd._capi import Options
from plssvm_amd.csvm import CSVM, make_csvm
from plssvm_amd.data_set import DataSet
from plssvm_amd.datagen import make_blobs_multiclass, make_blobs_pm1
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.parameter import Parameter
from plssvm_amd.svc import SVC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEF0 = 0.5
KERNELS = [("rbf", 3), ("polynomial", 2), ("polynomial", 3), ("polynomial", 5)]
KERNEL_IDS = ["rbf", "poly2", "poly3", "poly5"]


@functools.lru_cache(maxsize=None)
def data(nsv, pool, d, dt=np.float64, seed=23):
    X, _ = make_blobs_pm1(nsv + pool, d, seed=seed, dtype=dt)
    return X[:nsv], X[nsv:]


def weights(k, nsv, dt=np.float64, seed=17):
    rng = np.random.default_rng(seed + k)
    return rng.standard_normal((k, nsv)).astype(dt), 0.125 + 0.25 * np.arange(k)


def check_model(prm, sv, pool, k, batches, opts=None, resident=1, dt=np.float64):
    """the every_form predictor of k vectors on every batch: info, the bits of predict_values_multi, the bits of the single-vector every_form predictors, a second call"""
    opts = opts or {}
    alpha, rho = weights(k, sv.shape[0], dt)
    singles = [backend.Predictor(prm, sv, alpha[v], float(rho[v]), options=Options(**opts), every_form=True) for v in range(k)]
    try:
        with backend.Predictor(prm, sv, alpha, rho, options=Options(**opts), every_form=True) as pred:
            for npts in batches:
                pts = pool[:npts]
                info, multi = {}, {}
                got = pred.predict(pts, info_out=info)
                one, _ = backend.predict_values_multi(prm, sv, alpha, rho.astype(dt), None, pts, options=Options(**opts), info_out=multi)
                print(f"{prm.kernel_type} degree {prm.degree} k={k} d={sv.shape[1]} nsv={sv.shape[0]} {opts} {npts} points: resident {info['resident']}, vectors_per_launch "
                      f"{info['vectors_per_launch']}, kernel {info['kernel_ms']:.3f} ms, total {info['total_ms']:.3f} ms (one-shot {multi['total_ms']:.3f} ms), "
                      f"values differing from the one-shot call: {int(np.sum(got != one))}")
                assert got.shape == (npts, k) and got.dtype == dt
                assert info["resident"] == resident, (npts, info)
                if resident:
                    assert info["vectors_per_launch"] == (2 if k >= 2 else 1), (npts, info)
                else:
                    assert info["vectors_per_launch"] == multi["vectors_per_launch"], (npts, info, multi)
                assert info["kernel_ms"] > 0 and info["total_ms"] >= info["kernel_ms"], info
                assert np.all(np.isfinite(got))
                assert np.array_equal(got, one), (npts, int(np.sum(got != one)))
                for v in range(k):
                    single = {}
                    want = singles[v].predict(pts, info_out=single)
                    assert np.array_equal(got[:, v], want), (npts, v, int(np.sum(got[:, v] != want)))
                    assert single["resident"] == resident and single["vectors_per_launch"] == 0, single
                assert np.array_equal(pred.predict(pts), got)  # (a second call: the resident records are read, never written)
    finally:
        for s in singles:
            s.close()


# ------------------------------------------------------------------------------------------------------------ 1. bits, every chunk count
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("kernel, degree", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("d", [16, 40, 64, 80, 100, 136, 256])
def test_every_chunk_count_has_the_bits_of_the_one_shot_call(d, kernel, degree, k):
    """1, 3, 4, 5, 7, 10 and 16 k-chunks (4 -> 5: from two workgroups per CU to one; 6 -> 7: the two translation units); k = 1: a single record, 2: one pair, 3: a pair
    and an odd vector.  At d = 16 and 100 also with one column tile per work item: three column chunks (the row slabs are reduced across chunks), and at d = 16 the
    short prologue (nsteps == 2)."""
    sv, pool = data(300, 300, d)
    prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=COEF0)
    check_model(prm, sv, pool, k, (1, 100, 300))
    if d in (16, 100):
        check_model(prm, sv, pool, k, (1, 100, 300), {"j_chunk_tiles": 1})


# ------------------------------------------------------------------------------------------------------------ 2. ragged last column tile
@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 3)], ids=["rbf", "poly3"])
@pytest.mark.parametrize("nsv", [1, 127, 129])
def test_ragged_last_column_tile(nsv, kernel, degree):
    sv, pool = data(nsv, 300, 40)
    check_model(Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / 40, coef0=COEF0), sv, pool, 3, (300,))


# ------------------------------------------------------------------------------------------------------------ 3. negative degree
def test_negative_degree_zeroes_the_padded_columns_for_both_vectors():
    """degree -1 with coef0 = 0: a zero-padded column has the base 0, whose power is inf -- without the kernel's padcol rule every value of BOTH vectors would be inf or NaN
    (150 support vectors are padded to 256 columns)."""
    rng = np.random.default_rng(31)
    S = rng.uniform(0.5, 1.5, size=(150, 40))
    P = rng.uniform(0.5, 1.5, size=(100, 40))
    check_model(Parameter(kernel_type="polynomial", degree=-1, gamma=1.0 / 40, coef0=0.0), S, P, 2, (100,))


# ------------------------------------------------------------------------------------------------------------ 4. the automatic chunking
@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 3)], ids=["rbf", "poly3"])
def test_automatic_column_chunking(kernel, degree):
    """3 001 support vectors = 24 column tiles: 2 tiles per work item for the small batches, 3 for 9 000 points (72 row blocks)"""
    sv, pool = data(3001, 9000, 100)
    check_model(Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / 100, coef0=COEF0), sv, pool, 5, (1, 100, 9000))


# ------------------------------------------------------------------------------------------------------------ 5. what the form does not cover
@pytest.mark.parametrize("case", ["300_features", "tile_kernel_1"])
def test_outside_the_form_the_handle_takes_the_one_shot_path(case):
    d = 300 if case == "300_features" else 100
    sv, pool = data(300, 300, d)
    opts = {"tile_kernel": 1} if case == "tile_kernel_1" else {}
    check_model(Parameter(kernel_type="rbf", gamma=1.0 / d), sv, pool, 3, (100, 300), opts, resident=0)


def test_an_fp32_model_is_served_as_by_create_multi():
    sv, pool = data(3001, 9000, 100, np.float32)
    alpha, rho = weights(3, 3001, np.float32)
    prm = Parameter(kernel_type="rbf", gamma=1.0 / 100)
    with backend.Predictor(prm, sv, alpha, rho, options=Options(), every_form=True) as pred, backend.Predictor(prm, sv, alpha, rho, options=Options()) as default:
        for npts in (100, 9000):
            a, b = {}, {}
            got, want = pred.predict(pool[:npts], info_out=a), default.predict(pool[:npts], info_out=b)
            assert np.array_equal(got, want)
            times = ("total_ms", "setup_ms", "kernel_ms")
            assert {n: v for n, v in a.items() if n not in times} == {n: v for n, v in b.items() if n not in times}, (a, b)
            assert a["resident"] == 1, a


# ------------------------------------------------------------------------------------------------------------ 6. the old entry points stand beside it
def test_the_default_predictor_keeps_its_routing_beside_the_new_one():
    sv, pool = data(300, 300, 100)
    alpha, rho = weights(3, 300)
    prm = Parameter(kernel_type="rbf", gamma=1.0 / 100)
    with backend.Predictor(prm, sv, alpha, rho, every_form=True) as pred:
        a = {}
        got = pred.predict(pool, info_out=a)
        assert a["resident"] == 1 and a["vectors_per_launch"] == 2, a
        with backend.Predictor(prm, sv, alpha, rho) as default, backend.Predictor(prm, sv, alpha[0], float(rho[0])) as single:
            b, c = {}, {}
            assert np.array_equal(default.predict(pool, info_out=b), got)
            assert b["resident"] == 0 and b["vectors_per_launch"] == 1, b
            assert np.array_equal(single.predict(pool, info_out=c), got[:, 0])
            assert c["resident"] == 0 and c["vectors_per_launch"] == 0, c


# ------------------------------------------------------------------------------------------------------------ 7. batch and values in HBM
def test_batch_and_values_in_hbm():
    """predict / predict_multi with LSSVM_MEM_DEVICE on an every_form handle: torch tensors on device 0 in, [npoints][k] out -- the bits and the info of the call from host
    buffers.  In a process of its own, as tests/test_gpu_predictor_multi.py runs torch."""
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests')
import torch
from plssvm_amd import backend
from plssvm_amd.parameter import Parameter
from plssvm_amd.datagen import make_blobs_pm1
rng = np.random.default_rng(5)
k = 3
X, _ = make_blobs_pm1(700 + 1000, 96, seed=3, dtype=np.float64)
sv, pts = X[:700], X[700:]
alpha = rng.standard_normal((k, 700))
for kernel in ('rbf', 'polynomial'):
    with backend.Predictor(Parameter(kernel_type=kernel, degree=2, gamma=1.0 / 96, coef0=1.0), sv, alpha, np.array([0.25, 0.5, -1.0]), every_form=True) as pred:
        for batch in (pts, pts[:77]):
            info_h, info_d = {}, {}
            want = pred.predict(batch, info_out=info_h)
            Pd = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
            Od = torch.full((batch.shape[0], k), float('nan'), dtype=Pd.dtype, device='cuda')
            torch.cuda.synchronize()
            pred.predict_device(Pd.data_ptr(), batch.shape[0], Od.data_ptr(), info_out=info_d)
            got = Od.cpu().numpy()
            assert np.array_equal(got, want), (kernel, batch.shape, float(np.max(np.abs(got - want))))
            times = ('total_ms', 'setup_ms', 'kernel_ms')
            assert {n: v for n, v in info_d.items() if n not in times} == {n: v for n, v in info_h.items() if n not in times}, (kernel, info_d, info_h)
            assert info_d['resident'] == 1 and info_d['vectors_per_launch'] == 2, info_d
            assert np.array_equal(Pd.cpu().numpy(), batch)  # the caller's tensor is read only
print('OK')
""" % (ROOT, ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------------------ 8. handle rule
def test_the_single_vector_entry_point_refuses_a_handle_of_three_vectors():
    sv, pool = data(300, 300, 64)
    alpha, rho = weights(3, 300)
    with backend.Predictor(Parameter(kernel_type="rbf", gamma=1.0 / 64), sv, alpha, rho, every_form=True) as pred:
        out = np.zeros(100 * 3)
        with pytest.raises(InvalidParameterError, match="more than one weight vector"):
            _capi.check(_capi.lib.lssvm_mi355_predictor_predict(pred._h, _capi.ptr(np.ascontiguousarray(pool[:100])), C.c_int(_capi.LSSVM_MEM_HOST), C.c_size_t(100), _capi.ptr(out), None))
        assert np.all(out == 0)
        info = {}
        assert pred.predict(pool[:100], info_out=info).shape == (100, 3)  # (the handle is as good as before)
        assert info["resident"] == 1 and info["vectors_per_launch"] == 2, info


# ------------------------------------------------------------------------------------------------------------ 9. what residency is for
@pytest.mark.parametrize("kernel", ["rbf", "polynomial"])
@pytest.mark.parametrize("npts", [100, 4096])
def test_the_resident_call_takes_less_time_than_the_one_shot_call(kernel, npts):
    """k = 4: the support vectors are not uploaded and prepared again and no record is packed per launch (the least of three calls each: the form and the reason of the
    fp32 predictor's assertion in tests/test_gpu_predictor_multi.py -- a condition, not a measured margin)."""
    sv, pool = data(3001, 9000, 100)
    alpha, rho = weights(4, 3001)
    prm = Parameter(kernel_type=kernel, degree=3, gamma=1.0 / 100, coef0=COEF0)
    pts = pool[:npts]
    with backend.Predictor(prm, sv, alpha, rho, every_form=True) as pred:
        pred.predict(pts)
        t_res, t_one = [], []
        for _ in range(3):
            a, b = {}, {}
            pred.predict(pts, info_out=a)
            backend.predict_values_multi(prm, sv, alpha, rho, None, pts, info_out=b)
            assert a["resident"] == 1
            t_res.append(a["total_ms"])
            t_one.append(b["total_ms"])
    print(f"{kernel} {npts} points, k = 4: resident {min(t_res):.3f} ms, one-shot {min(t_one):.3f} ms")
    assert min(t_res) < min(t_one), (t_res, t_one)


# ------------------------------------------------------------------------------------------------------------ 10. Python surface
def test_csvm_predict_keeps_a_binary_fp64_model_resident():
    X, y = make_blobs_pm1(600, 16, seed=41, dtype=np.float64)
    ds = DataSet(X, [int(v) for v in y], real_type=np.float64)
    svm = make_csvm("mi355", params=Parameter(kernel_type="rbf"))
    model = svm.fit(ds, epsilon=1e-6, max_iter=100)
    labels = svm.predict(model, ds)
    assert svm.last_predict_phases["resident"] == 1, svm.last_predict_phases
    assert list(labels) == list(CSVM.predict(svm, model, ds))
    assert list(svm.predict(model, ds)) == list(labels) and svm.last_predict_phases["resident"] == 1


class LoopOnlyBackend:
    """a backend object that offers only predict_values_multi: multiclass.decision_values then takes the one-shot call"""

    def __init__(self, svm):
        self._svm = svm

    def predict_values_multi(self, *args):
        return self._svm.predict_values_multi(*args)


def test_svc_decision_function_of_three_fp64_classes_has_the_bits_of_the_one_shot_call():
    X, y = make_blobs_multiclass(600 + 500, 32, 3, seed=11, dtype=np.float64)
    Xt, yt, Xh = X[:600], y[:600], X[600:]
    clf = SVC(kernel="rbf", C=1.0, gamma=1.0 / 32, tol=1e-3).fit(Xt, yt)  # (real_type: float64, the default)
    m = clf._model
    got = clf.decision_function(Xh)
    assert got.dtype == np.float64 and got.shape == (500, 3)
    assert np.array_equal(got, multiclass.decision_values(LoopOnlyBackend(clf._svm), m, Xh))
    info = {}
    m._predictor["predictor"].predict(Xh, info_out=info)
    assert info["resident"] == 1 and info["vectors_per_launch"] == 2, info
