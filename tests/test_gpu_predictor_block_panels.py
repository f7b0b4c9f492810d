"""GPU (-m gpu): the block panel form of the resident fp32 predictor -- lssvm_mi355_predictor_create_block_panels, ``backend.Predictor(..., block_panels=True)`` -- and
the sixteen-vector full-square panel kernel behind it (tile_matvec_f32_blk_wide, plssvm_amd/csrc/lssvm_tile_f32_blk_wide.hip.hpp).

Values: against numpy in ``np.longdouble`` on the float32 data, in units of u_iv = eps32 * sum_j |alpha_jv k_ij| (the summand scale), as tests/test_gpu_predictor_block32.py.
e_old is the largest error of the single-vector lssvm_mi355_predict_values_f32 on the same case, e_new that of the block panel handle; asserted: e_new <= e_old + (L + 3),
L = padded columns + column chunks (each fp32 MFMA of four columns counted as four additions, then the chunks' slabs in order; chunks of j_chunk_tiles column tiles,
automatically 2 at these sizes).  Both paths evaluate a kernel value by the panel kernel's chain of operations, so e_new - e_old is the summation's share; a wrong index, a
dropped panel or a stale record is an error of 1 / eps32 units.
Bits: a repeated call, a vector alone against the same vector in a block of 17, and every declined case against the handle it is said to be."""

import numpy as np
import pytest

from plssvm_amd import backend
from plssvm_amd._capi import Options
from plssvm_amd.datagen import make_blobs_multiclass, make_blobs_pm1
from plssvm_amd.parameter import KernelFunctionType, Parameter
from plssvm_amd.svc import SVC

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS32 = float(np.finfo(np.float32).eps)
FORMS = {"rbf": ("rbf", 3, 0.0), "poly5": ("polynomial", 5, 0.5), "poly2": ("polynomial", 2, 0.5), "poly3": ("polynomial", 3, -0.25)}
NOT_TIMES = ("rbf_exponent_scale", "f16_row_rel_error", "gram_mode", "rbf_direct", "resident", "vectors_per_launch")
F4 = ("rbf", "poly5", "poly2", "poly3")

# (form, support vectors, points, features, vectors, j_chunk_tiles or 0, gram_mode or 0 = the default planes)
CASES = ([(F4[i % 4], 200, 130, d, 15, 0, i % 2) for i, d in enumerate((129, 192, 256, 257, 384, 385, 513, 784))]              # one feature past a panel, 2 ... 7 panels
         + [(F4[(i + 1) % 4], 200, 130, d, 15, 0, (i + 1) % 2) for i, d in enumerate((129, 257, 385, 784))]                   # ... on the other plane kind
         + [(f, nsv, 129, 200, 16, 0, gm) for f, nsv, gm in zip(("rbf", "poly5", "poly2", "poly3", "rbf"), (1, 63, 64, 65, 129), (0, 1, 0, 1, 1))]  # sub-tile and tile edges
         + [(f, 300, 129, 200, 17, 1, gm) for f in FORMS for gm in (0, 1)]                                                     # three column chunks, every form
         + [(f, 150, npts, 257, 2, 0, gm) for f, npts, gm in zip(("poly3", "rbf", "poly5", "poly2"), (1, 127, 129, 300), (0, 1, 0, 1))]  # row-block edges
         + [("rbf", 300, 300, 200, k, 0, gm) for k, gm in zip((1, 2, 15, 16, 17, 33), (0, 1, 0, 1, 0, 1))])                    # one group, a padded one, three groups


def model(form, nsv, npts, d, k):
    kernel, degree, coef0 = FORMS[form]
    X, _ = make_blobs_pm1(nsv + npts, d, seed=23, dtype=np.float32)
    alpha = np.random.default_rng(17 + k).standard_normal((k, nsv)).astype(np.float32)
    return Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=coef0), X[:nsv], X[nsv:], alpha, 0.125 + 0.25 * np.arange(k)


def reference(prm, sv, pts, alpha, rho):
    """(values, units u_iv) in longdouble"""
    P, S, A = pts.astype(LD), sv.astype(LD), alpha.astype(LD)
    G = P @ S.T
    if prm.kernel_type == KernelFunctionType.RBF:
        K = np.exp(-LD(prm.gamma) * ((P * P).sum(axis=1)[:, None] + (S * S).sum(axis=1)[None, :] - 2 * G))
    else:
        K = (LD(prm.gamma) * G + LD(prm.coef0)) ** int(prm.degree)
    return K @ A.T - rho.astype(LD)[None, :], EPS32 * (np.abs(K) @ np.abs(A).T)


@pytest.mark.parametrize("form, nsv, npts, d, k, jct, gm", CASES, ids=lambda c: str(c))
def test_values_against_longdouble(form, nsv, npts, d, k, jct, gm):
    prm, sv, pts, alpha, rho = model(form, nsv, npts, d, k)
    opts = Options(**({"j_chunk_tiles": jct} if jct else {}), **({"gram_mode": gm} if gm else {}))
    want, unit = reference(prm, sv, pts, alpha, rho)
    col_tiles = -(-nsv // 128)
    L = col_tiles * 128 + -(-col_tiles // (jct or 2))
    with backend.Predictor(prm, sv, alpha, rho, options=opts, block_panels=True) as pred:
        info = {}
        got = pred.predict(pts, info_out=info)
        assert np.array_equal(pred.predict(pts), got)  # a repeat has the same bits
    old = np.stack([backend.predict_values(prm, sv, alpha[v], float(rho[v]), None, pts, options=opts)[0] for v in range(k)], axis=1)
    e_new, e_old = float(np.max(np.abs(got - want) / unit)), float(np.max(np.abs(old - want) / unit))
    print(f"{form} nsv={nsv} points={npts} d={d} k={k} j_chunk_tiles={jct} gram_mode={info['gram_mode']}: e_new {e_new:.2f}, e_old {e_old:.2f} units, excess {e_new - e_old:.2f}, L = {L}")
    assert got.shape == (npts, k) and np.all(np.isfinite(got))
    assert info["resident"] == 1 and info["vectors_per_launch"] == 16, info
    assert e_new <= e_old + (L + 3), (e_new, e_old, L)


def test_a_column_has_the_bits_of_its_vector_alone():
    prm, sv, pts, alpha, rho = model("rbf", 300, 300, 200, 17)
    with backend.Predictor(prm, sv, alpha, rho, block_panels=True) as pred:
        got = pred.predict(pts)
    for v in (0, 5, 15, 16):  # slots 0, 5, 15 of the first group, slot 0 of the second
        with backend.Predictor(prm, sv, alpha[v:v + 1], rho[v:v + 1], block_panels=True) as alone:
            assert np.array_equal(alone.predict(pts)[:, 0], got[:, v]), v


@pytest.mark.parametrize("case", ["fp64", "100_features", "linear", "gram_mode_0", "tile_kernel_1", "rbf_form_1", "rbf_fold_0", "negative_degree"])
def test_a_declined_case_is_the_handle_it_is_said_to_be(case):
    dt = np.float64 if case == "fp64" else np.float32
    d = 100 if case == "100_features" else 200
    X, _ = make_blobs_pm1(600, d, seed=23, dtype=dt)
    alpha = np.random.default_rng(3).standard_normal((3, 300)).astype(dt)
    rho = np.array([0.25, 0.5, -1.0])
    prm = {"linear": Parameter(kernel_type="linear"), "negative_degree": Parameter(kernel_type="polynomial", degree=-2, gamma=1.0 / d, coef0=8.0)}.get(case, Parameter(kernel_type="rbf", gamma=1.0 / d))
    opts = {"gram_mode_0": {"gram_mode": 0}, "tile_kernel_1": {"tile_kernel": 1}, "rbf_form_1": {"rbf_form": 1}, "rbf_fold_0": {"rbf_fold": 0}}.get(case, {})
    said = {"fp64": {"block": True}, "100_features": {"block32": True}}.get(case, {"panels": True})
    with backend.Predictor(prm, X[:300], alpha, rho, options=Options(**opts), block_panels=True) as blk, backend.Predictor(prm, X[:300], alpha, rho, options=Options(**opts), **said) as res:
        a, b = {}, {}
        assert np.array_equal(blk.predict(X[300:], info_out=a), res.predict(X[300:], info_out=b))
        assert {n: a[n] for n in NOT_TIMES} == {n: b[n] for n in NOT_TIMES} and (a["vectors_per_launch"] == 16) == (case in ("fp64", "100_features")), (a, b)


def test_decision_values_resident_reaches_the_block_panel_form():
    X, y = make_blobs_multiclass(600 + 200, 200, 3, seed=11, dtype=np.float32)
    clf = SVC(kernel="rbf", C=1.0, gamma=1.0 / 200, tol=1e-3, real_type=np.float32).fit(X[:600], y[:600])
    svm, m = clf._svm, clf._model
    plain = svm.decision_values_resident(m, X[600:])
    got = svm.decision_values_resident(m, X[600:], block_panels=True)
    info = {}
    m._predictor["predictor"].predict(X[600:], info_out=info)
    assert got.dtype == np.float32 and info["resident"] == 1 and info["vectors_per_launch"] == 16, info
    # both are sums of the same 640 padded columns' terms, |k| <= 1: chains of at most 640 and of 643 additions, each within its length in eps of sum_j |alpha_j|
    assert np.all(np.abs(got - plain) <= 1283 * EPS32 * np.abs(m.alpha).sum(axis=1)[None, :])
