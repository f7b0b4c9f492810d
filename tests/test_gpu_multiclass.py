"""GPU (-m gpu): several weight vectors over one set of support vectors -- predict_values_multi (two weight vectors per pass of the rectangular 256-row kernel), the k
solves of a one-vs-all model on ONE resident problem, and the multi-class SVC end to end.

What is asserted, and why:
  * predict_values_multi against the single-vector predict_values: EXACT equality.  Per weight vector the multi call performs the operations of the single call in the
    same order (tile order, fma chain, lane reduction, reduction of the partial sums, the subtraction of rho), so there is nothing to tolerate.
  * against the float64 oracle: 16 eps_fp32 on the scale of the point's summands (|K| @ |alpha_v| + |rho_v|) -- the bound and the scale of
    tests/test_gpu_parity.py::test_predict_values_on_the_bf16_matrix_cores.
  * the solves on one resident problem against fresh one-shot solves: exact equality of alpha, rho and the iteration count (the one-shot solve is create / begin /
    step / finish itself; nothing may survive cg_begin on a reused handle).
  * SVC end to end: the labels of EVERY held-out point equal the labels of the float64 oracle's one-vs-all model, and the true labels.  The test prints the smallest gap
    between the best and the second-best decision value; measured on an MI355X: rbf 1.6, linear 1.5 (0.39 for k = 5 in float32, whose five CG iterations at tol 1e-3
    leave the intercepts less settled), polynomial 0.003 to 0.007 (with coef0 = 0 and gamma = 1 / 32 its decision values are of the order 0.01 themselves) -- every one
    far beyond the rounding of either side.
"""

import functools

import numpy as np
import pytest

from plssvm_amd import _capi, backend
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.datagen import make_blobs_multiclass
from plssvm_amd.multiclass import one_vs_all_targets
from plssvm_amd.parameter import Parameter
from plssvm_amd.svc import SVC

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


def uniform_case(nsv, npts, d, k, dt, seed):
    """Support vectors, points and weights uniform in [-1, 1] (tests/test_gpu_parity.py:213-216), k weight vectors, distinct rho."""
    rng = np.random.default_rng(seed)
    sv = rng.uniform(-1, 1, size=(nsv, d)).astype(dt)
    alpha = rng.uniform(-1, 1, size=(k, nsv)).astype(dt)
    pts = rng.uniform(-1, 1, size=(npts, d)).astype(dt)
    rho = (0.125 + 0.25 * np.arange(k)).astype(dt)
    return sv, alpha, rho, pts


def param(kernel, degree, d):
    return Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=0.5)


def assert_columns_equal_single(p, sv, alpha, rho, pts, options, vectors_per_launch, ws=None):
    """Every column of the multi call against the single-vector call with that column's weight vector; returns (values, info of the multi call)."""
    info = {}
    got, w_got = backend.predict_values_multi(p, sv, alpha, rho, ws, pts, options=options, info_out=info)
    assert got.shape == (pts.shape[0], alpha.shape[0]) and got.dtype == sv.dtype
    assert info["vectors_per_launch"] == vectors_per_launch, info
    for v in range(alpha.shape[0]):
        single = {}
        want, w_want = backend.predict_values(p, sv, alpha[v], float(rho[v]), None if ws is None else ws[v], pts, options=options, info_out=single)
        differ = np.flatnonzero(got[:, v] != want)
        print(f"vector {v}: {differ.size} of {want.size} values differ" + (f", first at {differ[0]}: {got[differ[0], v]!r} != {want[differ[0]]!r}" if differ.size else ""))
        assert np.array_equal(got[:, v], want), (v, differ.size)
        assert info["gram_mode"] == single["gram_mode"] and info["rbf_direct"] == single["rbf_direct"]
        assert single["vectors_per_launch"] == 0
        if w_want is None:
            assert w_got is None
        else:
            assert np.array_equal(w_got[v], w_want)
    return got, info


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4 (a)
@pytest.mark.parametrize("gram_mode", [3, 1])
@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 3), ("polynomial", 2)])
@pytest.mark.parametrize("d", [40, 128])
def test_two_vectors_per_pass_equal_the_single_vector_kernel(d, kernel, degree, k, gram_mode):
    """The rectangular 256-row kernel with two weight vectors per pass (66 row blocks of points; one and two 64-feature chunks; f16x3 and bf16x6 planes): every
    column is bit-identical to the single-vector call, an odd last vector included."""
    sv, alpha, rho, pts = uniform_case(3000, 8448, d, k, np.float32, seed=3000 + d + k)
    with_mode = _capi.Options(gram_mode=gram_mode)
    assert_columns_equal_single(param(kernel, degree, d), sv, alpha, rho, pts, with_mode, vectors_per_launch=2)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4 (b)
@pytest.mark.parametrize("kernel, case", [(kernel, case) for kernel in ("rbf", "polynomial") for case in ("few_points", "wide", "gram_mode_1", "gram_mode_0", "fp64")]
                         + [("rbf", "rbf_form_1")])
def test_per_vector_paths_equal_the_single_vector_call(kernel, case):
    """Where the two-vector kernel does not apply, every weight vector has a launch of its own on the shared preparation: the same bits as the single-vector call."""
    npts, d, dt, opts = 700, 128, np.float32, {}
    if case == "wide":
        d = 384
    elif case == "gram_mode_1":
        opts = {"gram_mode": 1}
    elif case == "gram_mode_0":
        opts = {"gram_mode": 0}
    elif case == "rbf_form_1":
        npts, opts = 8448, {"rbf_form": 1}  # (enough points for the 256-row kernel, which the direct rbf form excludes)
    elif case == "fp64":
        dt = np.float64
    sv, alpha, rho, pts = uniform_case(1300, npts, d, 3, dt, seed=1300 + d)
    assert_columns_equal_single(param(kernel, 3, d), sv, alpha, rho, pts, _capi.Options(**opts), vectors_per_launch=1)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 4 (c)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_linear_kernel_equals_the_single_vector_call(dt):
    """The linear kernel: w per weight vector, then w.x per vector on the one uploaded point matrix -- without and with a cached w."""
    sv, alpha, rho, pts = uniform_case(1300, 2000, 100, 3, dt, seed=77)
    p = Parameter(kernel_type="linear")
    _, _ = assert_columns_equal_single(p, sv, alpha, rho, pts, None, vectors_per_launch=1)
    ws = np.stack([backend.calculate_w(sv, a) for a in alpha])
    got, w = backend.predict_values_multi(p, sv, alpha, rho, None, pts)
    assert np.array_equal(w, ws)
    assert_columns_equal_single(p, sv, alpha, rho, pts, None, vectors_per_launch=1, ws=ws)
    # a cached w is USED (not recomputed): a different w gives its own values
    got2, w2 = backend.predict_values_multi(p, sv, alpha, rho, 2 * ws, pts)
    assert np.array_equal(w2, 2 * ws) and not np.array_equal(got2, got)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("kernel", ["rbf", "polynomial"])
@pytest.mark.parametrize("d", [40, 128])
def test_two_vectors_per_pass_against_the_float64_oracle(oracle, kernel, d):
    """Every column within 16 eps_fp32 of the float64 oracle on the scale of the point's summands."""
    k = 3
    sv, alpha, rho, pts = uniform_case(3000, 8448, d, k, np.float32, seed=3000 + d + k)
    info = {}
    got, _ = backend.predict_values_multi(param(kernel, 3, d), sv, alpha, rho, None, pts, info_out=info)
    assert info["vectors_per_launch"] == 2
    sv64, pts64 = sv.astype(np.float64), pts.astype(np.float64)
    G = pts64 @ sv64.T
    if kernel == "rbf":
        sq_s, sq_p = np.einsum("ij,ij->i", sv64, sv64), np.einsum("ij,ij->i", pts64, pts64)
        K = np.exp(-(1.0 / d) * np.maximum(sq_p[:, None] + sq_s[None, :] - 2.0 * G, 0.0))
    else:
        K = (G / d + 0.5) ** 3
    for v in range(k):
        want, _ = oracle.predict_values(kernel, sv64, alpha[v].astype(np.float64), float(rho[v]), pts64, degree=3, gamma=1.0 / d, coef0=0.5)
        scale = np.abs(K) @ np.abs(alpha[v].astype(np.float64)) + abs(float(rho[v]))
        err = float(np.max(np.abs(got[:, v] - want) / scale))
        print(f"{kernel} d={d} vector {v}: max error {err / EPS32:.2f} eps_fp32 of the summands' scale")
        assert err < 16 * EPS32, (v, err / EPS32)


# ---------------------------------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kernel", ["rbf", "polynomial", "linear"])
def test_solves_on_one_resident_problem_equal_fresh_one_shot_solves(kernel, dt, weighted):
    """k right-hand sides one after the other on ONE resident problem: per class the alpha, rho and iteration count of a fresh one-shot solve."""
    X, y = make_blobs_multiclass(3000, 32, 5, seed=7, dtype=dt)
    B = one_vs_all_targets(np.arange(5), y, dt)
    p = Parameter(kernel_type=kernel, degree=3, gamma=1.0 / 32, coef0=0.0, cost=1.0)
    w = np.random.default_rng(5).uniform(0.25, 4.0, size=3000) if weighted else None
    eps = 1e-3 if dt == np.float32 else 1e-8
    svm = MI355CSVM(params=p)
    alphas, rhos, infos = svm.solve_systems_of_linear_equations(p, X, B, eps, 3000, sample_weight=w)
    assert alphas.shape == (5, 3000) and alphas.dtype == dt and rhos.shape == (5,) and len(infos) == 5
    for c in range(5):
        a, rho, info = backend.solve_system_of_linear_equations(p, X, B[c], eps, 3000, sample_weight=w)
        print(f"class {c}: {infos[c]['iterations']} iterations (one-shot {info['iterations']}), {np.count_nonzero(alphas[c] != a)} alpha differ, rho {rhos[c]!r} / {rho!r}")
        assert infos[c]["iterations"] == info["iterations"] and infos[c]["iterations"] >= 1
        assert np.array_equal(alphas[c], a) and rhos[c] == rho


# ---------------------------------------------------------------------------------------------------------------------------------------------- 7
HELD_OUT = 8448


@functools.lru_cache(maxsize=None)
def oracle_labels(kernel, k, seed):
    """The labels of the float64 oracle's one-vs-all model on the held-out points: per class oracle.solve, oracle.predict_values, then argmax."""
    import oracle_lib
    orc = oracle_lib.oracle()
    X, y = make_blobs_multiclass(3000 + HELD_OUT, 32, k, seed=seed, dtype=np.float64)
    Xt, yt, Xh = X[:3000], y[:3000], X[3000:]
    kw = dict(degree=3, gamma=1.0 / 32, coef0=0.0)
    values = np.empty((HELD_OUT, k))
    for c in range(k):
        a, rho, _ = orc.solve(kernel, Xt, np.where(yt == c, 1.0, -1.0), 1e-3, 3000, cost=1.0, **kw)
        values[:, c], _ = orc.predict_values(kernel, Xt, np.asarray(a, dtype=np.float64), float(rho), Xh, **kw)
    return np.argmax(values, axis=1)


@pytest.mark.parametrize("real_type", [np.float32, np.float64])
@pytest.mark.parametrize("kernel", ["linear", "poly", "rbf"])
@pytest.mark.parametrize("k, seed", [(3, 11), (5, 7)])
def test_svc_one_vs_all_end_to_end(k, seed, kernel, real_type):
    """SVC on k blobs: every held-out point gets the oracle's label, which is the true one."""
    X, y = make_blobs_multiclass(3000 + HELD_OUT, 32, k, seed=seed, dtype=np.float64)
    Xt, yt, Xh, yh = X[:3000], y[:3000], X[3000:], y[3000:]
    clf = SVC(kernel=kernel, C=1.0, gamma=1.0 / 32, tol=1e-3, real_type=real_type).fit(Xt, yt)
    assert np.array_equal(clf.classes_, np.arange(k))
    assert clf.dual_coef_.shape == (k, 3000) and clf.dual_coef_.dtype == real_type and clf.intercept_.shape == (k,)
    assert clf.n_iter_.shape == (k,) and np.issubdtype(clf.n_iter_.dtype, np.integer) and np.all(clf.n_iter_ > 0)
    assert clf.n_support_.shape == (k,) and clf.n_support_.sum() == 3000 and clf.class_weight_.shape == (k,)
    values = clf.decision_function(Xh)
    assert values.shape == (HELD_OUT, k)
    predicted = clf.predict(Xh)
    assert np.array_equal(predicted, clf.classes_[np.argmax(values, axis=1)])
    want = oracle_labels("polynomial" if kernel == "poly" else kernel, k, seed)
    top2 = np.sort(values, axis=1)[:, -2:]
    print(f"{kernel} k={k} {np.dtype(real_type).name}: {np.count_nonzero(predicted != want)} labels differ from the oracle's, smallest gap {float(np.min(top2[:, 1] - top2[:, 0])):.3f}, "
          f"accuracy {float(np.mean(predicted == yh)):.4f}, iterations {clf.n_iter_.tolist()}")
    assert np.array_equal(predicted, want)
    assert clf.score(Xh, yh) == 1.0
    if kernel == "linear":
        assert clf.coef_.shape == (k, 32)
        assert np.allclose(Xh.astype(real_type) @ clf.coef_.T + clf.intercept_, values, rtol=0, atol=1e-3)
    else:
        with pytest.raises(AttributeError):
            clf.coef_
