"""GPU (-m gpu): the fixed-size LS-SVM on a resident problem (lssvm_mi355_problem_fit_reduced / _landmark_gram, lssvm_mi355_fit_reduced_*, MI355CSVM.fit_reduced,
svc.fit_reduced).  The yardstick is numpy float64 (tests/reduced_model.py); tests/test_reduced_host.py shows every input to meet the conditions
the bounds below rest on.

Operator.  landmark_gram against numpy's Pt^T Pt at N in {255, 257, 777} x rank in {1, 15, 16, 17, 64, 65} x k in {1, 3} x slab_rows in {256, 0} (several slabs with a
ragged last one; one slab) x both dtypes x the three kernel functions, and once at rank 1 024 (N = 1 100, d = 3).  The bound of entry (j, k) is derived, not tuned:

    2 N eps64 (|Pt|^T |Pt|)_jk  +  (dPt^T |Pt| + |Pt|^T dPt)_jk

  * first term: an entry is ONE sequence of at most N fused multiply-adds and additions (the MFMA chain of a row range, the partial tiles in ascending row order, the
    slabs in ascending order), so its error is at most gamma_N = N u / (1 - N u) times the sum of |summands| (Higham, Accuracy and Stability, section 3.1); 2 N eps64 = 4 N u
    covers that with the fused products' single rounding and leaves a factor of about 4.
  * second term: dPt is the element error of Phi itself (the 1 and y columns are exact).  With u64 = eps64 and u_h the eps of the type in which the problem RESCALED the
    data it holds (r roundings per coordinate; 0 where it holds the data as given):
      rbf         Phi [ gamma sum_f 2 |a_f - b_f| r u_h (|a_f| + |b_f|)  +  (d + 6) u64 (1 + gamma (|a|^2 + |b|^2)) ]   (the exponent's own error, the sum of d
                  squares, gamma / scale^2, exp to 2 ulp; numpy's |a|^2 + |b|^2 - 2 a.b form of the distance, which loses u64 of the LARGER terms, on the reference's side)
      polynomial  3 base^2 [ gamma sum_f |a_f b_f| (2 r u_h + (d + 2) u64) + u64 |base| ] + 3 u64 |k|
      linear      (d + 2) u64 sum_f |a_f b_f|
    fp64 rbf centres (and may scale) in float64: r = 2, u_h = eps64.  fp64 polynomial scales by sqrt(gamma) in float64: r = 1.  fp32 rbf off the direct form centres
    and scales in FLOAT32: there the yardstick is evaluated on reduced_model.held_data -- the data as the problem holds it, which is what the formulation asks -- and r = 0.
    Everything else holds the data as given.
The result must be symmetric to the bit.

Fit.  Decision values at 200 held-out points, formed in numpy float64 from the returned betas and rhos, against the model's: rbf_777x5 (gamma 0.2, C 100, rank 64) and
poly_777x16 (rank 64), fp64 and fp32 data, k = 1 and 3, within 8 max(e_model, cond(M) eps64) max |f| -- both terms from the model, the 8 the margin of
tests/test_gpu_pcg.py.  All-landmarks (200 x 4 rbf, C 10) and linear (m >= d) against the DENSE full LS-SVM solution under the same rule (linear: with the condition
number on the range of Phi as well -- cond(M + nu I) itself is ~ 1 / eps64 there and bounds nothing).

Bit equality (repeats; row c of a k = 3 call against the single-column call; the library's landmarks against precond_landmarks), the problem left as it was (matvec, CG,
solve_pcg before and after), the refusals that need a device, and the surface: MI355CSVM.fit_reduced with Model.save / load / predict / score, svc.fit_reduced for two and
three classes, the float32 model through predict_values.

Measured on an MI355X (for the record; the assertions are the bounds above): MEASURED below."""

import functools

import numpy as np
import pytest

import pcg_model as pm
import reduced_model as rm
from plssvm_amd import backend, svc
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.model import Model
from plssvm_amd.parameter import Parameter

pytestmark = pytest.mark.gpu

EPS64, EPS32 = rm.EPS64, rm.EPS32
KERNELS = {"rbf": dict(gamma=0.2), "polynomial": dict(gamma=1.0 / 16, coef0=1.0, degree=3), "linear": dict(gamma=1.0)}
OPERATOR_N, OPERATOR_RANKS, OPERATOR_D = (255, 257, 777), (1, 15, 16, 17, 64, 65), 5

# what one run on an MI355X gave, for the record (the assertions are the bounds of the module docstring, not these figures)
MEASURED = {
    "operator: largest error / bound over all ranks, k and slab sizes": {"float64": (0.007, 0.016), "float32": (0.007, 0.015), "rank 1024": (0.004, 0.010)},
    "fit: (|f_device - f_model|, tolerance)": {
        "rbf_777x5 float64 k=1": (5.9e-09, 6.6e-08), "rbf_777x5 float64 k=3": (2.1e-08, 2.2e-07), "rbf_777x5 float32 k=1": (1.9e-08, 7.9e-08), "rbf_777x5 float32 k=3": (2.0e-08, 1.8e-07),
        "poly_777x16 float64 k=1": (1.0e-11, 7.8e-11), "poly_777x16 float64 k=3": (1.8e-11, 8.4e-11), "poly_777x16 float32 k=1": (9.6e-12, 3.3e-11), "poly_777x16 float32 k=3": (1.1e-11, 5.5e-11)},
    "all landmarks: (|f_device - f_full|, tolerance)": {"float64": (1.3e-09, 3.0e-06), "float32": (9.5e-10, 3.0e-06)},
    "linear: (|f_device - f_full|, tolerance on the range of Phi)": {"float64": (1.5e-13, 2.5e-12), "float32": (1.8e-13, 6.4e-12)},
    "float32 model through predict_values": "0.42 eps32 of the summands' scale",
}


def parameter(kernel, kw, cost):
    return Parameter(kernel_type=kernel, cost=cost, gamma=kw.get("gamma"), coef0=kw.get("coef0", 0.0), degree=kw.get("degree", 3))


def phi_error(kernel, X, lm, kw, r, u_h):
    """dPhi of the module docstring, N x m, on the data the yardstick is evaluated on."""
    A = np.asarray(X, dtype=np.float64)
    B = A[np.asarray(lm, dtype=np.int64)]
    d = A.shape[1]
    gamma = kw["gamma"]
    if kernel == "rbf":
        Ac, Bc = A - A.mean(axis=0), B - A.mean(axis=0)  # (the held data is centred; distances do not change)
        held = gamma * 2.0 * r * u_h * (np.abs(Ac[:, None, :] - Bc[None, :, :]) * (np.abs(Ac)[:, None, :] + np.abs(Bc)[None, :, :])).sum(axis=2)
        own = (d + 6) * EPS64 * (1.0 + gamma * ((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :]))
        return pm.kernel_matrix(kernel, A, B, **kw) * (held + own)
    absdot = np.abs(A) @ np.abs(B).T
    if kernel == "polynomial":
        base = gamma * (A @ B.T) + kw["coef0"]
        return 3.0 * base * base * (gamma * absdot * (2.0 * r * u_h + (d + 2) * EPS64) + EPS64 * np.abs(base)) + 3.0 * EPS64 * np.abs(base) ** 3
    return (d + 2) * EPS64 * gamma * absdot


def operator_bound(kernel, X, Y, lm, kw, r, u_h):
    P = rm.augmented(kernel, X, Y, lm, **kw)
    dP = np.zeros_like(P)
    dP[:, :len(lm)] = phi_error(kernel, X, lm, kw, r, u_h)
    absP = np.abs(P)
    return P.T @ P, 2.0 * P.shape[0] * EPS64 * (absP.T @ absP) + dP.T @ absP + absP.T @ dP


def operator_setup(kernel, dtype, X, prob):
    """(the data the yardstick is evaluated on, its kernel parameters, r, u_h) for this problem: see the module docstring."""
    kw = rm.rounded_parameters(dtype, **KERNELS[kernel])
    if np.dtype(dtype) == np.float32:
        held, kw_held = rm.held_data(kernel, X, direct=bool(prob.info()["rbf_direct"]), **kw)
        return held, kw_held, kw, 0, 0.0
    return X, kw, kw, {"rbf": 2, "polynomial": 1, "linear": 0}[kernel], EPS64


@pytest.mark.parametrize("N", OPERATOR_N)
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_operator_against_numpy(dtype, kernel, N):
    X, y = pm.make_data(N, OPERATOR_D, pm.DATA_SEED, dtype)
    rng = np.random.default_rng(7)
    Y3 = np.stack([y, np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(dtype), np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(dtype)])
    worst = 0.0
    with backend.ResidentProblem(parameter(kernel, rm.rounded_parameters(dtype, **KERNELS[kernel]), 10.0), X) as prob:
        Xy, kw_y, _, r, u_h = operator_setup(kernel, dtype, X, prob)
        for rank in OPERATOR_RANKS:
            lm = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
            for k in (1, 3):
                ref, bound = operator_bound(kernel, Xy, Y3[:k], lm, kw_y, r, u_h)
                for slab_rows in (256, 0):
                    G = prob.landmark_gram(Y3[:k], rank, landmarks=lm, slab_rows=slab_rows)
                    assert G.shape == (rank + 1 + k, rank + 1 + k) and np.all(np.isfinite(G))
                    assert np.array_equal(G, G.T), (rank, k, slab_rows)
                    ratio = float(np.max(np.abs(G - ref) / bound))
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (np.dtype(dtype).name, kernel, N, rank, k, slab_rows, ratio)
    print(f"operator {np.dtype(dtype).name} {kernel} N={N}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("slab_rows", [256, 0])
def test_operator_at_the_largest_rank(slab_rows):
    N, rank = 1100, rm.MAX_RANK
    X, y = pm.make_data(N, 3, pm.DATA_SEED, np.float64)
    lm = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
    kw = KERNELS["rbf"]
    ref, bound = operator_bound("rbf", X, y[None, :], lm, kw, 2, EPS64)
    with backend.ResidentProblem(parameter("rbf", kw, 10.0), X) as prob:
        G = prob.landmark_gram(y, rank, landmarks=lm, slab_rows=slab_rows)
    ratio = float(np.max(np.abs(G - ref) / bound))
    print(f"operator at rank {rank}, slab_rows {slab_rows}: largest error / bound {ratio:.3f}")
    assert np.array_equal(G, G.T) and ratio <= 1.0


# ---------------------------------------------------------------- the fit ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_reference(name, dtype, k):
    """(case, model, e_model): float64 numpy, once per case, shared, never modified."""
    p = rm.fit_case(name, dtype, k)
    model = rm.ReducedModel(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], held=p["held"], **p["kw"])
    e = rm.e_model(p["kernel"], p["X"], p["Y"], p["cost"], p["landmarks"], p["points"], held=p["held"], **p["kw"])
    for a in (p["X"], p["Y"], p["points"], model.betas, model.rhos):
        a.setflags(write=False)
    return p, model, e


def fit_on_device(p, **kw):
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], p["cost"]), p["X"]) as prob:
        assert p["held"][0] is p["X"] or prob.info()["rbf_direct"] == 0  # (the yardstick's data is the data this problem holds)
        return prob.fit_reduced(p["Y"] if p["Y"].shape[0] > 1 else p["Y"][0], len(p["landmarks"]), landmarks=p["landmarks"], **kw)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", [c[0] for c in rm.FIT_CASES])
def test_fit_against_the_model(name, dtype, k):
    p, model, e = fit_reference(name, dtype, k)
    betas, rhos, used, info = fit_on_device(p)
    assert np.array_equal(used, p["landmarks"]) and info["rank"] == 64 and info["slabs"] == 1 and info["jitter"] > 0.0
    assert np.asarray(betas).dtype == np.float64 and np.asarray(betas).shape == ((3, 64) if k == 3 else (64,))
    f = model.decision_values(p["points"])
    g = model.decision_values(p["points"], betas, rhos)
    tol = rm.fit_tolerance(model, e, f)
    diff = float(np.max(np.abs(f - g)))
    print(f"fit {name} {np.dtype(dtype).name} k={k}: |f_device - f_model| {diff:.2e}, tolerance {tol:.2e} (e_model {e:.1e}, cond(M) eps64 {model.cond * EPS64:.1e}), "
          f"jitter {info['jitter']:.2e} (model {model.nu:.2e})")
    assert abs(info["jitter"] / model.nu - 1.0) <= 1e-6  # (no retry on either side)
    assert diff <= tol, (name, diff, tol)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_point_a_landmark_is_the_full_solution(dtype):
    p, model, e = fit_reference("rbf_200x4", dtype, 1)
    betas, rhos, _, info = fit_on_device(p)
    full = rm.dense_full_solution(p["kernel"], p["X"], p["Y"][0], p["cost"], p["points"], held=p["held"], **p["kw"])
    g = model.decision_values(p["points"], betas, rhos)[0]
    tol = rm.fit_tolerance(model, e, full)
    diff = float(np.max(np.abs(full - g)))
    print(f"all landmarks {np.dtype(dtype).name}: |f_device - f_full| {diff:.2e}, tolerance {tol:.2e}, jitter {info['jitter']:.2e}")
    assert info["rank"] == 200 and diff <= tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_linear_kernel_with_enough_landmarks_is_the_full_solution(dtype):
    p, model, e = fit_reference("linear_300x6", dtype, 1)
    betas, rhos, _, info = fit_on_device(p)
    full = rm.dense_full_solution(p["kernel"], p["X"], p["Y"][0], p["cost"], p["points"], **p["kw"])
    g = model.decision_values(p["points"], betas, rhos)[0]
    diff = float(np.max(np.abs(full - g)))
    print(f"linear {np.dtype(dtype).name}: |f_device - f_full| {diff:.2e}, tolerance {rm.fit_tolerance(model, e, full):.2e}, on the range of Phi {rm.range_tolerance(model, e, full):.2e}")
    assert diff <= rm.fit_tolerance(model, e, full) and diff <= rm.range_tolerance(model, e, full)


# ---------------------------------------------------------------- bit equality, the problem left as it was, refusals ----------------------------------------------------------------
@pytest.mark.parametrize("name, dtype", [("rbf_777x5", np.float32), ("poly_777x16", np.float64)])
def test_repeats_columns_and_own_landmarks_are_bit_equal(name, dtype):
    p, _, _ = fit_reference(name, dtype, 3)
    N = p["X"].shape[0]
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], p["cost"]), p["X"]) as prob:
        for slab_rows in (0, 256):
            b3, r3, used, _ = prob.fit_reduced(p["Y"], 64, slab_rows=slab_rows)  # the library's own landmarks
            again = prob.fit_reduced(p["Y"], 64, slab_rows=slab_rows)
            assert np.array_equal(b3, again[0]) and np.array_equal(r3, again[1]) and np.array_equal(used, again[2])
            for c in range(3):  # row c of the k = 3 call: the bits of the single-column call
                b1, r1, _, _ = prob.fit_reduced(p["Y"][c], 64, slab_rows=slab_rows)
                assert np.array_equal(b3[c], b1) and r3[c] == r1, (slab_rows, c)
            G3, G1 = prob.landmark_gram(p["Y"], 64, slab_rows=slab_rows), prob.landmark_gram(p["Y"][2], 64, slab_rows=slab_rows)
            assert np.array_equal(G3[:65, :65], G1[:65, :65]) and np.array_equal(G3[67, :65], G1[65, :65]) and G3[67, 67] == G1[65, 65]
            given = prob.fit_reduced(p["Y"], 64, landmarks=used, slab_rows=slab_rows)  # ... given explicitly: the same fit
            assert np.array_equal(b3, given[0]) and np.array_equal(r3, given[1])
        prob.build_preconditioner(64)
        assert np.array_equal(prob.precond_landmarks(), used) and np.array_equal(used, rm.library_landmarks(N, 64))
    one_shot = backend.fit_reduced(parameter(p["kernel"], p["kw"], p["cost"]), p["X"], p["Y"], 64, slab_rows=256)  # the one-shot entry point: the bits of the resident path
    assert np.array_equal(one_shot[0], b3) and np.array_equal(one_shot[1], r3) and np.array_equal(one_shot[2], used)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_problem_is_left_as_it_was(dtype):
    p, _, _ = fit_reference("rbf_777x5", dtype, 1)
    n = p["X"].shape[0] - 1
    y = p["Y"][0]
    eps = pm.GPU_EPS[np.dtype(dtype)]
    d = np.random.default_rng(3).standard_normal(n).astype(dtype)

    def state(prob):
        prob.cg_begin(y, eps)
        prob.cg_step(2000)
        alpha, rho, info = prob.cg_finish()
        a_pcg, rho_pcg, i_pcg = prob.solve_pcg(y, eps, 2000)
        return prob.matvec(d, np.zeros(n, dtype)), alpha, rho, info["iterations"], a_pcg, rho_pcg, i_pcg["iterations"], prob.precond_landmarks()

    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], p["cost"]), p["X"]) as prob:
        prob.build_preconditioner(landmarks=p["landmarks"][:37])
        before = state(prob)
        prob.fit_reduced(p["Y"], 64)
        prob.landmark_gram(y, 16, slab_rows=256)
        after = state(prob)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_refusals_on_a_problem():
    p, _, _ = fit_reference("rbf_777x5", np.float64, 1)
    N, y = p["X"].shape[0], p["Y"][0]
    prm = parameter(p["kernel"], p["kw"], p["cost"])
    with backend.ResidentProblem(prm, p["X"]) as prob:
        calls = (lambda: prob.fit_reduced(y, 8), lambda: prob.landmark_gram(y, 8))
        prob.set_weights(np.full(N, 2.0))
        for call in calls:
            with pytest.raises(InvalidParameterError, match="weights"):
                call()
        prob.set_weights(None)
        prob.cg_begin(y, 1e-6)
        for call in calls:
            with pytest.raises(InvalidParameterError, match="between cg_begin and cg_finish"):
                call()
        prob.cg_step(1)
        prob.cg_finish()
        with pytest.raises(InvalidParameterError, match="distinct"):
            prob.fit_reduced(y, 3, landmarks=[3, 7, 3])
        with pytest.raises(InvalidParameterError, match="index of a data point"):
            prob.fit_reduced(y, 2, landmarks=[3, N])
        with pytest.raises(InvalidParameterError, match="preconditioner"):
            prob.time_gram_kernels(1)
        betas, _, used, _ = prob.fit_reduced(y, 2, landmarks=[0, N - 1])  # (the last point is allowed, and the handle still works)
        assert np.array_equal(used, [0, N - 1]) and np.all(np.isfinite(betas))
    with backend.ResidentProblem(prm, p["X"], devices=[0, 0]) as shard:  # two shards on the one device
        for call in (lambda: shard.fit_reduced(y, 8), lambda: shard.landmark_gram(y, 8)):
            with pytest.raises(InvalidParameterError, match="one device and one rank"):
                call()
    X2, labels = rm.blobs(200, 4, 2, seed=5)
    data = DataSet(X2, labels.tolist())
    with pytest.raises(InvalidParameterError, match='no point of the class "1"'):
        MI355CSVM(kernel_type="rbf").fit_reduced(data, 4, landmarks=[0, 2, 4, 6])
    with pytest.raises(InvalidParameterError, match="one device"):
        MI355CSVM(num_devices=0, kernel_type="rbf").fit_reduced(data, 4)


# ---------------------------------------------------------------- the surface ----------------------------------------------------------------
def surface_reference(classes, dtype):
    X, labels = rm.blobs(2000, 8, classes, seed=31, dtype=dtype)
    kw = rm.rounded_parameters(dtype, gamma=1.0 / 8)
    lm = rm.library_landmarks(2000, 64)
    Y = np.where(labels[None, :] == np.arange(classes)[:, None], 1.0, -1.0)
    if classes == 2:
        Y = Y[1:]
    held = rm.held_data("rbf", X, **kw)
    model = rm.ReducedModel("rbf", X, Y, 10.0, lm, held=held, **kw)
    e = rm.e_model("rbf", X, Y, 10.0, lm, X, held=held, **kw)
    f = model.decision_values(X)
    return X, labels, lm, model, f, rm.fit_tolerance(model, e, f)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_csvm_fit_reduced_saves_loads_predicts_and_scores(dtype, tmp_path):
    X, labels, lm, model_np, f, tol = surface_reference(2, dtype)
    data = DataSet(X, labels.tolist(), real_type=dtype)
    svm = MI355CSVM(kernel_type="rbf", cost=10.0, gamma=1.0 / 8)
    model = svm.fit_reduced(data, 64)
    assert svm.last_cg_info["iterations"] == 0 and svm.last_cg_info["rank"] == 64 and np.array_equal(svm.last_cg_info["landmarks"], lm)
    assert model.num_support_vectors() == 64 and np.array_equal(model.support_vectors(), X[lm.astype(int)]) and model.alpha.dtype == np.dtype(dtype)
    path = tmp_path / "reduced.model"
    model.save(str(path))
    loaded = Model.load(str(path), real_type=dtype, label_type=int)
    assert loaded.num_support_vectors() == 64
    # the decision-value tolerance of the fit, plus -- float32 model -- the rounding of beta and of the float32 evaluation on the summands' scale
    slack = tol + (16 * EPS32 * float(np.max(rm.summand_scale("rbf", model_np.X_L, model_np.betas, model_np.rhos, X, **model_np.kw))) if dtype == np.float32 else 0.0)
    clear = np.abs(f[0]) > slack
    assert np.mean(~clear) <= 0.01
    expected = (f[0] > 0).astype(int)
    for m in (model, loaded):
        predicted = np.array(svm.predict(m, data))
        assert np.array_equal(predicted[clear], expected[clear])
    assert svm.score(model) >= 0.97 and svm.score(loaded, data) >= 0.97
    print(f"surface {np.dtype(dtype).name}: score {svm.score(model):.4f}, points within the tolerance {np.mean(~clear):.4f}")


@pytest.mark.parametrize("classes", [2, 3])
def test_svc_fit_reduced(classes):
    X, labels, lm, model_np, f, tol = surface_reference(classes, np.float64)
    est = svc.SVC(kernel="rbf", C=10.0, gamma=1.0 / 8)
    fitted = svc.fit_reduced(est, X, labels, 64)
    k = 1 if classes == 2 else classes
    assert est._fit is None and fitted.dual_coef_.shape == (k, 64) and np.array_equal(fitted.support_, lm) and np.all(np.asarray(fitted.n_iter_) == 0)
    assert np.array_equal(fitted.support_vectors_, X[lm.astype(int)]) and np.array_equal(fitted.classes_, np.arange(classes))
    assert sorted(fitted.get_params()) == sorted(est.get_params())
    predicted = fitted.predict(X)
    if classes == 2:
        clear, expected = np.abs(f[0]) > tol, (f[0] > 0).astype(int)
    else:
        top = np.sort(f, axis=0)
        clear, expected = top[-1] - top[-2] > 2 * tol, np.argmax(f, axis=0)
    assert np.mean(~clear) <= 0.01 and np.array_equal(predicted[clear], expected[clear])
    values = np.asarray(fitted.decision_function(X))
    assert np.max(np.abs((values if classes > 2 else values[:, None]) - f.T)) <= tol
    given = svc.fit_reduced(est, X, labels, None, landmarks=lm)  # the caller's list: the same model
    assert np.array_equal(given.dual_coef_, fitted.dual_coef_) and np.array_equal(given.support_, lm)


def test_float32_model_through_predict_values():
    p, model, e = fit_reference("rbf_777x5", np.float32, 1)
    betas, rhos, used, _ = fit_on_device(p)
    sv = np.ascontiguousarray(p["X"][used.astype(int)])
    values, _ = backend.predict_values(parameter(p["kernel"], p["kw"], p["cost"]), sv, np.asarray(betas).astype(np.float32), float(rhos), None, p["points"])
    f64 = model.decision_values(p["points"], betas, rhos)[0]
    scale = rm.summand_scale(p["kernel"], model.X_L, betas, rhos, p["points"], **p["kw"])[0]
    ratio = float(np.max(np.abs(np.asarray(values, dtype=np.float64) - f64) / scale)) / EPS32
    print(f"float32 model through predict_values: largest error {ratio:.2f} eps32 of the summands' scale")
    assert ratio <= 16.0
