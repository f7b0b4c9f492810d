"""GPU (-m gpu): the fixed-size kernel logistic regression (lssvm_mi355_problem_fit_reduced_logistic / _reduced_logistic_step and the one-shot forms,
MI355CSVM.fit_reduced_logistic, svc.fit_reduced_logistic / ProbabilisticSVC) against the numpy model tests/reduced_logistic_model.py.

The step operator, in two stages with derived bounds (u = eps64; Phi, dPhi, r, u_h as in tests/test_gpu_reduced.py):
  * eta against numpy: 2 (m + 4) u (sum_j |phi_ij beta_j| + |b|) + sum_j dPhi_ij |beta_j| -- the m products and the sums of the kernel's fixed tree, and what the
    evaluation of Phi itself costs;
  * q and z - eta against the numpy formulas evaluated AT THE DEVICE'S OWN eta: 16 u relative -- each side has at most four roundings and one <= 1-ulp exp / log1p, 16 is
    twice the sum.  z is stored as the double eta + (z - eta): the rounding of that one sum on either side, 2 u |z|, is added to the bound on z - eta (where the floor
    holds and the label agrees, z - eta is far below an ulp of eta: no stored z can carry it to 16 u of itself);
  * the loss sums against sum_i a_i l_i of the numpy formulas at the device's own eta: (N + 16) u of it.  (The entry point returns the sums, not the rows' losses.)
Bits: eta, q and z of a class change with neither slab_rows nor the number of classes of the call; rows of weight 0 have q == 0.0.

The fit: decision values on the training points and on 200 held-out points within 8 max(e_model, cond(M_last) eps64) max |eta| of the model (the linear case: cond on
the range of Phi), converged, the reported objective against its recomputation from the returned coefficients within (N + 16) u J; the warm start from -1 x the optimum
halves and arrives at the same values.  Bit equalities: repeats (both factors), column c of a k = 3 call, sample_weight of ones against None, one-shot against resident,
and max_iter = 1 from zeros = exactly 2 x fit_reduced at cost C / 4.
"""

import functools

import numpy as np
import pytest

import pcg_model as pm
import reduced_logistic_model as lg
import reduced_model as rm
import reduced_weighted_model as wm
import test_gpu_reduced as base
from plssvm_amd import backend, svc
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.model import Model

pytestmark = pytest.mark.gpu

EPS64 = rm.EPS64
STEP_N, STEP_RANKS, STEP_D = (255, 777), (1, 16, 64, 65, 129, 300), 5
CLASSES_PER_LAUNCH = 4                                  # lssvm_logistic.hip: LG_CLASSES
STEP_K = (1, 3, CLASSES_PER_LAUNCH, CLASSES_PER_LAUNCH + 1)  # 3 is also the value below it
FIT_TOL = 1e-10


def step_inputs(N, rank, k, dtype, seed=11):
    rng = np.random.default_rng(seed + rank)
    betas = rng.standard_normal((k, rank)) / np.sqrt(rank)
    rhos = rng.standard_normal(k)
    Y = np.where(rng.random((k, N)) < 0.5, -1.0, 1.0).astype(dtype)
    return betas, rhos, Y, wm.make_weights(N)


def check_step(prob, kernel, Xy, kw_y, r, u_h, lm, betas, rhos, Y, w, slab_rows, label):
    """One call of the step operator under the bounds of the module docstring; returns (eta, q, z, floored, the largest error / bound of the three stages)."""
    N, m = Xy.shape[0], len(lm)
    Phi = pm.kernel_matrix(kernel, Xy, np.asarray(Xy)[np.asarray(lm, dtype=np.int64)], **kw_y)
    dPhi = base.phi_error(kernel, Xy, lm, kw_y, r, u_h)
    eta, q, z, loss, floored = prob.reduced_logistic_step(Y, betas, rhos, landmarks=lm, sample_weight=w, slab_rows=slab_rows)
    assert eta.shape == q.shape == z.shape == Y.shape and np.all(np.isfinite(eta)) and np.all(np.isfinite(q)) and np.all(np.isfinite(z))
    ref = betas @ Phi.T - rhos[:, None]
    bound = 2.0 * (m + 4) * EPS64 * (np.abs(betas) @ np.abs(Phi).T + np.abs(rhos)[:, None]) + np.abs(betas) @ dPhi.T
    r_eta = float(np.max(np.abs(eta - ref) / bound))
    q_ref, z_ref, l_ref, mu_ref, _ = lg.row_quantities(Y, w[None, :], eta)
    r_q = float(np.max(np.abs(q - q_ref) / np.where(q_ref > 0, 16 * EPS64 * q_ref, 1.0)))
    t_ref = z_ref - eta
    r_z = float(np.max(np.abs((z - eta) - t_ref) / (16 * EPS64 * np.abs(t_ref) + 2 * EPS64 * np.abs(z_ref))))
    sums = (w[None, :] * l_ref).sum(axis=1)
    r_l = float(np.max(np.abs(loss - sums) / ((N + 16) * EPS64 * sums)))
    assert np.all(q[:, w == 0.0] == 0.0)
    assert np.array_equal(floored, (mu_ref < lg.DELTA).sum(axis=1)), (label, floored)
    assert r_eta <= 1.0 and r_q <= 1.0 and r_z <= 1.0 and r_l <= 1.0, (label, r_eta, r_q, r_z, r_l)
    return eta, q, z, floored, max(r_eta, r_q, r_z, r_l)


@pytest.mark.parametrize("N", STEP_N)
@pytest.mark.parametrize("kernel", list(base.KERNELS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_step_operator_against_numpy(dtype, kernel, N):
    X, _ = pm.make_data(N, STEP_D, pm.DATA_SEED, dtype)
    worst, most_floored = 0.0, 0
    kmax = max(STEP_K)
    with backend.ResidentProblem(base.parameter(kernel, rm.rounded_parameters(dtype, **base.KERNELS[kernel]), 10.0), X) as prob:
        Xy, kw_y, _, r, u_h = base.operator_setup(kernel, dtype, X, prob)
        for rank in STEP_RANKS:
            if rank > N:
                continue
            lm = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
            betas, rhos, Y, w = step_inputs(N, rank, kmax, dtype)
            for scale in (1.0, 40.0):  # (40: rows at the floor of the curvature)
                eta, q, z, floored, ratio = check_step(prob, kernel, Xy, kw_y, r, u_h, lm, scale * betas, scale * rhos, Y, w, 0, (rank, scale))
                worst, most_floored = max(worst, ratio), max(most_floored, int(floored.max()))
                for slab_rows in (256, 0):
                    for k in STEP_K:
                        if k == kmax and slab_rows == 0:
                            continue
                        if scale != 1.0 and (k != kmax):
                            continue
                        e2, q2, z2, _, fl2 = prob.reduced_logistic_step(Y[:k], scale * betas[:k], scale * rhos[:k], landmarks=lm, sample_weight=w, slab_rows=slab_rows)
                        assert np.array_equal(e2, eta[:k]) and np.array_equal(q2, q[:k]) and np.array_equal(z2, z[:k]) and np.array_equal(fl2, floored[:k]), (rank, scale, k, slab_rows)
    print(f"step {np.dtype(dtype).name} {kernel} N={N}: largest error / bound {worst:.3f}, most rows at the floor {most_floored}")
    assert most_floored > 0


def test_step_operator_at_the_largest_rank():
    N, rank = 1100, rm.MAX_RANK
    X, _ = pm.make_data(N, 3, pm.DATA_SEED, np.float64)
    lm = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
    kw = base.KERNELS["rbf"]
    betas, rhos, Y, w = step_inputs(N, rank, 2, np.float64)
    with backend.ResidentProblem(base.parameter("rbf", kw, 10.0), X) as prob:
        first = check_step(prob, "rbf", X, kw, 2, EPS64, lm, betas, rhos, Y, w, 0, "rank 1024")
        again = prob.reduced_logistic_step(Y, betas, rhos, landmarks=lm, sample_weight=w, slab_rows=256)
    assert all(np.array_equal(a, b) for a, b in zip(first[:3], again[:3]))
    print(f"step at rank {rank}: largest error / bound {first[4]:.3f}")


# ---------------------------------------------------------------- the fit ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_reference(name, dtype, cost):
    """(case, model at FIT_TOL, e_model, tolerance on the decision values at [X; points]): float64 numpy, once per case, shared, never modified."""
    p = lg.case(name, dtype)
    model = lg.LogisticModel(p["kernel"], p["X"], p["y"], cost, p["landmarks"], held=p["held"], tol=FIT_TOL, **p["kw"])
    points = np.vstack([p["X"], p["points"]])
    e = lg.e_model(p, cost, points)
    f = model.decision_values(points)
    for a in (p["X"], p["y"], p["points"], model.beta, f):
        a.setflags(write=False)
    return p, model, points, f, lg.fit_tolerance(model, e, f, linear=name.startswith("linear"))


def problem_of(p, cost):
    return backend.ResidentProblem(base.parameter(p["kernel"], p["kw"], cost), p["X"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", lg.CASE_NAMES)
def test_fit_against_the_model(name, dtype):
    for cost in lg.COSTS:
        p, model, points, f, tol = fit_reference(name, dtype, cost)
        N, rank = p["y"].size, len(p["landmarks"])
        with problem_of(p, cost) as prob:
            assert p["held"][0] is p["X"] or prob.info()["rbf_direct"] == 0  # (the yardstick's data is the data this problem holds)
            for factor in ("host", "device"):
                beta, rho, used, info = prob.fit_reduced_logistic(p["y"], rank, landmarks=p["landmarks"], tol=FIT_TOL, factor=factor)
                g = model.decision_values(points, beta, rho)
                diff = float(np.max(np.abs(f - g)))
                J = lg.objective(model.Phi, model.K_mm, model.y, np.ones(N), cost, beta, -rho)
                print(f"fit {name} {np.dtype(dtype).name} C={cost} {factor}: passes {info['passes']} (model {model.result['passes']}), halvings {info['halvings']}, |eta_device - eta_model| "
                      f"{diff:.2e}, tolerance {tol:.2e}, objective {info['objective']:.12g} against {J:.12g} ({abs(info['objective'] - J) / ((N + 16) * EPS64 * J):.2f} of its bound), "
                      f"max |eta| {info['max_abs_eta']:.3g}, floored {info['floored']}")
                assert np.array_equal(used, p["landmarks"]) and np.asarray(beta).shape == (rank,) and info["converged"] == 1 and info["halvings"] == 0
                assert diff <= tol, (name, cost, factor, diff, tol)
                assert abs(info["objective"] - J) <= (N + 16) * EPS64 * J
                assert info["jitter"] > 0.0 and info["step_ms"] > 0.0 and info["gram_ms"] > 0.0 and info["landmark_ms"] > 0.0
            if name == "rbf_600x4" and cost == 100.0:  # the safeguard: from -1 x the optimum
                beta, rho, _, info = prob.fit_reduced_logistic(p["y"], rank, landmarks=p["landmarks"], tol=FIT_TOL, start=(-model.beta, -model.rho))
                diff = float(np.max(np.abs(f - model.decision_values(points, beta, rho))))
                print(f"warm start from -1 x the optimum: halvings {info['halvings']}, passes {info['passes']}, |eta_device - eta_model| {diff:.2e}, tolerance {tol:.2e}")
                assert info["halvings"] > 0 and info["converged"] == 1 and diff <= tol


@pytest.mark.parametrize("name, dtype", [("rbf_777x5", np.float32), ("poly_600x8", np.float64)])
def test_bit_equalities(name, dtype):
    cost = 100.0
    p, _, _, _, _ = fit_reference(name, dtype, cost)
    N, rank, lm = p["y"].size, len(p["landmarks"]), p["landmarks"]
    rng = np.random.default_rng(23)
    Y3 = np.stack([p["y"]] + [np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(dtype) for _ in range(2)])
    same = lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])  # noqa: E731
    with problem_of(p, cost) as prob:
        for factor in ("host", "device"):  # repeats
            one = prob.fit_reduced_logistic(p["y"], rank, landmarks=lm, factor=factor)
            assert same(one, prob.fit_reduced_logistic(p["y"], rank, landmarks=lm, factor=factor)), factor
        b3, r3, _, infos = prob.fit_reduced_logistic(Y3, rank, landmarks=lm)
        print(f"k = 3 in lockstep: passes {[info['passes'] for info in infos]}")  # (where they differ, a finished class sat out the later passes)
        assert len(infos) == 3
        for c in range(3):  # column c of the k = 3 call: the bits of the single call
            b1, r1, _, i1 = prob.fit_reduced_logistic(Y3[c], rank, landmarks=lm)
            assert np.array_equal(b3[c], b1) and r3[c] == r1 and infos[c]["passes"] == i1["passes"] and infos[c]["objective"] == i1["objective"], c
        host = prob.fit_reduced_logistic(p["y"], rank, landmarks=lm)
        assert same(host, prob.fit_reduced_logistic(p["y"], rank, landmarks=lm, sample_weight=np.ones(N)))
        first = prob.fit_reduced_logistic(p["y"], rank, landmarks=lm, max_iter=1)
        assert first[3]["passes"] == 1 and first[3]["converged"] == 0  # ... with the objective of the iterate before it: J(0, 0) = C N log 2
        assert abs(first[3]["objective"] - cost * N * np.log(2.0)) <= (N + 16) * EPS64 * first[3]["objective"]
    one_shot = backend.fit_reduced_logistic(base.parameter(p["kernel"], p["kw"], cost), p["X"], p["y"], rank, landmarks=lm)
    assert same(one_shot, host) and one_shot[3]["passes"] == host[3]["passes"]
    with problem_of(p, cost / 4.0) as quarter:  # one pass from zeros: v = 1/4 and z = 2 y exactly, so 2 x the least-squares fit at a quarter of the cost, to the bit
        ls = quarter.fit_reduced(p["y"], rank, landmarks=lm)
    assert np.array_equal(first[0], 2.0 * ls[0]) and first[1] == 2.0 * ls[1]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_problem_is_left_as_it_was(dtype):
    p, _, _, _, _ = fit_reference("rbf_777x5", dtype, 100.0)
    n = p["X"].shape[0] - 1
    eps = pm.GPU_EPS[np.dtype(dtype)]
    d = np.random.default_rng(3).standard_normal(n).astype(dtype)

    def state(prob):
        prob.cg_begin(p["y"], eps)
        prob.cg_step(2000)
        alpha, rho, info = prob.cg_finish()
        return prob.matvec(d, np.zeros(n, dtype)), alpha, rho, info["iterations"], prob.precond_landmarks()

    with problem_of(p, 100.0) as prob:
        prob.build_preconditioner(landmarks=p["landmarks"][:37])
        before = state(prob)
        prob.fit_reduced_logistic(p["y"], 64)
        prob.fit_reduced_logistic(p["y"], 16, slab_rows=256, factor="device", max_iter=3)
        after = state(prob)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_refusals_on_a_problem():
    p, _, _, _, _ = fit_reference("rbf_777x5", np.float64, 100.0)
    N, y = p["X"].shape[0], p["y"]
    with problem_of(p, 100.0) as prob:
        calls = (lambda: prob.fit_reduced_logistic(y, 8), lambda: prob.reduced_logistic_step(y, np.zeros(8), 0.0))
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
            prob.fit_reduced_logistic(y, 3, landmarks=[3, 7, 3])
        with pytest.raises(InvalidParameterError, match="exactly -1 or"):
            prob.fit_reduced_logistic(np.r_[y[:-1], 0.0], 8)
        beta, _, used, info = prob.fit_reduced_logistic(y, 2, landmarks=[0, N - 1])  # (the handle still works)
        assert np.array_equal(used, [0, N - 1]) and np.all(np.isfinite(beta)) and info["converged"] == 1
    with backend.ResidentProblem(base.parameter(p["kernel"], p["kw"], 100.0), p["X"], devices=[0, 0]) as shard:  # two shards on the one device
        with pytest.raises(InvalidParameterError, match="one device and one rank"):
            shard.fit_reduced_logistic(y, 8)
    X2, labels = rm.blobs(200, 4, 2, seed=5)
    with pytest.raises(InvalidParameterError, match="one device"):
        MI355CSVM(num_devices=0, kernel_type="rbf").fit_reduced_logistic(DataSet(X2, labels.tolist()), 4)


# ---------------------------------------------------------------- the surface ----------------------------------------------------------------
def test_two_classes_on_the_surface(tmp_path):
    X, labels = rm.blobs(600, 4, 2, 7, 1.0)
    est = svc.SVC(kernel="rbf", C=10.0, gamma=0.5)
    fitted = svc.fit_reduced_logistic(est, X, labels, 32)
    assert isinstance(fitted, svc.ProbabilisticSVC) and est._fit is None and fitted.dual_coef_.shape == (1, 32) and 1 < fitted.n_iter_ <= 50
    proba, values = fitted.predict_proba(X), np.asarray(fitted.decision_function(X), dtype=np.float64)
    assert proba.shape == (600, 2) and np.all(proba >= 0.0) and np.max(np.abs(proba.sum(axis=1) - 1.0)) <= 4 * EPS64
    assert np.array_equal(fitted.predict(X), fitted.classes_[np.argmax(proba, axis=1)])
    assert np.max(np.abs(proba[:, 1] - 1.0 / (1.0 + np.exp(-values)))) <= 4 * EPS64
    assert np.allclose(fitted.predict_log_proba(X), np.log(proba)) and fitted.score(X, labels) >= 0.95
    # the log-odds are those of the model: the numpy fit of the same objective (class 1 is the positive label)
    lm = rm.library_landmarks(600, 32)
    model = lg.LogisticModel("rbf", X, np.where(labels == 1, 1.0, -1.0), 10.0, lm, gamma=0.5)
    assert np.array_equal(fitted.support_, lm)
    assert np.max(np.abs(values - model.decision_values(X))) <= 1e-6 * np.max(np.abs(values))  # (two iterations stopped at tol 1e-8)
    # class weights and sample weights reach the fit as fit_reduced_weighted passes them
    sw = wm.make_weights(600)
    weighted = svc.fit_reduced_logistic(svc.SVC(kernel="rbf", C=10.0, gamma=0.5, class_weight={0: 1.0, 1: 3.0}), X, labels, 32, sample_weight=sw)
    direct = backend.fit_reduced_logistic(base.parameter("rbf", dict(gamma=0.5), 10.0), X, np.where(labels == 1, 1.0, -1.0), 32, sample_weight=sw * np.where(labels == 1, 3.0, 1.0))
    assert np.array_equal(weighted.dual_coef_[0], direct[0]) and weighted.intercept_[0] == -direct[1]
    # the Model: saves, loads, predicts the same values; no probability field in the file
    data = DataSet(X, labels.tolist())
    svm = MI355CSVM(kernel_type="rbf", cost=10.0, gamma=0.5)
    model = svm.fit_reduced_logistic(data, 32)
    assert svm.last_cg_info["iterations"] == svm.last_cg_info["passes"] == fitted.n_iter_ and model.num_support_vectors() == 32
    assert np.array_equal(np.asarray(model.alpha), fitted.dual_coef_[0])
    path = tmp_path / "logistic.model"
    model.save(str(path))
    assert "prob" not in open(path).read()
    loaded = Model.load(str(path), real_type=np.float64, label_type=int)
    assert np.array_equal(np.array(svm.predict(loaded, data)), np.array(svm.predict(model, data))) and np.array_equal(np.array(svm.predict(model, data)), fitted.predict(X))
    with pytest.raises(AttributeError, match="not implemented"):
        svc.SVC().predict_proba


def test_three_classes_one_vs_all():
    X, labels = rm.blobs(600, 4, 3, 7)
    fitted = svc.fit_reduced_logistic(svc.SVC(kernel="rbf", C=10.0, gamma=0.5), X, labels, 32, landmarks="rpcholesky")
    proba, values = fitted.predict_proba(X), np.asarray(fitted.decision_function(X))
    assert proba.shape == values.shape == (600, 3) and fitted.n_iter_.shape == (3,) and np.all(fitted.n_iter_ > 1)
    assert np.max(np.abs(proba.sum(axis=1) - 1.0)) <= 4 * EPS64
    predicted = fitted.predict(X)
    assert np.array_equal(predicted, fitted.classes_[np.argmax(proba, axis=1)]) and np.array_equal(predicted, fitted.classes_[np.argmax(values, axis=1)])
    log_loss = float(-np.mean(np.log(proba[np.arange(600), labels])))
    print(f"three classes: accuracy {np.mean(predicted == labels):.4f}, mean log-loss {log_loss:.4f} (log 3 = {np.log(3.0):.4f})")
    assert np.isfinite(log_loss) and log_loss < np.log(3.0)
