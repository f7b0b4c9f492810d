"""GPU (-m gpu): the leave-one-out scores of the fixed-size LS-SVM over a (gamma, cost) grid in one call on one resident problem (lssvm_mi355_problem_fit_reduced_grid /
_landmark_acc, lssvm_mi355_fit_reduced_grid_*, MI355CSVM.fit_reduced_grid, svc.fit_reduced_grid_cv).  The yardstick is numpy float64
(tests/reduced_grid_model.py); tests/test_reduced_grid_host.py shows the model alone to meet the bounds below.  slab_rows = 256 throughout, so that several slabs occur.

The anchor.  product "ordered" with ONE gamma equal to the problem's own: every output has the BITS of fit_reduced_loo at the same factor -- without weights, with random
weights (some of them exact zeros), and with weights of 1.0 against the unweighted call.  N = 255 among the shapes: a Phi row from N on that was not an exact zero would
enter St (exp(0) is 1) and move every bit.

Operator.  landmark_acc -- D[l, i], what every gamma shares -- at N in {255, 777} x d in {5, 16, 33, 130} (one chunk; past one 16-chunk in fp64; past one 32-chunk in
fp32; past 128) x rank in {1, 16, 17, 129, 300} (across a 16-tile, into a second 128-block, several blocks) and once at rank 1 024, both dtypes, rbf and polynomial of
degree 3 and of degree -2.  D is compared THROUGH the kernel value: Phi = k(gamma', D) in numpy against numpy's Phi on the data the yardstick is evaluated on, because
that is the quantity whose element bound tests/test_gpu_reduced.py derives (its phi_error, with its r and u_h).  The factor the held data of a float64 problem carries
(gamma' = gamma / x_scale^2) is computed on the host as the library computes it -- 1, or sqrt(2 gamma log2 e) (rbf) / sqrt(gamma) (polynomial) on the fp64 matrix-core
path -- and the ordered D must agree with one of the two to 1e-9: a constant mis-scaling of D does not cancel out of the comparison.
  * product "ordered": |Phi_dev - Phi_numpy| <= phi_error.
  * product "matrix": <= phi_error + dPhi(dD), derived here.  A dot product x_i . x_l is one MFMA chain of ldx fused multiply-adds in ascending feature order on operands
    converted exactly to double: |d| <= gamma_ldx sum_f |a_f b_f|, and (ldx + 2) eps64 sum_f |a_f b_f| = 2 (ldx + 2) u covers it with a factor of about 2.  For rbf
    D = (n_i + n_l) - 2 a . b: each norm is a chain of ldx fused multiply-adds (gamma_ldx n), their sum and the final fused multiply-add round once more each, so
    |dD| <= (ldx + 2) u (n_i + n_l) + 2 ldx u sum_f |a_f b_f| + ...; (ldx + 4) eps64 (n_i + n_l + 2 sum_f |a_f b_f|) covers it with the same factor.  The clamp at 0
    and the exact 0 at the landmark itself only move D towards its true value.  dD is carried into Phi by the derivative of the kernel value: gamma' k dD (rbf) or
    |deg| gamma' |base|^(|deg| - 1) dD (polynomial; a negative degree: times k^2) -- reduced_grid_model.values_error.
  * D is exactly 0 at i == lm[l] and >= 0 everywhere (rbf), for both products.

Fits and scores.  Every (gamma, C) cell -- G = 3, S = 2, k = 3 -- against reduced_grid_model.GridModel under reduced_loo_model.tolerance, the bound of
tests/test_gpu_reduced_loo.py: h, f and loo within 8 max(e_loo, cond(M) eps64) x the largest |value|; both products, both factors, both dtypes, with and without weights;
N = 255 among the shapes.  The coefficients too, THROUGH the decision function they stand for: B Phi^T - rho formed in numpy from the returned betas and rhos on the held
data against the cell's f under the same tolerance (rho does NOT enter the fitted values, which take ybar; here a rho that is off by 1e-7 fails).  The coefficients
themselves are printed beside the model's and not bounded: M = S - s s^T / N cancels for a wide kernel, so two correct solves of it differ in beta by far more than
cond(M) eps64 max |beta| while their decision functions agree -- measured on the ordered product with the host factorisation, the path whose bits ARE fit_reduced_loo's:
rbf_777x5 at gamma 0.05, C 100: |dbeta| 9.5e-2 of max |beta| ~ 1e5 (2.7 x that figure) with |df| 6e-10 against 6.7e-8; poly_777x16: |drho| 1.0e-8 with |df| 5e-11
against 3.3e-10.  The sibling files bound decision values only, for the same reason.  press is recomputed from loo in row order and must match to the bit, loo_errors and max_leverage likewise.  The models MI355CSVM.fit_reduced_grid returns,
evaluated by the predict path, agree with the fitted values the call returned within the cell's tolerance -- for a float32 model plus 16 eps32 of the summands' scale (the
float tolerance of tests/test_gpu_reduced.py) and the kernel values' move between the held and the given data; the test's comment derives it.

Rows from N on of a Phi slab are exact zeros.  k_kernel_values writes them, for BOTH products, from the row index alone -- D is not read there.  The anchor at N = 255
is the check through the Gram operator: fit_reduced_loo's St is summed over k_landmark_block's slab, whose row 255 is an exact zero; the grid's St is summed over
k_kernel_values' slab by the same Gram kernels, and every bit of betas, rhos, h, f and loo agrees.  A row 255 of exp(0) = 1 or of coef0^degree would add 1 to S[j][l] and
s[j] -- a relative 4e-3 -- where one ulp moves the bits; the matrix product at N = 255 (rbf_255x5, poly-2_255x16 of the fits) goes through the same kernel and is held
to the model's tolerance, 1e-11 ... 1e-10 there for rbf.

Bit equalities, for both products: repeats; a gamma of the grid against the call with that gamma alone; a cost against the one-cost call; column c against the
single-column call; h for k = 1 and k = 3; one-shot against resident; the problem left as it was (a matvec, a CG solve and a solve_pcg before and after).

Surface: shapes and ordering of every output, svc.fit_reduced_grid_cv on three-class blobs, the refusals that need a device.

Measured on an MI355X (for the record; the assertions are the bounds above): MEASURED below."""

import functools

import numpy as np
import pytest

import pcg_model as pm
import reduced_grid_model as gm
import reduced_loo_model as lm
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
SLAB = 256
parameter = base.parameter
OPERATOR_N, OPERATOR_D, OPERATOR_RANKS = (255, 777), (5, 16, 33, 130), (1, 16, 17, 129, 300)
KINDS = {"rbf": ("rbf", lambda d: dict(gamma=1.0 / d)), "poly3": ("polynomial", lambda d: dict(gamma=1.0 / d, coef0=1.0, degree=3)),
         "poly-2": ("polynomial", lambda d: dict(gamma=1.0 / d, coef0=1.0, degree=-2))}
REPORT_ARRAYS = ("leverage", "fitted", "loo", "press", "loo_errors", "max_leverage", "jitter")

# what one run on an MI355X gave, for the record (the assertions are the bounds of the module docstring, not these figures)
MEASURED = {
    "operator: largest error / bound over d and the ranks (ordered, matrix)": {
        "float64": {"rbf": (0.166, 0.072), "poly3": (0.493, 0.475), "poly-2": (0.415, 0.403)}, "float32": {"rbf": (0.143, 0.047), "poly3": (0.466, 0.233), "poly-2": (0.406, 0.209)},
        "rank 1024": (0.060, 0.025)},
    "fit: largest |device - model| / tolerance over the cells, both factors, with and without weights (ordered, matrix)": {
        "rbf_777x5": {"float64": (0.144, 0.137), "float32": (0.154, 0.155)}, "poly_777x16": {"float64": (0.150, 0.155), "float32": (0.183, 0.183)},
        "rbf_255x5": {"float64": (0.089, 0.119), "float32": (0.075, 0.073)}, "poly-2_255x16": "below 1e-8 of a tolerance of 0.03: that model's e_loo is large, the bound says little there"},
    "f formed from the returned betas and rhos: largest |device - model| / tolerance": {"rbf_777x5": 0.009, "poly_777x16": 0.150, "rbf_255x5": 0.119},
    "models through the predict path against the fitted values: largest difference / bound": {"float64": "below 1e-3 (bounds 2e-11 ... 1e-7)", "float32": "0.02 ... 0.13 (bounds 9e-6 ... 1e-3)"},
}


def same(a, b, names=REPORT_ARRAYS):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and all(np.array_equal(a[3][n], b[3][n]) for n in names)


def cell_of(grid_result, g):
    """(betas, rhos, landmarks, report) of gamma g of a grid call, shaped as fit_reduced_loo returns them."""
    betas, rhos, used, report = grid_result
    return betas[g], rhos[g], used, {n: report[n][g] for n in REPORT_ARRAYS}


def weights_for(N, kind):
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones(N)
    return wm.make_weights(N, large=(64.0,))


# ---------------------------------------------------------------- the anchor ----------------------------------------------------------------
@pytest.mark.parametrize("factor", ["host", "device"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ordered_grid_of_the_own_gamma_has_the_bits_of_fit_reduced_loo(dtype, kind, factor):
    kernel, kw_of = KINDS[kind]
    costs = (1.0, 100.0)
    for N, d, rank in ((255, 5, 16), (777, 33, 129)):
        X, y = pm.make_data(N, d, pm.DATA_SEED, dtype)
        rng = np.random.default_rng(23)
        Y = np.stack([y] + [np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(dtype) for _ in range(2)])
        kw = rm.rounded_parameters(dtype, **kw_of(d))
        lms = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
        with backend.ResidentProblem(parameter(kernel, kw, 7.0), X) as prob:
            plain = prob.fit_reduced_loo(Y, rank, costs, landmarks=lms, slab_rows=SLAB, factor=factor)
            for weights in ("none", "ones", "random"):
                w = weights_for(N, weights)
                ref = plain if weights == "ones" else prob.fit_reduced_loo(Y, rank, costs, landmarks=lms, slab_rows=SLAB, factor=factor, sample_weight=w)
                got = prob.fit_reduced_grid(Y, rank, [kw["gamma"]], costs, landmarks=lms, sample_weight=w, factor=factor, product="ordered", slab_rows=SLAB)
                assert same(cell_of(got, 0), ref), (np.dtype(dtype).name, kind, factor, N, weights)
                assert got[3]["infos"][0][1]["cost"] == 100.0 and got[3]["infos"][0][0]["gamma"] == kw["gamma"]


# ---------------------------------------------------------------- the operator ----------------------------------------------------------------
def operator_setup(kernel, dtype, X, kw, prob):
    """(the data the yardstick is evaluated on, its kernel parameters, r, u_h): test_gpu_reduced.operator_setup for this file's kernel parameters."""
    if np.dtype(dtype) == np.float32:
        held, kw_held = rm.held_data(kernel, X, direct=bool(prob.info()["rbf_direct"]), **kw)
        return held, kw_held, 0, 0.0
    return X, kw, {"rbf": 2, "polynomial": 1}[kernel], EPS64


def held_in_double(kernel, dtype, Xy, s2, direct):
    """What the norms of the expansion are taken of.  float32: the yardstick's data IS the held data.  float64: the data as given, centred where the problem centres
    (rbf off the direct form), times the factor the problem's data carries (s2 = its square)."""
    A = np.asarray(Xy, dtype=np.float64)
    if np.dtype(dtype) == np.float32:
        return A
    return (A - A.mean(axis=0) if kernel == "rbf" and not direct else A) * np.sqrt(s2)


def phi_bound(kernel, Xy, lms, kw_y, r, u_h):
    """test_gpu_reduced.phi_error; for a polynomial of another degree than its 3 the same derivation with that degree: the base carries
    gamma sum_f |a_f b_f| (2 r u_h + (d + 2) u64) + u64 |base|, the power multiplies it by the derivative of the kernel value and rounds |degree| + 1 times more."""
    if kernel != "polynomial" or kw_y["degree"] == 3:
        return base.phi_error(kernel, Xy, lms, kw_y, r, u_h)
    A = np.asarray(Xy, dtype=np.float64)
    B = A[np.asarray(lms, dtype=np.int64)]
    dot = A @ B.T
    d_base = kw_y["gamma"] * (np.abs(A) @ np.abs(B).T) * (2.0 * r * u_h + (A.shape[1] + 2) * EPS64) + EPS64 * np.abs(kw_y["gamma"] * dot + kw_y["coef0"])
    return gm.values_error(kernel, dot, d_base / kw_y["gamma"], kw_y) + (abs(kw_y["degree"]) + 1) * EPS64 * np.abs(gm.kernel_values(kernel, dot, kw_y))


def check_operator(prob, kernel, dtype, Xy, kw_y, r, u_h, lms, direct):
    rank, at = len(lms), np.asarray(lms, dtype=np.int64)
    D_numpy = gm.direct_sums(kernel, Xy, lms)  # N x m, in the yardstick's units
    Phi = pm.kernel_matrix(kernel, Xy, np.asarray(Xy)[at], **kw_y)
    dPhi = phi_bound(kernel, Xy, lms, kw_y, r, u_h)
    D0 = prob.landmark_acc(rank, landmarks=lms, product="ordered").T
    D1 = prob.landmark_acc(rank, landmarks=lms, product="matrix").T
    assert D0.shape == D1.shape == D_numpy.shape and np.all(np.isfinite(D0)) and np.all(np.isfinite(D1))
    # The square of the factor the held data carries, computed on the HOST as the library computes it -- never read off D, or a constant mis-scaling of D would cancel.
    # float32: the yardstick's data is the held data already (reduced_model.held_data): 1.  float64: rbf off the direct form holds sqrt(2 gamma log2 e) (x - mean) on
    # the fp64 matrix-core path and x - mean elsewhere; a polynomial problem holds sqrt(gamma) x on that path and x elsewhere.  Which of the two a problem took is not
    # in its info: it is the candidate the ordered D agrees with to 1e-9, and one of them MUST agree.
    candidates = [1.0]
    if np.dtype(dtype) == np.float64 and not (kernel == "rbf" and direct):
        candidates.append(float(np.sqrt(2.0 * kw_y["gamma"] * rm.LOG2E)) ** 2 if kernel == "rbf" else float(np.sqrt(kw_y["gamma"])) ** 2)
    big = np.abs(D_numpy) > 0.05 * np.max(np.abs(D_numpy))
    seen = float(np.median(D0[big] / D_numpy[big])) if np.any(big) else 1.0
    s2 = min(candidates, key=lambda c: abs(seen / c - 1.0))
    assert abs(seen / s2 - 1.0) <= 1e-9, (kernel, np.dtype(dtype).name, seen, candidates)
    kw_dev = dict(kw_y, gamma=kw_y["gamma"] / s2)
    if kernel == "rbf":
        for D in (D0, D1):
            assert np.all(D >= 0.0) and np.all(D[at, np.arange(rank)] == 0.0)
    ratio0 = float(np.max(np.abs(gm.kernel_values(kernel, D0, kw_dev) - Phi) / dPhi))
    held = held_in_double(kernel, dtype, Xy, s2, direct)
    dD = gm.expansion_bound(kernel, held, lms, gm.padded_features(np.asarray(Xy).shape[1], dtype))
    bound1 = dPhi + gm.values_error(kernel, gm.direct_sums(kernel, held, lms), dD, kw_dev)
    ratio1 = float(np.max(np.abs(gm.kernel_values(kernel, D1, kw_dev) - Phi) / bound1))
    assert ratio0 <= 1.0 and ratio1 <= 1.0, (kernel, np.dtype(dtype).name, np.asarray(Xy).shape, rank, ratio0, ratio1)
    assert np.array_equal(D1, prob.landmark_acc(rank, landmarks=lms, product="matrix").T)
    # a landmark's column does not depend on the other landmarks: the order of every sum depends on ldx only
    if rank > 1:
        assert np.array_equal(prob.landmark_acc(1, landmarks=lms[-1:], product="matrix")[0], D1[:, -1])
    return ratio0, ratio1


@pytest.mark.parametrize("N", OPERATOR_N)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_operator_against_numpy(dtype, kind, N):
    kernel, kw_of = KINDS[kind]
    worst = [0.0, 0.0]
    for d in OPERATOR_D:
        X, _ = pm.make_data(N, d, pm.DATA_SEED, dtype)
        kw = rm.rounded_parameters(dtype, **kw_of(d))
        with backend.ResidentProblem(parameter(kernel, kw, 10.0), X) as prob:
            Xy, kw_y, r, u_h = operator_setup(kernel, dtype, X, kw, prob)
            direct = bool(prob.info()["rbf_direct"])
            for rank in OPERATOR_RANKS:
                if rank > N:
                    continue
                got = check_operator(prob, kernel, dtype, Xy, kw_y, r, u_h, pm.draw_landmarks(N, rank, pm.LANDMARK_SEED), direct)
                worst = [max(a, b) for a, b in zip(worst, got)]
    print(f"grid operator {np.dtype(dtype).name} {kind} N={N}: largest error / bound, ordered {worst[0]:.3f}, matrix {worst[1]:.3f}")


def test_operator_at_the_largest_rank():
    N, rank, d = 1100, rm.MAX_RANK, 33
    X, _ = pm.make_data(N, d, pm.DATA_SEED, np.float64)
    kw = dict(gamma=1.0 / d)
    with backend.ResidentProblem(parameter("rbf", kw, 10.0), X) as prob:
        got = check_operator(prob, "rbf", np.float64, X, kw, 2, EPS64, pm.draw_landmarks(N, rank, pm.LANDMARK_SEED), bool(prob.info()["rbf_direct"]))
    print(f"grid operator at rank {rank}: largest error / bound, ordered {got[0]:.3f}, matrix {got[1]:.3f}")


# ---------------------------------------------------------------- fits and scores ----------------------------------------------------------------
FIT_COSTS = (1.0, 100.0)
FIT_ROWS = {"rbf_777x5": (777, 5, "rbf", dict(gamma=0.2), (0.05, 0.2, 0.8), 64), "poly_777x16": (777, 16, "polynomial", dict(gamma=1.0 / 16, coef0=1.0, degree=3), (0.02, 1.0 / 16, 0.2), 64),
            "rbf_255x5": (255, 5, "rbf", dict(gamma=0.2), (0.05, 0.2, 0.8), 17), "poly-2_255x16": (255, 16, "polynomial", dict(gamma=1.0 / 16, coef0=1.0, degree=-2), (0.02, 1.0 / 16, 0.2), 17)}


@functools.lru_cache(maxsize=None)
def fit_reference(name, dtype, weighted):
    """(case, GridModel): float64 numpy, once per case, shared, never modified.  (rbf in float32 off the direct form: the test asserts the problem is off it.)"""
    N, d, kernel, own_kw, gammas, rank = FIT_ROWS[name]
    X, y = pm.make_data(N, d, pm.DATA_SEED, dtype)
    rng = np.random.default_rng(23)
    Y = np.stack([y] + [np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(dtype) for _ in range(2)])
    kw = rm.rounded_parameters(dtype, **own_kw)
    lms = pm.draw_landmarks(N, rank, pm.LANDMARK_SEED)
    w = weights_for(N, "random") if weighted else None
    model = gm.GridModel(kernel, X, Y, lms, gammas, FIT_COSTS, kw, w=w)
    for row in model.cells:
        for cell in row:
            for a in (cell.h, cell.f, cell.loo):
                a.setflags(write=False)
    for a in (X, Y):
        a.setflags(write=False)
    return dict(X=X, Y=Y, kernel=kernel, kw=kw, gammas=gammas, rank=rank, landmarks=lms, w=w), model


def sequential_press(y, loo, w=None):
    """sum_i [w_i] (y_i - loo_i)^2 in row order, as the header defines press."""
    total = 0.0
    for i, (a, b) in enumerate(zip(np.asarray(y, dtype=np.float64).tolist(), loo.tolist())):
        d = a - b
        total += d * d if w is None else w[i] * (d * d)
    return total


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(FIT_ROWS))
def test_every_cell_against_the_model(name, dtype, weighted):
    p, model = fit_reference(name, dtype, weighted)
    N = p["X"].shape[0]
    X_held, kws = model.held
    Phi_held = [pm.kernel_matrix(p["kernel"], X_held, np.asarray(X_held)[p["landmarks"].astype(np.int64)], **kw_g) for kw_g in kws]
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 3.0), p["X"]) as prob:  # (the problem's own cost plays no part)
        assert np.dtype(dtype) == np.float64 or p["kernel"] != "rbf" or prob.info()["rbf_direct"] == 0
        for product in ("ordered", "matrix"):
            for factor in ("host", "device"):
                betas, rhos, used, report = prob.fit_reduced_grid(p["Y"], p["rank"], p["gammas"], FIT_COSTS, landmarks=p["landmarks"], sample_weight=p["w"], factor=factor,
                                                                  product=product, slab_rows=SLAB)
                assert betas.shape == (3, 2, 3, p["rank"]) and rhos.shape == (3, 2, 3) and report["leverage"].shape == (3, 2, N) and report["loo"].shape == (3, 2, 3, N)
                assert report["press"].shape == report["loo_errors"].shape == (3, 2, 3) and report["jitter"].shape == report["max_leverage"].shape == (3, 2)
                assert np.array_equal(used, p["landmarks"]) and np.array_equal(report["gammas"], p["gammas"]) and np.array_equal(report["costs"], FIT_COSTS)
                for g in range(3):
                    for s in range(2):
                        cell, e = model.cells[g][s], model.e[g][s]
                        info = report["infos"][g][s]
                        assert info["gamma"] == p["gammas"][g] and info["cost"] == FIT_COSTS[s] and info["accumulate_ms"] > 0.0 and info["values_ms"] > 0.0
                        for what, got, ref in (("h", report["leverage"][g, s], cell.h), ("f", report["fitted"][g, s], cell.f), ("loo", report["loo"][g, s], cell.loo)):
                            tol = lm.tolerance(cell, e, np.max(np.abs(ref)))
                            diff = float(np.max(np.abs(got - ref)))
                            print(f"grid fit {name} {np.dtype(dtype).name} w={weighted} {product}/{factor} gamma={p['gammas'][g]:g} C={FIT_COSTS[s]:g} {what}: |device - model| {diff:.2e}, "
                                  f"tolerance {tol:.2e} (e_loo {e:.1e}, cond(M) eps64 {cell.cond * EPS64:.1e})")
                            assert diff <= tol, (name, product, factor, g, s, what, diff, tol)
                        # the coefficients (rho does not enter the fitted values: the leverage kernel takes ybar) through the decision function they stand for on the held
                        # data, B Phi^T - rho in numpy: the quantity the tolerance is derived for.  The coefficients themselves are printed, not bounded (module docstring).
                        f_coef = betas[g, s] @ Phi_held[g].T - rhos[g, s][:, None]
                        tol = lm.tolerance(cell, e, np.max(np.abs(cell.f)))
                        diff = float(np.max(np.abs(f_coef - cell.f)))
                        print(f"grid fit {name} {np.dtype(dtype).name} w={weighted} {product}/{factor} gamma={p['gammas'][g]:g} C={FIT_COSTS[s]:g} f from betas and rhos: "
                              f"|device - model| {diff:.2e}, tolerance {tol:.2e}; |betas - model's| {np.max(np.abs(betas[g, s] - cell.betas)):.2e} of {np.max(np.abs(cell.betas)):.2e}, "
                              f"|rhos - model's| {np.max(np.abs(rhos[g, s] - cell.rhos)):.2e}")
                        assert diff <= tol, (name, product, factor, g, s, diff, tol)
                        assert report["max_leverage"][g, s] == report["leverage"][g, s].max()
                        for c in range(3):
                            assert report["press"][g, s, c] == sequential_press(p["Y"][c], report["loo"][g, s, c], p["w"]), (g, s, c)
                        if weighted:
                            assert np.array_equal(report["loo_errors"][g, s], wm.errors_of(p["Y"], report["loo"][g, s], p["w"]))
                        else:
                            assert np.array_equal(report["loo_errors"][g, s], lm.errors_of(p["Y"], report["loo"][g, s]))


# ---------------------------------------------------------------- bit equalities ----------------------------------------------------------------
@pytest.mark.parametrize("product", ["ordered", "matrix"])
@pytest.mark.parametrize("name, dtype, factor", [("rbf_777x5", np.float32, "host"), ("poly_777x16", np.float64, "device"), ("rbf_255x5", np.float64, "device")])
def test_repeats_gammas_costs_and_columns_are_bit_equal(name, dtype, factor, product):
    p, _ = fit_reference(name, dtype, True)
    kwargs = dict(landmarks=p["landmarks"], sample_weight=p["w"], factor=factor, product=product, slab_rows=SLAB)
    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 5.0), p["X"]) as prob:
        full = prob.fit_reduced_grid(p["Y"], p["rank"], p["gammas"], FIT_COSTS, **kwargs)
        assert same(full, prob.fit_reduced_grid(p["Y"], p["rank"], p["gammas"], FIT_COSTS, **kwargs))
        b3, r3, _, rep3 = full
        for g, gamma in enumerate(p["gammas"]):  # a gamma of the grid: the bits of the call with that gamma alone
            assert same(cell_of(full, g), cell_of(prob.fit_reduced_grid(p["Y"], p["rank"], [gamma], FIT_COSTS, **kwargs), 0)), (g,)
        for s, cost in enumerate(FIT_COSTS):  # a cost: the bits of the one-cost call
            b, r, _, rep = prob.fit_reduced_grid(p["Y"], p["rank"], p["gammas"], [cost], **kwargs)
            assert np.array_equal(b[:, 0], b3[:, s]) and np.array_equal(r[:, 0], r3[:, s])
            for n in REPORT_ARRAYS:
                assert np.array_equal(rep[n][:, 0], rep3[n][:, s]), (s, n)
        for c in range(3):  # column c: the bits of the single-column call; h does not depend on k
            b1, r1, _, rep1 = prob.fit_reduced_grid(p["Y"][c], p["rank"], p["gammas"], FIT_COSTS, **kwargs)
            assert np.array_equal(rep1["leverage"], rep3["leverage"]) and np.array_equal(rep1["max_leverage"], rep3["max_leverage"])
            assert np.array_equal(b3[:, :, c], b1) and np.array_equal(r3[:, :, c], r1)
            for n in ("fitted", "loo", "press", "loo_errors"):
                assert np.array_equal(rep3[n][:, :, c], rep1[n]), (c, n)
    one_shot = backend.fit_reduced_grid(parameter(p["kernel"], p["kw"], 5.0), p["X"], p["Y"], p["rank"], p["gammas"], FIT_COSTS, landmarks=p["landmarks"], slab_rows=SLAB,
                                        factor=factor, sample_weight=p["w"], product=product)
    assert same(one_shot, full)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_problem_is_left_as_it_was(dtype):
    p, _ = fit_reference("rbf_777x5", dtype, False)
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

    with backend.ResidentProblem(parameter(p["kernel"], p["kw"], 100.0), p["X"]) as prob:
        prob.build_preconditioner(landmarks=p["landmarks"][:37])
        before = state(prob)
        for product in ("ordered", "matrix"):
            prob.fit_reduced_grid(p["Y"], 64, p["gammas"], FIT_COSTS, product=product, slab_rows=SLAB)
            prob.landmark_acc(16, product=product)
        after = state(prob)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_refusals_on_a_problem():
    p, _ = fit_reference("rbf_777x5", np.float64, False)
    N, y = p["X"].shape[0], p["Y"][0]
    prm = parameter(p["kernel"], p["kw"], 1.0)
    with backend.ResidentProblem(prm, p["X"]) as prob:
        calls = (lambda: prob.fit_reduced_grid(y, 8, [0.2], [1.0]), lambda: prob.landmark_acc(8))
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
        for gammas in ([], [0.0], [-1.0], [float("nan")], [float("inf")], np.full(65, 0.5)):
            with pytest.raises(InvalidParameterError, match="gamma|cells"):
                prob.fit_reduced_grid(y, 8, gammas, [1.0])
        with pytest.raises(InvalidParameterError, match="cells"):
            prob.fit_reduced_grid(y, 8, np.full(9, 0.5), np.ones(8))
        with pytest.raises(InvalidParameterError, match="product"):
            prob.fit_reduced_grid(y, 8, [0.2], [1.0], product="fast")
        with pytest.raises(InvalidParameterError, match="factor"):
            prob.fit_reduced_grid(y, 8, [0.2], [1.0], factor="gpu")
        with pytest.raises(InvalidParameterError, match="distinct"):
            prob.fit_reduced_grid(y, 3, [0.2], [1.0], landmarks=[3, 7, 3])
        with pytest.raises(InvalidParameterError, match="slab_rows"):
            prob.fit_reduced_grid(y, 8, [0.2], [1.0], slab_rows=100)
        _, _, used, report = prob.fit_reduced_grid(y, 2, [0.2], [1.0], landmarks=[0, N - 1])  # (the last point is allowed, and the handle still works)
        assert np.array_equal(used, [0, N - 1]) and np.all(np.isfinite(report["loo"])) and report["loo"].shape == (1, 1, N)
    with backend.ResidentProblem(parameter("linear", dict(gamma=1.0), 1.0), p["X"]) as linear:
        with pytest.raises(InvalidParameterError, match="linear kernel has no gamma"):
            linear.fit_reduced_grid(y, 8, [0.2], [1.0])
    with backend.ResidentProblem(prm, p["X"], devices=[0, 0]) as shard:  # two shards on the one device
        with pytest.raises(InvalidParameterError, match="one device and one rank"):
            shard.fit_reduced_grid(y, 8, [0.2], [1.0])


# ---------------------------------------------------------------- the surface ----------------------------------------------------------------
SURFACE_GAMMAS, SURFACE_COSTS = (0.05, 0.125, 0.5), (0.1, 10.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_csvm_fit_reduced_grid_models_carry_their_cell_save_load_and_predict(dtype, tmp_path):
    X, labels = rm.blobs(1000, 8, 2, seed=31, dtype=dtype)
    data = DataSet(X, labels.tolist(), real_type=dtype)
    svm = MI355CSVM(kernel_type="rbf", cost=3.0, gamma=0.125)
    models, report = svm.fit_reduced_grid(data, 48, SURFACE_GAMMAS, SURFACE_COSTS)
    lms = rm.library_landmarks(1000, 48)
    assert len(models) == 3 and all(len(row) == 2 for row in models) and report["loo"].shape == (3, 2, 1000) and report["loo_accuracy"].shape == (3, 2)
    assert np.array_equal(report["landmarks"], lms) and [[i["iterations"] for i in row] for row in svm.last_cg_info] == [[0, 0]] * 3
    y = data.mapped_labels().astype(np.float64)
    own_kw = rm.rounded_parameters(dtype, gamma=0.125)
    reference = gm.GridModel("rbf", X, y[None, :], lms, SURFACE_GAMMAS, SURFACE_COSTS, own_kw)
    for g, gamma in enumerate(SURFACE_GAMMAS):
        kw_g = gm.given_kw(own_kw, dtype, gamma)
        for s, cost in enumerate(SURFACE_COSTS):
            model, cell, e = models[g][s], reference.cells[g][s], reference.e[g][s]
            assert model.params.gamma == gamma and model.params.cost == cost and model.alpha.dtype == np.dtype(dtype) and model.num_support_vectors() == 48
            # The model through the predict path against the fitted values the call returned, under the tolerance of the sibling files: the fit's own,
            # 8 max(e_loo, cond(M) eps64) max |f|, and for a float32 model two more terms.  (a) beta rounded to float32 and the float32 evaluation of the sum: 16 eps32 of the
            # summands' scale (test_float32_model_through_predict_values of tests/test_gpu_reduced.py).  (b) the fit saw the data as the problem holds it, the predict
            # path sees it as given: a held coordinate is (x - mean) scale rounded twice in float32, eps32 |x - mean| per point, which moves a kernel value by
            # test_gpu_reduced.phi_error with r = 1, u_h = eps32; through |beta|.
            fitted = report["fitted"][g, s]
            values = np.asarray(svm.predict_values(model.params, model.support_vectors(), model.alpha, float(model.rho), model.w, data.data())[0], dtype=np.float64).reshape(-1)
            bound = np.full(1000, lm.tolerance(cell, e, np.max(np.abs(cell.f))))
            if np.dtype(dtype) == np.float32:
                bound = bound + 16 * rm.EPS32 * rm.summand_scale("rbf", X[lms.astype(int)], cell.betas, cell.rhos, X, **kw_g)[0]
                bound = bound + base.phi_error("rbf", X, lms, kw_g, 1, rm.EPS32) @ np.abs(cell.betas[0])
            ratio = float(np.max(np.abs(values - fitted) / bound))
            print(f"grid surface {np.dtype(dtype).name} gamma={gamma:g} C={cost:g}: largest |predict - fitted| / bound {ratio:.3f} (largest bound {np.max(bound):.2e})")
            assert ratio <= 1.0, (g, s, ratio)
            clear = np.abs(fitted) > bound
            predicted = np.array([1.0 if label == data.mapping.label_of(1) else -1.0 for label in svm.predict(model, data)])
            assert np.mean(~clear) <= 0.01 and np.array_equal(predicted[clear], np.sign(fitted)[clear])
            assert report["loo_errors"][g, s] == np.count_nonzero(np.sign(report["loo"][g, s]) != y) and report["loo_accuracy"][g, s] == 1.0 - int(report["loo_errors"][g, s]) / 1000
    path = tmp_path / "cell.model"
    models[2][1].save(str(path))
    loaded = Model.load(str(path), real_type=dtype, label_type=int)
    assert loaded.num_support_vectors() == 48 and loaded.params.gamma == pytest.approx(SURFACE_GAMMAS[2]) and svm.predict(loaded, data) == svm.predict(models[2][1], data)
    # the cell at the object's own gamma, ordered product: what fit_reduced_path gives
    own, _ = svm.fit_reduced_grid(data, 48, [0.125], SURFACE_COSTS, product="ordered")
    path_models, _ = svm.fit_reduced_path(data, 48, SURFACE_COSTS)
    for a, b in zip(own[0], path_models):
        assert np.array_equal(a.alpha, b.alpha) and a.rho == b.rho


@pytest.mark.parametrize("class_weight", [None, "balanced"])
def test_svc_fit_reduced_grid_cv_on_three_classes(class_weight):
    X, labels = lm.overlapping_blobs(900, 4, 3, seed=41)
    est = svc.SVC(kernel="rbf", C=3.0, gamma=0.25, class_weight=class_weight)
    scores, clones = svc.fit_reduced_grid_cv(est, X, labels, 32, SURFACE_COSTS, SURFACE_GAMMAS)
    assert est._fit is None and scores.shape == (3, 2) and np.all(scores > 1.0 / 3) and np.all(scores < 1.0) and len(set(scores.reshape(-1).tolist())) > 1
    g, s = np.unravel_index(int(np.argmax(scores)), scores.shape)
    best = clones[g][s]
    assert best.gamma == SURFACE_GAMMAS[g] and best.C == SURFACE_COSTS[s] and best.dual_coef_.shape == (3, 32)
    assert float(np.mean(best.predict(X) == labels)) >= scores[g, s] - 0.05
    # the column of the problem's own gamma: what the cost-only call gives there under the same weighting (another product: close, not the bits)
    ref_scores, _ = svc.fit_reduced_cv_weighted(est, X, labels, 32, SURFACE_COSTS)
    own_scores, own_clones = svc.fit_reduced_grid_cv(est, X, labels, 32, SURFACE_COSTS, [0.25], product="ordered")
    assert np.array_equal(own_scores[0], ref_scores)
    two = labels % 2
    scores2, clones2 = svc.fit_reduced_grid_cv(svc.SVC(kernel="rbf", gamma=0.25), X, two, 32, SURFACE_COSTS, SURFACE_GAMMAS)
    assert scores2.shape == (3, 2) and np.array_equal(clones2[0][1].predict(X[:50]).shape, (50,)) and clones2[2][0].gamma == SURFACE_GAMMAS[2]
