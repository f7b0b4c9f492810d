"""GPU (-m gpu): the fixed-size LS-SVM from a stream of chunks (lssvm_mi355_reduced_stream_*, backend.ReducedStream, MI355CSVM.fit_reduced_stream,
svc.fit_reduced_stream).  The yardstick is numpy float64 (tests/reduced_stream_model.py and the sibling models it imports), evaluated on the rows as
the stream stages them: X.astype(float64) - centre, the centre read back from the handle (and equal, to the bit, to the model's own).  tests/test_reduced_stream_host.py
shows the model alone to meet the bounds below.  slab_rows = 256 nearly everywhere, so that a chunk wraps the pending slab and several slabs are summed.

Kernel, through lssvm_mi355_reduced_stream_phi: Phi of a chunk at d in {1, 5, 16, 17, 33, 130} x rank in {1, 16, 17, 128, 129, 300} x chunk lengths in
{1, 127, 128, 129, 255, 257}, both dtypes, rbf, polynomial of degree 3 and of degree -2, linear; once at rank 1 024 against 1 100 rows.  The bound is the one
tests/test_gpu_reduced_grid.py derives for product "matrix", |Phi_dev - Phi_numpy| <= phi_error + values_error(expansion_bound), with ldx = d rounded up to 16 and r = 0
(the yardstick's rows ARE the staged rows: the subtraction of the centre is the same single rounding on both sides).  D itself is not exposed; D >= 0 for rbf is checked
as Phi <= 1.  The rows of a chunk do not depend on the chunk: Phi of the first n rows has the bits of the first n rows of Phi.  K_mm has a diagonal of exactly 1 (rbf) and
is symmetric to the bit.

Cut independence, bit for bit: 777 rows, k = 3, with and without weights (some exact zeros): one update against the updates (1, 127, 129, 520) against 777 updates of one
row -- the exported S~, betas and rhos on both factors; update -> solve -> update -> solve against update -> update -> solve; repeats; column c against the single-column
stream; a cost of a grid against the one-cost solve; weights of 1.0 against the unweighted stream.

Gram: the exported S~ against numpy's P^T diag(w) P with P = [Phi_dev | 1 | Y] and Phi_dev from the testing entry -- the first term of the bound of
tests/test_gpu_reduced.py (Phi_dev carries no element error against itself): 2 N eps64 (|P|^T diag(w) |P|), with weights 2 (N + 4) eps64 (sqrt(w_i) and its products with
both operands round four times more per summand).  S~[m][m] == N exactly on an unweighted stream.

Fits and scores: rbf_777x5 (gamma 0.05 / 0.2 / 0.8), poly_777x16 and rbf_255x5 at rank 64 and the costs (1, 100), both dtypes, both factors, with and without weights,
k = 3, against reduced_loo_model.LooModel / reduced_weighted_model.WeightedLooModel with held = the centred rows: the decision values formed in numpy from the returned
betas and rhos under reduced_model.fit_tolerance (with the model's e_loo: the yardstick of the leave-one-out models), and h, fitted and loo of the two-pass walk (the
stream is fed in the chunks (1, 127, 129, rest) and scored in other chunks) under reduced_loo_model.tolerance.  The coefficients are printed and not bounded, for the
reason tests/test_gpu_reduced_grid.py states.  One case has landmarks that are NOT among the streamed rows: its yardstick is the weighted model with the landmark rows
appended at weight 0.

Merge: two and three shard streams merged into an empty one and into the first shard agree with the single stream within the Gram bound; the same merge order gives the
same bits; a foreign fingerprint (another gamma, other landmarks, another dtype) is refused.

Surface: MI355CSVM.fit_reduced_stream (save, load, predict; the decision values against the call's fitted values within the tolerance tests/test_gpu_reduced.py uses for
models), svc.fit_reduced_stream on three-class blobs with class_weight None and "balanced", and the refusals that need a device.

Measured on an MI355X (for the record; the assertions are the bounds above): MEASURED below."""

import functools

import numpy as np
import pytest

import pcg_model as pm
import reduced_loo_model as lm
import reduced_model as rm
import reduced_stream_model as sm
import reduced_weighted_model as wm
import test_gpu_reduced as base
import test_gpu_reduced_grid as grid
from plssvm_amd import backend, svc
from plssvm_amd.csvm import MI355CSVM
from plssvm_amd.data_set import DataSet
from plssvm_amd.exceptions import InvalidParameterError
from plssvm_amd.model import Model

pytestmark = pytest.mark.gpu

EPS64 = rm.EPS64
SLAB = 256
CUTS = (1, 127, 129, 520)
COSTS = (1.0, 100.0)
KINDS = dict(grid.KINDS, linear=("linear", lambda d: dict(gamma=1.0)))
PHI_D, PHI_RANKS, PHI_CHUNKS = (1, 5, 16, 17, 33, 130), (1, 16, 17, 128, 129, 300), (1, 127, 128, 129, 255, 257)

# what one run on an MI355X gave, for the record (the assertions are the bounds of the module docstring, not these figures)
MEASURED = {
    "phi: largest error / bound over d, the ranks and the chunk lengths": {
        "float64": {"rbf": 0.074, "poly3": 0.296, "poly-2": 0.287, "linear": 0.040}, "float32": {"rbf": 0.071, "poly3": 0.287, "poly-2": 0.266, "linear": 0.034}, "rank 1024": 0.025},
    "exported gram against numpy on the device's Phi: largest error / bound": "0.003 ... 0.004 (both kernels, both dtypes, with and without weights)",
    "fit: largest |device - model| / tolerance over h, f, loo and f from betas and rhos, both factors (without, with weights)": {
        "rbf_777x5_g0.05": {"float64": (0.111, 0.147), "float32": (0.154, 0.209)}, "rbf_777x5_g0.2": {"float64": (0.051, 0.055), "float32": (0.063, 0.085)},
        "rbf_777x5_g0.8": {"float64": (0.020, 0.009), "float32": (0.018, 0.012)}, "poly_777x16": {"float64": (0.118, 0.113), "float32": (0.164, 0.200)},
        "rbf_255x5": {"float64": (0.011, 0.035), "float32": (0.010, 0.036)}, "landmarks not among the rows": (0.102, 0.091)},
    "merge: |merged - single stream| / Gram bound": {"2 shards": 0.003, "3 shards": 0.001},
    "models through the predict path against the fitted values: (difference, tolerance)": {"float64": "(7e-15 ... 2e-14, 2e-8 ... 7e-8)", "float32": "(2e-6 ... 7e-6, 1e-4 ... 3e-4)"},
    "svc decision_function against the numpy model: difference / tolerance": "0.0006 ... 0.008",
}


def open_stream(kernel, kw, XL, k=1, weighted=False, slab_rows=SLAB):
    return backend.ReducedStream(base.parameter(kernel, kw, 1.0), XL, num_rhs=k, weighted=weighted, slab_rows=slab_rows)


def feed(stream, X, Y, w, cuts):
    at = 0
    for n in cuts:
        stream.update(X[at:at + n], Y[:, at:at + n], None if w is None else w[at:at + n])
        at += n
    assert at == X.shape[0]
    return stream


# ---------------------------------------------------------------- the kernel ----------------------------------------------------------------
def phi_bounds(kernel, Xh, XLh, kw):
    """(Phi_numpy, the bound of the module docstring), N x m, on the staged rows."""
    N, m = Xh.shape[0], XLh.shape[0]
    both, at = np.vstack([Xh, XLh]), np.arange(N, N + m)
    Phi = pm.kernel_matrix(kernel, Xh, XLh, **kw)
    dPhi = grid.phi_bound(kernel, both, at, kw, 0, 0.0)[:N]
    direct, dD = sm.direct_and_bound(kernel, Xh, XLh, sm.padded_features(Xh.shape[1]))
    if kernel == "linear":
        return Phi, dPhi + dD  # (the kernel value is the dot product itself)
    return Phi, dPhi + sm.gm.values_error(kernel, direct, dD, kw)


def check_phi(stream, kernel, kw, X, XL, chunks):
    centre = stream.centre
    assert np.array_equal(centre, sm.centre_of(kernel, XL))
    Xh, XLh = sm.held(X, centre), sm.held(XL, centre)
    Phi, bound = phi_bounds(kernel, Xh, XLh, kw)
    got = stream.phi(X)
    assert got.shape == Phi.shape and np.all(np.isfinite(got))
    ratio = float(np.max(np.abs(got - Phi) / bound))
    assert ratio <= 1.0, (kernel, X.dtype.name, X.shape, XL.shape[0], ratio)
    if kernel == "rbf":
        assert np.all(got <= 1.0) and np.all(got >= 0.0)  # D >= 0
    for n in chunks:
        assert np.array_equal(stream.phi(X[:n]), got[:n]), n
    K = stream.landmark_gram
    Kref, Kbound = phi_bounds(kernel, XLh, XLh, kw)
    assert np.array_equal(K, K.T) and float(np.max(np.abs(K - Kref) / Kbound)) <= 1.0
    if kernel == "rbf":
        assert np.all(np.diag(K) == 1.0)
    return ratio


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_phi_against_numpy(dtype, kind):
    kernel, kw_of = KINDS[kind]
    N, worst = max(PHI_CHUNKS), 0.0
    for d in PHI_D:
        X = pm.make_data(N, d, pm.DATA_SEED, dtype)[0]
        kw = rm.rounded_parameters(dtype, **kw_of(d))
        pool = pm.make_data(max(PHI_RANKS), d, pm.DATA_SEED + 1, dtype)[0]  # landmark rows that are no rows of the chunk
        for rank in PHI_RANKS:
            XL = np.vstack([X[:rank // 2], pool[:rank - rank // 2]])  # ... and some that are
            with open_stream(kernel, kw, XL) as stream:
                worst = max(worst, check_phi(stream, kernel, kw, X, XL, PHI_CHUNKS))
                assert stream.num_points == 0 and stream.info["pending"] == 0  # (the testing entry leaves the state alone)
    print(f"stream phi {np.dtype(dtype).name} {kind}: largest error / bound {worst:.3f}")


def test_phi_at_the_largest_rank():
    N, rank, d = 1100, rm.MAX_RANK, 33
    X = pm.make_data(N, d, pm.DATA_SEED, np.float64)[0]
    kw = dict(gamma=1.0 / d)
    XL = X[pm.draw_landmarks(N, rank, pm.LANDMARK_SEED).astype(np.int64)]
    with open_stream("rbf", kw, XL) as stream:
        ratio = check_phi(stream, "rbf", kw, X, XL, (257,))
    print(f"stream phi at rank {rank}: largest error / bound {ratio:.3f}")


# ---------------------------------------------------------------- cut independence ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cut_case(kernel, dtype):
    name = {"rbf": "rbf_777x5", "polynomial": "poly_777x16"}[kernel]
    p = rm.fit_case(name, dtype, 3)
    w = wm.make_weights(p["X"].shape[0], large=(64.0,))
    assert np.any(w == 0.0)
    XL = np.ascontiguousarray(p["X"][p["landmarks"].astype(np.int64)])
    for a in (p["X"], p["Y"], w, XL):
        a.setflags(write=False)
    return p, w, XL


def results(stream, factors=("host", "device")):
    state = stream.export_state()
    out = [state["gram"], np.array([state["num_points"]])]
    for factor in factors:
        betas, rhos, _ = stream.solve(COSTS, factor=factor)
        out += [betas, rhos]
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kernel, dtype", [("rbf", np.float64), ("rbf", np.float32), ("polynomial", np.float64), ("polynomial", np.float32)])
def test_results_do_not_depend_on_the_cuts(kernel, dtype, weighted):
    p, w, XL = cut_case(kernel, dtype)
    X, Y, kw = p["X"], p["Y"], p["kw"]
    w = w if weighted else None
    N = X.shape[0]
    with open_stream(kernel, kw, XL, 3, weighted) as one:
        whole = results(feed(one, X, Y, w, (N,)))
        assert same(whole, results(one))  # a solve and an export leave the state as it was
        assert one.num_points == N and one.info["pending"] == N % SLAB
    for cuts in (CUTS, (1,) * N, (256, 256, 265), (255, 2, 520)):
        with open_stream(kernel, kw, XL, 3, weighted) as cut:
            assert same(whole, results(feed(cut, X, Y, w, cuts))), (cuts[:4],)
    # update -> solve -> update -> solve: the second solve has the bits of update -> update -> solve
    with open_stream(kernel, kw, XL, 3, weighted) as twice:
        feed(twice, X[:300], Y[:, :300], None if w is None else w[:300], (300,))
        first = results(twice)
        assert not same(first, whole)
        feed(twice, X[300:], Y[:, 300:], None if w is None else w[300:], (N - 300,))
        assert same(whole, results(twice))
    # another slab size is another order of the sums: close, and in general not the same bits -- while S~[m][m] is N either way
    m = XL.shape[0]
    if not weighted:
        assert whole[0][m, m] == N


@pytest.mark.parametrize("factor", ["host", "device"])
@pytest.mark.parametrize("kernel, dtype", [("rbf", np.float32), ("polynomial", np.float64)])
def test_columns_costs_and_unit_weights_are_bit_equal(kernel, dtype, factor):
    p, w, XL = cut_case(kernel, dtype)
    X, Y, kw = p["X"], p["Y"], p["kw"]
    N = X.shape[0]
    with open_stream(kernel, kw, XL, 3, True) as stream:
        feed(stream, X, Y, w, CUTS)
        betas, rhos, infos = stream.solve(COSTS, factor=factor)
        h, f, loo = stream.loo(X, Y, w)
        assert [i["cost"] for i in infos] == list(COSTS) and all(i["jitter"] > 0.0 for i in infos)
        for s, cost in enumerate(COSTS):  # a cost of a grid: the bits of the one-cost solve
            b1, r1, _ = stream.solve([cost], factor=factor)
            h1, f1, l1 = stream.loo(X, Y, w)
            assert np.array_equal(b1[0], betas[s]) and np.array_equal(r1[0], rhos[s])
            assert np.array_equal(h1[0], h[s]) and np.array_equal(f1[0], f[s]) and np.array_equal(l1[0], loo[s])
    for c in range(3):  # column c: the bits of the single-column stream; h does not depend on k
        with open_stream(kernel, kw, XL, 1, True) as single:
            feed(single, X, Y[c:c + 1], w, CUTS)
            b1, r1, _ = single.solve(COSTS, factor=factor)
            h1, f1, l1 = single.loo(X, Y[c], w)
            assert np.array_equal(b1[:, 0], betas[:, c]) and np.array_equal(r1[:, 0], rhos[:, c])
            assert np.array_equal(h1, h) and np.array_equal(f1[:, 0], f[:, c]) and np.array_equal(l1[:, 0], loo[:, c])
    # weights of 1.0 (given, and NULL on a weighted stream) against the unweighted stream
    with open_stream(kernel, kw, XL, 3, False) as plain:
        ref = results(feed(plain, X, Y, None, CUTS), (factor,)) + list(plain.loo(X, Y))
    for ones in (np.ones(N), None):
        with open_stream(kernel, kw, XL, 3, True) as unit:
            got = results(feed(unit, X, Y, ones, CUTS), (factor,)) + list(unit.loo(X, Y, ones))
        assert same(ref, got)


# ---------------------------------------------------------------- the Gram operator ----------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kernel, dtype", [("rbf", np.float64), ("rbf", np.float32), ("polynomial", np.float64), ("polynomial", np.float32)])
def test_exported_gram_against_numpy_on_the_device_phi(kernel, dtype, weighted):
    p, w, XL = cut_case(kernel, dtype)
    X, Y = p["X"], p["Y"]
    N, m = X.shape[0], XL.shape[0]
    w = w if weighted else None
    with open_stream(kernel, p["kw"], XL, 3, weighted) as stream:
        Phi_dev = stream.phi(X)
        state = feed(stream, X, Y, w, CUTS).export_state()
    P = np.hstack([Phi_dev, np.ones((N, 1)), Y.astype(np.float64).T])
    wv = np.ones(N) if w is None else w
    ref = P.T @ (wv[:, None] * P)
    bound = 2.0 * (N + (4 if weighted else 0)) * EPS64 * (np.abs(P).T @ (wv[:, None] * np.abs(P)))
    G = state["gram"]
    ratio = float(np.max(np.abs(G - ref) / bound))
    print(f"stream gram {kernel} {np.dtype(dtype).name} weighted={weighted}: largest error / bound {ratio:.3f}")
    assert np.array_equal(G, G.T) and ratio <= 1.0 and state["num_points"] == N
    if not weighted:
        assert G[m, m] == N


# ---------------------------------------------------------------- fits and scores ----------------------------------------------------------------
FIT_ROWS = {"rbf_777x5_g0.05": (777, 5, "rbf", dict(gamma=0.05)), "rbf_777x5_g0.2": (777, 5, "rbf", dict(gamma=0.2)), "rbf_777x5_g0.8": (777, 5, "rbf", dict(gamma=0.8)),
            "poly_777x16": (777, 16, "polynomial", dict(gamma=1.0 / 16, coef0=1.0, degree=3)), "rbf_255x5": (255, 5, "rbf", dict(gamma=0.2))}
FIT_RANK = 64


@functools.lru_cache(maxsize=None)
def fit_reference(name, dtype, weighted, foreign_landmarks=False):
    """(case, [model per cost], [e_loo per cost]): float64 numpy on the staged rows, once per case, shared, never modified."""
    N, d, kernel, own_kw = FIT_ROWS[name]
    X, y = pm.make_data(N, d, pm.DATA_SEED, dtype)
    rng = np.random.default_rng(23)
    Y = np.stack([y] + [np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(dtype) for _ in range(2)])
    kw = rm.rounded_parameters(dtype, **own_kw)
    w = wm.make_weights(N, large=(64.0,)) if weighted else None
    if foreign_landmarks:
        XL = pm.make_data(FIT_RANK, d, pm.DATA_SEED + 5, dtype)[0]
    else:
        lms = pm.draw_landmarks(N, FIT_RANK, pm.LANDMARK_SEED)
        XL = np.ascontiguousarray(X[lms.astype(np.int64)])
    centre = sm.centre_of(kernel, XL)
    Xh, XLh = sm.held(X, centre), sm.held(XL, centre)
    if foreign_landmarks:
        Xm, Ym, wm_, lms = sm.with_landmark_rows(Xh, Y, w, XLh)
    else:
        Xm, Ym, wm_ = Xh, Y.astype(np.float64), w
    models, es = [], []
    for cost in COSTS:
        if wm_ is None:
            cell = lm.LooModel(kernel, Xm, Ym, cost, lms, held=(Xm, kw), **kw)
            e = lm.e_loo(cell, lm.stable(kernel, Xm, Ym, cost, lms, held=(Xm, kw), **kw)[2])
        else:
            cell = wm.WeightedLooModel(kernel, Xm, Ym, cost, lms, wm_, held=(Xm, kw), **kw)
            e = wm.e_loo(cell, wm.stable(kernel, Xm, Ym, cost, lms, wm_, held=(Xm, kw), **kw)[2])
        for a in (cell.h, cell.f, cell.loo, cell.betas, cell.rhos):
            a.setflags(write=False)
        models.append(cell)
        es.append(e)
    Phi_held = pm.kernel_matrix(kernel, Xh, XLh, **kw)
    for a in (X, Y, XL, Phi_held, centre):
        a.setflags(write=False)
    return dict(X=X, Y=Y, w=w, XL=XL, kernel=kernel, kw=kw, centre=centre, Phi=Phi_held, N=N), models, es


def check_fit(tag, p, models, es, factor):
    N, X, Y, w = p["N"], p["X"], p["Y"], p["w"]
    worst = 0.0
    with open_stream(p["kernel"], p["kw"], p["XL"], 3, w is not None) as stream:
        assert np.array_equal(stream.centre, p["centre"])
        feed(stream, X, Y, w, (1, 127, 129, N - 257) if N > 257 else (1, 127, N - 128))
        betas, rhos, infos = stream.solve(COSTS, factor=factor)
        assert betas.shape == (2, 3, FIT_RANK) and rhos.shape == (2, 3)
        h, f, loo = np.zeros((2, N)), np.zeros((2, 3, N)), np.zeros((2, 3, N))
        at = 0
        for n in (130, 1, N - 131):  # the second walk, in other chunks than the first
            hh, ff, ll = stream.loo(X[at:at + n], Y[:, at:at + n], None if w is None else w[at:at + n])
            h[:, at:at + n], f[:, :, at:at + n], loo[:, :, at:at + n] = hh, ff, ll
            at += n
        whole = stream.loo(X, Y, w)
        assert np.array_equal(h, whole[0]) and np.array_equal(f, whole[1]) and np.array_equal(loo, whole[2])  # a row's scores do not depend on its chunk
    for s, cost in enumerate(COSTS):
        cell, e = models[s], es[s]
        for what, got, ref in (("h", h[s], cell.h[:N]), ("f", f[s], cell.f[:, :N]), ("loo", loo[s], cell.loo[:, :N])):
            tol = lm.tolerance(cell, e, np.max(np.abs(ref)))
            diff = float(np.max(np.abs(got - ref)))
            worst = max(worst, diff / tol)
            print(f"stream fit {tag} {factor} C={cost:g} {what}: |device - model| {diff:.2e}, tolerance {tol:.2e} (e_loo {e:.1e}, cond(M) eps64 {cell.cond * EPS64:.1e})")
            assert diff <= tol, (tag, factor, s, what, diff, tol)
        # the coefficients through the decision function they stand for (rho does not enter the fitted values): B Phi^T - rho in numpy on the staged rows
        f_coef = betas[s] @ p["Phi"].T - rhos[s][:, None]
        tol = rm.fit_tolerance(cell, e, cell.f[:, :N])
        diff = float(np.max(np.abs(f_coef - cell.f[:, :N])))
        worst = max(worst, diff / tol)
        print(f"stream fit {tag} {factor} C={cost:g} f from betas and rhos: |device - model| {diff:.2e}, tolerance {tol:.2e}; |betas - model's| "
              f"{np.max(np.abs(betas[s] - cell.betas)):.2e} of {np.max(np.abs(cell.betas)):.2e}, |rhos - model's| {np.max(np.abs(rhos[s] - cell.rhos)):.2e}")
        assert diff <= tol, (tag, factor, s, diff, tol)
        if w is not None:  # a row of weight 0 is a held-out point: leverage 0, loo = the fitted value itself
            out = w == 0.0
            assert np.all(h[s][out] == 0.0) and np.array_equal(loo[s][:, out], f[s][:, out])
    return worst


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(FIT_ROWS))
def test_fits_and_scores_against_the_model(name, dtype, weighted):
    p, models, es = fit_reference(name, dtype, weighted)
    worst = max(check_fit(f"{name} {np.dtype(dtype).name} w={weighted}", p, models, es, factor) for factor in ("host", "device"))
    print(f"stream fit {name} {np.dtype(dtype).name} w={weighted}: largest |device - model| / tolerance {worst:.3f}")


@pytest.mark.parametrize("weighted", [False, True])
def test_landmarks_that_are_not_among_the_streamed_rows(weighted):
    p, models, es = fit_reference("rbf_777x5_g0.2", np.float64, weighted, True)
    worst = max(check_fit(f"foreign landmarks w={weighted}", p, models, es, factor) for factor in ("host", "device"))
    print(f"stream fit, landmarks not among the rows, w={weighted}: largest |device - model| / tolerance {worst:.3f}")


# ---------------------------------------------------------------- merge ----------------------------------------------------------------
@pytest.mark.parametrize("kernel, dtype", [("rbf", np.float64), ("polynomial", np.float32)])
def test_merged_shard_streams_agree_with_the_single_stream(kernel, dtype):
    p, w, XL = cut_case(kernel, dtype)
    X, Y, kw = p["X"], p["Y"], p["kw"]
    N, m = X.shape[0], XL.shape[0]
    with open_stream(kernel, kw, XL, 3, True) as one:
        Phi_dev = one.phi(X)
        single = feed(one, X, Y, w, (N,)).export_state()
    P = np.hstack([Phi_dev, np.ones((N, 1)), Y.astype(np.float64).T])
    bound = 2.0 * (N + 4) * EPS64 * (np.abs(P).T @ (w[:, None] * np.abs(P)))
    for shards in (2, 3):
        edges = np.linspace(0, N, shards + 1).astype(int)
        states = []
        for a, b in zip(edges[:-1], edges[1:]):
            with open_stream(kernel, kw, XL, 3, True) as shard:
                states.append(shard.update(X[a:b], Y[:, a:b], w[a:b]).export_state())
        merged = []
        for _ in range(2):
            with open_stream(kernel, kw, XL, 3, True) as root:
                for st in states:
                    root.merge(st)
                assert root.num_points == N and root.info["pending"] == 0
                merged.append(results(root))
        assert same(merged[0], merged[1])  # the same merge order: the same bits
        ratio = float(np.max(np.abs(merged[0][0] - single["gram"]) / bound))
        print(f"merge of {shards} shards {kernel} {np.dtype(dtype).name}: |merged - single| / bound {ratio:.3f}")
        assert ratio <= 1.0
        # rank 0 streams its own shard and merges the others: its pending rows stay pending and are summed behind the merged part
        a, b = edges[0], edges[1]
        with open_stream(kernel, kw, XL, 3, True) as root:
            root.update(X[a:b], Y[:, a:b], w[a:b])
            pending = root.info["pending"]
            for st in states[1:]:
                root.merge(st)
            assert root.info["pending"] == pending and root.num_points == N
            G = root.export_state()["gram"]
        assert float(np.max(np.abs(G - single["gram"]) / bound)) <= 1.0


def test_a_foreign_fingerprint_is_refused():
    p, w, XL = cut_case("rbf", np.float64)
    X, Y, kw = p["X"], p["Y"], p["kw"]
    with open_stream("rbf", kw, XL, 3) as stream:
        state = stream.update(X[:100], Y[:, :100]).export_state()
        other = XL.copy()
        other[0, 0] += 1.0
        for foreign in (open_stream("rbf", dict(kw, gamma=2.0 * kw["gamma"]), XL, 3), open_stream("rbf", kw, other, 3), open_stream("rbf", kw, XL.astype(np.float32), 3),
                        open_stream("rbf", kw, XL[:-1], 3)):
            with foreign:
                if foreign.rank != stream.rank:
                    with pytest.raises(InvalidParameterError):
                        foreign.merge(state)
                    continue
                with pytest.raises(InvalidParameterError, match="fingerprint"):
                    foreign.merge(state)
                assert foreign.num_points == 0
        with open_stream("rbf", kw, XL, 3, slab_rows=512) as twin:  # the slab size and the weighted flag are no part of the fingerprint
            assert twin.merge(state).num_points == 100


# ---------------------------------------------------------------- the surface ----------------------------------------------------------------
EPS32 = rm.EPS32
SURFACE_COSTS = (1.0, 10.0)


@functools.lru_cache(maxsize=None)
def surface_reference(classes, dtype, balanced=False):
    """Blobs with unequal class counts, in three chunks; the numpy models per cost on the staged rows (the weighted sibling model: ones, or the balanced class weights)."""
    X, labels = rm.blobs(2000, 8, classes, seed=31, dtype=dtype)
    keep = (labels != 0) | (np.arange(2000) % 2 == 0)  # half of class 0 goes: the classes are not balanced
    X, labels = np.ascontiguousarray(X[keep]), labels[keep]
    N = X.shape[0]
    kw = rm.rounded_parameters(dtype, gamma=1.0 / 8)
    lms = pm.draw_landmarks(N, 64, pm.LANDMARK_SEED)
    XL, yL = np.ascontiguousarray(X[lms.astype(np.int64)]), labels[lms.astype(np.int64)]
    assert set(yL.tolist()) == set(range(classes))
    Y = np.where(labels[None, :] == np.arange(classes)[:, None], 1.0, -1.0)
    if classes == 2:
        Y = Y[1:]
    counts = np.array([np.count_nonzero(labels == c) for c in range(classes)], dtype=np.float64)
    cw = N / (classes * counts) if balanced else np.ones(classes)
    w = cw[labels]
    centre = sm.centre_of("rbf", XL)
    Xh = sm.held(X, centre)
    models, fs, tols = [], [], []
    for cost in SURFACE_COSTS:
        model = wm.WeightedReducedModel("rbf", Xh, Y, cost, lms, w, held=(Xh, kw), **kw)
        e = wm.e_model("rbf", Xh, Y, cost, lms, w, Xh, held=(Xh, kw), **kw)
        f = model.decision_values(Xh)
        models.append(model), fs.append(f), tols.append(rm.fit_tolerance(model, e, f))
    edges = (0, 700, 701, N)
    chunks = [(X[a:b], labels[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    return dict(X=X, labels=labels, XL=XL, yL=yL, kw=kw, Y=Y, w=w, cw=cw, chunks=chunks, models=models, f=fs, tol=tols, N=N)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_csvm_fit_reduced_stream_saves_loads_and_predicts(dtype, tmp_path):
    r = surface_reference(2, dtype)
    X, labels, N = r["X"], r["labels"], r["N"]
    landmarks = DataSet(r["XL"], r["yL"].tolist(), real_type=dtype)
    chunks = [DataSet(*r["chunks"][0][:1], r["chunks"][0][1].tolist(), real_type=dtype)] + r["chunks"][1:]  # a DataSet and (X, y) pairs alike
    svm = MI355CSVM(kernel_type="rbf", cost=10.0, gamma=1.0 / 8)
    models, report = svm.fit_reduced_stream(landmarks, chunks, costs=SURFACE_COSTS, loo=True)
    assert len(models) == 2 and report["press"].shape == report["loo_errors"].shape == report["loo_accuracy"].shape == report["max_leverage"].shape == report["jitter"].shape == (2,)
    assert report["num_points"] == N and np.all(report["loo_accuracy"] >= 0.97) and np.all(report["max_leverage"] < 1.0) and [i["iterations"] for i in svm.last_cg_info] == [0, 0]
    one = svm.fit_reduced_stream(landmarks, chunks)  # this object's cost, no second walk: the model of that cost
    assert np.array_equal(one.alpha, models[1].alpha) and one.rho == models[1].rho and one.params.cost == 10.0
    for device in ("host", "device"):
        assert svm.fit_reduced_stream(landmarks, iter(chunks), factor=device).num_support_vectors() == 64  # (one walk: an iterator serves)
    with pytest.raises(InvalidParameterError, match="second walk"):
        svm.fit_reduced_stream(landmarks, iter(chunks), costs=SURFACE_COSTS, loo=True)
    with pytest.raises(InvalidParameterError, match="label"):
        svm.fit_reduced_stream(landmarks, [(X[:10], np.full(10, 7))])
    # the fitted values of the call: the same stream by hand
    Y = r["Y"].astype(dtype)
    with backend.ReducedStream(base.parameter("rbf", r["kw"], 1.0), r["XL"]) as stream:
        for Xc, yc in r["chunks"]:
            stream.update(Xc, np.where(yc == 1, 1.0, -1.0).astype(dtype))
        betas, rhos, _ = stream.solve(SURFACE_COSTS)
        h, fitted, loo = stream.loo(X, Y)
        centre = stream.centre
    data = DataSet(X, labels.tolist(), real_type=dtype)
    for s, model in enumerate(models):
        assert model.num_support_vectors() == 64 and np.array_equal(model.support_vectors(), r["XL"]) and model.alpha.dtype == np.dtype(dtype) and model.params.cost == SURFACE_COSTS[s]
        assert np.array_equal(model.alpha, betas[s, 0].astype(dtype)) and model.rho == np.dtype(dtype).type(rhos[s, 0])
        assert report["loo_errors"][s] == lm.errors_of(Y, loo[s])[0] and report["press"][s] == grid.sequential_press(Y[0], loo[s, 0])
        path = tmp_path / f"stream{s}.model"
        model.save(str(path))
        loaded = Model.load(str(path), real_type=dtype, label_type=int)
        assert loaded.num_support_vectors() == 64
        ref = r["models"][s]
        slack = r["tol"][s] + (16 * EPS32 * float(np.max(rm.summand_scale("rbf", ref.X_L, ref.betas, ref.rhos, sm.held(X, centre), **ref.kw))) if dtype == np.float32 else 0.0)
        values, _ = svm.predict_values(model.params, model.support_vectors(), model.alpha, float(model.rho), None, X)
        diff = float(np.max(np.abs(np.asarray(values, dtype=np.float64) - fitted[s, 0])))
        print(f"stream surface {np.dtype(dtype).name} C={SURFACE_COSTS[s]:g}: |decision values - fitted| {diff:.2e}, tolerance {slack:.2e}; against the numpy model "
              f"{np.max(np.abs(fitted[s, 0] - r['f'][s][0])):.2e}")
        assert diff <= slack and float(np.max(np.abs(fitted[s, 0] - r["f"][s][0]))) <= r["tol"][s]
        clear = np.abs(r["f"][s][0]) > slack
        assert np.mean(~clear) <= 0.01
        for m in (model, loaded):
            assert np.array_equal(np.array(svm.predict(m, data))[clear], (r["f"][s][0] > 0).astype(int)[clear])


@pytest.mark.parametrize("class_weight", [None, "balanced"])
@pytest.mark.parametrize("classes", [2, 3])
def test_svc_fit_reduced_stream(classes, class_weight):
    r = surface_reference(classes, np.float64, class_weight == "balanced")
    X, labels, N, k = r["X"], r["labels"], r["N"], 1 if classes == 2 else classes
    est = svc.SVC(kernel="rbf", C=10.0, gamma=1.0 / 8, class_weight=class_weight)
    scores, clones = svc.fit_reduced_stream(est, r["chunks"], (r["XL"], r["yL"]), np.arange(classes), Cs=SURFACE_COSTS)
    fitted = svc.fit_reduced_stream(est, r["chunks"], (r["XL"], r["yL"]), np.arange(classes))
    assert est._fit is None and np.array_equal(fitted.dual_coef_, clones[1].dual_coef_) and np.array_equal(fitted.intercept_, clones[1].intercept_)
    assert scores.shape == (2,) and np.all(scores >= 0.97)
    # the same stream by hand: the (weighted) leave-one-out accuracy from its own leave-one-out values
    weighted = class_weight is not None
    with backend.ReducedStream(base.parameter("rbf", r["kw"], 1.0), r["XL"], num_rhs=k, weighted=weighted) as stream:
        stream.update(X, r["Y"], r["w"] if weighted else None)
        stream.solve(SURFACE_COSTS)
        _, _, loo = stream.loo(X, r["Y"], r["w"] if weighted else None)
    for s, clone in enumerate(clones):
        assert clone.C == SURFACE_COSTS[s] and clone.dual_coef_.shape == (k, 64) and np.array_equal(clone.classes_, np.arange(classes)) and np.all(np.asarray(clone.n_iter_) == 0)
        assert np.allclose(clone.class_weight_, r["cw"], rtol=1e-15, atol=0.0) and np.array_equal(clone.support_vectors_, r["XL"]) and clone.shape_fit_ == (N, 8)
        right = np.sign(loo[s, 0]) == np.sign(r["Y"][0]) if classes == 2 else np.argmax(loo[s], axis=0) == labels
        assert abs(scores[s] - float(np.average(right, weights=r["w"]))) <= 1e-12
        f, tol = r["f"][s], r["tol"][s]
        values = np.asarray(clone.decision_function(X))
        diff = float(np.max(np.abs((values if classes > 2 else values[:, None]) - f.T)))
        print(f"svc stream classes={classes} class_weight={class_weight} C={SURFACE_COSTS[s]:g}: |decision_function - model| {diff:.2e}, tolerance {tol:.2e}")
        assert diff <= tol
        predicted = clone.predict(X)
        if classes == 2:
            clear, expected = np.abs(f[0]) > tol, (f[0] > 0).astype(int)
        else:
            top = np.sort(f, axis=0)
            clear, expected = top[-1] - top[-2] > 2 * tol, np.argmax(f, axis=0)
        assert np.mean(~clear) <= 0.01 and np.array_equal(predicted[clear], expected[clear])
    with pytest.raises(InvalidParameterError, match="re-iterable"):
        svc.fit_reduced_stream(est, iter(r["chunks"]), (r["XL"], r["yL"]), np.arange(classes))
    if classes == 2:
        with pytest.raises(InvalidParameterError, match="labels"):
            svc.fit_reduced_stream(est, r["chunks"], r["XL"], np.arange(classes))


# ---------------------------------------------------------------- the refusals that need a device ----------------------------------------------------------------
def test_refusals_on_a_stream():
    p, w, XL = cut_case("rbf", np.float64)
    X, Y, kw = p["X"], p["Y"], p["kw"]
    with open_stream("rbf", kw, XL, 3) as stream:
        with pytest.raises(InvalidParameterError, match="no rows"):
            stream.solve([1.0])
        with pytest.raises(InvalidParameterError, match="without weights"):
            stream.update(X[:10], Y[:, :10], np.ones(10))
        with pytest.raises(InvalidParameterError, match="at least 1 row"):
            stream.update(X[:0], Y[:, :0])
        with pytest.raises(InvalidParameterError, match="shape"):
            stream.update(X[:10], Y[:2, :10])
        with pytest.raises(InvalidParameterError, match="features"):
            stream.update(X[:10, :3], Y[:, :10])
        assert stream.num_points == 0
        stream.update(X[:300], Y[:, :300])
        with pytest.raises(InvalidParameterError, match="needs a solve"):
            stream.loo(X[:10], Y[:, :10])
        for costs in ([0.0], [-1.0], [float("nan")], [float("inf")], [], [1.0] * 65):
            with pytest.raises(InvalidParameterError, match="cost"):
                stream.solve(costs)
        with pytest.raises(InvalidParameterError, match="factor"):
            stream.solve([1.0], factor="gpu")
        stream.solve([1.0])
        stream.loo(X[:10], Y[:, :10])
        stream.update(X[300:310], Y[:, 300:310])
        with pytest.raises(InvalidParameterError, match="needs a solve"):  # an update followed the solve
            stream.loo(X[:10], Y[:, :10])
        assert stream.num_points == 310
    with open_stream("rbf", kw, XL, 3, True) as stream:
        for bad in (-1.0, float("nan"), float("inf")):
            wbad = np.ones(10)
            wbad[3] = bad
            with pytest.raises(InvalidParameterError, match="weight"):
                stream.update(X[:10], Y[:, :10], wbad)
        stream.update(X[:10], Y[:, :10], np.zeros(10))
        with pytest.raises(InvalidParameterError, match="sum greater than 0"):
            stream.solve([1.0])
