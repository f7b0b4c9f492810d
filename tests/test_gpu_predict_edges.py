"""The predict paths at their data-dependent edges: `predict_values` (the one-shot call), the resident predictor (`backend.Predictor`) and `MI355CSVM.predict` on top of
it, compared with each other and with the float64 oracle at every decision they make per batch -- f16x3 or bf16x6 planes, resident or one-shot, folded or unfolded rbf
records, the 256-row or the 128-row kernels, the run-time integer power (polynomial degree <= 0 included) -- and the cached predictor of `MI355CSVM.predict` after the
model or the options change.  The bar is the suite's fp32 bar: 16 eps of a point's summands, sum_j |alpha_j| |K_ij| + |rho|."""

import numpy as np
import pytest

from plssvm_amd import _capi, backend
from plssvm_amd._capi import Options
from plssvm_amd.csvm import make_csvm
from plssvm_amd.data_set import DataSet
from plssvm_amd.datagen import make_blobs_pm1
from plssvm_amd.model import Model
from plssvm_amd.parameter import Parameter

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
LOG2E = 1.4426950408889634
# the constants of the representability check (plssvm_amd/csrc/lssvm_problem.hip.hpp)
F16_REL2_MAX = 2.0 ** -44
F16_ABS_MAX = 2.0 ** -22
F16_RBF_SHIFT = 6
F16_TARGET_EXP = 14
F16_MAX_SHIFT = 40
RBF_DIRECT_ABOVE = 32.0


# ------------------------------------------------------------------------------------------------------------ a host model of the f16 split
def rbf_prescale(gamma):
    """sqrt(2 gamma log2 e) in fp32, from gamma as the library holds it (fp32)"""
    return np.float32(np.sqrt(2.0 * float(np.float32(gamma)) * LOG2E))


def sv_mean(S):
    """the support vectors' column means (k_colsum_*: a double sum, rounded to fp32)"""
    return (S.astype(np.float64).sum(axis=0) / S.shape[0]).astype(np.float32)


def centred(M, mean, scale):
    """k_center: (x - mean) * scale in fp32"""
    return ((M.astype(np.float32) - mean) * np.float32(scale)).astype(np.float32)


def poly_shift(amax):
    """make_planes, linear / polynomial: the power of two that moves the largest entry to [2^14, 2^15)"""
    return int(min(max(F16_TARGET_EXP - (np.frexp(np.float32(amax))[1] - 1), -F16_MAX_SHIFT), F16_MAX_SHIFT))


def split_f16x2(Y, scale=1.0, shift=0):
    """numpy restatement of k_split_f16x2 (tile_launch_f32h.hip): the planes of `scale` * Y -- shift 0: (hi, mid), shift s: the rbf planes (2^-s hi, 2^s mid, 2^s hi) --
    and the statistics the check reads: rel2 = max over the rows of |rest|^2 / |y|^2, rest2 = max |rest|^2, x2 = max |y|^2 (rel2 NaN where a plane overflows)"""
    with np.errstate(over="ignore", invalid="ignore"):
        y = (np.asarray(Y, dtype=np.float32) * np.float32(scale)).astype(np.float32)
        up, down = np.float32(2.0 ** shift), np.float32(2.0 ** -shift)
        p0 = (y * down).astype(np.float16)
        hi = p0.astype(np.float32) * up
        r1 = y - hi
        p1 = (r1 * up).astype(np.float16)
        rest = r1 - p1.astype(np.float32) * down
        sr = np.einsum("ij,ij->i", rest.astype(np.float64), rest.astype(np.float64))
        sx = np.einsum("ij,ij->i", y.astype(np.float64), y.astype(np.float64))
        overflow = shift != 0 and not np.all(np.abs(hi * up) <= 65504.0)
    rows = (sx > 0) | np.isnan(sr)
    rel2 = float(np.max(sr[rows] / sx[rows])) if rows.any() else 0.0
    return {"rel2": float("nan") if overflow else rel2, "rest2": float(np.max(sr)), "x2": float(np.max(sx))}


def both(a, b):
    """the statistics of one `stats` buffer that both sides were split into (make_planes with M2)"""
    return {k: max(a[k], b[k]) for k in a}


def abs_bound(st):
    """the rbf fallback criterion's quantity, 2 max|rest| max|x| (accepted up to F16_ABS_MAX)"""
    return 2.0 * np.sqrt(st["rest2"] * st["x2"])


def passes(st, rbf):
    """the check of make_planes: row-relative, else (rbf) the absolute bound"""
    return st["rel2"] <= F16_REL2_MAX or (rbf and np.isfinite(st["rel2"]) and abs_bound(st) <= F16_ABS_MAX)


def rbf_stats(sv, pts, gamma):
    """the statistics of each side as the one-shot call splits them: centred at the support vectors' mean, prescaled, the shifted planes"""
    mean, pre = sv_mean(sv), rbf_prescale(gamma)
    return split_f16x2(centred(sv, mean, pre), shift=F16_RBF_SHIFT), split_f16x2(centred(pts, mean, pre), shift=F16_RBF_SHIFT)


def exponent_scale(sv, pts, gamma):
    """2 gamma log2(e) max |x - mean|^2 over both sides (mean: the support vectors')"""
    mean = sv_mean(sv).astype(np.float64)
    sq = max(float(np.max(np.sum((M.astype(np.float64) - mean) ** 2, axis=1))) for M in (sv, pts))
    return 2.0 * float(np.float32(gamma)) * LOG2E * sq


# ------------------------------------------------------------------------------------------------------------ comparisons
def kernel_matrix(kernel, pts, sv, degree, gamma, coef0):
    P, S = pts.astype(np.float64), sv.astype(np.float64)
    if kernel == "rbf":
        sq = np.sum(P * P, axis=1)[:, None] + np.sum(S * S, axis=1)[None, :] - 2.0 * (P @ S.T)
        return np.exp(-gamma * np.maximum(sq, 0.0))
    return (gamma * (P @ S.T) + coef0) ** degree


def summand_scale(kernel, pts, sv, alpha, rho, degree=3, gamma=1.0, coef0=0.0):
    """sum_j |alpha_j| |K_ij| + |rho| for every point"""
    out = np.empty(pts.shape[0])
    for b in range(0, pts.shape[0], 2048):
        out[b:b + 2048] = np.abs(kernel_matrix(kernel, pts[b:b + 2048], sv, degree, gamma, coef0)) @ np.abs(alpha.astype(np.float64)) + abs(float(rho))
    return out


def eps_of(got, want, scale):
    """the largest distance in eps of the summands' scale (inf for a non-finite value)"""
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float(np.max(np.abs(got.astype(np.float64) - want) / scale)) / EPS32


def three_way(oracle, kernel, sv, alpha, rho, pts, options=None, degree=3, gamma=1.0, coef0=0.0, bar=16.0):
    """the resident predictor, the one-shot call and the float64 oracle on one batch; both GPU paths within `bar` eps of float64.
    Returns (resident values, one-shot values, resident info, one-shot info, resident eps, one-shot eps)."""
    prm = Parameter(kernel_type=kernel, degree=degree, gamma=gamma, coef0=coef0)
    kw = dict(degree=degree, gamma=float(np.float32(gamma)), coef0=coef0)
    info, info1 = {}, {}
    with backend.Predictor(prm, sv, alpha, rho, options=options) as pred:
        got = pred.predict(pts, info_out=info)
    one, _ = backend.predict_values(prm, sv, alpha, rho, None, pts, options=options, info_out=info1)
    want, _ = oracle.predict_values(kernel, sv.astype(np.float64), alpha.astype(np.float64), float(rho), pts.astype(np.float64), **kw)
    scale = summand_scale(kernel, pts, sv, alpha, rho, **kw)
    e_res, e_one = eps_of(got, want, scale), eps_of(one, want, scale)
    assert e_res < bar and e_one < bar, (e_res, e_one, info, info1)
    assert info["gram_mode"] == info1["gram_mode"] and info["rbf_direct"] == info1["rbf_direct"], (info, info1)
    # (both: 2 gamma log2(e) max centred |x|^2 against the support vectors' mean, in the same order of operations)
    assert info["rbf_exponent_scale"] == info1["rbf_exponent_scale"], (info, info1)
    return got, one, info, info1, e_res, e_one


# ------------------------------------------------------------------------------------------------------------ A. the f16 check over both sides
def _shell(rng, n, d, norm):
    u = rng.standard_normal((n, d))
    return (u / np.linalg.norm(u, axis=1, keepdims=True) * norm).astype(np.float32)


def _cross_term_data(reverse):
    """rbf data (d = 64, prescale exactly 1) on which the support vectors alone and the batch alone pass the representability check and the pair does not: one side holds
    small rows (norm 0.5) and two rows near the mean (norm 2^-10: their mid plane is subnormal, the row-relative test fails, the absolute one passes), the other side rows
    eight times larger (norm 4: the row-relative test passes).  Together the row-relative test fails (the near-mean rows) and so does the absolute one (the large rows'
    rest times their norm).  Forward: the near-mean rows among the support vectors; reverse: in the batch.  The support vectors come in +- pairs (mean 0)."""
    rng = np.random.default_rng(31 + int(reverse))
    d = 64
    small, near, large = _shell(rng, 150, d, 0.5), _shell(rng, 2, d, 2.0 ** -10), _shell(rng, 150, d, 4.0)
    if not reverse:
        sv, pts = np.concatenate([small, -small, near, -near]), large
    else:
        sv, pts = np.concatenate([large, -large]), np.concatenate([small, near])
    gamma = float(np.float32(0.5 / LOG2E))
    assert rbf_prescale(gamma) == 1.0
    alpha = rng.standard_normal(sv.shape[0]).astype(np.float32)
    return sv, pts, alpha, gamma


def test_host_model_of_the_f16_split_matches_the_device():
    """The host model's sqrt(max rel2) over both sides is what predict_values reports as f16_row_rel_error (within 16 ulp): the host-side construction of the cases
    below is then the library's own view of the data."""
    for reverse in (False, True):
        sv, pts, alpha, gamma = _cross_term_data(reverse)
        st_s, st_p = rbf_stats(sv, pts, gamma)
        info = {}
        backend.predict_values(Parameter(kernel_type="rbf", gamma=gamma), sv, alpha, 0.0, None, pts, info_out=info)
        host = np.sqrt(both(st_s, st_p)["rel2"])
        assert abs(info["f16_row_rel_error"] - host) <= 16 * EPS32 * host, (reverse, info["f16_row_rel_error"], host)
    # blobs, polynomial: the planes of 2^shift x with the shift of both sides
    X, _ = make_blobs_pm1(700, 100, seed=3, dtype=np.float32)
    sv, pts = X[:400], X[400:]
    shift = poly_shift(max(np.abs(sv).max(), np.abs(pts).max()))
    host = np.sqrt(both(split_f16x2(sv, 2.0 ** shift), split_f16x2(pts, 2.0 ** shift))["rel2"])
    info = {}
    backend.predict_values(Parameter(kernel_type="polynomial", degree=3, gamma=0.01, coef0=1.0), sv, np.ones(400, np.float32), 0.0, None, pts, info_out=info)
    assert info["gram_mode"] == 2 and abs(info["f16_row_rel_error"] - host) <= 16 * EPS32 * host, (info, host)


@pytest.mark.parametrize("reverse", [False, True], ids=["near_mean_rows_in_the_support_vectors", "near_mean_rows_in_the_batch"])
def test_resident_predictor_applies_the_f16_check_to_both_sides(oracle, reverse):
    """The resident predictor's f16 check must judge the support vectors and the batch together, as make_planes does for the one-shot call: the batch (forward) or the
    support vectors (reverse) alone pass, the pair does not -- the one-shot call runs bf16x6, and the resident predictor must hand the batch to it (same bits, same
    gram_mode, resident = 0).  A batch that passes together with the support vectors stays resident on f16x3 with the same bits."""
    sv, pts, alpha, gamma = _cross_term_data(reverse)
    st_s, st_p = rbf_stats(sv, pts, gamma)
    one_side, other = (st_s, st_p) if not reverse else (st_p, st_s)
    # (i) the side with the near-mean rows fails the row-relative test and passes the absolute one, (ii) the other side passes, (iii) the pair fails -- margins of 2x
    assert np.sqrt(one_side["rel2"]) >= 2 * 2.0 ** -22 and abs_bound(one_side) <= F16_ABS_MAX / 2, one_side
    assert np.sqrt(other["rel2"]) <= 2.0 ** -22 / 2, other
    pair = both(st_s, st_p)
    assert np.sqrt(pair["rel2"]) >= 2 * 2.0 ** -22 and abs_bound(pair) >= 2 * F16_ABS_MAX, pair
    assert exponent_scale(sv, pts, gamma) <= RBF_DIRECT_ABOVE  # the norm expansion, on both paths
    prm = Parameter(kernel_type="rbf", gamma=gamma)
    info, info1 = {}, {}
    with backend.Predictor(prm, sv, alpha, 0.125) as pred:
        got = pred.predict(pts, info_out=info)
    one, _ = backend.predict_values(prm, sv, alpha, 0.125, None, pts, info_out=info1)
    # what f16x3 planes give on this pair (the one-shot call with the check switched off: the planes the resident predictor ran before it judged both sides)
    forced, _ = backend.predict_values(prm, sv, alpha, 0.125, None, pts, options=Options(gram_mode=2))
    want, _ = oracle.predict_values("rbf", sv.astype(np.float64), alpha.astype(np.float64), 0.125, pts.astype(np.float64), gamma=gamma)
    scale = summand_scale("rbf", pts, sv, alpha, 0.125, gamma=gamma)
    e_res, e_one, e_f16 = eps_of(got, want, scale), eps_of(one, want, scale), eps_of(forced, want, scale)
    print(f"\ncross-term case ({'reverse' if reverse else 'forward'}): one-shot {e_one:.3f} eps (gram_mode {info1['gram_mode']}), resident path {e_res:.3f} eps "
          f"(gram_mode {info['gram_mode']}, resident {info['resident']}, {int(np.sum(got != one))} of {got.size} values differ from the one-shot call's); "
          f"f16x3 planes on the pair {e_f16:.3f} eps")
    assert e_res < 16 and e_one < 16, (e_res, e_one)
    assert info1["gram_mode"] == 1, info1
    assert info["gram_mode"] == info1["gram_mode"] and info["rbf_exponent_scale"] == info1["rbf_exponent_scale"], (info, info1)
    assert np.array_equal(got, one), np.max(np.abs(got - one))
    assert info["resident"] == 0, info
    # a batch that passes beside these support vectors: resident, f16x3, the one-shot call's bits
    calm = _shell(np.random.default_rng(3), 100, sv.shape[1], 0.5)
    assert passes(both(*rbf_stats(sv, calm, gamma)), True)
    got, one, info, info1, _, _ = three_way(oracle, "rbf", sv, alpha, 0.125, calm, gamma=gamma)
    assert info["resident"] == 1 and info["gram_mode"] == info1["gram_mode"] == 2 and np.array_equal(got, one), (info, info1)


# ------------------------------------------------------------------------------------------------------------ B. every per-batch switch
def _model(kernel, nsv, npts, d, seed=7, degree=3):
    X, _ = make_blobs_pm1(nsv + npts, d, seed=seed, dtype=np.float32)
    alpha = np.random.default_rng(seed).standard_normal(nsv).astype(np.float32)
    kw = dict(degree=degree, gamma=1.0 / d, coef0=(0.5 if kernel == "polynomial" else 0.0))
    return X[:nsv], X[nsv:], alpha, kw


def _check_paths(got, one, kernel):
    """rbf: the resident form prepares the batch exactly as the one-shot call does -- the same bits; polynomial: within the bar (three_way), the plane shift of the
    resident form comes from the support vectors alone"""
    if kernel == "rbf":
        assert np.array_equal(got, one), np.max(np.abs(got - one))


@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 2), ("polynomial", 3), ("polynomial", 5)], ids=["rbf", "poly2", "poly3", "poly5"])
@pytest.mark.parametrize("d", [64, 65, 128, 129, 192])
def test_feature_counts_either_side_of_the_resident_limit(oracle, kernel, degree, d):
    """round_up(d, 64) <= 128 runs resident; 129 and 192 features go to the one-shot call inside the predictor"""
    sv, pts, alpha, kw = _model(kernel, 300, 300, d, seed=d, degree=degree)
    got, one, info, _, _, _ = three_way(oracle, kernel, sv, alpha, 0.25, pts, **kw)
    assert info["resident"] == (1 if d <= 128 else 0), info
    _check_paths(got, one, kernel)


@pytest.mark.parametrize("kernel, degree", [("rbf", 3), ("polynomial", 2), ("polynomial", 7)], ids=["rbf", "poly2", "poly7"])
@pytest.mark.parametrize("npts", [1, 255, 256, 257, 7936, 7937])
def test_batch_sizes_either_side_of_the_256_row_kernel(oracle, kernel, degree, npts):
    """rows padded to pairs of row blocks: 7 936 points are 62 blocks (the 128-row kernels), 7 937 are 64 (the rectangular 256-row kernel, not for a generic degree)"""
    sv, pts, alpha, kw = _model(kernel, 700, npts, 48, seed=npts, degree=degree)
    got, one, info, _, _, _ = three_way(oracle, kernel, sv, alpha, -0.5, pts, **kw)
    assert info["resident"] == 1, info
    _check_paths(got, one, kernel)


@pytest.mark.parametrize("kernel", ["rbf", "polynomial"])
@pytest.mark.parametrize("nsv", [1, 127, 129])
def test_support_vector_counts_with_a_ragged_last_column_tile(oracle, kernel, nsv):
    sv, pts, alpha, kw = _model(kernel, nsv, 8000, 32, seed=nsv)
    got, one, info, _, _, _ = three_way(oracle, kernel, sv, alpha, 0.0, pts, **kw)
    assert info["resident"] == 1, info
    _check_paths(got, one, kernel)


@pytest.mark.parametrize("r2", [48.0, 128.0, 400.0], ids=["pair_folded_c_le_32", "folded_128_row", "unfolded"])
@pytest.mark.parametrize("npts", [300, 8000])
def test_rbf_form_2_at_exponent_scales_beyond_the_automatic_range(oracle, r2, npts):
    """Options(rbf_form=2): the norm expansion whatever the exponent scale R2.  (32, 64]: folded records, the 256-row kernel for a large batch; (64, 200]: folded records,
    the 128-row kernels; above 200: unfolded records.  The norm expansion's absolute error grows with R2 (2^-22 R2 of the summands: the bound of the training matvec's
    tests at these scales); the resident form gives the one-shot call's bits and exponent scale."""
    d = 64
    sv, pts, alpha, _ = _model("rbf", 500, npts, d, seed=int(r2))
    mean = sv_mean(sv).astype(np.float64)
    sq = max(float(np.max(np.sum((M.astype(np.float64) - mean) ** 2, axis=1))) for M in (sv, pts))
    gamma = float(np.float32(r2 / (2.0 * LOG2E * sq)))
    assert r2 * 0.999 <= exponent_scale(sv, pts, gamma) <= r2 * 1.001
    got, one, info, info1, _, _ = three_way(oracle, "rbf", sv, alpha, 0.0, pts, options=Options(rbf_form=2), gamma=gamma, bar=max(16.0, 2.0 ** -22 * r2 / EPS32))
    assert info["resident"] == 1 and info["rbf_direct"] == 0 and info1["rbf_direct"] == 0 and info1["gram_mode"] in (1, 2), (info, info1)
    assert abs(info["rbf_exponent_scale"] - r2) <= 1e-3 * r2
    assert np.array_equal(got, one), np.max(np.abs(got - one))


@pytest.mark.parametrize("kernel", ["rbf", "polynomial"])
@pytest.mark.parametrize("opts, resident", [({"gram_mode": 0}, 0), ({"gram_mode": 1}, 1), ({"gram_mode": 2}, 1), ({"mfma_shape": 2}, 1), ({"j_chunk_tiles": 3}, 1),
                                            ({"tile_kernel": 1}, 0)], ids=["gram0", "gram1", "gram2", "mfma2", "jchunk3", "tile1"])
def test_options_handed_to_the_predictor_and_to_predict_values(oracle, kernel, opts, resident):
    """the same Options object in both: the same Gram mode and, for rbf, the same bits -- on a batch large enough for the 256-row kernel"""
    sv, pts, alpha, kw = _model(kernel, 600, 8000, 100, seed=5)
    got, one, info, info1, _, _ = three_way(oracle, kernel, sv, alpha, 0.25, pts, options=Options(**opts), **kw)
    assert info["resident"] == resident, info
    if "gram_mode" in opts:
        assert info1["gram_mode"] == opts["gram_mode"], info1
    _check_paths(got, one, kernel)


@pytest.mark.parametrize("target, resident", [(65000.0, 1), (66000.0, 0)], ids=["below_65504", "above_65504"])
def test_polynomial_batch_at_the_f16_overflow_of_the_support_vectors_shift(oracle, target, resident):
    """The resident form splits a polynomial batch with the support vectors' plane scale 2^shift (F16_TARGET_EXP): a batch whose scaled maximum stays below f16's 65 504
    runs resident; one above overflows the planes and goes to the one-shot call (which takes its scale from both sides) with the same values."""
    sv, pts, alpha, kw = _model("polynomial", 400, 600, 64, seed=11, degree=3)
    shift = poly_shift(np.abs(sv).max())
    pts = (pts * np.float32(target / (2.0 ** shift) / np.abs(pts).max())).astype(np.float32)
    st = split_f16x2(pts, 2.0 ** shift)
    assert (np.isfinite(st["rel2"]) and st["rel2"] <= F16_REL2_MAX) if resident else np.isnan(st["rel2"]), st
    kw["gamma"] = 1.0 / (64 * float(np.abs(pts).max()) * float(np.abs(sv).max()))
    got, one, info, info1, _, _ = three_way(oracle, "polynomial", sv, alpha, 0.0, pts, **kw)
    assert info["resident"] == resident and info["gram_mode"] == info1["gram_mode"] == 2, (info, info1)
    if not resident:
        assert np.array_equal(got, one)


# ------------------------------------------------------------------------------------------------------------ C. polynomial degree <= 0 in fp32
@pytest.mark.parametrize("gram_mode", [0, 1, 3])
@pytest.mark.parametrize("d", [7, 100, 300], ids=["narrow", "split", "wide"])
@pytest.mark.parametrize("degree", [-1, -2, -3, 0])
def test_polynomial_degree_zero_and_negative_in_fp32(oracle, degree, d, gram_mode):
    """(gamma x.0 + 0)^-n = inf on the zero-padded support-vector columns must not reach a valid sum: data in U(0.5, 1.5), coef0 = 0, N and nsv not multiples of 128 --
    the training matvec, predict_values and the resident predictor, every value finite and within the bar of float64"""
    rng = np.random.default_rng(100 * d - degree)
    gamma = 1.0 / d
    kw = dict(degree=degree, gamma=float(np.float32(gamma)), coef0=0.0)
    prm = Parameter(kernel_type="polynomial", degree=degree, gamma=gamma, coef0=0.0)
    opts = Options(gram_mode=gram_mode)
    # the training matvec (the symmetric problem, N - 1 = 199 rows and columns)
    X = rng.uniform(0.5, 1.5, size=(200, d)).astype(np.float32)
    n = X.shape[0] - 1
    q = backend.generate_q(prm, X, options=opts)
    QA = float(oracle.kernel_function("polynomial", X[-1].astype(np.float64), X[-1].astype(np.float64), **kw)) + 1.0
    rhs = rng.uniform(-1, 1, size=n).astype(np.float32)
    got = backend.run_device_kernel(prm, q, np.zeros(n, np.float32), rhs, X, QA, 1.0, options=opts)
    X64, q64, rhs64 = X.astype(np.float64), q.astype(np.float64), rhs.astype(np.float64)
    want = oracle.matvec("polynomial", X64, q64, rhs64, np.zeros(n), QA, 1.0, 1.0, **kw)
    K = np.abs(kernel_matrix("polynomial", X64[:n], X64[:n], **kw))
    absd = np.abs(rhs64)
    scale = K @ absd + (abs(QA) + np.abs(q64)) * absd.sum() + np.abs(q64) @ absd + absd
    assert eps_of(got, want, scale) < 16, eps_of(got, want, scale)
    # predict: 150 support vectors, 100 points
    S = rng.uniform(0.5, 1.5, size=(150, d)).astype(np.float32)
    P = rng.uniform(0.5, 1.5, size=(100, d)).astype(np.float32)
    alpha = rng.standard_normal(150).astype(np.float32)
    got, one, info, _, _, _ = three_way(oracle, "polynomial", S, alpha, 0.5, P, options=opts, **kw)
    assert info["resident"] == (1 if d <= 128 and gram_mode != 0 else 0), info


# ------------------------------------------------------------------------------------------------------------ D. the cached predictor of MI355CSVM.predict
@pytest.fixture(scope="module", params=["rbf", "polynomial"])
def fitted(request):
    X, y = make_blobs_pm1(600, 16, seed=41, dtype=np.float32)
    data = DataSet(X, [int(v) for v in y], real_type=np.float32)
    kw = dict(kernel_type="polynomial", degree=2, coef0=1.0) if request.param == "polynomial" else dict(kernel_type="rbf")
    model = make_csvm("mi355", params=Parameter(**kw)).fit(data, epsilon=1e-4, max_iter=60)
    return data, model


def _one_shot_labels(svm, model, data):
    """a fresh one-shot call with the current state: the labels, and which of them are far enough from 0 to be compared between two summation orders"""
    values = svm.predict_values(model.params, model.support_vectors(), model.alpha, float(model.rho), None, data.data())[0]
    labels = np.where(values > 0, model.data.mapping.label_of(1), model.data.mapping.label_of(-1))
    return labels, np.abs(values) > 1e-4 * np.abs(values).max()


@pytest.mark.parametrize("change", ["set_option", "assign_alpha", "alpha_in_place", "assign_rho", "process_option"])
def test_csvm_predict_follows_the_model_and_the_options(fitted, change):
    """MI355CSVM.predict keeps a resident predictor on the model: after a change of this object's options, of the process defaults (an object without options of its own),
    of `alpha` (assigned or edited in place) or of `rho`, it must give the labels of a fresh one-shot call with the state of the moment, and report which path ran"""
    data, fit = fitted
    model = Model(fit.params, data, alpha=np.array(fit.alpha, copy=True), rho=fit.rho)
    svm = make_csvm("mi355", params=fit.params)
    first = np.array(svm.predict(model, data))
    labels, sure = _one_shot_labels(svm, model, data)
    assert np.array_equal(first[sure], labels[sure])
    first_phases = dict(svm.last_predict_phases)
    if change == "set_option":
        svm.set_option("gram_mode", 0)
    elif change == "assign_alpha":
        model.alpha = -model.alpha
    elif change == "alpha_in_place":
        model.alpha *= -1
    elif change == "assign_rho":
        model.rho = np.float32(float(model.rho) + 2.0 * float(np.max(np.abs(svm.predict_values(model.params, model.support_vectors(), model.alpha, 0.0, None, data.data())[0]))))
    else:
        _capi.set_option("gram_mode", 0)  # (the autouse fixture of conftest.py restores the process defaults)
    again = np.array(svm.predict(model, data))
    labels, sure = _one_shot_labels(svm, model, data)
    assert np.array_equal(again[sure], labels[sure]), (change, int(np.sum(again[sure] != labels[sure])))
    assert first_phases.get("resident") == 1, first_phases
    assert svm.last_predict_phases.get("resident") == (0 if change in ("set_option", "process_option") else 1), svm.last_predict_phases
    if change in ("assign_alpha", "alpha_in_place", "assign_rho"):
        assert np.sum(again != first) > data.num_data_points() // 4  # (the change flips labels: a stale predictor cannot pass)
