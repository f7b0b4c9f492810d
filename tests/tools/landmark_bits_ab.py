#!/usr/bin/env python3
"""Everything that walks the landmark block K(X, X_L) -- the Nystrom preconditioner, the fixed-size fit, its leave-one-out pass -- in this build against a library built
from the PARENT commit: the same bits (default) and the same time (--timing).

usage: landmark_bits_ab.py --parent-lib <libplssvm_amd.so of the parent commit> [--out profiles/landmark_bits.json]
       landmark_bits_ab.py --parent-lib <...> --timing [--rounds 2] [--reps 5] [--out profiles/landmark_bits.json]

Written for a change that moves the host code around the landmark kernels without touching arithmetic (cg_bits_ab.py is the model): every returned array and the integer /
jitter fields of the info structs must be bit-equal, so the condition is equality of SHA-256 digests with no tolerance; millisecond fields are left out.  Error messages are
compared as strings.

Bits.  fp32 / fp64; linear, polynomial degree 3, rbf; blobs of 5 features with 3 one-vs-all right-hand sides:
  landmark_gram, fit_reduced   N in {255, 257, 777}, rank in {1, 16, 17, 64, 129}, k in {1, 3}, slab_rows in {256, 0}, the library's landmarks and explicit ones that
                               contain point N - 1 and (rank >= 2) point 0.  slab_rows = 256 at N = 777: four slabs, the last of 9 rows, landmarks in different slabs
  fit_reduced_loo              N in {777, 300}, rank in {1, 16, 65, 129}, k in {1, 3}, costs [0.1, 10, 1000] and [5], both slab_rows: the six outputs and loo_errors
  reduced_leverage             N = 777, rank in {16, 129}, k in {0, 1, 3}, both slab_rows
  build_preconditioner         N in {300, 700}, rank in {1, 16, 65, 256}: precond_landmarks, precond_apply of one fixed vector, solve_pcg for k = 1 and 3 (alphas, rhos,
                               iterations), lssvm_precond_info.jitter
  one-shot entry points        fit_reduced, fit_reduced_loo, solve_pcg, solve_cost_path at 300 x 5 rbf per real type
  largest rank                 1024 at N = 1100, fp64 rbf: the fit and the leave-one-out pass
  near-singular                one data set for the reduced fit and the preconditioner whose jitter loop makes more than one attempt; asserted on the parent's result
                               (near_singular_case has the construction and why duplicate landmarks alone do not do it)
  error texts                  the refusals that tests/test_gpu_reduced.py, test_gpu_reduced_loo.py and test_gpu_pcg.py provoke on a problem by argument alone, and the two
                               "data" refusals of every one-shot entry point
Timing (--timing).  Host wall clock of the whole call (every call ends in a device synchronise), medians over rounds x reps samples per library after one untimed call,
and the parent's spread (max - min) / median:
  a  fit_reduced, 50 000 x 128 rbf fp32, rank 256
  b  fit_reduced_loo on the same data, 8 costs
  c  build_preconditioner + solve_pcg, 50 000 x 128 rbf fp32, rank 256, eps 1e-3 (problem set-up not included)
  d  fit_reduced, 2 000 x 16, rank 64: host code and launches dominate, an added allocation or synchronisation would show
Condition per shape: median(new) <= median(parent) * (1 + spread(parent)).
Child processes alternate between the two libraries (PLSSVM_AMD_LIBRARY).  Every child runs under a time limit of its own; a child that fails ends the run: nothing more
is started on the device.  The tool exits non-zero on any difference / any shape over its bound, after it has written --out.
"""

import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = {"linear": ("linear", 3), "poly3": ("polynomial", 3), "rbf": ("rbf", 3)}
FEATURES = 5
COST = 10.0
DBL_EPSILON = 2.220446049250313e-16


def digest(*parts) -> str:
    import numpy as np

    h = hashlib.sha256()
    for part in parts:
        a = np.ascontiguousarray(part)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def explicit_landmarks(N: int, rank: int):
    """`rank` distinct points in a fixed shuffled order: point N - 1 first, then point 0."""
    import numpy as np

    return np.concatenate(([N - 1, 0], np.random.default_rng(11).permutation(np.arange(1, N - 1))))[:rank].astype(np.uint64)


def near_singular_case():
    """(params, X, Y, landmarks) in fp64 on which BOTH jitter loops retry.

    Duplicate rows among the landmarks are part of it (rows 0 ... 3 are rows 4 ... 7), but they cannot make the loops retry on their own: for a positive semidefinite
    kernel matrix the first jitter eps * trace exceeds what rounding does to a pivot (the pivot of a duplicate comes out near 2 nu), which is what the schedule is for.  So
    the kernel function is made slightly indefinite as well: polynomial of degree 3 on 2 features spans 10 monomials, the 24 landmarks leave a null space, and a coef0
    just below zero (-2e-13) puts eigenvalues near -2e-13 * trace there -- beyond eps * trace, within the seven attempts.  The cost is small so that sigma K_mm carries
    the same into the matrix of the reduced model."""
    import numpy as np

    from plssvm_amd.parameter import Parameter

    rng = np.random.default_rng(29)
    X = rng.uniform(-1.0, 1.0, size=(300, 2))
    X[4:8] = X[0:4]
    Y = np.where(X[:, :1].T + 0.3 * rng.standard_normal((1, 300)) > 0.0, 1.0, -1.0)
    landmarks = np.concatenate((np.arange(8), np.arange(20, 300, 18)[:16])).astype(np.uint64)
    return Parameter(kernel_type="polynomial", degree=3, gamma=1.0, coef0=-2e-13, cost=1e-3), X, Y, landmarks


def bits_child() -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd.datagen import make_blobs_multiclass
    from plssvm_amd.exceptions import PlssvmError
    from plssvm_amd.multiclass import one_vs_all_targets
    from plssvm_amd.parameter import Parameter

    out = {}

    def data(N, dt, features=FEATURES):
        X, labels = make_blobs_multiclass(N, features, 3, seed=7 + N, dtype=dt)
        return X, one_vs_all_targets(np.arange(3), labels, dt)

    def fitted(res):  # (betas, rhos, landmarks, info) of a fit
        betas, rhos, used, info = res
        return digest(betas, np.float64(rhos), used, np.array([info["rank"], info["slabs"], info["workspace_bytes"]], dtype=np.uint64), np.float64(info["jitter"]))

    def scored(res):  # (betas, rhos, landmarks, report) of the leave-one-out scores
        betas, rhos, used, rep = res
        return digest(betas, rhos, used, rep["leverage"], rep["fitted"], rep["loo"], rep["press"], rep["loo_errors"], rep["max_leverage"], rep["jitter"])

    def solved(res):  # (alphas, rhos, infos) of solve_pcg
        alphas, rhos, infos = res
        infos = [infos] if isinstance(infos, dict) else infos
        return digest(alphas, np.asarray(rhos), np.array([[i["iterations"], i["gram_passes"], i["converged"], i["rank"]] for i in infos], dtype=np.uint64),
                      np.array([[i["residuum"], i["jitter"]] for i in infos]))

    def landmark_sets(N, rank):
        return (("library", None), ("explicit", explicit_landmarks(N, rank)))

    for dt in (np.float32, np.float64):
        eps = 1e-8 if dt == np.float64 else 1e-3
        for kernel, (name, degree) in KERNELS.items():
            p = Parameter(kernel_type=name, degree=degree, gamma=1.0 / FEATURES, coef0=0.5, cost=COST)
            head = f"{np.dtype(dt).name} {kernel}"
            for N in (255, 257, 777, 300):
                X, Y = data(N, dt)
                with backend.ResidentProblem(p, X) as prob:
                    if N != 300:
                        for rank in (1, 16, 17, 64, 129):
                            for k in (1, 3):
                                for slab_rows in (256, 0):
                                    for which, lm in landmark_sets(N, rank):
                                        key = f"{head} {N}: rank {rank} k {k} slab_rows {slab_rows} {which} landmarks"
                                        out[f"{key}: landmark_gram"] = digest(prob.landmark_gram(Y[:k], rank, landmarks=lm, slab_rows=slab_rows))
                                        out[f"{key}: fit_reduced"] = fitted(prob.fit_reduced(Y[:k], rank, landmarks=lm, slab_rows=slab_rows))
                    if N in (777, 300):
                        for rank in (1, 16, 65, 129):
                            for k in (1, 3):
                                for costs in ([0.1, 10.0, 1000.0], [5.0]):
                                    for slab_rows in (256, 0):
                                        out[f"{head} {N}: rank {rank} k {k} costs {costs} slab_rows {slab_rows}: fit_reduced_loo"] = scored(prob.fit_reduced_loo(Y[:k], rank, costs, slab_rows=slab_rows))
                    if N == 777:
                        rng = np.random.default_rng(5)
                        for rank in (16, 129):
                            V, shift = np.tril(rng.standard_normal((rank, rank))), rng.standard_normal(rank)
                            for k in (0, 1, 3):
                                for slab_rows in (256, 0):
                                    h, f = prob.reduced_leverage(V, shift, rng.standard_normal((rank, k)) if k else None, slab_rows=slab_rows)
                                    out[f"{head} {N}: rank {rank} k {k} slab_rows {slab_rows}: reduced_leverage"] = digest(h, f)
            for N in (300, 700):
                X, Y = data(N, dt)
                r = np.random.default_rng(3).standard_normal(N - 1).astype(dt)
                with backend.ResidentProblem(p, X) as prob:
                    for rank in (1, 16, 65, 256):
                        key = f"{head} {N}: preconditioner of rank {rank}"
                        built = prob.build_preconditioner(rank)
                        out[f"{key}: landmarks, jitter, device_bytes"] = digest(prob.precond_landmarks(), np.float64(built["jitter"]), np.array([built["rank"], built["device_bytes"]], dtype=np.uint64))
                        out[f"{key}: precond_apply"] = digest(prob.precond_apply(r))
                        for k in (1, 3):
                            out[f"{key}: solve_pcg k = {k}"] = solved(prob.solve_pcg(Y[:k], eps, N))
                    built = prob.build_preconditioner(landmarks=explicit_landmarks(N, 17))
                    out[f"{head} {N}: preconditioner of explicit landmarks"] = digest(prob.precond_landmarks(), np.float64(built["jitter"]), prob.precond_apply(r))
        # ---- the one-shot entry points ----
        X, Y = data(300, dt)
        p = Parameter(kernel_type="rbf", gamma=1.0 / FEATURES, cost=COST)
        head = f"{np.dtype(dt).name} rbf 300 one-shot"
        out[f"{head}: fit_reduced"] = fitted(backend.fit_reduced(p, X, Y, 64, slab_rows=256))
        out[f"{head}: fit_reduced_loo"] = scored(backend.fit_reduced_loo(p, X, Y, 64, [0.1, 10.0], landmarks=explicit_landmarks(300, 64)))
        out[f"{head}: solve_pcg"] = solved(backend.solve_pcg(p, X, Y, eps, 300, rank=64))
        alphas, rhos, infos, passes = backend.solve_cost_path(p, X, Y[0], [0.1, 10.0, 1000.0], eps, 300)
        out[f"{head}: solve_cost_path"] = digest(alphas, rhos, np.array([[i["iterations"], i["converged"], i["verified"]] for i in infos], dtype=np.uint64), np.array(passes, dtype=np.uint64))

    # ---- the largest rank ----
    X, Y = data(1100, np.float64)
    with backend.ResidentProblem(Parameter(kernel_type="rbf", gamma=1.0 / FEATURES, cost=COST), X) as prob:
        out["float64 rbf 1100: rank 1024: fit_reduced"] = fitted(prob.fit_reduced(Y, 1024, slab_rows=512))
        out["float64 rbf 1100: rank 1024: fit_reduced_loo"] = scored(prob.fit_reduced_loo(Y[:1], 1024, [0.1, 10.0], slab_rows=512))

    # ---- near-singular: both jitter loops retry ----
    p, X, Y, lm = near_singular_case()
    with backend.ResidentProblem(p, X) as prob:
        res = prob.fit_reduced(Y, len(lm), landmarks=lm)
        out["near-singular: fit_reduced"] = fitted(res)
        out["near-singular: fit_reduced_loo"] = scored(prob.fit_reduced_loo(Y, len(lm), [p.cost, 1.0], landmarks=lm))
        St = prob.landmark_gram(Y, len(lm), landmarks=lm)
        m = len(lm)
        Kmm_diag = (p.gamma * np.einsum("ij,ij->i", X[lm.astype(np.int64)], X[lm.astype(np.int64)]) + p.coef0) ** 3
        trace_M = float(np.sum(np.diag(St)[:m] - St[m, :m] ** 2 / X.shape[0] + Kmm_diag / p.cost))
        built = prob.build_preconditioner(landmarks=lm)
        out["near-singular: preconditioner"] = digest(np.float64(built["jitter"]), prob.precond_apply(np.ones(X.shape[0] - 1)))
        # a first attempt that succeeds leaves eps * trace (the host's trace and this one agree far better than the factor 5)
        out["near-singular: attempts beyond the first"] = {"reduced": bool(res[3]["jitter"] > 5.0 * DBL_EPSILON * trace_M), "reduced_jitter_over_eps_trace": res[3]["jitter"] / (DBL_EPSILON * trace_M),
                                                           "preconditioner": bool(built["jitter"] > 5.0 * DBL_EPSILON * float(np.sum(Kmm_diag))),
                                                           "preconditioner_jitter_over_eps_trace": built["jitter"] / (DBL_EPSILON * float(np.sum(Kmm_diag)))}

    # ---- error texts: the refusals the three test files provoke on a problem, and the data refusals of the one-shot entry points ----
    def refusal(call):
        try:
            call()
        except PlssvmError as e:
            return str(e)
        return "no refusal"

    X, Y = data(777, np.float64)
    N, y = 777, Y[0]
    p = Parameter(kernel_type="rbf", gamma=1.0 / FEATURES, cost=COST)
    with backend.ResidentProblem(p, X) as prob:
        reduced = {"fit_reduced": lambda: prob.fit_reduced(y, 8), "landmark_gram": lambda: prob.landmark_gram(y, 8), "fit_reduced_loo": lambda: prob.fit_reduced_loo(y, 8, [1.0]),
                   "reduced_leverage": lambda: prob.reduced_leverage(np.eye(8), np.zeros(8))}
        precond = {"solve_pcg": lambda: prob.solve_pcg(y, 1e-6, 10), "build_preconditioner": lambda: prob.build_preconditioner(4), "precond_apply": lambda: prob.precond_apply(np.ones(N - 1))}
        for name in ("solve_pcg", "precond_apply"):
            out[f"refusal: no preconditioner: {name}"] = refusal(precond[name])
        out["refusal: no preconditioner: precond_landmarks"] = refusal(prob.precond_landmarks)
        out["refusal: no preconditioner: time_gram_kernels"] = refusal(lambda: prob.time_gram_kernels(1))
        for rank in (0, N, 513):
            out[f"refusal: build_preconditioner({rank})"] = refusal(lambda: prob.build_preconditioner(rank))
        for name, call in {"build_preconditioner": lambda lm: prob.build_preconditioner(landmarks=lm), "fit_reduced": lambda lm: prob.fit_reduced(y, len(lm), landmarks=lm),
                           "fit_reduced_loo": lambda lm: prob.fit_reduced_loo(y, len(lm), [1.0], landmarks=lm)}.items():
            out[f"refusal: landmarks not distinct: {name}"] = refusal(lambda: call([3, 7, 3]))
            out[f"refusal: landmark beyond the data: {name}"] = refusal(lambda: call([3, N]))
        prob.build_preconditioner(landmarks=[0, N - 1])
        out["refusal: solve_pcg eps 0"] = refusal(lambda: prob.solve_pcg(y, 0.0, 10))
        out["refusal: solve_pcg max_iter 0"] = refusal(lambda: prob.solve_pcg(y, 1e-6, 0))
        out["refusal: solve_pcg short right-hand side"] = refusal(lambda: prob.solve_pcg(y[:-1], 1e-6, 10))
        out["refusal: precond_apply long vector"] = refusal(lambda: prob.precond_apply(np.ones(N)))
        for n, costs in enumerate(([], np.ones(65), [1.0, 0.0], [-1.0], [float("nan")])):
            out[f"refusal: fit_reduced_loo costs {n}"] = refusal(lambda: prob.fit_reduced_loo(y, 8, costs))
        out["refusal: fit_reduced_loo rank N + 1"] = refusal(lambda: prob.fit_reduced_loo(y, N + 1, [1.0]))
        out["refusal: fit_reduced_loo slab_rows 100"] = refusal(lambda: prob.fit_reduced_loo(y, 8, [1.0], slab_rows=100))
        out["refusal: reduced_leverage short shift"] = refusal(lambda: prob.reduced_leverage(np.eye(8), np.zeros(7)))
        prob.set_weights(np.full(N, 2.0))
        for name, call in {**reduced, **precond}.items():
            out[f"refusal: weights set: {name}"] = refusal(call)
        gram_ms, leverage_ms = prob.time_leverage_kernel(8, repeats=1)  # (the aid does not look at the weights)
        out["weights set: time_leverage_kernel runs"] = bool(gram_ms.size == 1 and leverage_ms.size == 1)
        prob.set_weights(None)
        prob.cg_begin(y, 1e-6)
        for name, call in {**reduced, **precond, "time_leverage_kernel": lambda: prob.time_leverage_kernel(8, repeats=1)}.items():
            out[f"refusal: between cg_begin and cg_finish: {name}"] = refusal(call)
        prob.cg_step(1)
        prob.cg_finish()
    with backend.ResidentProblem(p, X, devices=[0, 0]) as prob:  # two shards on the one device
        for name, call in {**reduced, **precond, "time_leverage_kernel": lambda: prob.time_leverage_kernel(8, repeats=1)}.items():
            if name != "precond_apply":
                out[f"refusal: two shards: {name}"] = refusal(call)
    # the one-shot entry points without data (the Python layer never passes that on): called as the C program would
    X32, ps = X.astype(np.float32), backend._params_struct(p, FEATURES)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    buf = np.zeros(4 * N)
    costs = np.array([1.0])
    pcg_infos, path_infos = (_capi.LssvmPcgInfo * 1)(), (_capi.LssvmPathInfo * 1)()
    for suffix, Xt in (("f32", X32), ("f64", X)):
        Yt = np.ascontiguousarray(Y[0], dtype=Xt.dtype)
        for what, Xp, n, d in (("no points", _capi.ptr(Xt), 0, FEATURES), ("NULL data", None, N, FEATURES), ("no features", _capi.ptr(Xt), N, 0)):
            b, u = buf.ctypes.data_as(dp), buf.ctypes.data_as(up)
            calls = {
                "fit_reduced": lambda: _capi.reduced_entry(f"lssvm_mi355_fit_reduced_{suffix}")(C.byref(ps), Xp, n, d, _capi.ptr(Yt), 1, 2, None, 0, b, b, u, None, None),
                "fit_reduced_loo": lambda: _capi.reduced_loo_entry(f"lssvm_mi355_fit_reduced_loo_{suffix}")(C.byref(ps), Xp, n, d, _capi.ptr(Yt), 1, 2, None, 0, costs.ctypes.data_as(dp), 1, b, b, None,
                                                                                                         None, None, None, None, None, None, None),
                "solve_pcg": lambda: _capi.pcg_entry(f"lssvm_mi355_solve_pcg_{suffix}")(C.byref(ps), Xp, n, d, _capi.ptr(Yt), 1, 2, None, 1e-3, 10, _capi.ptr(Yt), b, pcg_infos, None),
                "solve_cost_path": lambda: _capi.cost_path_entry(f"lssvm_mi355_solve_cost_path_{suffix}")(C.byref(ps), Xp, n, d, _capi.ptr(Yt), costs.ctypes.data_as(dp), 1, 1e-3, 10, 0, _capi.ptr(Yt), b,
                                                                                                         path_infos, None, None),
            }
            for name, call in calls.items():
                out[f"refusal: {what}: {name}_{suffix}"] = f"status {call()}: {_capi.last_error()}"
    print("RESULT " + json.dumps(out), flush=True)


def timing_child(reps: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    out = {}

    def timed(name, call):
        for keep in [False] + [True] * reps:
            t0 = time.perf_counter()
            call()
            if keep:
                out.setdefault(name, []).append(1e3 * (time.perf_counter() - t0))

    X, y = make_blobs_pm1(2_000, 16, seed=42, dtype=np.float32)
    with backend.ResidentProblem(Parameter(kernel_type="rbf", gamma=1.0 / 16, cost=1.0), X) as prob:
        timed("d_fit_reduced_2000x16_rbf_f32_rank64", lambda: prob.fit_reduced(y, 64))
    X, y = make_blobs_pm1(50_000, 128, seed=42, dtype=np.float32)
    costs = np.logspace(-2, 2, 8)
    with backend.ResidentProblem(Parameter(kernel_type="rbf", gamma=1.0 / 128, cost=1.0), X) as prob:
        timed("a_fit_reduced_50000x128_rbf_f32_rank256", lambda: prob.fit_reduced(y, 256))
        timed("b_fit_reduced_loo_50000x128_rbf_f32_rank256_8_costs", lambda: prob.fit_reduced_loo(y, 256, costs))

        def pcg():
            prob.build_preconditioner(256)
            prob.solve_pcg(y, 1e-3, 50_000)

        timed("c_build_preconditioner_solve_pcg_50000x128_rbf_f32_rank256_eps1e-3", pcg)
    print("RESULT " + json.dumps(out), flush=True)


def run_child(which, parent_lib, mode, reps, limit):
    env = dict(os.environ)
    if which == "parent":
        env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(parent_lib)
    else:
        env.pop("PLSSVM_AMD_LIBRARY", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(reps)]
    try:
        proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"{which}: child exceeded {limit} s; stopping", file=sys.stderr)
        return None
    line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if proc.returncode != 0 or line is None:
        print(f"{which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}", file=sys.stderr)
        return None
    return json.loads(line[len("RESULT "):])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmark_bits.json"))
    ap.add_argument("--child", choices=["bits", "timing"])
    args = ap.parse_args()
    if args.child:
        bits_child() if args.child == "bits" else timing_child(args.reps)
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    res = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    failed = []
    if args.timing:
        samples = {"parent": {}, "new": {}}
        for rnd in range(args.rounds):
            for which in ("parent", "new"):
                got = run_child(which, args.parent_lib, "timing", args.reps, args.child_timeout)
                if got is None:
                    return 1
                for name, vals in got.items():
                    samples[which].setdefault(name, []).extend(vals)
                print(f"round {rnd}, {which}: done", flush=True)
        res["timing"] = {}
        for name in sorted(samples["new"]):
            a, b = samples["new"][name], samples["parent"][name]
            med_a, med_b = statistics.median(a), statistics.median(b)
            spread = (max(b) - min(b)) / med_b
            ok = med_a <= med_b * (1.0 + spread)
            res["timing"][name] = {"new_median_ms": med_a, "parent_median_ms": med_b, "ratio": med_a / med_b, "parent_spread": spread, "new_spread": (max(a) - min(a)) / med_a,
                                   "samples_per_library": len(b), "within_parent_spread": ok}
            if not ok:
                failed.append(name)
        res["timing_method"] = (f"{args.rounds} alternating child processes per library, {args.reps} timed repetitions each after a warm-up; host wall clock of the whole call; "
                                "condition: new median <= parent median * (1 + parent spread), spread = (max - min) / median")
        print(json.dumps(res["timing"], indent=1))
    else:
        got = {}
        for which in ("parent", "new"):
            got[which] = run_child(which, args.parent_lib, "bits", args.reps, args.child_timeout)
            if got[which] is None:
                return 1
            print(f"{which}: {len(got[which])} cases", flush=True)
        names = sorted(set(got["parent"]) | set(got["new"]))
        failed = [name for name in names if got["parent"].get(name) != got["new"].get(name)]
        # the record stays small: a case that differs stands in full; the equal ones are counted per group (first and last part of the name), with one digest over the
        # group's "name=value" lines, so that a later run can still be compared with this one
        groups = {}
        for name in names:
            if name not in failed:
                parts = name.split(": ")
                groups.setdefault(parts[0] if len(parts) == 1 or parts[0] == "refusal" else f"{parts[0]}: {parts[-1]}", []).append(f"{name}={json.dumps(got['new'][name], sort_keys=True)}")
        res["bits"] = {"different": {name: {"parent": got["parent"].get(name), "new": got["new"].get(name)} for name in failed},
                       "equal": {g: f"{len(lines)} cases, sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}" for g, lines in groups.items()}}
        retried = got["parent"].get("near-singular: attempts beyond the first", {})
        res["near_singular_parent"] = retried
        if not (retried.get("reduced") and retried.get("preconditioner")):  # (else the near-singular case proves nothing)
            failed.append("near-singular: the parent's jitter loops did not both retry")
        res["bits_summary"] = {"cases": len(names), "equal": sum(len(lines) for lines in groups.values()), "different": failed}
        print(json.dumps(res["bits_summary"], indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
