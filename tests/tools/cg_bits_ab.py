#!/usr/bin/env python3
"""The CG drivers of this build against a library built from the PARENT commit: the same bits (default) and the same time (--timing).

usage: cg_bits_ab.py --parent-lib <libplssvm_amd.so of the parent commit> [--out profiles/cg_recipe_bits.json]
       cg_bits_ab.py --parent-lib <...> --timing [--rounds 2] [--reps 5] [--out profiles/cg_recipe_bits.json]

Written for a change that moves host code of the CG recipe without touching arithmetic: every output of every entry point must be bit-equal, so the condition is equality
of SHA-256 digests with no tolerance, and the time of a call must be the parent's within the parent's own spread.

Bits.  Per (real type, kernel function, weighted, shape) -- fp32 / fp64; linear, polynomial degree 3, rbf; 130 x 17, 300 x 20, 700 x 20 -- digests of: the one-shot
solve; cg_begin / cg_step / cg_finish cut into several calls across the refresh of iteration 50; matvec with add = +1 / -1; matvec_pair; solve_lockstep for k = 1, 2, 3, 7;
the same solve sharded over [0, 0] (two shards of one device: the peer exchange); in fp64 solve_refined for k = 1 and 3.  Once: the refinement's take-over case (linear
400 x 8, C = 1e8) and its fall-back for data beyond float32.  Where two devices are visible, the two-device solve over both exchanges; else that is recorded as not run.
For a change to the Gram pass's walk over the row-block bands or to PCG's use of the recipe (gram_pass_cases; --out profiles/gram_pass_bits.json): solve_pcg one-shot and
resident, k = 1 and 3, rank 32, 60 forced iterations (across the refresh of iteration 50), and solve_cost_path with verify over 5 costs -- fp32 / fp64, rbf / polynomial,
300 x 20 and 700 x 20; matvec, matvec_pair and solve_lockstep k = 1, 2, 3 at 300 x 200 fp32 (the two-vector symmetric split kernel); with colslab_band_mb = 1 (two bands)
5 900 x 20 fp64 and 8 400 x 192 fp32: matvec, matvec_pair, six cg_step iterations, lockstep k = 3; the linear kernel over feature panels: 300 x 300 fp64, 300 x 200 fp32
(and 300 x 300 fp32, which runs as ONE launch of the polynomial kernel of degree 1), matvec and twelve iterations.
Timing (--timing).  Host wall clock of the whole call, medians over rounds x reps samples per library and the parent's spread (max - min) / median:
  a  10 000 x 32 rbf fp32, 200 iterations forced (eps 1e-30): short matvecs, the host's launch sequence and the enqueue-ahead path dominate
  b  50 000 x 128 rbf fp32, eps 1e-3
  c  solve_lockstep, 100 000 x 64 polynomial degree 3 fp64, k = 4, eps 1e-3 (problem set-up included)
  d  solve_refined, 50 000 x 128 rbf, eps 1e-10, C = 1
  e  solve_pcg, 50 000 x 32 rbf fp32, rank 256, eps 1e-3 (problem set-up and the preconditioner's build included)
  f  solve_lockstep, 30 000 x 192 polynomial degree 3 fp32, k = 4, eps 1e-3 (problem set-up included)
Condition per shape: median(new) <= median(parent) * (1 + spread(parent)).
Child processes alternate between the two libraries (PLSSVM_AMD_LIBRARY).  Every child runs under a time limit of its own; a child that fails ends the run: nothing more
is started on the device.  The tool exits non-zero on any difference / any shape over its bound, after it has written --out.
"""

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = {"linear": ("linear", 3), "poly3": ("polynomial", 3), "rbf": ("rbf", 3)}
SHAPES = [(130, 17), (300, 20), (700, 20)]
COST = 100.0


def digest(*parts) -> str:
    import numpy as np

    h = hashlib.sha256()
    for part in parts:
        a = np.ascontiguousarray(part)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def bits_child() -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd.datagen import make_blobs_multiclass
    from plssvm_amd.multiclass import one_vs_all_targets
    from plssvm_amd.parameter import Parameter

    out = {}

    def solved(res):  # (alpha, rho, info) of a solve
        alpha, rho, info = res
        return digest(alpha, np.float64(rho), np.float64(info["residuum"]), np.uint64(info["iterations"]), np.uint64(info["converged"]))

    def several(alphas, rhos, infos):
        return digest(alphas, np.asarray(rhos, dtype=np.float64), np.array([i["residuum"] for i in infos]), np.array([i["iterations"] for i in infos], dtype=np.uint64))

    two_devices = _capi.device_count() >= 2
    for dt in (np.float32, np.float64):
        eps = 1e-8 if dt == np.float64 else 1e-3
        for points, features in SHAPES:
            X, y = make_blobs_multiclass(points, features, 5, seed=7, dtype=dt)
            ova = one_vs_all_targets(np.arange(5), y, np.float64)
            rng = np.random.default_rng(3)
            unit = np.zeros(points)
            unit[5] = 1.0
            B = np.stack([ova[0], ova[1], rng.choice([-1.0, 1.0], size=points), rng.standard_normal(points), unit, np.ones(points), 1e6 * ova[2]]).astype(dt)
            w = np.random.default_rng(5).uniform(0.25, 4.0, size=points)
            v0, v1, r0, r1 = (rng.standard_normal(points - 1).astype(dt) for _ in range(4))
            cuts = (3, 1, 44, 9) if points > 200 else (5, 5, 2)
            for kernel, (name, degree) in KERNELS.items():
                p = Parameter(kernel_type=name, degree=degree, gamma=1.0 / features, coef0=0.5, cost=COST)
                for weighted in (False, True):
                    key = f"{np.dtype(dt).name} {kernel} {'weighted' if weighted else 'unweighted'} {points}x{features}"
                    sw = w if weighted else None
                    out[f"{key}: one-shot"] = solved(backend.solve_system_of_linear_equations(p, X, B[0], eps, points, sample_weight=sw))
                    with backend.ResidentProblem(p, X) as prob:
                        if weighted:
                            prob.set_weights(w)
                        prob.cg_begin(B[0], 1e-30)
                        for k in cuts:
                            prob.cg_step(k)
                        out[f"{key}: cg_begin / cg_step {cuts} / cg_finish"] = solved(prob.cg_finish())
                        for add in (1.0, -1.0):
                            out[f"{key}: matvec add {add:+.0f}"] = digest(prob.matvec(v0, r0, add))
                            m0, m1, _ = prob.matvec_pair(v0, v1, r0, r1, add)
                            out[f"{key}: matvec_pair add {add:+.0f}"] = digest(m0, m1)
                        for k in (1, 2, 3, 7):
                            alphas, rhos, infos, passes = prob.solve_lockstep(B[:k], eps, points)
                            out[f"{key}: solve_lockstep k = {k}"] = digest(several(alphas, rhos, infos), np.array(passes, dtype=np.uint64))
                    with backend.ResidentProblem(p, X, devices=[0, 0]) as prob:  # two shards on one device: the sharded driver and the peer exchange
                        if weighted:
                            prob.set_weights(w)
                        prob.cg_begin(B[0], 1e-30)
                        for k in cuts:
                            prob.cg_step(k)
                        out[f"{key}: two shards of device 0, cg_step {cuts}"] = solved(prob.cg_finish())
                        out[f"{key}: two shards of device 0, matvec"] = digest(prob.matvec(v0, r0, 1.0))
                    for exchange in (1, 2):
                        name2 = f"{key}: devices [0, 1], exchange {exchange}"
                        if two_devices:
                            out[name2] = solved(backend.solve_system_of_linear_equations(p, X, B[0], eps, points, devices=[0, 1], options=_capi.Options(exchange=exchange), sample_weight=sw))
                        else:
                            out[name2] = "not run: one device visible"
                    if dt == np.float64:
                        for k in (1, 3):
                            alphas, rhos, infos, ris = backend.solve_refined(p, X, B[:k], 1e-9, 10 * points, sample_weight=sw)
                            out[f"{key}: solve_refined k = {k}"] = digest(several(alphas, rhos, infos), np.array([[r["outer_steps"], r["inner_iterations"], r["f64_cg_iterations"]] for r in ris],
                                                                                                                dtype=np.uint64))

    def refined_data(N, d):  # (tests/test_gpu_refined.py: data)
        rng = np.random.default_rng(1000 * N + d)
        X = rng.uniform(-1.0, 1.0, size=(N, d))
        return X, np.where(X @ rng.standard_normal(d) + 0.3 * rng.standard_normal(N) > 0.0, 1.0, -1.0)

    X, y = refined_data(400, 8)
    alpha, rho, info, ri = backend.solve_refined(Parameter(kernel_type="linear", gamma=1.0 / 8, cost=1e8), X, y, 1e-6, 4000)
    assert ri["took_over_f64"] == 1, ri
    out["refined: fp64 CG takes over (linear 400x8, C = 1e8)"] = digest(solved((alpha, rho, info)), np.array([ri["outer_steps"], ri["inner_iterations"], ri["f64_cg_iterations"]], dtype=np.uint64))
    X, y = refined_data(300, 20)
    X[7, 3] = 1e300
    with np.errstate(all="ignore"):
        for k in (1, 2):
            alphas, rhos, infos, ris = backend.solve_refined(Parameter(kernel_type="linear", gamma=1.0 / 20, cost=1.0), X, np.stack([y, -y])[:k], 1e-6, 300)
            assert all(r["refined"] == 0 for r in ris), ris
            out[f"refined: data beyond float32 falls back, k = {k}"] = several(alphas, rhos, infos)
    gram_pass_cases(out)
    print("RESULT " + json.dumps(out), flush=True)


def gram_pass_cases(out) -> None:
    """What runs the band walk of the Gram pass or PCG's recipe steps and the cases above do not reach (see the module's docstring)."""
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd.datagen import make_blobs_multiclass
    from plssvm_amd.multiclass import one_vs_all_targets
    from plssvm_amd.parameter import Parameter

    def param(kernel, features):
        name, degree = KERNELS[kernel]
        return Parameter(kernel_type=name, degree=degree, gamma=1.0 / features, coef0=0.5, cost=COST)

    def case(points, features, dt, classes=3):
        X, y = make_blobs_multiclass(points, features, classes, seed=7, dtype=dt)
        rng = np.random.default_rng(3)
        return X, one_vs_all_targets(np.arange(classes), y, np.float64).astype(dt), [rng.standard_normal(points - 1).astype(dt) for _ in range(4)]

    def lockstep(prob, B, eps, max_iter):
        alphas, rhos, infos, passes = prob.solve_lockstep(B, eps, max_iter)
        return digest(alphas, np.asarray(rhos, dtype=np.float64), np.array([i["residuum"] for i in infos]), np.array([i["iterations"] for i in infos], dtype=np.uint64),
                      np.array(passes, dtype=np.uint64))

    def matvecs(prob, key, vecs):
        v0, v1, r0, r1 = vecs
        out[f"{key}: matvec"] = digest(prob.matvec(v0, r0, 1.0))
        m0, m1, two = prob.matvec_pair(v0, v1, r0, r1, -1.0)
        out[f"{key}: matvec_pair"] = digest(m0, m1, np.uint64(two))

    def cg_steps(prob, b, steps):
        prob.cg_begin(b, 1e-30)
        for _ in range(steps):
            prob.cg_step(1)
        alpha, rho, info = prob.cg_finish()
        return digest(alpha, np.float64(rho), np.float64(info["residuum"]), np.uint64(info["iterations"]))

    def pcg(res, k):  # (alphas, rhos, infos) of solve_pcg, one right-hand side or several
        alphas, rhos, infos = res
        infos = [infos] if k == 1 else infos
        return digest(alphas, np.asarray(rhos, dtype=np.float64), np.array([i["residuum"] for i in infos]), np.array([[i["iterations"], i["gram_passes"]] for i in infos], dtype=np.uint64))

    def path(res):
        alphas, rhos, infos, passes = res
        return digest(alphas, np.asarray(rhos, dtype=np.float64), np.array([[i["residuum"], i["true_residuum"]] for i in infos]), np.array([i["iterations"] for i in infos], dtype=np.uint64),
                      np.array(passes, dtype=np.uint64))

    # PCG across the refresh of iteration 50 (60 iterations forced), and the cost path with its verification passes
    for dt in (np.float32, np.float64):
        for points, features in SHAPES[1:]:
            X, B, _ = case(points, features, dt)
            for kernel in ("rbf", "poly3"):
                key = f"{np.dtype(dt).name} {kernel} {points}x{features}"
                p = param(kernel, features)
                costs = [0.5, 3.0, 20.0, 100.0, 1000.0]
                eps = 1e-8 if dt == np.float64 else 1e-3
                for k in (1, 3):
                    out[f"{key}: solve_pcg one-shot, rank 32, k = {k}"] = pcg(backend.solve_pcg(p, X, B[0] if k == 1 else B[:k], 1e-30, 60, rank=32), k)
                out[f"{key}: solve_cost_path one-shot, 5 costs, verify"] = path(backend.solve_cost_path(p, X, B[0], costs, eps, points, verify=True))
                with backend.ResidentProblem(p, X) as prob:
                    prob.build_preconditioner(32)
                    for k in (1, 3):
                        out[f"{key}: solve_pcg resident, rank 32, k = {k}"] = pcg(prob.solve_pcg(B[0] if k == 1 else B[:k], 1e-30, 60), k)
                    out[f"{key}: solve_cost_path resident, 5 costs, verify"] = path(prob.solve_cost_path(B[0], costs, eps, points, verify=True))
    # fp32 beyond 128 features: the two-vector symmetric split kernel
    X, B, vecs = case(300, 200, np.float32)
    for kernel in ("poly3", "rbf"):
        key = f"float32 {kernel} 300x200"
        with backend.ResidentProblem(param(kernel, 200), X) as prob:
            matvecs(prob, key, vecs)
            for k in (1, 2, 3):
                out[f"{key}: solve_lockstep k = {k}"] = lockstep(prob, B[:k], 1e-3, 300)
    # more than one row-block band under the lanes (colslab_band_mb = 1: tests/test_gpu_lockstep_bands.py has the arithmetic of the two shapes)
    for dt, points, features in ((np.float64, 5900, 20), (np.float32, 8400, 192)):
        X, B, vecs = case(points, features, dt)
        for kernel in ("poly3", "rbf"):
            key = f"{np.dtype(dt).name} {kernel} {points}x{features} colslab_band_mb 1"
            with backend.ResidentProblem(param(kernel, features), X, options=_capi.Options(colslab_band_mb=1)) as prob:
                matvecs(prob, key, vecs)
                out[f"{key}: cg_begin / 6 x cg_step / cg_finish"] = cg_steps(prob, B[0], 6)
                out[f"{key}: solve_lockstep k = 3, 6 iterations"] = lockstep(prob, B, 1e-30, 6)
                out[f"{key}: tile launches per matvec"] = str(prob.info()["tile_launches_per_matvec"])
    # the linear kernel over feature panels: fp64 beyond 256 features; fp32 beyond 128 -- but below 10 000 points only up to 256, beyond that one launch of the polynomial
    # kernel of degree 1 takes over (300 x 300), so 300 x 200 is the fp32 shape with the panel loop inside
    for dt, points, features in ((np.float32, 300, 300), (np.float32, 300, 200), (np.float64, 300, 300)):
        X, B, vecs = case(points, features, dt)
        key = f"{np.dtype(dt).name} linear {points}x{features}"
        with backend.ResidentProblem(param("linear", features), X) as prob:
            matvecs(prob, key, vecs)
            out[f"{key}: cg_begin / 12 x cg_step / cg_finish"] = cg_steps(prob, B[0], 12)
            out[f"{key}: tile launches per matvec"] = str(prob.info()["tile_launches_per_matvec"])


def timing_child(reps: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_multiclass, make_blobs_pm1
    from plssvm_amd.multiclass import one_vs_all_targets
    from plssvm_amd.parameter import Parameter

    out = {}

    def timed(name, call):
        for keep in [False] + [True] * reps:
            t0 = time.perf_counter()
            call()
            if keep:
                out.setdefault(name, []).append(1e3 * (time.perf_counter() - t0))

    X, y = make_blobs_pm1(10_000, 32, seed=42, dtype=np.float32)
    p = Parameter(kernel_type="rbf", gamma=1.0 / 32, cost=1.0)
    timed("a_10000x32_rbf_f32_200_iterations", lambda: backend.solve_system_of_linear_equations(p, X, y, 1e-30, 200))
    X, y = make_blobs_pm1(50_000, 128, seed=42, dtype=np.float32)
    p = Parameter(kernel_type="rbf", gamma=1.0 / 128, cost=1.0)
    timed("b_50000x128_rbf_f32_eps1e-3", lambda: backend.solve_system_of_linear_equations(p, X, y, 1e-3, 50_000))
    X64 = X.astype(np.float64)
    y64 = y.astype(np.float64)
    timed("d_solve_refined_50000x128_rbf_eps1e-10", lambda: backend.solve_refined(p, X64, y64, 1e-10, 50_000))
    del X64
    X, labels = make_blobs_multiclass(100_000, 64, 4, seed=42, dtype=np.float64)
    B = one_vs_all_targets(np.arange(4), labels, np.float64)
    p = Parameter(kernel_type="polynomial", degree=3, gamma=1.0 / 64, coef0=0.0, cost=1.0)

    def lockstep():
        with backend.ResidentProblem(p, X) as prob:
            prob.solve_lockstep(B, 1e-3, 100_000)

    timed("c_solve_lockstep_100000x64_poly3_f64_k4", lockstep)
    X, y = make_blobs_pm1(50_000, 32, seed=42, dtype=np.float32)
    p = Parameter(kernel_type="rbf", gamma=1.0 / 32, cost=1.0)
    timed("e_solve_pcg_50000x32_rbf_f32_rank256_eps1e-3", lambda: backend.solve_pcg(p, X, y, 1e-3, 50_000, rank=256))
    X, labels = make_blobs_multiclass(30_000, 192, 4, seed=42, dtype=np.float32)
    B = one_vs_all_targets(np.arange(4), labels, np.float64).astype(np.float32)
    p = Parameter(kernel_type="polynomial", degree=3, gamma=1.0 / 192, coef0=0.0, cost=1.0)
    timed("f_solve_lockstep_30000x192_poly3_f32_k4", lockstep)
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
    ap.add_argument("--child-timeout", type=int, default=400, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cg_recipe_bits.json"))
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
        res["bits"] = {name: {"parent": got["parent"].get(name), "new": got["new"].get(name)} for name in sorted(set(got["parent"]) | set(got["new"]))}
        failed = [name for name, d in res["bits"].items() if d["parent"] != d["new"]]
        not_run = sum(1 for d in res["bits"].values() if str(d["new"]).startswith("not run"))
        res["bits_summary"] = {"cases": len(res["bits"]), "equal": len(res["bits"]) - len(failed), "different": failed, "not_run": not_run}
        print(json.dumps(res["bits_summary"], indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
