#!/usr/bin/env python3
"""What the fixed-size LS-SVM costs and gives against a library built from the PARENT commit.

usage: reduced_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 10] [--rows a,b] [--ranks 64,256,1024] [--budget-s S] [--out profiles/reduced.json]

(a) kernel   100 000 x 64 float64: Bhat^T Bhat of the rank-512 preconditioner (513 columns), ON ITS OWN BUFFER, by the parent's k_precond_gram<double> and by this
             build's matrix-core kernels (partial tiles + their sum): `reps` device times each after an untimed run, median and spread, achieved TFLOP/s = N cols^2 /
             time (the flop of the lower triangle) beside the 78.6 TFLOP/s fp64 matrix-core peak.  The 1 000 000 x rank 1 024 figure is gram_ms of the rbf1m_f32 row.
(b) call     per row and rank: backend.fit_reduced of this build (whole one-shot call: upload, preparation, the slabs, the host's solve; medians of `reps` after a
             warm-up) with its landmark / gram / host milliseconds, against the PARENT's one-shot fit at eps = 1e-3 on the same make_blobs data (whole call).  Held-out
             accuracy of both models on 20 000 fresh points.  The relative rms difference of the reduced model's decision values there is taken against the parent's
             fit carried to eps = 1e-8 (one more solve, not timed; at eps = 1e-3 CG stops after a few iterations and that model is itself far from the solution).
             From 1 000 000 points on the parent's fit is ONE sample without a warm-up and there is no eps = 1e-8 fit (both labelled so).
(c) predict  200 000 points against the reduced model and against the full one, resident predictor in both cases (the model in HBM before the clock starts).
Rows where the reduced model is less accurate or not faster are printed like the others.  One child process per library and row (PLSSVM_AMD_LIBRARY), each under a time
limit of its own; a child that fails ends the run and nothing more is started on the device.  A run adds its rows to an existing --out file."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FP64_PEAK_TFLOPS = 78.6
HELD_OUT, PREDICT_POINTS = 20_000, 200_000
# name -> (N, d, kernel, dtype, cost)
ROWS = {
    "rbf50k_f32": (50_000, 128, "rbf", "float32", 100.0),
    "rbf50k_f64": (50_000, 128, "rbf", "float64", 100.0),
    "poly100k_f64": (100_000, 64, "polynomial", "float64", 10.0),
    "rbf1m_f32": (1_000_000, 128, "rbf", "float32", 100.0),
}
EPS, TIGHT_EPS = 1e-3, 1e-8


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def child(args) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    def timed(fn, reps, warm=True):
        if warm:
            fn()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            result = fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        return ms, result

    if args.row == "kernel":
        N, d, rank = 100_000, 64, 512
        X, _ = make_blobs_pm1(N, d, seed=42, dtype=np.float64)
        with backend.ResidentProblem(Parameter(kernel_type="polynomial", degree=3, gamma=1.0 / d, coef0=0.0, cost=10.0), X) as prob:
            prob.build_preconditioner(rank)
            parent_ms, mfma_ms, diff = prob.time_gram_kernels(args.reps)
        print("RESULT " + json.dumps({"N": N, "cols": rank + 1, "parent_ms": parent_ms.tolist(), "mfma_ms": mfma_ms.tolist(), "max_rel_diff": diff}), flush=True)
        return

    N, d, kernel, dtype, cost = ROWS[args.row]
    dtype = np.dtype(dtype).type
    X_all, y_all = make_blobs_pm1(N + HELD_OUT, d, seed=42, dtype=dtype)
    X, y, X_test, y_test = X_all[:N], y_all[:N], X_all[N:], y_all[N:]
    P = np.resize(X_test, (PREDICT_POINTS, d))  # the held-out points, repeated: the predict batch
    prm = Parameter(kernel_type=kernel, degree=3, gamma=1.0 / d, coef0=0.0, cost=cost)

    def evaluate(sv, alpha, rho, time_it=True):
        with backend.Predictor(prm, sv, np.ascontiguousarray(alpha, dtype=dtype), float(rho), every_form=True) as predictor:
            values = np.asarray(predictor.predict(X_test), dtype=np.float64)
            ms = timed(lambda: predictor.predict(P), args.reps)[0] if time_it else []
        return values, ms

    out = {}
    if args.child == "parent":
        big = N >= 1_000_000
        ms, (alpha, rho, info) = timed(lambda: backend.solve_system_of_linear_equations(prm, X, y, EPS, N), 1 if big else args.reps, warm=not big)
        values, predict_ms = evaluate(X, alpha, rho)
        out = {"ms": ms, "single_sample": big, "iterations": info["iterations"], "converged": info["converged"], "avg_iteration_ms": info["avg_iteration_ms"],
               "accuracy": float(np.mean(np.where(values > 0, 1.0, -1.0) == y_test)), "predict_ms": predict_ms, "values": values.tolist(), "values_eps": EPS}
        if not big:  # the yardstick of the reduced models' decision values: the same fit carried to eps = 1e-8 (at eps = 1e-3 CG stops after a few iterations)
            alpha, rho, info = backend.solve_system_of_linear_equations(prm, X, y, TIGHT_EPS, N)
            values, _ = evaluate(X, alpha, rho, time_it=False)
            out.update({"values": values.tolist(), "values_eps": TIGHT_EPS, "tight_iterations": info["iterations"], "tight_converged": info["converged"],
                        "tight_accuracy": float(np.mean(np.where(values > 0, 1.0, -1.0) == y_test))})
    else:
        full = np.asarray(json.load(open(args.full_values)), dtype=np.float64) if args.full_values else None
        for rank in (int(r) for r in args.ranks.split(",")):
            ms, (betas, rho, used, _) = timed(lambda: backend.fit_reduced(prm, X, y, rank), args.reps)
            infos = [backend.fit_reduced(prm, X, y, rank)[3] for _ in range(3)]
            values, predict_ms = evaluate(np.ascontiguousarray(X[used.astype(np.int64)]), betas, rho)
            cols = rank + 2
            gram_ms = statistics.median(i["gram_ms"] for i in infos)
            out[str(rank)] = {"ms": ms, "landmark_ms": statistics.median(i["landmark_ms"] for i in infos), "gram_ms": gram_ms, "host_ms": statistics.median(i["host_ms"] for i in infos),
                              "library_total_ms": statistics.median(i["total_ms"] for i in infos), "slabs": infos[0]["slabs"], "jitter": infos[0]["jitter"],
                              "workspace_bytes": infos[0]["workspace_bytes"], "gram_tflops": N * cols * cols / (gram_ms * 1e-3) / 1e12,
                              "accuracy": float(np.mean(np.where(values > 0, 1.0, -1.0) == y_test)), "predict_ms": predict_ms,
                              "rel_rms_diff_to_full": None if full is None else float(np.sqrt(np.mean((values - full) ** 2) / np.mean(full ** 2)))}
            print(f"  [{args.row} rank {rank}] {statistics.median(ms):.0f} ms", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default="kernel," + ",".join(ROWS))
    ap.add_argument("--ranks", default="64,256,1024")
    ap.add_argument("--budget-s", type=float, default=0.0, help="start no further row after this many seconds (0: no limit)")
    ap.add_argument("--child-timeout", type=int, default=420, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduced.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    ap.add_argument("--row")
    ap.add_argument("--full-values")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    t_start = time.time()
    res = json.load(open(args.out)) if os.path.isfile(args.out) else {"rows": {}}
    res["not_measured"] = []

    def run_child(which, row, extra=()):
        env = dict(os.environ)
        if which == "parent":
            env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
        else:
            env.pop("PLSSVM_AMD_LIBRARY", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--row", row, "--reps", str(args.reps), "--ranks", args.ranks] + list(extra)
        try:
            proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
        except subprocess.TimeoutExpired:
            print(f"{row}, {which}: child exceeded {args.child_timeout} s; stopping", file=sys.stderr)
            return None
        line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if proc.returncode != 0 or line is None:
            print(f"{row}, {which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}", file=sys.stderr)
            return None
        return json.loads(line[len("RESULT "):])

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")

    failed = False
    for row in args.rows.split(","):
        if failed or (args.budget_s > 0 and time.time() - t_start > args.budget_s):
            res["not_measured"].append(row)
            continue
        if row == "kernel":
            k = run_child("new", "kernel")
            if k is None:
                failed = True
                res["not_measured"].append(row)
                continue
            parent, mfma = summary(k["parent_ms"]), summary(k["mfma_ms"])
            flop = k["N"] * k["cols"] ** 2
            res["kernel"] = {"shape": f"{k['N']} x {k['cols']} columns, float64", "parent_ms": parent["median"], "parent_spread": parent["spread"], "mfma_ms": mfma["median"],
                             "mfma_spread": mfma["spread"], "speedup": parent["median"] / mfma["median"], "parent_tflops": flop / (parent["median"] * 1e-3) / 1e12,
                             "mfma_tflops": flop / (mfma["median"] * 1e-3) / 1e12, "fraction_of_fp64_peak": flop / (mfma["median"] * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                             "max_rel_diff_of_the_results": k["max_rel_diff"], "samples": mfma["n"]}
            print("kernel", json.dumps(res["kernel"]), flush=True)
            write()
            continue
        parent = run_child("parent", row)
        new = None
        if parent is not None:
            values_file = args.out + f".{row}.values.tmp"
            with open(values_file, "w") as f:
                json.dump(parent.pop("values"), f)
            new = run_child("new", row, ["--full-values", values_file])
            os.remove(values_file)
        if parent is None or new is None:
            failed = True
            res["not_measured"].append(row)
            continue
        N, d, kernel, dtype, cost = ROWS[row]
        fit, predict = summary(parent["ms"]), summary(parent["predict_ms"])
        rec = {"shape": f"{N}x{d}", "kernel": kernel, "dtype": dtype, "cost": cost, "eps": EPS, "parent_fit_ms": fit["median"], "parent_fit_spread": fit["spread"],
               "parent_fit_samples": fit["n"], "parent_fit_single_sample_without_warm_up": parent["single_sample"], "parent_iterations": parent["iterations"],
               "parent_converged": parent["converged"], "parent_avg_iteration_ms": parent["avg_iteration_ms"], "parent_accuracy": parent["accuracy"],
               "parent_predict_ms": predict["median"], "parent_predict_spread": predict["spread"], "support_vectors": N, "rel_rms_diff_is_against_the_parent_at_eps": parent["values_eps"],
               "parent_tight_iterations": parent.get("tight_iterations"), "parent_tight_converged": parent.get("tight_converged"), "parent_tight_accuracy": parent.get("tight_accuracy"),
               "reduced": {}}
        for rank, r in new.items():
            s, ps = summary(r["ms"]), summary(r["predict_ms"])
            rec["reduced"][rank] = {"fit_ms": s["median"], "fit_spread": s["spread"], "fit_ratio": s["median"] / fit["median"], "landmark_ms": r["landmark_ms"], "gram_ms": r["gram_ms"],
                                    "host_ms": r["host_ms"], "library_total_ms": r["library_total_ms"], "slabs": r["slabs"], "jitter": r["jitter"], "workspace_bytes": r["workspace_bytes"],
                                    "gram_tflops": r["gram_tflops"], "gram_fraction_of_fp64_peak": r["gram_tflops"] / FP64_PEAK_TFLOPS, "accuracy": r["accuracy"],
                                    "rel_rms_diff_to_full": r["rel_rms_diff_to_full"], "predict_ms": ps["median"], "predict_spread": ps["spread"],
                                    "predict_ratio": ps["median"] / predict["median"], "less_accurate": r["accuracy"] < parent["accuracy"],
                                    "fit_not_faster": s["median"] >= fit["median"], "predict_not_faster": ps["median"] >= predict["median"]}
        res["rows"][row] = rec
        print(row, json.dumps({"parent_fit_ms": round(rec["parent_fit_ms"], 1), "parent_iterations": rec["parent_iterations"], "parent_accuracy": rec["parent_accuracy"],
                               "parent_predict_ms": round(rec["parent_predict_ms"], 2),
                               "reduced": {rk: {"fit_ms": round(v["fit_ms"], 1), "landmark_ms": round(v["landmark_ms"], 2), "gram_ms": round(v["gram_ms"], 2), "host_ms": round(v["host_ms"], 1),
                                                "accuracy": v["accuracy"], "rms": v["rel_rms_diff_to_full"], "predict_ms": round(v["predict_ms"], 2), "tflops": round(v["gram_tflops"], 2)}
                                           for rk, v in rec["reduced"].items()}}), flush=True)
        write()
    res["method"] = (f"one child process per library and row; {args.reps} timed repetitions after a warm-up, medians, spread = (max - min) / median; fit = wall clock of the whole "
                     f"one-shot call; the parent's fit at eps = {EPS} (from 1 000 000 points on: one sample without a warm-up); landmark / gram / host ms: medians of 3 calls' "
                     f"lssvm_reduced_info; gram_tflops = N (rank + 2)^2 / gram_ms against the {FP64_PEAK_TFLOPS} TFLOP/s fp64 matrix-core peak; accuracy on {HELD_OUT} fresh points of the "
                     f"same make_blobs_pm1 draw; predict = {PREDICT_POINTS} points through a resident predictor created before the clock starts")
    write()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
