#!/usr/bin/env python3
"""What the Nystrom preconditioner saves -- and where it loses -- against a library built from the PARENT commit.

usage: pcg_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 10] [--rows a,b] [--ranks 64,256,512] [--budget-s S] [--out profiles/pcg.json]

Rows (C = 100 unless named; gamma = 1 / features; blobs = make_blobs_pm1, uniform = [-1, 1]^d with random labels):
  rbf50k_f64_1e-6, rbf50k_f64_1e-10   50 000 x 128 rbf blobs, float64
  rbf50k_f32_1e-4                     the same model in float32
  poly100k_f64_1e-6, _1e-10           100 000 x 64 polynomial(3) blobs, float64, C = 10
  rbf50kx8_f32_1e-4                   a low-dimensional rbf set, 50 000 x 8 blobs, float32
  adverse20kx256_f32_1e-4             deliberately adverse: 20 000 x 256 uniform data (flat spectrum), rank 64 only
  ova4_rbf50k_f32_1e-4                k = 4 one-vs-all right-hand sides of 50 000 x 128 blobs: four parent solves against ONE solve_pcg call
Per row this records, as medians of `--reps` repetitions after a warm-up,
  cg    the parent's one-shot lssvm_mi355_solve_* at the same eps (the stop test is the same, so iterations and times compare directly): whole-call wall time,
        iterations, its tile kernel's time per Gram pass, and its run-to-run spread (max - min) / median -- the yardstick beside every ratio;
  pcg   per rank, backend.solve_pcg of this build (one-shot: upload, preparation, the preconditioner, the solves): whole-call wall time, iterations, and from one
        resident run build_ms on its own, apply_ms per iteration and the bytes per second the apply's two streaming kernels reach together
        (2 x (rank + 1) x n reals / apply_ms: a lower bound, the small solve kernel between them is inside the time);
  both  the true relative residual |b - Abar x| / |b - Abar 1| by a matvec of the resident problem.
ratio = pcg / cg: below 1 PCG is faster.  `wx_bytes_per_s`: what the linear predictor's w.x kernel reaches on the same box (400 000 x 128 float32), measured once per run.
One child process per library and row (PLSSVM_AMD_LIBRARY), each under a time limit of its own; a child that fails ends the run, and nothing more is started on the
device.  With --budget-s no further row is started once that many seconds have passed.  A run adds its rows to an existing --out file."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# name -> (N, d, kernel, dtype, data, cost, eps, right-hand sides, ranks or None for --ranks)
ROWS = {
    "rbf50k_f64_1e-6": (50_000, 128, "rbf", "float64", "blobs", 100.0, 1e-6, 1, None),
    "rbf50k_f64_1e-10": (50_000, 128, "rbf", "float64", "blobs", 100.0, 1e-10, 1, None),
    "rbf50k_f32_1e-4": (50_000, 128, "rbf", "float32", "blobs", 100.0, 1e-4, 1, None),
    "poly100k_f64_1e-6": (100_000, 64, "polynomial", "float64", "blobs", 10.0, 1e-6, 1, None),
    "poly100k_f64_1e-10": (100_000, 64, "polynomial", "float64", "blobs", 10.0, 1e-10, 1, None),
    "rbf50kx8_f32_1e-4": (50_000, 8, "rbf", "float32", "blobs", 100.0, 1e-4, 1, None),
    "adverse20kx256_f32_1e-4": (20_000, 256, "rbf", "float32", "uniform", 100.0, 1e-4, 1, [64]),
    "ova4_rbf50k_f32_1e-4": (50_000, 128, "rbf", "float32", "blobs4", 100.0, 1e-4, 4, None),
}


def child(args) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    N, d, kernel, dtype, data, cost, eps, k, _ = ROWS[args.row]
    dtype = np.dtype(dtype).type
    if data == "uniform":
        rng = np.random.default_rng(42)
        X = rng.uniform(-1.0, 1.0, (N, d)).astype(dtype)
        Y = np.where(rng.random((1, N)) < 0.5, -1.0, 1.0).astype(dtype)
    else:
        X, y = make_blobs_pm1(N, d, seed=42, dtype=dtype)
        Y = y[None, :]
        if data == "blobs4":  # four one-vs-all targets from the quadrant of the first two features
            cls = (X[:, 0] > np.median(X[:, 0])).astype(int) * 2 + (X[:, 1] > np.median(X[:, 1])).astype(int)
            Y = np.where(cls[None, :] == np.arange(4)[:, None], 1.0, -1.0).astype(dtype)
    prm = Parameter(kernel_type=kernel, degree=3, gamma=1.0 / d, coef0=0.0, cost=cost)
    n = N - 1

    def timed(fn):
        fn()  # warm-up
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            result = fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        return ms, result

    out = {}
    with backend.ResidentProblem(prm, X) as prob:
        def true_residual(alpha, y):
            b = (y[:n] - y[n]).astype(np.float64)
            zero = np.zeros(n, dtype)
            r0 = b - prob.matvec(np.ones(n, dtype), zero).astype(np.float64)
            r = b - prob.matvec(np.ascontiguousarray(alpha[:n]), zero).astype(np.float64)
            return float(np.linalg.norm(r) / np.linalg.norm(r0))

        if args.child == "parent":
            ms, solved = timed(lambda: [backend.solve_system_of_linear_equations(prm, X, y, eps, args.max_iter) for y in Y])
            out = {"ms": ms, "iterations": [s[2]["iterations"] for s in solved], "converged": [s[2]["converged"] for s in solved],
                   "gram_kernel_ms": [s[2]["matvec_kernel_ms"] for s in solved], "true_rel_residual": [true_residual(s[0], y) for s, y in zip(solved, Y)]}
        else:
            for rank in (int(r) for r in args.ranks.split(",")):
                ms, (alphas, _, infos) = timed(lambda: backend.solve_pcg(prm, X, Y, eps, args.max_iter, rank=rank))
                built = prob.build_preconditioner(rank)
                _, _, resident = prob.solve_pcg(Y, eps, args.max_iter)
                apply_ms = statistics.median(i["apply_ms"] for i in resident)
                streamed = 2.0 * (rank + 1) * n * np.dtype(dtype).itemsize
                out[str(rank)] = {"ms": ms, "iterations": [i["iterations"] for i in infos], "converged": [i["converged"] for i in infos],
                                  "gram_passes": [i["gram_passes"] for i in infos], "build_ms": built["build_ms"], "build_host_ms": built["host_ms"], "jitter": built["jitter"],
                                  "device_bytes": built["device_bytes"], "apply_ms": apply_ms, "apply_bytes_per_s": streamed / (apply_ms * 1e-3) if apply_ms > 0 else None,
                                  "true_rel_residual": [true_residual(a, y) for a, y in zip(alphas, Y)]}
                print(f"  [{args.row} rank {rank}] {statistics.median(ms):.0f} ms, {out[str(rank)]['iterations']} iterations", file=sys.stderr, flush=True)
    if args.child == "new" and args.wx:
        P = np.random.default_rng(1).standard_normal((400_000, 128)).astype(np.float32)
        sv, alpha = P[:1000].copy(), np.ones(1000, np.float32)
        info, kernel_ms = {}, []
        _, w = backend.predict_values(Parameter(kernel_type="linear"), sv, alpha, 0.0, None, P, info_out=info)
        for _ in range(args.reps):
            backend.predict_values(Parameter(kernel_type="linear"), sv, alpha, 0.0, w, P, info_out=info)
            kernel_ms.append(info["kernel_ms"])
        out["wx_bytes_per_s"] = P.nbytes / (statistics.median(kernel_ms) * 1e-3)
    print("RESULT " + json.dumps(out), flush=True)


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--ranks", default="64,256,512")
    ap.add_argument("--max-iter", type=int, default=5000, help="iterations one solve may take")
    ap.add_argument("--budget-s", type=float, default=0.0, help="start no further row after this many seconds (0: no limit)")
    ap.add_argument("--child-timeout", type=int, default=600, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    ap.add_argument("--row")
    ap.add_argument("--wx", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    t_start = time.time()
    res = json.load(open(args.out)) if os.path.isfile(args.out) else {"rows": {}}  # (a later run adds its rows to the file)
    res["not_measured"] = []

    def run_child(which, row, extra=()):
        env = dict(os.environ)
        if which == "parent":
            env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
        else:
            env.pop("PLSSVM_AMD_LIBRARY", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--row", row, "--reps", str(args.reps), "--max-iter", str(args.max_iter)] + list(extra)
        try:
            proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)  # (its progress lines go to this process's stderr)
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

    failed, wx_done = False, "wx_bytes_per_s" in res
    for row in args.rows.split(","):
        if failed or (args.budget_s > 0 and time.time() - t_start > args.budget_s):
            res["not_measured"].append(row)
            continue
        ranks = ROWS[row][8] or [int(r) for r in args.ranks.split(",")]
        parent = run_child("parent", row)
        new = run_child("new", row, ["--ranks", ",".join(str(r) for r in ranks)] + ([] if wx_done else ["--wx"])) if parent is not None else None
        if parent is None or new is None:
            failed = True
            res["not_measured"].append(row)
            continue
        if "wx_bytes_per_s" in new:
            res["wx_bytes_per_s"] = new.pop("wx_bytes_per_s")
            wx_done = True
        cg = summary(parent["ms"])
        N, d, kernel, dtype, data, cost, eps, k, _ = ROWS[row]
        rec = {"shape": f"{N}x{d}", "kernel": kernel, "dtype": dtype, "data": data, "cost": cost, "eps": eps, "right_hand_sides": k, "samples": cg["n"],
               "cg_ms": cg["median"], "cg_spread": cg["spread"], "cg_iterations": parent["iterations"], "cg_converged": parent["converged"],
               "cg_gram_kernel_ms": statistics.median(parent["gram_kernel_ms"]), "cg_true_rel_residual": parent["true_rel_residual"], "pcg": {}}
        for rank, r in new.items():
            s = summary(r["ms"])
            saved = sum(parent["iterations"]) - sum(r["iterations"])
            per_iteration = rec["cg_gram_kernel_ms"]  # what an iteration saved is worth, at least: its Gram pass
            rec["pcg"][rank] = {"ms": s["median"], "spread": s["spread"], "ratio": s["median"] / cg["median"], "iterations": r["iterations"], "converged": r["converged"],
                                "gram_passes": r["gram_passes"], "build_ms": r["build_ms"], "build_host_ms": r["build_host_ms"], "apply_ms": r["apply_ms"],
                                "apply_bytes_per_s": r["apply_bytes_per_s"], "device_bytes": r["device_bytes"], "jitter": r["jitter"], "true_rel_residual": r["true_rel_residual"],
                                "iterations_saved": saved,
                                "break_even_iterations_saved": (r["build_ms"] + sum(r["iterations"]) * r["apply_ms"]) / per_iteration if per_iteration > 0 else None}
        res["rows"][row] = rec
        print(row, json.dumps({"cg_ms": rec["cg_ms"], "cg_spread": rec["cg_spread"], "cg_iterations": rec["cg_iterations"],
                               "pcg": {rk: (round(v["ms"], 1), round(v["ratio"], 3), v["iterations"]) for rk, v in rec["pcg"].items()}}), flush=True)
        write()
    res["method"] = (f"one child process per library and row, {args.reps} timed repetitions after a warm-up, medians; wall clock of the whole one-shot call(s), upload, preparation and "
                     f"the preconditioner's build included; at most {args.max_iter} iterations per solve; spread = (max - min) / median of the parent's solves; ratio = pcg / cg; "
                     "break_even_iterations_saved = (build_ms + iterations x apply_ms) / the parent's tile-kernel time per Gram pass: the iterations PCG must save to pay for itself")
    write()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
