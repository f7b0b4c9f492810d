#!/usr/bin/env python3
"""What the exact leave-one-out scores of the fixed-size LS-SVM cost, against a library built from the PARENT commit.

usage: reduced_loo_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 10] [--rows a,b] [--ranks 64,256,1024] [--costs 1,8] [--ks 1,4] [--budget-s S]
                             [--out profiles/reduced_loo.json]

(a) kernel   per row, rank and k, on ONE slab of the problem (its first min(N, 65 536) points, rows padded to 256): k_reduced_leverage beside the Gram kernels of the fit
             (k_reduced_gram + k_reduced_sum over rank + 1 + k columns, as time_gram_kernels measures them), `reps` device times each after an untimed run, median and
             spread.  What is counted, in multiplied entries (one multiply-add each, 2 flop):
               leverage, useful    rows x (m (m + 1) / 2 + m k)             the lower triangle of V and the k fitted columns
               leverage, executed  rows x sum over the 128-column blocks of 128 x (the block's contraction length: 128 (bk + 1) inside V^T, m rounded up to 16 otherwise)
               gram                rows x cols^2 / 2                         the lower triangle, cols = m + 1 + k (reduced_timing.py's count)
             TFLOP/s of each beside the 78.6 TFLOP/s fp64 matrix-core peak.  No rate is promised; the Gram kernel on the same slab is the yardstick.
(b) call     per row, rank, k and number of costs S: backend.fit_reduced_loo of this build (whole one-shot call: upload, preparation, pass 1, the S host factorisations
             and inverses, pass 2 with S leverage launches per slab, the downloads; medians of `reps` after a warm-up) with its landmark / gram / leverage / host
             milliseconds, against the PARENT's backend.fit_reduced -- which yields no leave-one-out value -- called once per cost: S x the median of `reps` single calls
             (their spread is reported; from 1 000 000 points on 3 samples).  ratio = loo call / (S x parent call): the price of the leave-one-out pass and of the per-cost
             V_s.  host_share = the S costs' host milliseconds / the call.
Rows where the ratio is poor are printed like the others.  One child process per library and row (PLSSVM_AMD_LIBRARY), each under a time limit of its own; a child that
fails ends the run and nothing more is started on the device.  A run adds its rows to an existing --out file."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FP64_PEAK_TFLOPS = 78.6
SLAB = 65536
# name -> (N, d, kernel, dtype): the shapes of profiles/reduced.json
ROWS = {
    "rbf50k_f32": (50_000, 128, "rbf", "float32"),
    "rbf50k_f64": (50_000, 128, "rbf", "float64"),
    "poly100k_f64": (100_000, 64, "polynomial", "float64"),
    "rbf1m_f32": (1_000_000, 128, "rbf", "float32"),
}


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def cost_grid(S):
    return [10.0 ** (-1 + 4 * s / max(S - 1, 1)) for s in range(S)] if S > 1 else [100.0]


def executed_entries(rows, m, k):
    m16 = (m + 15) // 16 * 16
    blocks = (m + k + 127) // 128
    return rows * sum(128 * (128 * (bk + 1) if 128 * (bk + 1) <= m else m16) for bk in range(blocks))


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
            fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        return ms

    N, d, kernel, dtype = ROWS[args.row]
    dtype = np.dtype(dtype).type
    X, y = make_blobs_pm1(N, d, seed=42, dtype=dtype)
    prm = Parameter(kernel_type=kernel, degree=3, gamma=1.0 / d, coef0=0.0, cost=100.0)
    ranks, ks, counts = [int(v) for v in args.ranks.split(",")], [int(v) for v in args.ks.split(",")], [int(v) for v in args.costs.split(",")]
    rng = np.random.default_rng(5)
    Y = {k: (y if k == 1 else np.stack([y] + [np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(dtype) for _ in range(k - 1)])) for k in ks}
    big = N >= 1_000_000
    out = {}
    if args.child == "parent":
        for rank in ranks:
            for k in ks:
                out[f"{rank},{k}"] = timed(lambda: backend.fit_reduced(prm, X, Y[k], rank), 3 if big else args.reps)
                print(f"  [{args.row} parent rank {rank} k {k}] {statistics.median(out[f'{rank},{k}']):.0f} ms", file=sys.stderr, flush=True)
    else:
        with backend.ResidentProblem(prm, X) as prob:
            for rank in ranks:
                for k in ks:
                    gram_ms, lev_ms = prob.time_leverage_kernel(rank, k, repeats=args.reps)
                    out[f"kernel,{rank},{k}"] = {"gram_ms": gram_ms.tolist(), "leverage_ms": lev_ms.tolist()}
        for rank in ranks:
            for k in ks:
                for S in counts:
                    costs = cost_grid(S)
                    ms = timed(lambda: backend.fit_reduced_loo(prm, X, Y[k], rank, costs), 3 if big else args.reps)
                    infos = backend.fit_reduced_loo(prm, X, Y[k], rank, costs)[3]["infos"]
                    out[f"call,{rank},{k},{S}"] = {"ms": ms, "landmark_ms": infos[0]["landmark_ms"], "gram_ms": infos[0]["gram_ms"], "leverage_ms": sum(i["leverage_ms"] for i in infos),
                                                   "host_ms": sum(i["host_ms"] for i in infos), "max_leverage": max(i["max_leverage"] for i in infos),
                                                   "jitter": max(i["jitter"] for i in infos)}
                    print(f"  [{args.row} rank {rank} k {k} costs {S}] {statistics.median(ms):.0f} ms", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--ranks", default="64,256,1024")
    ap.add_argument("--costs", default="1,8", help="numbers of costs of a grid")
    ap.add_argument("--ks", default="1,4", help="numbers of right-hand sides")
    ap.add_argument("--budget-s", type=float, default=0.0, help="start no further row after this many seconds (0: no limit)")
    ap.add_argument("--child-timeout", type=int, default=420, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduced_loo.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    ap.add_argument("--row")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    t_start = time.time()
    res = json.load(open(args.out)) if os.path.isfile(args.out) else {"rows": {}}
    res["not_measured"] = []

    def run_child(which, row):
        env = dict(os.environ)
        if which == "parent":
            env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
        else:
            env.pop("PLSSVM_AMD_LIBRARY", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--row", row, "--reps", str(args.reps), "--ranks", args.ranks, "--costs", args.costs, "--ks", args.ks]
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
        parent = run_child("parent", row)
        new = run_child("new", row) if parent is not None else None
        if parent is None or new is None:
            failed = True
            res["not_measured"].append(row)
            continue
        N, d, kernel, dtype = ROWS[row]
        rows = (min(N, SLAB) + 255) // 256 * 256
        rec = {"shape": f"{N}x{d}", "kernel": kernel, "dtype": dtype, "kernel_slab_rows": rows, "kernels": {}, "calls": {}}
        for key, v in new.items():
            what, *rest = key.split(",")
            if what == "kernel":
                m, k = (int(x) for x in rest)
                g, lv = summary(v["gram_ms"]), summary(v["leverage_ms"])
                useful, executed, gram = rows * (m * (m + 1) // 2 + m * k), executed_entries(rows, m, k), rows * (m + 1 + k) ** 2 // 2
                rec["kernels"][f"rank {m}, k {k}"] = {
                    "leverage_ms": lv["median"], "leverage_spread": lv["spread"], "gram_ms": g["median"], "gram_spread": g["spread"], "samples": lv["n"],
                    "leverage_tflops_useful": 2 * useful / (lv["median"] * 1e-3) / 1e12, "leverage_tflops_executed": 2 * executed / (lv["median"] * 1e-3) / 1e12,
                    "gram_tflops": 2 * gram / (g["median"] * 1e-3) / 1e12, "leverage_executed_fraction_of_fp64_peak": 2 * executed / (lv["median"] * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                    "leverage_over_gram_time": lv["median"] / g["median"]}
            else:
                m, k, S = (int(x) for x in rest)
                s, base = summary(v["ms"]), summary(parent[f"{m},{k}"])
                rec["calls"][f"rank {m}, k {k}, costs {S}"] = {
                    "loo_call_ms": s["median"], "loo_call_spread": s["spread"], "samples": s["n"], "parent_fit_reduced_ms": base["median"], "parent_fit_reduced_spread": base["spread"],
                    "parent_samples": base["n"], "parent_once_per_cost_ms": S * base["median"], "ratio": s["median"] / (S * base["median"]), "landmark_ms": v["landmark_ms"],
                    "gram_ms": v["gram_ms"], "leverage_ms": v["leverage_ms"], "host_ms": v["host_ms"], "host_share": v["host_ms"] / s["median"], "max_leverage": v["max_leverage"],
                    "jitter": v["jitter"], "slower_than_parent_once_per_cost": s["median"] > S * base["median"]}
        res["rows"][row] = rec
        print(row, json.dumps({"kernels": {n: {"lev_ms": round(v["leverage_ms"], 3), "gram_ms": round(v["gram_ms"], 3), "lev_TF_exec": round(v["leverage_tflops_executed"], 1),
                                              "lev_TF_useful": round(v["leverage_tflops_useful"], 1), "gram_TF": round(v["gram_tflops"], 1)} for n, v in rec["kernels"].items()},
                               "calls": {n: {"loo_ms": round(v["loo_call_ms"], 1), "parent_x_S_ms": round(v["parent_once_per_cost_ms"], 1), "ratio": round(v["ratio"], 2),
                                             "host_share": round(v["host_share"], 2), "leverage_ms": round(v["leverage_ms"], 2)} for n, v in rec["calls"].items()}}), flush=True)
        write()
    res["method"] = (f"one child process per library and row; {args.reps} timed repetitions after a warm-up (3 from 1 000 000 points on), medians, spread = (max - min) / median; "
                     f"kernels: device time on one slab of min(N, {SLAB}) rows padded to 256; TFLOP/s = 2 x multiplied entries / time, entries as the tool's docstring counts them, "
                     f"against the {FP64_PEAK_TFLOPS} TFLOP/s fp64 matrix-core peak; calls: wall clock of the whole one-shot call; parent_once_per_cost_ms = S x the median of the "
                     f"parent's single fit_reduced call (which yields no leave-one-out value); landmark / gram / leverage / host ms: one further call's lssvm_reduced_loo_info, "
                     f"leverage and host summed over the costs; cost grids: 100 (S = 1), 0.1 ... 1000 logarithmic (S = 8)")
    write()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
