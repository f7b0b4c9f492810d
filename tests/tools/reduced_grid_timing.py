#!/usr/bin/env python3
"""What the (gamma, cost) grid of the fixed-size LS-SVM costs against G separate leave-one-out calls.  Reported, not asserted; no ratio is fixed
in advance.

usage: reduced_grid_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--rows a,b] [--ranks 64,256,1024] [--gammas 1,4,8] [--reps 10] [--factor device]
                              [--out profiles/reduced_grid.json]

Per row (the shapes of profiles/reduced_loo.json), rank and number of gammas G (a geometric grid around the row's own gamma; 4 costs, one right-hand side, the library's
landmarks):

  grid      this build: ONE resident problem created with the first gamma, fit_reduced_grid with product "matrix" and with product "ordered"
  parent    the PARENT commit's library (one child process per library and row: PLSSVM_AMD_LIBRARY): G problems created with the grid's gammas, fit_reduced_loo on each

Wall-clock medians of `reps` repeats after a warm-up (3 at a million points), spread = (max - min) / median; the set-up (creating the problem: upload and preparation) is
timed and reported apart from the calls, and `ratio` = grid / parent is given with and without it.  A cell is a GAIN only where 1 - ratio exceeds the larger of the parent's and this build's spread; the
cells that lose are listed (G = 1 must: it adds a pass over D).  Kernel level, from the device times the calls report: D per pass (`accumulate_ms` / 2) against the
parent's landmark block per pass (`landmark_ms` / 2), the matrix product's TFLOP/s counting 2 rows m ldx flop beside the 78.6 TFLOP/s fp64 matrix-core peak, and
k_kernel_values in TB/s (16 bytes per entry).  A child that fails ends the run and nothing more is started on the device.  A run adds its rows to an existing --out file."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# name -> (N, d, kernel, dtype)
ROWS = {
    "rbf50k_f32": (50_000, 128, "rbf", "float32"),
    "rbf50k_f64": (50_000, 128, "rbf", "float64"),
    "poly100k_f64": (100_000, 64, "polynomial", "float64"),
    "rbf1m_f32": (1_000_000, 128, "rbf", "float32"),
}
COSTS = (0.1, 1.0, 10.0, 100.0)
PEAK_TFLOPS = 78.6


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def gammas_of(d, G):
    return [(1.0 / d) * 2.0 ** (g - G // 2) for g in range(G)]


def padded(d, dtype):
    kc = 32 if dtype == "float32" else 16
    return (d + kc - 1) // kc * kc  # (the rows' feature counts are multiples of 64: no further padding)


def child(args):
    """One library, one row, all ranks and grid sizes: a JSON line."""
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    N, d, kernel, dtype = ROWS[args.child]
    X, y = make_blobs_pm1(N, d, seed=42, dtype=np.dtype(dtype))
    reps = args.reps if N < 1_000_000 else min(args.reps, 3)
    result = {}
    for rank in (int(r) for r in args.ranks.split(",")):
        for G in (int(g) for g in args.gammas.split(",")):
            gammas = gammas_of(d, G)
            cell = {}
            if args.parent:
                setup, calls, landmark = [], [], []
                for rep in range(reps + 1):
                    t_setup = t_call = lm_ms = 0.0
                    for gamma in gammas:
                        t0 = time.perf_counter()
                        with backend.ResidentProblem(Parameter(kernel_type=kernel, gamma=gamma, cost=1.0), X) as prob:
                            prob.synchronize()
                            t1 = time.perf_counter()
                            report = prob.fit_reduced_loo(y, rank, COSTS, factor=args.factor)[3]
                            t2 = time.perf_counter()
                        t_setup, t_call, lm_ms = t_setup + (t1 - t0) * 1e3, t_call + (t2 - t1) * 1e3, lm_ms + report["infos"][0]["landmark_ms"]
                    if rep:
                        setup.append(t_setup)
                        calls.append(t_call)
                        landmark.append(lm_ms / (2 * G))
                cell["parent"] = {"setup_ms": summary(setup), "calls_ms": summary(calls), "landmark_block_ms_per_pass": summary(landmark)}
            else:
                for product in ("matrix", "ordered"):
                    setup, calls, acc, val = [], [], [], []
                    for rep in range(reps + 1):
                        t0 = time.perf_counter()
                        with backend.ResidentProblem(Parameter(kernel_type=kernel, gamma=gammas[0], cost=1.0), X) as prob:
                            prob.synchronize()
                            t1 = time.perf_counter()
                            report = prob.fit_reduced_grid(y, rank, gammas, COSTS, factor=args.factor, product=product)[3]
                            t2 = time.perf_counter()
                        if rep:
                            setup.append((t1 - t0) * 1e3)
                            calls.append((t2 - t1) * 1e3)
                            acc.append(report["infos"][0][0]["accumulate_ms"] / 2)
                            val.append(sum(row[0]["values_ms"] for row in report["infos"]) / (2 * G))
                    a, v = summary(acc), summary(val)
                    cell[product] = {"setup_ms": summary(setup), "calls_ms": summary(calls), "accumulate_ms_per_pass": a, "values_ms_per_pass_and_gamma": v,
                                     "accumulate_tflops": 2.0 * N * rank * padded(d, dtype) / (a["median"] * 1e-3) / 1e12 if product == "matrix" else None,
                                     "values_tb_per_s": 16.0 * N * rank / (v["median"] * 1e-3) / 1e12}
            result[f"{rank}x{G}"] = cell
    print(json.dumps(result))


def run_child(name, args, parent):
    env = dict(os.environ)
    env.pop("PLSSVM_AMD_LIBRARY", None)
    if parent:
        env["PLSSVM_AMD_LIBRARY"] = args.parent_lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps), "--ranks", args.ranks, "--gammas", args.gammas, "--factor", args.factor]
    done = subprocess.run(cmd + (["--parent"] if parent else []), env=env, capture_output=True, text=True, timeout=1100)
    if done.returncode != 0:
        print(done.stdout + done.stderr)
        sys.exit(f"{name}: the child of {'the parent library' if parent else 'this build'} failed ({done.returncode}); nothing more is started")
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--ranks", default="64,256,1024")
    ap.add_argument("--gammas", default="1,4,8")
    ap.add_argument("--factor", default="device")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduced_grid.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--parent", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        sys.exit("--parent-lib: the parent commit's libplssvm_amd.so is the yardstick; without it nothing is measured")
    out = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    out["method"] = ("one right-hand side, 4 costs, the library's landmarks, a geometric gamma grid around 1 / d; this build: one resident problem and one fit_reduced_grid call per "
                     "product; parent: G problems and G fit_reduced_loo calls with the PARENT commit's library; one child process per library and row; wall-clock medians after a "
                     "warm-up, spread = (max - min) / median; set-up (creating the problem) apart from the calls; kernel-level figures from the calls' own device times")
    out.setdefault("rows", {})
    for name in args.rows.split(","):
        N, d, kernel, dtype = ROWS[name]
        this, parent = run_child(name, args, False), run_child(name, args, True)
        row = out["rows"].setdefault(name, {"N": N, "d": d, "kernel": kernel, "dtype": dtype, "cells": {}})
        row["factor"], row["reps"] = args.factor, args.reps if N < 1_000_000 else min(args.reps, 3)
        for key in this:
            r = dict(this[key], **parent[key])
            p = r["parent"]
            for product in ("matrix", "ordered"):
                c = r[product]
                c["ratio_calls"] = c["calls_ms"]["median"] / p["calls_ms"]["median"]
                c["ratio_with_setup"] = (c["calls_ms"]["median"] + c["setup_ms"]["median"]) / (p["calls_ms"]["median"] + p["setup_ms"]["median"])
                c["parent_spread_calls"] = p["calls_ms"]["spread"]
                c["spread_calls"] = max(p["calls_ms"]["spread"], c["calls_ms"]["spread"])  # (of either side: a cell inside it is a tie)
                c["gain"] = 1.0 - c["ratio_calls"] > c["spread_calls"]
                c["loses"] = c["ratio_calls"] - 1.0 > c["spread_calls"]
                c["accumulate_over_parent_landmark_block"] = c["accumulate_ms_per_pass"]["median"] / p["landmark_block_ms_per_pass"]["median"]
            row["cells"][key] = r
            m = r["matrix"]
            print(f"{name} rank x G {key}: parent calls {p['calls_ms']['median']:.1f} ms (spread {p['calls_ms']['spread']:.3f}, set-up {p['setup_ms']['median']:.1f} ms); matrix x{m['ratio_calls']:.3f} "
                  f"(with set-up x{m['ratio_with_setup']:.3f}), ordered x{r['ordered']['ratio_calls']:.3f}; D per pass {m['accumulate_ms_per_pass']['median']:.3f} ms = "
                  f"{m['accumulate_tflops']:.1f} TFLOP/s ({m['accumulate_tflops'] / PEAK_TFLOPS:.2f} of peak), x{m['accumulate_over_parent_landmark_block']:.3f} of the parent's block; "
                  f"values {m['values_tb_per_s']:.2f} TB/s", flush=True)
        row["cells_that_lose"] = sorted(f"{key}/{product}" for key, r in row["cells"].items() for product in ("matrix", "ordered") if r[product]["loses"])
        row["cells_that_gain"] = sorted(f"{key}/{product}" for key, r in row["cells"].items() for product in ("matrix", "ordered") if r[product]["gain"])
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
