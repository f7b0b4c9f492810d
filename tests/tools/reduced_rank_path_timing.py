#!/usr/bin/env python3
"""What the rank path of the fixed-size LS-SVM costs against one leave-one-out call per rank.  Reported, not asserted; no ratio is fixed in
advance.  Both baselines come from the PARENT commit's library, never from the build under test.

usage: reduced_rank_path_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--rows a,b] [--reps 10] [--out profiles/reduced_rank_path.json]

Per row (the four shapes of the README's fixed-size tables), one child process per library and row (PLSSVM_AMD_LIBRARY selects the library):

  (a) kernel   on one slab (lssvm_mi355_problem_time_leverage_kernel and, beside it, _time_leverage_prefix_kernel: the same slab, an identity V, ones for z / beta), device
               time: the parent's k_reduced_leverage at rank 64 / 256 / 1 024 with k = 1, 4 against this build's k_reduced_leverage_prefix at the same rank with R = 1, 4, 16
               checkpoints (R = 1: the rank itself; else evenly spaced up to the rank).  ratio = prefix / parent, spread = the parent's (max - min) / median; a cell is
               `acceptable` where ratio + spread < 2 (R checkpoints for less than two launches of the old kernel).
  (b) call     wall clock: this build's fit_reduced_rank_path at rank 1 024 with the checkpoints (64, 128, 256, 512, 1 024) and 4 costs against the parent's
               fit_reduced_loo called once per rank on landmarks[:r] with the same 4 costs, summed; both factors, k = 1 and k = 4.  A cell is a GAIN only where 1 - ratio
               exceeds the parent's spread.  And the case that cannot pay: the single checkpoint (1 024,) against the parent's one call at rank 1 024.

Medians of `reps` repeats after a warm-up (3 at a million points).  A child that fails ends the run and nothing more is started on the device.  A run adds its rows to an
existing --out file; a row that was not run is listed under `not_measured`."""

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
KERNEL_RANKS, KERNEL_R, KS = (64, 256, 1024), (1, 4, 16), (1, 4)
CALL_RANKS = (64, 128, 256, 512, 1024)
FACTORS = ("host", "device")


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def checkpoints(rank, R):
    return [rank * (i + 1) // R for i in range(R)]


def child(args):
    """One library, one row: a JSON line."""
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    N, d, kernel, dtype = ROWS[args.child]
    X, y = make_blobs_pm1(N, d, seed=42, dtype=np.dtype(dtype))
    rng = np.random.default_rng(7)
    Y4 = np.stack([y] + [np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(y.dtype) for _ in range(3)])
    reps = args.reps if N < 1_000_000 else min(args.reps, 3)
    result = {"kernel": {}, "call": {}}
    with backend.ResidentProblem(Parameter(kernel_type=kernel, gamma=1.0 / d, cost=1.0), X) as prob:
        for rank in KERNEL_RANKS:
            for k in KS:
                if args.parent:
                    result["kernel"][f"rank {rank}, k {k}"] = summary(prob.time_leverage_kernel(rank, k=k, repeats=reps)[1].tolist())
                else:
                    for R in KERNEL_R:
                        result["kernel"][f"rank {rank}, k {k}, R {R}"] = summary(prob.time_leverage_prefix_kernel(rank, checkpoints(rank, R), k=k, repeats=reps).tolist())
        lms = prob.fit_reduced(y, CALL_RANKS[-1])[2]  # the library's landmarks, in their order
        for factor in FACTORS:
            for k in KS:
                Y = y if k == 1 else Y4
                key = f"factor {factor}, k {k}"
                if args.parent:
                    per_rank = {r: [] for r in CALL_RANKS}
                    for rep in range(reps + 1):
                        for r in CALL_RANKS:
                            t0 = time.perf_counter()
                            prob.fit_reduced_loo(Y, r, COSTS, landmarks=lms[:r], factor=factor)
                            if rep:
                                per_rank[r].append((time.perf_counter() - t0) * 1e3)
                    result["call"][key] = {"once_per_rank_ms": summary([sum(per_rank[r][i] for r in CALL_RANKS) for i in range(reps)]),
                                           "rank_1024_alone_ms": summary(per_rank[CALL_RANKS[-1]])}
                else:
                    path, single = [], []
                    for rep in range(reps + 1):
                        t0 = time.perf_counter()
                        prob.fit_reduced_rank_path(Y, CALL_RANKS[-1], CALL_RANKS, COSTS, landmarks=lms, factor=factor)
                        t1 = time.perf_counter()
                        prob.fit_reduced_rank_path(Y, CALL_RANKS[-1], CALL_RANKS[-1:], COSTS, landmarks=lms, factor=factor)
                        if rep:
                            path.append((t1 - t0) * 1e3)
                            single.append((time.perf_counter() - t1) * 1e3)
                    result["call"][key] = {"rank_path_ms": summary(path), "single_checkpoint_ms": summary(single)}
    print(json.dumps(result))


def run_child(name, args, parent):
    env = dict(os.environ)
    env.pop("PLSSVM_AMD_LIBRARY", None)
    if parent:
        env["PLSSVM_AMD_LIBRARY"] = args.parent_lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps)]
    done = subprocess.run(cmd + (["--parent"] if parent else []), env=env, capture_output=True, text=True, timeout=1100)
    if done.returncode != 0:
        print(done.stdout + done.stderr)
        sys.exit(f"{name}: the child of {'the parent library' if parent else 'this build'} failed ({done.returncode}); nothing more is started")
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduced_rank_path.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--parent", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        sys.exit("--parent-lib: the parent commit's libplssvm_amd.so is the yardstick; without it nothing is measured")
    out = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    out["method"] = ("(a) device time on one slab: the PARENT library's k_reduced_leverage (time_leverage_kernel) against this build's k_reduced_leverage_prefix "
                     "(time_leverage_prefix_kernel) at the same rank; acceptable where ratio + the parent's spread < 2.  (b) wall clock: fit_reduced_rank_path at rank 1024 with the "
                     "checkpoints 64, 128, 256, 512, 1024 and 4 costs against the PARENT library's fit_reduced_loo once per rank on landmarks[:r] with the same costs; the single "
                     "checkpoint (1024,) against the parent's one call at rank 1024.  One child process per library and row; medians after a warm-up; spread = (max - min) / median")
    out.setdefault("rows", {})
    for name in args.rows.split(","):
        N, d, kernel, dtype = ROWS[name]
        this, parent = run_child(name, args, False), run_child(name, args, True)
        row = {"N": N, "d": d, "kernel": kernel, "dtype": dtype, "reps": args.reps if N < 1_000_000 else min(args.reps, 3), "kernel_cells": {}, "call_cells": {}}
        for key, mine in this["kernel"].items():
            base = parent["kernel"][key.rsplit(", R", 1)[0]]
            ratio = mine["median"] / base["median"]
            row["kernel_cells"][key] = {"prefix_ms": mine, "parent_leverage_ms": base, "ratio": ratio, "parent_spread": base["spread"], "acceptable": ratio + base["spread"] < 2.0}
            print(f"{name} kernel {key}: parent {base['median']:.3f} ms (spread {base['spread']:.3f}), prefix {mine['median']:.3f} ms, ratio {ratio:.3f}", flush=True)
        for key, mine in this["call"].items():
            base = parent["call"][key]
            ratio = mine["rank_path_ms"]["median"] / base["once_per_rank_ms"]["median"]
            single = mine["single_checkpoint_ms"]["median"] / base["rank_1024_alone_ms"]["median"]
            row["call_cells"][key] = dict(mine, **base, ratio=ratio, parent_spread=base["once_per_rank_ms"]["spread"], gain=1.0 - ratio > base["once_per_rank_ms"]["spread"],
                                          loses=ratio - 1.0 > base["once_per_rank_ms"]["spread"], single_checkpoint_ratio=single,
                                          single_checkpoint_parent_spread=base["rank_1024_alone_ms"]["spread"])
            print(f"{name} call {key}: parent once per rank {base['once_per_rank_ms']['median']:.1f} ms (spread {base['once_per_rank_ms']['spread']:.3f}), rank path "
                  f"{mine['rank_path_ms']['median']:.1f} ms, ratio {ratio:.3f}; single checkpoint x{single:.3f} of the parent's call at rank 1024", flush=True)
        row["kernel_cells_not_acceptable"] = sorted(key for key, c in row["kernel_cells"].items() if not c["acceptable"])
        out["rows"][name] = row
        out["not_measured"] = sorted(set(ROWS) - set(out["rows"]))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
