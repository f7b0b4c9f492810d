#!/usr/bin/env python3
"""What the device-factored fixed-size fits cost (factor="device"), against a library built from the PARENT commit.

usage: reduced_dense_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 10] [--rows a,b] [--ranks 64,256,512,1024] [--costs 1,8] [--ks 1,4]
                               [--budget-s S] [--out profiles/reduced_dense.json]

Per row (the four shapes of profiles/reduced_loo.json), rank and k: the whole one-shot call, wall clock, medians of `reps` after a warm-up (3 from 1 000 000 points on) with
the spread (max - min) / median, of
  fit       backend.fit_reduced                          this build with factor="device" | this build with factor="host" | the PARENT's call
  loo, S    backend.fit_reduced_loo with S costs         likewise
and from one further device-factored call the last attempt's assemble / factor / solve / invert milliseconds (summed over the costs), the kernels launched, the attempts,
beside the parent's host_ms.  ratio = device-factored call / parent's call; `faster` is set only where the gain exceeds the parent's spread.  No ratio is promised.
One child process per library and row (PLSSVM_AMD_LIBRARY), each under a time limit of its own; a child that fails ends the run and nothing more is started on the
device.  A run adds its rows to an existing --out file."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# name -> (N, d, kernel, dtype): the shapes of profiles/reduced_loo.json
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


def child(args) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    def timed(fn, reps):
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
    reps = 3 if N >= 1_000_000 else args.reps
    factors = [None] if args.child == "parent" else ["device", "host"]  # (the parent's entry points have no such keyword)
    out = {}
    for rank in ranks:
        for k in ks:
            for factor in factors:
                kw = {} if factor is None else {"factor": factor}
                name = factor or "parent"
                rec = {"ms": timed(lambda: backend.fit_reduced(prm, X, Y[k], rank, **kw), reps)}
                info = backend.fit_reduced(prm, X, Y[k], rank, **kw)[3]
                rec["host_ms"] = info["host_ms"]
                if factor == "device":
                    rec.update({n: info[n] for n in ("assemble_ms", "factor_ms", "solve_ms", "invert_ms", "launches", "attempts", "block")})
                out[f"fit,{rank},{k},{name}"] = rec
                for S in counts:
                    costs = cost_grid(S)
                    rec = {"ms": timed(lambda: backend.fit_reduced_loo(prm, X, Y[k], rank, costs, **kw), reps)}
                    infos = backend.fit_reduced_loo(prm, X, Y[k], rank, costs, **kw)[3]["infos"]
                    rec["host_ms"] = sum(i["host_ms"] for i in infos)
                    rec["leverage_ms"] = sum(i["leverage_ms"] for i in infos)
                    if factor == "device":
                        rec.update({n: sum(i[n] for i in infos) for n in ("assemble_ms", "factor_ms", "solve_ms", "invert_ms", "launches", "attempts")})
                    out[f"loo{S},{rank},{k},{name}"] = rec
                print(f"  [{args.row} {name} rank {rank} k {k}] fit {statistics.median(out[f'fit,{rank},{k},{name}']['ms']):.1f} ms", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--ranks", default="64,256,512,1024")
    ap.add_argument("--costs", default="1,8", help="numbers of costs of a leave-one-out grid")
    ap.add_argument("--ks", default="1,4", help="numbers of right-hand sides")
    ap.add_argument("--budget-s", type=float, default=0.0, help="start no further row after this many seconds (0: no limit)")
    ap.add_argument("--child-timeout", type=int, default=420, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduced_dense.json"))
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
        res["not_measured"] = [row for row in ROWS if row not in res["rows"]]  # (against ALL rows: one a run was not asked for is as unmeasured as one that failed)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")

    failed = False
    for row in args.rows.split(","):
        if failed or (args.budget_s > 0 and time.time() - t_start > args.budget_s):
            continue
        parent = run_child("parent", row)
        new = run_child("new", row) if parent is not None else None
        if parent is None or new is None:
            failed = True
            res["rows"].pop(row, None)  # (an earlier run's figures of a row that now fails are not kept as this build's)
            continue
        N, d, kernel, dtype = ROWS[row]
        rec = {"shape": f"{N}x{d}", "kernel": kernel, "dtype": dtype, "calls": {}}
        for key, v in new.items():
            what, m, k, factor = key.split(",")
            if factor != "device":
                continue
            dev, host, base = summary(v["ms"]), summary(new[f"{what},{m},{k},host"]["ms"]), summary(parent[f"{what},{m},{k},parent"]["ms"])
            ratio = dev["median"] / base["median"]
            call = "fit_reduced" if what == "fit" else f"fit_reduced_loo, costs {what[3:]}"
            rec["calls"][f"{call}, rank {m}, k {k}"] = {
                "device_ms": dev["median"], "device_spread": dev["spread"], "host_ms": host["median"], "host_spread": host["spread"], "parent_ms": base["median"],
                "parent_spread": base["spread"], "samples": dev["n"], "ratio_device_over_parent": ratio, "ratio_host_over_parent": host["median"] / base["median"],
                "faster": ratio < 1.0 - base["spread"], "slower": ratio > 1.0 + base["spread"], "assemble_ms": v["assemble_ms"], "factor_ms": v["factor_ms"], "solve_ms": v["solve_ms"],
                "invert_ms": v["invert_ms"], "launches": v["launches"], "attempts": v["attempts"], "host_left_ms": v["host_ms"], "parent_host_ms": parent[f"{what},{m},{k},parent"]["host_ms"]}
        res["rows"][row] = rec
        print(row, json.dumps({n: {"device_ms": round(c["device_ms"], 1), "host_ms": round(c["host_ms"], 1), "parent_ms": round(c["parent_ms"], 1), "ratio": round(c["ratio_device_over_parent"], 2),
                                   "parent_spread": round(c["parent_spread"], 2), "dense_ms": round(c["assemble_ms"] + c["factor_ms"] + c["solve_ms"] + c["invert_ms"], 2),
                                   "parent_host_ms": round(c["parent_host_ms"], 1), "launches": c["launches"]} for n, c in rec["calls"].items()}), flush=True)
        write()
    res["method"] = (f"one child process per library and row; {args.reps} timed repetitions after a warm-up (3 from 1 000 000 points on), medians, spread = (max - min) / median; wall clock "
                     f"of the whole one-shot call; device = this build with factor=\"device\", host = this build with factor=\"host\", parent = the parent commit's library; assemble / "
                     f"factor / solve / invert ms, launches and attempts: one further device-factored call's lssvm_dense_info, summed over the costs; parent_host_ms: the parent's "
                     f"host_ms summed over the costs; faster / slower: the ratio lies outside 1 -/+ the parent's spread; cost grids: 100 (S = 1), 0.1 ... 1000 logarithmic (S = 8)")
    write()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
