#!/usr/bin/env python3
"""What the weights cost the fixed-size fit.  Reported, not asserted; no threshold is fixed in advance.

usage: reduced_weighted_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--rows a,b] [--ranks 64,256,1024] [--reps 10] [--out profiles/reduced_weighted.json]

Per row (the shapes of profiles/reduced.json) and rank, fit_reduced on a resident problem, one right-hand side, the library's own landmarks, factor "host":

  weighted        this build with sample_weight = exp(N(0, 1)), 5 % exact zeros        (lssvm_mi355_problem_fit_reduced_weighted)
  unweighted      this build with sample_weight = None                                  (lssvm_mi355_problem_fit_reduced)
  parent          the PARENT commit's library, the same unweighted call                 (one child process per library: PLSSVM_AMD_LIBRARY)

gram_ms and total_ms of lssvm_reduced_info: medians of `reps` calls after a warm-up (3 at a million points), spread = (max - min) / median.  The comparison is against the
parent's library, never against the code under test: weighted / parent says what the weights cost, unweighted / parent -- which must lie within the parent's spread --
that no weighted code leaked into the unweighted instantiation of the Gram kernel.  A child that fails ends the run and nothing more is started on the device.  A run adds
its rows to an existing --out file."""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# name -> (N, d, kernel, dtype, cost)
ROWS = {
    "rbf50k_f32": (50_000, 128, "rbf", "float32", 100.0),
    "rbf50k_f64": (50_000, 128, "rbf", "float64", 100.0),
    "poly100k_f64": (100_000, 64, "polynomial", "float64", 10.0),
    "rbf1m_f32": (1_000_000, 128, "rbf", "float32", 100.0),
}


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def child(args):
    """One library (this process was started with or without PLSSVM_AMD_LIBRARY), one row, all ranks: a JSON line of {rank: {call: {gram_ms, total_ms}}}."""
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    N, d, kernel, dtype, cost = ROWS[args.child]
    X, y = make_blobs_pm1(N, d, seed=42, dtype=np.dtype(dtype))
    rng = np.random.default_rng(29)
    w = np.exp(rng.standard_normal(N))
    w[rng.random(N) < 0.05] = 0.0
    reps = args.reps if N < 1_000_000 else min(args.reps, 3)
    calls = {"unweighted": None} if args.parent else {"weighted": w, "unweighted": None}
    result = {}
    with backend.ResidentProblem(Parameter(kernel_type=kernel, cost=cost), X) as prob:
        for rank in (int(r) for r in args.ranks.split(",")):
            result[rank] = {}
            for name, weights in calls.items():
                kw = {} if weights is None else {"sample_weight": weights}  # (the parent's package has no such keyword)
                gram, total = [], []
                for rep in range(reps + 1):
                    info = prob.fit_reduced(y, rank, **kw)[3]
                    if rep:
                        gram.append(info["gram_ms"])
                        total.append(info["total_ms"])
                result[rank][name] = {"gram_ms": summary(gram), "total_ms": summary(total), "slabs": info["slabs"], "jitter": info["jitter"]}
    print(json.dumps(result))


def run_child(name, args, parent):
    env = dict(os.environ)
    env.pop("PLSSVM_AMD_LIBRARY", None)
    if parent:
        env["PLSSVM_AMD_LIBRARY"] = args.parent_lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps), "--ranks", args.ranks] + (["--parent"] if parent else [])
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if done.returncode != 0:
        print(done.stdout + done.stderr)
        sys.exit(f"{name}: the child of {'the parent library' if parent else 'this build'} failed ({done.returncode}); nothing more is started")
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--ranks", default="64,256,1024")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduced_weighted.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--parent", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        sys.exit("--parent-lib: the parent commit's libplssvm_amd.so is the yardstick; without it nothing is measured")
    out = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    out["method"] = ("fit_reduced on a resident problem, one right-hand side, the library's landmarks, factor host; one child process per library and row; medians of 10 "
                     "calls' lssvm_reduced_info after a warm-up (3 at 1 000 000 points), spread = (max - min) / median; weights exp(N(0, 1)) with 5 % exact zeros; ratios "
                     "against the PARENT commit's library")
    out.setdefault("rows", {})
    for name in args.rows.split(","):
        N, d, kernel, dtype, cost = ROWS[name]
        this, parent = run_child(name, args, False), run_child(name, args, True)
        row = out["rows"].setdefault(name, {"N": N, "d": d, "kernel": kernel, "dtype": dtype, "cost": cost, "ranks": {}})
        for rank in this:
            r = dict(this[rank], parent=parent[rank]["unweighted"])
            for key in ("gram_ms", "total_ms"):
                base = r["parent"][key]["median"]
                r[f"{key}_weighted_over_parent"] = r["weighted"][key]["median"] / base
                r[f"{key}_unweighted_over_parent"] = r["unweighted"][key]["median"] / base
                r[f"{key}_parent_spread"] = r["parent"][key]["spread"]
                r[f"{key}_unweighted_within_parent_spread"] = abs(r["unweighted"][key]["median"] / base - 1.0) <= r["parent"][key]["spread"]
            row["ranks"][rank] = r
            print(f"{name} rank {rank}: gram parent {r['parent']['gram_ms']['median']:.3f} ms (spread {r['gram_ms_parent_spread']:.3f}), unweighted x{r['gram_ms_unweighted_over_parent']:.3f}, "
                  f"weighted x{r['gram_ms_weighted_over_parent']:.3f}; total parent {r['parent']['total_ms']['median']:.2f} ms (spread {r['total_ms_parent_spread']:.3f}), "
                  f"unweighted x{r['total_ms_unweighted_over_parent']:.3f}, weighted x{r['total_ms_weighted_over_parent']:.3f}", flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
