#!/usr/bin/env python3
"""What the cost path saves on a grid of costs, against a library built from the PARENT commit.

usage: cost_path_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 10] [--shapes a,b] [--grids 5,9] [--eps 1e-3,1e-6] [--budget-s S]
                           [--out profiles/cost_path.json]

Shapes (make_blobs_pm1 data, gamma = 1 / features): 50000x128_rbf_f32, 50000x128_rbf_f64, 100000x64_poly3_f64.  Grids: 5 costs, decade-spaced 1e-1 ... 1e3, and 9 costs,
half-decade-spaced over the same range.  Tolerances: eps 1e-3 and 1e-6.  Per shape, grid and eps this records, as medians of `--reps` repetitions after a warm-up,
  path   backend.solve_cost_path of this build (one-shot: upload, preparation, the multi-shift CG, the verification passes): wall time, iterations per cost, Gram passes;
  (a)    the parent's one-shot solves, one per cost, at the same eps -- their stop test is NOT the path's (x0 = 1, the 2-norm, relative to |b - A 1|);
  (b)    the parent's one-shot solves with eps tightened by decades until each cost's TRUE relative residual |P (b - Abar x)| / |P b| is no larger than the path's -- the
         equal-accuracy baseline.  Both true residuals are evaluated by a float64 ResidentProblem.matvec of the data as the solve saw it.  eps goes no lower than the
         resolution of the number format (1e-8 in float32, 1e-14 in float64); a cost the parent cannot bring there (float32 at a tight eps) is listed under
         `b_not_reached`, and a configuration with such a cost has `ratio_b` = null: no ratio against solves of lesser accuracy.
with the parent's own run-to-run spread (max - min) / median.  ratio = path / baseline: below 1 the path is faster.  --max-iter bounds every solve, both sides alike
(default 5000; 0: the number of points, the bound `fit` uses); the `*_converged` lists say whether a solve met its stop test within it.
One child process per library and configuration (PLSSVM_AMD_LIBRARY), each under a time limit of its own; a child that fails ends the run, and nothing more is started on
the device.  With --budget-s no further configuration is started once that many seconds have passed; the file lists what was measured and what the last run left out.
A run adds its configurations to an existing --out file."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = {"50000x128_rbf_f32": (50_000, 128, "rbf", "float32"), "50000x128_rbf_f64": (50_000, 128, "rbf", "float64"), "100000x64_poly3_f64": (100_000, 64, "polynomial", "float64")}
EPS_FLOOR = {"float32": 1e-8, "float64": 1e-14}  # (b) tightens eps no further: below the resolution of the format the recipe's own residual stops falling
GRIDS = {5: [10.0 ** k for k in range(-1, 4)], 9: [10.0 ** (k / 2.0) for k in range(-2, 7)]}


def child(args) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    N, d, kernel, dtype = SHAPES[args.shape]
    dtype = np.dtype(dtype).type
    costs, eps = GRIDS[args.grid], args.one_eps
    max_iter = args.max_iter if args.max_iter > 0 else N
    floor = EPS_FLOOR[np.dtype(dtype).name]
    X, y = make_blobs_pm1(N, d, seed=42, dtype=dtype)
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    n = N - 1
    theta = (1.0 - 1.0 / np.sqrt(N)) / n

    def P(v):
        return v - theta * v.sum()

    b = y64[:n] - y64[n]
    norm_b = float(np.linalg.norm(P(b)))

    def prm(cost):
        return Parameter(kernel_type=kernel, degree=3, gamma=1.0 / d, coef0=0.0, cost=cost)

    def note(text):
        print(f"  [{args.child} {args.shape} grid {args.grid} eps {eps:g}] {text}", file=sys.stderr, flush=True)

    with backend.ResidentProblem(prm(1.0), X64) as at_one:  # Abar(1 / C) = Abar(1) + (1 / C - 1) (I + 1 1^T): ONE float64 problem evaluates every cost's residual
        def true_residual(cost, alpha):
            """|P (b - Abar(1 / C) x)| / |P b| by a float64 matvec"""
            x = np.asarray(alpha[:n], dtype=np.float64)
            ax = at_one.matvec(x, np.zeros(n)) + (1.0 / cost - 1.0) * (x + x.sum())
            return float(np.linalg.norm(P(b - ax))) / norm_b

        def timed(fn):
            fn()  # warm-up
            ms = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                result = fn()
                ms.append(1e3 * (time.perf_counter() - t0))
            return ms, result

        out = {}
        if args.child == "new":
            ms, (alphas, _, infos, passes) = timed(lambda: backend.solve_cost_path(prm(1.0), X, y, costs, eps, max_iter))
            out = {"path_ms": ms, "iterations": [i["iterations"] for i in infos], "converged": [i["converged"] for i in infos], "verified": [i["verified"] for i in infos],
                   "passes": list(passes), "true_rel_residual": [true_residual(c, a) for c, a in zip(costs, alphas)]}
        else:
            target = json.loads(args.path_residuals)

            def solves(eps_per_cost):
                return [backend.solve_system_of_linear_equations(prm(c), X, y, e, max_iter) for c, e in zip(costs, eps_per_cost)]

            ms, solved = timed(lambda: solves([eps] * len(costs)))
            res_a = [true_residual(c, s[0]) for c, s in zip(costs, solved)]
            out = {"a_ms": ms, "a_iterations": [s[2]["iterations"] for s in solved], "a_converged": [s[2]["converged"] for s in solved], "a_true_rel_residual": res_a}
            note(f"(a) {statistics.median(ms):.0f} ms")
            # (b): tighten eps by decades per cost until the true residual is no larger than the path's, down to the floor of the number format; a solve that runs
            # into max_iter, or the floor, without getting there leaves the cost "not reached"
            eps_b, res_b, not_reached = [], [], []
            for k, cost in enumerate(costs):
                e, r, converged = eps, res_a[k], bool(solved[k][2]["converged"])
                while r > target[k] and converged and e * 0.1 >= floor * 0.999:
                    e *= 0.1
                    alpha, _, info = backend.solve_system_of_linear_equations(prm(cost), X, y, e, max_iter)
                    r, converged = true_residual(cost, alpha), bool(info["converged"])
                if r > target[k]:
                    not_reached.append(cost)
                eps_b.append(e)
                res_b.append(r)
                note(f"(b) C = {cost:g}: eps {e:g}, residual {r:.2e} against the path's {target[k]:.2e}")
            out.update({"b_eps": eps_b, "b_true_rel_residual": res_b, "b_not_reached": not_reached})
            if not_reached:
                out.update({"b_ms": None, "b_iterations": None, "b_converged": None})  # no equal-accuracy baseline exists: nothing to time
            elif eps_b == [eps] * len(costs):
                out.update({"b_ms": ms, "b_iterations": out["a_iterations"], "b_converged": out["a_converged"]})
            else:
                ms_b, solved_b = timed(lambda: solves(eps_b))
                out.update({"b_ms": ms_b, "b_iterations": [s[2]["iterations"] for s in solved_b], "b_converged": [s[2]["converged"] for s in solved_b]})
    print("RESULT " + json.dumps(out), flush=True)


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--grids", default="5,9")
    ap.add_argument("--eps", default="1e-3,1e-6")
    ap.add_argument("--max-iter", type=int, default=5000, help="iterations one solve may take (0: the number of points)")
    ap.add_argument("--budget-s", type=float, default=0.0, help="start no further configuration after this many seconds (0: no limit)")
    ap.add_argument("--child-timeout", type=int, default=900, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_path.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    ap.add_argument("--shape")
    ap.add_argument("--grid", type=int)
    ap.add_argument("--one-eps", type=float)
    ap.add_argument("--path-residuals")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    t_start = time.time()
    res = json.load(open(args.out)) if os.path.isfile(args.out) else {"configurations": {}}  # (a later run adds its configurations to the file)
    res["not_measured"] = []

    def run_child(which, shape, grid, eps, extra=()):
        env = dict(os.environ)
        if which == "parent":
            env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
        else:
            env.pop("PLSSVM_AMD_LIBRARY", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--shape", shape, "--grid", str(grid), "--one-eps", repr(eps), "--reps", str(args.reps),
               "--max-iter", str(args.max_iter)] + list(extra)
        try:
            proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)  # (its progress lines go to this process's stderr)
        except subprocess.TimeoutExpired:
            print(f"{shape} grid {grid} eps {eps:g}, {which}: child exceeded {args.child_timeout} s; stopping", file=sys.stderr)
            return None
        line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if proc.returncode != 0 or line is None:
            print(f"{shape} grid {grid} eps {eps:g}, {which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}", file=sys.stderr)
            return None
        return json.loads(line[len("RESULT "):])

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")

    failed = False
    for shape in args.shapes.split(","):
        for grid in (int(g) for g in args.grids.split(",")):
            for eps in (float(e) for e in args.eps.split(",")):
                name = f"{shape}_grid{grid}_eps{eps:g}"
                if failed or (args.budget_s > 0 and time.time() - t_start > args.budget_s):
                    res["not_measured"].append(name)
                    continue
                new = run_child("new", shape, grid, eps)
                parent = run_child("parent", shape, grid, eps, ["--path-residuals", json.dumps(new["true_rel_residual"])]) if new is not None else None
                if new is None or parent is None:
                    failed = True
                    res["not_measured"].append(name)
                    continue
                path, a = summary(new["path_ms"]), summary(parent["a_ms"])
                b = summary(parent["b_ms"]) if parent["b_ms"] is not None else {"median": None, "spread": None}
                rec = {"costs": GRIDS[grid], "path_ms": path["median"], "path_spread": path["spread"], "path_iterations": new["iterations"], "path_passes": new["passes"],
                       "path_converged": new["converged"], "path_verified": new["verified"], "path_true_rel_residual": new["true_rel_residual"],
                       "a_ms": a["median"], "a_spread": a["spread"], "a_iterations": parent["a_iterations"], "a_converged": parent["a_converged"], "a_true_rel_residual": parent["a_true_rel_residual"],
                       "ratio_a": path["median"] / a["median"],
                       "b_ms": b["median"], "b_spread": b["spread"], "b_eps": parent["b_eps"], "b_iterations": parent["b_iterations"], "b_converged": parent["b_converged"], "b_true_rel_residual": parent["b_true_rel_residual"],
                       "b_not_reached": parent["b_not_reached"], "ratio_b": (path["median"] / b["median"]) if b["median"] is not None else None, "samples": path["n"]}
                res["configurations"][name] = rec
                print(name, json.dumps({k: rec[k] for k in ("path_ms", "a_ms", "ratio_a", "b_ms", "ratio_b", "path_passes", "b_not_reached")}), flush=True)
                write()
    res["method"] = (f"one child process per library and configuration, {args.reps} timed repetitions after a warm-up, medians; wall clock of the whole one-shot call(s), upload and "
                     f"preparation included; at most {args.max_iter if args.max_iter > 0 else 'as many iterations as points'} iterations per solve; (b) tightens eps by decades down to "
                     f"{EPS_FLOOR}; spread = (max - min) / median; ratio = path / baseline")
    write()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
