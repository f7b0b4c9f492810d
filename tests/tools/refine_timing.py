#!/usr/bin/env python3
"""What mixed-precision refinement saves a float64 solve, against a library built from the PARENT commit.

usage: refine_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 5] [--rounds 1] [--out profiles/refined_f64.json]

Shapes: 50 000 x 128 rbf with C = 1 and C = 100, 100 000 x 64 polynomial degree 3, float64, make_blobs_pm1(seed 42), each at eps = 1e-3, 1e-6, 1e-10.  Per case this
records
  parent    lssvm_mi355_solve_f64 of the parent's library: host wall clock of the whole call, the upload and preparation of the data included; iterations, Gram passes
  refined   lssvm_mi355_solve_refined_f64 of this build, the same clock; outer steps, inner fp32 iterations, fp64 / fp32 passes, the f64_ms / f32_ms split of the call,
            whether fp64 CG took over -- and `meets_stop_test`: residuum <= target_residuum on the TRUE fp64 residual, without which the time means nothing.
One child process per (library, shape), the libraries alternating (PLSSVM_AMD_LIBRARY); each child warms every case up once, then times `--reps` repetitions.  Medians, and
the parent's own run-to-run spread (max - min) / median.  `gain` = 1 - refined / parent; `faster` = the gain exceeds the parent's spread.
Every child runs under a time limit of its own; a child that fails ends the run: nothing more is started on the device.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [dict(name="50000x128_rbf_C1", n=50_000, d=128, kernel="rbf", cost=1.0), dict(name="50000x128_rbf_C100", n=50_000, d=128, kernel="rbf", cost=100.0),
          dict(name="100000x64_poly3", n=100_000, d=64, kernel="polynomial", cost=1.0)]
EPSILONS = (1e-3, 1e-6, 1e-10)


def child(which: str, shape_name: str, reps: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    new = which == "new"
    assert new == hasattr(_capi.lib, "lssvm_mi355_solve_refined_f64"), "the parent's library must not have the refined entry point, this build's must"
    shape = next(s for s in SHAPES if s["name"] == shape_name)
    X, y = make_blobs_pm1(shape["n"], shape["d"], seed=42, dtype=np.float64)
    prm = Parameter(kernel_type=shape["kernel"], degree=3, gamma=1.0 / shape["d"], coef0=0.0, cost=shape["cost"])
    out = {}
    for eps in EPSILONS:
        rec = {"ms": []}
        for keep in [False] + [True] * reps:
            t0 = time.perf_counter()
            if new:
                _, _, info, ri = backend.solve_refined(prm, X, y, eps, shape["n"])
            else:
                _, _, info = backend.solve_system_of_linear_equations(prm, X, y, eps, shape["n"])
            ms = 1e3 * (time.perf_counter() - t0)
            if keep:
                rec["ms"].append(ms)
        rec.update(iterations=int(info["iterations"]), converged=int(info["converged"]), residuum=info["residuum"], target_residuum=info["target_residuum"])
        if new:
            rec.update({k: ri[k] for k in ("refined", "took_over_f64", "outer_steps", "inner_iterations", "f64_cg_iterations", "f64_passes", "f32_passes", "f64_ms", "f32_ms",
                                           "inner_gram_mode", "inner_rbf_direct")})
            rec["meets_stop_test"] = bool(ri["residuum"] <= ri["target_residuum"])
        else:
            rec["passes"] = int(info["matvec_launches"])
        out[f"{shape_name}_eps{eps:g}"] = rec
    print("RESULT " + json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--child-timeout", type=int, default=280, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refined_f64.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    ap.add_argument("--shape", choices=[s["name"] for s in SHAPES])
    args = ap.parse_args()
    if args.child:
        child(args.child, args.shape, args.reps)
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    runs = {"parent": {}, "new": {}}
    for rnd in range(args.rounds):
        for shape in SHAPES:
            for which in ("parent", "new"):
                env = dict(os.environ)
                if which == "parent":
                    env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
                else:
                    env.pop("PLSSVM_AMD_LIBRARY", None)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--shape", shape["name"], "--reps", str(args.reps)]
                try:
                    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
                except subprocess.TimeoutExpired:
                    print(f"round {rnd}, {shape['name']}, {which}: child exceeded {args.child_timeout} s; stopping", file=sys.stderr)
                    return 1
                line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
                if proc.returncode != 0 or line is None:
                    print(f"round {rnd}, {shape['name']}, {which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}", file=sys.stderr)
                    return 1
                for name, rec in json.loads(line[len("RESULT "):]).items():
                    kept = runs[which].setdefault(name, rec)
                    if kept is not rec:
                        kept["ms"].extend(rec["ms"])
                print(f"round {rnd}, {shape['name']}, {which}: done", flush=True)
    cases = {}
    for name, p in runs["parent"].items():
        r = runs["new"][name]
        p_med, r_med = statistics.median(p["ms"]), statistics.median(r["ms"])
        spread = (max(p["ms"]) - min(p["ms"])) / p_med
        gain = 1.0 - r_med / p_med
        cases[name] = {"parent": {"ms": p_med, "spread": spread, "iterations": p["iterations"], "passes": p["passes"], "converged": p["converged"], "n": len(p["ms"])},
                       "refined": dict({k: v for k, v in r.items() if k != "ms"}, ms=r_med, spread=(max(r["ms"]) - min(r["ms"])) / r_med, n=len(r["ms"])),
                       "gain": gain, "faster": bool(gain > spread), "counts": bool(p["iterations"] >= 20)}
    res = {"cases": cases,
           "method": (f"{args.rounds} child process(es) per library and shape, alternating, {args.reps} timed repetitions after a warm-up of every case; host wall clock of the whole call "
                      "(data upload and preparation included); medians; spread = (max - min) / median; gain = 1 - refined / parent; faster: gain > the parent's spread; counts: "
                      "the parent needs at least 20 CG iterations")}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, c in cases.items():
        r = c["refined"]
        print(f"{name:32s} parent {c['parent']['ms']:9.1f} ms ({c['parent']['iterations']:5d} its, spread {c['parent']['spread']:.3f})  refined {r['ms']:9.1f} ms (outer {r['outer_steps']}, inner "
              f"{r['inner_iterations']}, f64 cg {r['f64_cg_iterations']}, f64 {r['f64_ms']:.1f} ms, f32 {r['f32_ms']:.1f} ms, stop test {r['meets_stop_test']})  gain {c['gain']:+.3f}"
              f"{'' if c['counts'] else '  (< 20 iterations)'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
