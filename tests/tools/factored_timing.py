#!/usr/bin/env python3
"""What one FACTORED linear-kernel pass K V = X (X^T V) costs, against the n x n pass of a library built from the PARENT commit.

usage: factored_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 10] [--call-reps 10] [--no-calls] [--out profiles/factored.json]

pass   per shape (points x features, real type): ONE factored pass of this build for groups of 1, 2 and 16 vectors -- HIP events around its three launches
       (lssvm_cg_info.matvec_kernel_ms of solves stopped by max_iter) -- against the parent's single-vector pass; ms, the bytes of X read twice over that time as TB/s, and
       the ratio to one and to sixteen of the parent's passes.  The parent's figure is and remains the n^2 product; the factored time is never an effective TFLOP/s.
call   MI355CSVM(lockstep="factored").solve_systems_of_linear_equations against the parent's default object: host wall clock, upload and set-up included.
One child process per library (PLSSVM_AMD_LIBRARY), one warm-up and `--reps` timed repetitions of every measurement; medians, and the parent's own run-to-run spread
(max - min) / median beside every ratio.  Nothing is routed on these figures.  Every child runs under a time limit of its own; a child that fails ends the run.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PASS_ITERS = 6
SHAPES = [(200_000, 256, "float32"), (50_000, 128, "float32"), (50_000, 128, "float64"), (1_000_000, 128, "float32"), (30_000, 784, "float32")]
CALLS = [dict(n=200_000, d=256, dtype="float32", eps=1e-4, k=(1, 4, 10)), dict(n=50_000, d=128, dtype="float32", eps=1e-4, k=(1, 4, 10))]


def child(which, reps, calls, call_reps):
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd.csvm import MI355CSVM
    from plssvm_amd.datagen import make_blobs_multiclass
    from plssvm_amd.multiclass import one_vs_all_targets
    from plssvm_amd.parameter import Parameter

    new = which == "new"
    assert new == hasattr(_capi.lib, "lssvm_mi355_problem_matvec_factored"), "the parent's library must not have the factored entry points, this build's must"
    out = {}
    rng = np.random.default_rng(1)
    prm = Parameter(kernel_type="linear", cost=1.0)
    for n, d, dtype in SHAPES:
        key = f"{n}x{d}_{dtype}"
        X = rng.uniform(-1, 1, size=(n, d)).astype(dtype)
        B = rng.choice([-1.0, 1.0], size=(16, n)).astype(dtype)
        with backend.ResidentProblem(prm, X, devices=[0]) as prob:
            for keep in [False] + [True] * reps:
                ms = {}
                if new:
                    for g in (1, 2, 16):
                        ms[f"factored{g}"] = prob.solve_lockstep_factored(B[:g], 1e-30, PASS_ITERS)[2][0]["matvec_kernel_ms"]
                else:
                    prob.cg_begin(B[0], 1e-30)
                    prob.cg_step(PASS_ITERS)
                    ms["single"] = prob.cg_finish()[2]["matvec_kernel_ms"]
                if keep:
                    for kind, v in ms.items():
                        out.setdefault(f"pass_{kind}_{key}", []).append(v)
    for shape in CALLS if calls else []:
        dtype = np.dtype(shape["dtype"]).type
        X, y = make_blobs_multiclass(shape["n"], shape["d"], max(shape["k"]), seed=42, dtype=dtype)
        for k in shape["k"]:
            Bk = one_vs_all_targets(np.arange(max(k, 2)), y % max(k, 2), dtype)[:k]
            key = f"{shape['n']}x{shape['d']}_{shape['dtype']}_k{k}"
            for keep in [False] + [True] * call_reps:
                svm = MI355CSVM(params=prm, lockstep="factored") if new else MI355CSVM(params=prm)
                t0 = time.perf_counter()
                infos = svm.solve_systems_of_linear_equations(prm, X, Bk, shape["eps"], shape["n"])[2]
                if keep:
                    out.setdefault(f"call_{key}", []).append((time.perf_counter() - t0) * 1e3)
            out[f"iterations_{key}"] = [max(i["iterations"] for i in infos)]
            print(f"{which} call {key}: {out[f'iterations_{key}'][0]} iterations, {out[f'call_{key}'][-1]:.1f} ms", file=sys.stderr, flush=True)  # (progress: the parent's calls are long)
    print("RESULT " + json.dumps(out), flush=True)


def run_child(which, lib, args):
    env = dict(os.environ, PLSSVM_AMD_LIBRARY=lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(args.reps), "--call-reps", str(args.call_reps)] + (["--no-calls"] if args.no_calls else [])
    done = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)  # (the child's progress lines go to this process's stderr as they come)
    if done.returncode != 0:
        sys.exit(f"the {which} child failed ({done.returncode}):\n{done.stdout[-2000:]}")
    return json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--call-reps", type=int, default=0, help="timed repetitions of a whole call (0: --reps)")
    ap.add_argument("--no-calls", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=900)
    ap.add_argument("--child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factored.json"))
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps, not args.no_calls, args.call_reps or args.reps)
        return
    new = run_child("new", os.path.join(ROOT, "plssvm_amd", "lib", "libplssvm_amd.so"), args)
    old = run_child("parent", os.path.abspath(args.parent_lib), args)
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v) if med(v) > 0 else 0.0
    report = {"reps": args.reps, "call_reps": args.call_reps or args.reps, "pass_iterations": PASS_ITERS, "pass": {}, "call": {}, "raw": {"new": new, "parent": old}}
    for n, d, dtype in SHAPES:
        key = f"{n}x{d}_{dtype}"
        single = med(old[f"pass_single_{key}"])
        f = {g: med(new[f"pass_factored{g}_{key}"]) for g in (1, 2, 16)}
        x_bytes = 2 * (n - 1) * d * (4 if dtype == "float32" else 8)  # X read twice
        report["pass"][key] = {"parent_single_ms": single, "parent_single_spread": spread(old[f"pass_single_{key}"]), "factored_ms": f,
                               "factored_tbps": {g: x_bytes / f[g] / 1e9 for g in f}, "factored_over_single": {g: f[g] / single for g in f},
                               "factored16_over_16_singles": f[16] / (16 * single)}
    for key in sorted(k[len("call_"):] for k in old if k.startswith("call_")):
        report["call"][key] = {"factored_ms": med(new[f"call_{key}"]), "parent_ms": med(old[f"call_{key}"]), "ratio": med(new[f"call_{key}"]) / med(old[f"call_{key}"]),
                               "parent_spread": spread(old[f"call_{key}"]), "iterations": new[f"iterations_{key}"][0], "parent_iterations": old[f"iterations_{key}"][0]}
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
    print(json.dumps({"pass": report["pass"], "call": report["call"]}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
