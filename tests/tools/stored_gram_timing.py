#!/usr/bin/env python3
"""What one pass over the STORED kernel matrix costs and saves, against a library built from the PARENT commit.

usage: stored_gram_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 10] [--points 30000,50000] [--features 16,128,784] [--no-calls]
                             [--out profiles/stored_gram.json]

pass   per (points, features, kernel function, real type): ONE stored pass of this build for groups of 1, 2 and 16 vectors against the parent's single-vector and
       two-vector (panels) passes and, where the parent has it, its sixteen-vector block pass -- HIP events around the tile launches (lssvm_cg_info.matvec_kernel_ms of
       solves stopped by max_iter, so that every pass is of the kind measured); the achieved GB/s of the stored pass over the bytes of its triangle; the device time of
       the assembly in units of the parent's single pass, and the iteration count from which assembly + stored passes beat the parent's single passes.
call   MI355CSVM(solver="stored") against the parent's MI355CSVM: host wall clock of solve_systems_of_linear_equations, upload, assembly and allocation included.
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
KERNELS = {"rbf": ("rbf", 3), "poly3": ("polynomial", 3)}
PASS_ITERS = 6
CALLS = [dict(name="50000x128_rbf_f64", n=50_000, d=128, dtype="float64", eps=(1e-6, 1e-10), cost=(1.0, 100.0), k=(1, 4, 10)),
         dict(name="30000x784_rbf_f32", n=30_000, d=784, dtype="float32", eps=(1e-4,), cost=(1.0,), k=(1, 10)),
         dict(name="30000x784_rbf_f64", n=30_000, d=784, dtype="float64", eps=(1e-6,), cost=(1.0,), k=(1, 10))]


def child(which, reps, points, features, calls):
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd.csvm import MI355CSVM
    from plssvm_amd.datagen import make_blobs_multiclass
    from plssvm_amd.multiclass import one_vs_all_targets
    from plssvm_amd.parameter import Parameter

    new = which == "new"
    assert new == hasattr(_capi.lib, "lssvm_mi355_problem_store_gram"), "the parent's library must not have the stored entry points, this build's must"
    out = {}
    rng = np.random.default_rng(1)
    for n in points:
        for d in features:
            for dtype in (np.float32, np.float64):
                X = rng.uniform(-1, 1, size=(n, d)).astype(dtype)
                B = rng.choice([-1.0, 1.0], size=(16, n)).astype(dtype)
                for name, (kernel, degree) in KERNELS.items():
                    key = f"{n}x{d}_{name}_{np.dtype(dtype).name}"
                    prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=0.0, cost=1.0)
                    with backend.ResidentProblem(prm, X, devices=[0]) as prob:
                        if new:
                            stored, nbytes, ms = prob.store_gram()
                            out[f"bytes_{key}"], out[f"assemble_ms_{key}"] = [nbytes], [ms]
                            if not stored:
                                continue
                        for keep in [False] + [True] * reps:
                            ms = {}
                            if new:
                                for g in (1, 2, 16):
                                    ms[f"stored{g}"] = prob.solve_lockstep_stored(B[:g], 1e-30, PASS_ITERS)[2][0]["matvec_kernel_ms"]
                            else:
                                ms["pair"] = prob.solve_lockstep(B[:2], 1e-30, PASS_ITERS, panels=True)[2][0]["matvec_kernel_ms"]
                                prob.cg_begin(B[0], 1e-30)
                                prob.cg_step(PASS_ITERS)
                                ms["single"] = prob.cg_finish()[2]["matvec_kernel_ms"]
                                _, _, infos, passes = prob.solve_lockstep_block(B, 1e-30, PASS_ITERS, block32=True)
                                if passes[0] > 0:
                                    ms["block"] = infos[0]["matvec_kernel_ms"]
                            if keep:
                                for kind, v in ms.items():
                                    out.setdefault(f"pass_{kind}_{key}", []).append(v)
    for shape in CALLS if calls else []:
        dtype = np.dtype(shape["dtype"]).type
        X, y = make_blobs_multiclass(shape["n"], shape["d"], max(shape["k"]), seed=42, dtype=dtype)
        for cost in shape["cost"]:
            prm = Parameter(kernel_type="rbf", gamma=1.0 / shape["d"], cost=cost)
            for eps in shape["eps"]:
                for k in shape["k"]:
                    Bk = one_vs_all_targets(np.arange(max(k, 2)), y % max(k, 2), dtype)[:k]
                    for keep in [False] + [True] * reps:
                        svm = MI355CSVM(params=prm, solver="stored") if new else MI355CSVM(params=prm)
                        t0 = time.perf_counter()
                        infos = svm.solve_systems_of_linear_equations(prm, X, Bk, eps, shape["n"])[2]
                        if keep:
                            out.setdefault(f"call_{shape['name']}_C{cost:g}_eps{eps:g}_k{k}", []).append((time.perf_counter() - t0) * 1e3)
                    out[f"iterations_{shape['name']}_C{cost:g}_eps{eps:g}_k{k}"] = [max(i["iterations"] for i in infos)]
    print("RESULT " + json.dumps(out), flush=True)


def run_child(which, lib, args):
    env = dict(os.environ, PLSSVM_AMD_LIBRARY=lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(args.reps), "--points", args.points, "--features", args.features] + (["--no-calls"] if args.no_calls else [])
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if done.returncode != 0:
        sys.exit(f"the {which} child failed ({done.returncode}):\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}")
    return json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", default="30000,50000")
    ap.add_argument("--features", default="16,128,784")
    ap.add_argument("--no-calls", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=900)
    ap.add_argument("--child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stored_gram.json"))
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps, [int(v) for v in args.points.split(",")], [int(v) for v in args.features.split(",")], not args.no_calls)
        return
    new = run_child("new", os.path.join(ROOT, "plssvm_amd", "lib", "libplssvm_amd.so"), args)
    old = run_child("parent", os.path.abspath(args.parent_lib), args)
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v) if med(v) > 0 else 0.0
    report = {"reps": args.reps, "pass_iterations": PASS_ITERS, "pass": {}, "call": {}, "raw": {"new": new, "parent": old}}
    for key in sorted(k[len("pass_single_"):] for k in old if k.startswith("pass_single_")):
        if f"pass_stored1_{key}" not in new:
            report["pass"][key] = {"stored": False, "bytes": new.get(f"bytes_{key}", [0])[0]}
            continue
        single, pair = med(old[f"pass_single_{key}"]), med(old[f"pass_pair_{key}"])
        s = {g: med(new[f"pass_stored{g}_{key}"]) for g in (1, 2, 16)}
        tri = int(key.split("x")[0]) - 1
        tri_bytes = (-(-tri // 128)) * (-(-tri // 128) + 1) // 2 * 128 * 128 * (4 if key.endswith("float32") else 8)
        asm = new[f"assemble_ms_{key}"][0]
        row = {"stored": True, "bytes": new[f"bytes_{key}"][0], "triangle_bytes": tri_bytes, "parent_single_ms": single, "parent_pair_ms": pair,
               "parent_single_spread": spread(old[f"pass_single_{key}"]), "parent_pair_spread": spread(old[f"pass_pair_{key}"]),
               "stored_ms": s, "stored16_gbps": tri_bytes / s[16] / 1e6, "stored1_over_single": s[1] / single, "stored2_over_pair": s[2] / pair,
               "stored16_over_16_singles": s[16] / (16 * single), "assemble_ms": asm, "assemble_in_single_passes": asm / single,
               "break_even_iterations_one_vector": asm / (single - s[1]) if single > s[1] else None}
        if f"pass_block_{key}" in old:
            row["parent_block_ms"] = med(old[f"pass_block_{key}"])
            row["parent_block_spread"] = spread(old[f"pass_block_{key}"])
            row["stored16_over_block"] = s[16] / row["parent_block_ms"]
        report["pass"][key] = row
    for key in sorted(k[len("call_"):] for k in old if k.startswith("call_")):
        report["call"][key] = {"stored_ms": med(new[f"call_{key}"]), "parent_ms": med(old[f"call_{key}"]), "ratio": med(new[f"call_{key}"]) / med(old[f"call_{key}"]),
                               "parent_spread": spread(old[f"call_{key}"]), "iterations": new[f"iterations_{key}"][0]}
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(json.dumps({"pass": report["pass"], "call": report["call"]}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
