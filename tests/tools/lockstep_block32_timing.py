#!/usr/bin/env python3
"""What sixteen right-hand sides per symmetric Gram pass cost and save in fp32 on at most 128 features, against a library built from the PARENT commit.

usage: lockstep_block32_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 10] [--no-calls] [--out profiles/lockstep_block32.json]
       lockstep_block32_timing.py --resources <plssvm_amd/lib/asm> [--out profiles/lockstep_block32.json]     (no device: adds the compiler's figures to the file)

pass   at 30 000 points (the parent runs its 256-row form) and at 3 000 (its 128-row form), 16 / 64 / 128 features, rbf and the three polynomial forms, f16x3 and bf16x6
       planes: ONE sixteen-vector pass of this build (tile_matvec_f32_blk_sym) against ONE single-vector symmetric pass of the parent, by HIP events around the
       tile-kernel launches (lssvm_cg_info.matvec_kernel_ms of solves stopped by max_iter, so that every pass is of the kind measured).
call   MI355CSVM(lockstep="block32").solve_systems_of_linear_equations of this build against the parent's MI355CSVM (which solves these shapes one right-hand side after
       the other) for k = 2, 4, 10, 16: 50 000 x 128 rbf on one-vs-all blobs (few iterations) and on random +-1 labels at cost 100 (more), 100 000 x 64 polynomial(3) on
       blobs; eps 1e-3, host wall clock of the whole call, upload and preparation included.  The slab memory of sixteen planes at those sizes is computed beside them.
One child process per library and part (PLSSVM_AMD_LIBRARY), a warm-up of every shape and `--reps` timed repetitions; medians, and the parent's own run-to-run spread
(max - min) / median beside each ratio.  Nothing is routed on these figures.  Every child runs under a time limit of its own; a child that fails ends the run.
"""

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CALLS = [dict(name="50000x128_rbf_blobs", n=50_000, d=128, kernel="rbf", cost=1.0, labels="blobs"), dict(name="50000x128_rbf_random_cost100", n=50_000, d=128, kernel="rbf", cost=100.0, labels="random"),
         dict(name="100000x64_poly3_blobs", n=100_000, d=64, kernel="polynomial", cost=1.0, labels="blobs")]
CALL_KS = (2, 4, 10, 16)
SWEEP_POINTS = (30_000, 3_000)
SWEEP_FEATURES = (16, 64, 128)
SWEEP_KERNELS = {"poly2": ("polynomial", 2), "poly3": ("polynomial", 3), "poly": ("polynomial", 4), "rbf": ("rbf", 3)}
PLANES = {"f16x3": {}, "bf16x6": {"gram_mode": 1}}
EPS, PASS_ITERS = 1e-3, 6


def child(which: str, part: str, reps: int, max_iter: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd._capi import Options
    from plssvm_amd.csvm import MI355CSVM
    from plssvm_amd.datagen import make_blobs_multiclass
    from plssvm_amd.multiclass import one_vs_all_targets
    from plssvm_amd.parameter import Parameter

    new = which == "new"
    assert new == hasattr(_capi.lib, "lssvm_mi355_problem_solve_lockstep_block32"), "the parent's library must not have the block32 entry point, this build's must"
    out = {}
    rng = np.random.default_rng(1)
    if part == "pass":
        for n in SWEEP_POINTS:
            B = rng.choice([-1.0, 1.0], size=(16, n)).astype(np.float32)
            for d in SWEEP_FEATURES:
                X = rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
                for planes, opts in PLANES.items():
                    for name, (kernel, degree) in SWEEP_KERNELS.items():
                        prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=0.0, cost=1.0)
                        with backend.ResidentProblem(prm, X, devices=[0], options=Options(**opts)) as prob:
                            for keep in [False] + [True] * reps:
                                if new:
                                    _, _, infos, passes = prob.solve_lockstep_block(B, 1e-30, PASS_ITERS, block32=True)
                                    assert passes == (1 + PASS_ITERS, 0, 0), passes
                                    ms = infos[0]["matvec_kernel_ms"]
                                else:
                                    prob.cg_begin(B[0], 1e-30)
                                    prob.cg_step(PASS_ITERS)
                                    ms = prob.cg_finish()[2]["matvec_kernel_ms"]
                                if keep:
                                    out.setdefault(f"pass_{name}_{planes}_d{d}_n{n}", []).append(ms)
    else:
        for shape in CALLS:
            X, y = make_blobs_multiclass(shape["n"], shape["d"], max(CALL_KS), seed=42, dtype=np.float32)
            prm = Parameter(kernel_type=shape["kernel"], degree=3, gamma=1.0 / shape["d"], coef0=0.0, cost=shape["cost"])
            for k in CALL_KS:
                Bk = one_vs_all_targets(np.arange(k), y % k, np.float32) if shape["labels"] == "blobs" else rng.choice([-1.0, 1.0], size=(k, shape["n"])).astype(np.float32)
                for keep in [False] + [True] * reps:
                    svm = MI355CSVM(params=prm, lockstep="block32") if new else MI355CSVM(params=prm)
                    t0 = time.perf_counter()
                    _, _, infos = svm.solve_systems_of_linear_equations(prm, X, Bk, EPS, max_iter)
                    if keep:
                        out.setdefault(f"call_{shape['name']}_k{k}", []).append(1e3 * (time.perf_counter() - t0))
                        out.setdefault(f"iters_{shape['name']}_k{k}", []).append(max(i["iterations"] for i in infos))
    print("RESULT " + json.dumps(out), flush=True)


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def kernel_resources(asm_dir):
    """VGPRs, AGPRs, scratch and occupancy of every instantiation from the build's resource-usage files (make -C plssvm_amd/csrc writes them beside the ISA)"""
    rows = {}
    for unit in ("tile_launch_f32blks_a", "tile_launch_f32blks_b"):
        text = open(os.path.join(asm_dir, f"resource_usage_{unit}.txt")).read()
        for block in text.split("Function Name: ")[1:]:
            m = re.match(r"_ZN5lssvm23tile_matvec_f32_blk_symILi(\d+)ELi(\d+)ELi(\d+)EEE", block)
            if not m:
                continue

            def field(label):
                return int(re.search(label + r": (\d+)", block).group(1))
            name = {1: "poly", 3: "poly2", 4: "poly3", 5: "rbf"}[int(m.group(1))]
            rows[f"{name}_nk64_{m.group(2)}_{'f16x3' if m.group(3) == '2' else 'bf16x6'}"] = {
                "vgprs": field("VGPRs"), "agprs": field("AGPRs"), "scratch_bytes": field(r"ScratchSize \[bytes/lane\]"), "waves_per_simd": field(r"Occupancy \[waves/SIMD\]"),
                "workgroups_per_cu": 1, "lds_bytes": 156672}
    return rows


def slab_memory():
    """bytes of the sixteen planes of either slab and of the records at the call shapes: 128-row items in chunks of 64 tiles (the automatic choice at these sizes), one band"""
    rows = {}
    for shape in CALLS:
        tiles = -(-(shape["n"] - 1) // 128)
        row_slabs = 16 * (-(-tiles // 64)) * (tiles + tiles % 2) * 128 * 4
        rows[shape["name"]] = {"column_slab_bytes": 16 * (tiles * (tiles - 1) // 2) * 512, "row_slab_bytes": row_slabs, "record_and_vector_bytes": tiles * (8704 + 128 * 64)}
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--resources", help="plssvm_amd/lib/asm of this build: only add the compiler's figures to --out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-calls", action="store_true")
    ap.add_argument("--no-passes", action="store_true")
    ap.add_argument("--max-iter", type=int, default=100_000, help="iteration limit of the call-level solves")
    ap.add_argument("--child-timeout", type=int, default=500, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lockstep_block32.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    ap.add_argument("--part", choices=["pass", "call"], default="pass")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.part, args.reps, args.max_iter)
        return 0
    res = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    if args.resources:
        res["kernels"] = kernel_resources(args.resources)
        res["memory_of_sixteen_planes"] = slab_memory()
    else:
        if not args.parent_lib or not os.path.isfile(args.parent_lib):
            ap.error("--parent-lib must name the library built from the parent commit")
        samples = {"parent": {}, "new": {}}
        for part in [p for p, skip in (("pass", args.no_passes), ("call", args.no_calls)) if not skip]:
            for which in ("parent", "new"):
                env = dict(os.environ)
                env.pop("PLSSVM_AMD_LIBRARY", None)
                if which == "parent":
                    env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--part", part, "--reps", str(args.reps), "--max-iter", str(args.max_iter)]
                try:
                    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
                except subprocess.TimeoutExpired:
                    print(f"{part}, {which}: child exceeded {args.child_timeout} s; stopping", file=sys.stderr)
                    return 1
                line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
                if proc.returncode != 0 or line is None:
                    print(f"{part}, {which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}", file=sys.stderr)
                    return 1
                for name, vals in json.loads(line[len("RESULT "):]).items():
                    samples[which].setdefault(name, []).extend(vals)
                print(f"{part}, {which}: done", flush=True)
        new = {name: summary(v) for name, v in samples["new"].items()}
        parent = {name: summary(v) for name, v in samples["parent"].items()}
        passes, calls = res.setdefault("pass", {}), res.setdefault("call", {})
        for name in sorted(new):
            a, b = new[name], parent[name]
            if name.startswith("pass_"):
                passes[name[len("pass_"):]] = {"block_pass_ms": a["median"], "block_spread": a["spread"], "parent_single_pass_ms": b["median"], "parent_single_spread": b["spread"],
                                               "block_in_single_passes": a["median"] / b["median"], "n": a["n"]}
            elif name.startswith("call_"):
                its = name.replace("call_", "iters_", 1)
                calls[name[len("call_"):]] = {"block32_ms": a["median"], "parent_ms": b["median"], "ratio": a["median"] / b["median"], "parent_spread": b["spread"], "block32_spread": a["spread"],
                                              "block32_iterations": new[its]["max"], "parent_iterations": parent[its]["max"], "n": a["n"]}
        res["expectation"] = ("from the instruction count: 128 fp32 MFMAs per wave and tile beside the 192 (f16x3, 128 features) of the first product, about twice the extra of the fp32 "
                              "predictor's block kernel (1.10 ... 1.61 single launches), at one workgroup per CU where the parent's 128-row kernels have two")
        res["method"] = (f"one child process per library and part, medians of the timed repetitions (n) after a warm-up of every shape; pass: lssvm_cg_info.matvec_kernel_ms (HIP events "
                         f"around the tile-kernel launches) of {PASS_ITERS} iterations; call: host wall clock of the whole call, eps {EPS}; spread = (max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k in ("pass", "call")}, indent=1)[:12000])
    return 0


if __name__ == "__main__":
    sys.exit(main())
