#!/usr/bin/env python3
"""What sixteen right-hand sides per symmetric Gram pass cost and save in fp64, against a library built from the PARENT commit.

usage: lockstep_block_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 10] [--rounds 1] [--no-calls] [--out profiles/lockstep_block.json]
       lockstep_block_timing.py --resources <plssvm_amd/lib/asm> [--out profiles/lockstep_block.json]     (no device: adds the compiler's figures to the file)

pass   at 30 000 points, for every (kernel function, chunk count) instantiation of tile_matvec_f64_blk_sym: ONE sixteen-vector pass of this build against ONE
       single-vector symmetric pass and against EIGHT two-vector passes of the parent, by HIP events around the tile-kernel launches (lssvm_cg_info.matvec_kernel_ms of
       solves stopped by max_iter, so that every pass is of the kind measured).
call   MI355CSVM(lockstep="block").solve_systems_of_linear_equations of this build against the parent's MI355CSVM (its pair lockstep) for k = 2, 4, 10, 16 one-vs-all
       targets at 100 000 x 64 polynomial(3) and 50 000 x 128 rbf, eps 1e-3: host wall clock of the whole call, upload and preparation included.
One child process per library and round (PLSSVM_AMD_LIBRARY), a warm-up of every measurement and `--reps` timed repetitions; medians, and the parent's own run-to-run
spread (max - min) / median beside each ratio.  Nothing is routed on these figures.  Every child runs under a time limit of its own; a child that fails ends the run.
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
SHAPES = [dict(name="100000x64_poly3", n=100_000, d=64, kernel="polynomial"), dict(name="50000x128_rbf", n=50_000, d=128, kernel="rbf")]
CALL_KS = (2, 4, 10, 16)
SWEEP_POINTS = 30_000
SWEEP_KERNELS = {"poly2": ("polynomial", 2), "poly3": ("polynomial", 3), "poly": ("polynomial", 4), "rbf": ("rbf", 3)}
CHUNKS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16)  # of 16 features
EPS, PASS_ITERS = 1e-3, 6


def child(which: str, reps: int, calls: bool, chunks) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd.csvm import MI355CSVM
    from plssvm_amd.datagen import make_blobs_multiclass
    from plssvm_amd.multiclass import one_vs_all_targets
    from plssvm_amd.parameter import Parameter

    new = which == "new"
    assert new == hasattr(_capi.lib, "lssvm_mi355_problem_solve_lockstep_block"), "the parent's library must not have the block entry point, this build's must"
    out = {}
    rng = np.random.default_rng(1)
    B = rng.choice([-1.0, 1.0], size=(16, SWEEP_POINTS))
    for nkc in chunks:
        X = rng.uniform(-1, 1, size=(SWEEP_POINTS, 16 * nkc))
        for name, (kernel, degree) in SWEEP_KERNELS.items():
            prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / (16 * nkc), coef0=0.0, cost=1.0)
            with backend.ResidentProblem(prm, X, devices=[0]) as prob:
                for keep in [False] + [True] * reps:
                    if new:
                        _, _, infos, passes = prob.solve_lockstep_block(B, 1e-30, PASS_ITERS)
                        assert passes == (1 + PASS_ITERS, 0, 0), passes
                        ms = {"block": infos[0]["matvec_kernel_ms"]}
                        if nkc == chunks[0] and name == "rbf":  # (the bands of a pass: one tile launch each)
                            ms["bands"] = infos[0]["tile_launches_per_matvec"]
                    else:
                        _, _, infos, passes = prob.solve_lockstep(B[:2], 1e-30, PASS_ITERS)
                        assert passes == (1 + PASS_ITERS, 0), passes
                        prob.cg_begin(B[0], 1e-30)
                        prob.cg_step(PASS_ITERS)
                        ms = {"pair": infos[0]["matvec_kernel_ms"], "single": prob.cg_finish()[2]["matvec_kernel_ms"]}
                    if keep:
                        for kind, v in ms.items():
                            out.setdefault(f"pass_{kind}_{name}_nkc{nkc}", []).append(v)
    if calls:
        for shape in SHAPES:
            X, y = make_blobs_multiclass(shape["n"], shape["d"], max(CALL_KS), seed=42, dtype=np.float64)
            prm = Parameter(kernel_type=shape["kernel"], degree=3, gamma=1.0 / shape["d"], coef0=0.0, cost=1.0)
            for k in CALL_KS:
                Bk = one_vs_all_targets(np.arange(k), y % k, np.float64)
                for keep in [False] + [True] * reps:
                    svm = MI355CSVM(params=prm, lockstep="block") if new else MI355CSVM(params=prm)
                    t0 = time.perf_counter()
                    svm.solve_systems_of_linear_equations(prm, X, Bk, EPS, shape["n"])
                    if keep:
                        out.setdefault(f"call_{shape['name']}_k{k}", []).append(1e3 * (time.perf_counter() - t0))
    print("RESULT " + json.dumps(out), flush=True)


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def kernel_resources(asm_dir):
    """VGPRs, AGPRs, scratch and occupancy of every instantiation from the build's resource-usage files (make -C plssvm_amd/csrc writes them beside the ISA)"""
    rows = {}
    for unit in ("tile_launch_f64blks_a", "tile_launch_f64blks_b"):
        text = open(os.path.join(asm_dir, f"resource_usage_{unit}.txt")).read()
        for block in text.split("Function Name: ")[1:]:
            m = re.match(r"_ZN5lssvm23tile_matvec_f64_blk_symILi(\d+)ELi(\d+)EEE", block)
            if not m:
                continue

            def field(label):
                return int(re.search(label + r": (\d+)", block).group(1))
            name = {1: "poly", 3: "poly2", 4: "poly3", 2: "rbf"}[int(m.group(1))]
            rows[f"{name}_nkc{m.group(2)}"] = {"vgprs": field("VGPRs"), "agprs": field("AGPRs"), "scratch_bytes": field(r"ScratchSize \[bytes/lane\]"),
                                              "waves_per_simd": field(r"Occupancy \[waves/SIMD\]"), "workgroups_per_cu": 1, "lds_bytes": 150528}
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--resources", help="plssvm_amd/lib/asm of this build: only add the compiler's figures to --out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--no-calls", action="store_true")
    ap.add_argument("--chunks", type=int, nargs="*", default=list(CHUNKS))
    ap.add_argument("--child-timeout", type=int, default=500, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lockstep_block.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps, not args.no_calls, tuple(args.chunks))
        return 0
    res = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    if args.resources:
        res["kernels"] = kernel_resources(args.resources)
    else:
        if not args.parent_lib or not os.path.isfile(args.parent_lib):
            ap.error("--parent-lib must name the library built from the parent commit")
        samples = {"parent": {}, "new": {}}
        for rnd in range(args.rounds):
            for which in ("parent", "new"):
                env = dict(os.environ)
                env.pop("PLSSVM_AMD_LIBRARY", None)
                if which == "parent":
                    env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(args.reps), "--chunks"] + [str(c) for c in args.chunks] + (["--no-calls"] if args.no_calls else [])
                try:
                    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
                except subprocess.TimeoutExpired:
                    print(f"round {rnd}, {which}: child exceeded {args.child_timeout} s; stopping", file=sys.stderr)
                    return 1
                line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
                if proc.returncode != 0 or line is None:
                    print(f"round {rnd}, {which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}", file=sys.stderr)
                    return 1
                for name, vals in json.loads(line[len("RESULT "):]).items():
                    samples[which].setdefault(name, []).extend(vals)
                print(f"round {rnd}, {which}: done", flush=True)
        new = {name: summary(v) for name, v in samples["new"].items()}
        parent = {name: summary(v) for name, v in samples["parent"].items()}
        passes = res.setdefault("pass", {})
        for name in sorted(new):
            if not name.startswith("pass_block_"):
                continue
            inst = name[len("pass_block_"):]
            blk, one, two = new[name], parent[f"pass_single_{inst}"], parent[f"pass_pair_{inst}"]
            passes[inst] = {"block_pass_ms": blk["median"], "block_spread": blk["spread"], "parent_single_pass_ms": one["median"], "parent_single_spread": one["spread"],
                            "parent_pair_pass_ms": two["median"], "parent_pair_spread": two["spread"], "block_in_single_passes": blk["median"] / one["median"],
                            "block_to_eight_pair_passes": blk["median"] / (8.0 * two["median"]), "n": blk["n"]}
        calls = res.setdefault("call", {})
        for name in sorted(new):
            if name.startswith("call_"):
                a, b = new[name], parent[name]
                calls[name[len("call_"):]] = {"block_ms": a["median"], "parent_lockstep_ms": b["median"], "ratio": a["median"] / b["median"], "parent_spread": b["spread"], "block_spread": a["spread"], "n": a["n"]}
        if args.chunks and "pass_bands_rbf_nkc%d" % args.chunks[0] in new:
            res["tile_launches_per_pass_at_30000_points"] = new["pass_bands_rbf_nkc%d" % args.chunks[0]]["median"]  # bands: one launch each
        res["method"] = (f"one child process per library and round, medians of the timed repetitions (n) after a warm-up; pass: lssvm_cg_info.matvec_kernel_ms (HIP events around the "
                         f"tile-kernel launches) of {PASS_ITERS} iterations at {SWEEP_POINTS} points, 16 features per chunk; call: host wall clock of the whole call, eps {EPS}; "
                         "spread = (max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k in ("pass", "call")}, indent=1)[:6000])
    return 0


if __name__ == "__main__":
    sys.exit(main())
