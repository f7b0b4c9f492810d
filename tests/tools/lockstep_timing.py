#!/usr/bin/env python3
"""What two right-hand sides per symmetric Gram pass save in fp64, against a library built from the PARENT commit.

usage: lockstep_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 5] [--rounds 2] [--out profiles/lockstep_f64.json]
       lockstep_timing.py --resources <plssvm_amd/lib/asm> [--out profiles/lockstep_f64.json]     (no device: adds the compiler's figures to the file)

Shapes: 100 000 x 64 polynomial degree 3 (BASELINE configs[3]'s shape) with k = 2, 4, 10 classes and 50 000 x 128 rbf with k = 4, fp64, one-vs-all targets of
make_blobs_multiclass, eps 1e-3.  Per shape this records
  pass      ONE two-vector Gram pass of this build against ONE single-vector pass of the parent, by HIP events around the tile-kernel launches
            (lssvm_cg_info.matvec_kernel_ms of a two-lane lockstep solve / of a single solve, both stopped by max_iter so that every pass is of the kind measured),
  solve     MI355CSVM.solve_systems_of_linear_equations of this build against the parent's (one resident problem, the right-hand sides one after the other), host wall
            clock of the whole call, the upload and preparation of the data included.
and, with --sweep (default), the pass comparison at 30 000 points for EVERY (kernel function, chunk count) instantiation of the two-vector kernel.
Child processes alternate between the two libraries (PLSSVM_AMD_LIBRARY), `--rounds` children per library, each with a warm-up of every shape and `--reps` timed
repetitions.  Medians, and the parent's own run-to-run spread (max - min) / median.

Condition for routing a (kernel function, chunk count) through the two-vector kernel: its pass takes less than two parent passes by more than the parent's own spread
(ratio + spread < 1, ratio = pair pass / (2 x parent pass)).  The file lists every instantiation with `routed`; one that fails is taken out of pair_kernel_routed
(lssvm_problem.hip) and falls back to two single passes.
Every child runs under a time limit of its own; a child that fails ends the run: nothing more is started on the device.
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
SHAPES = [dict(name="100000x64_poly3", n=100_000, d=64, kernel="polynomial", ks=(2, 4, 10)), dict(name="50000x128_rbf", n=50_000, d=128, kernel="rbf", ks=(4,))]
SWEEP_POINTS = 30_000
SWEEP_KERNELS = {"linear": ("linear", 3), "poly2": ("polynomial", 2), "poly3": ("polynomial", 3), "poly": ("polynomial", 4), "rbf": ("rbf", 3)}
CHUNKS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16)  # of 16 features
EPS, PASS_ITERS = 1e-3, 8


def child(which: str, reps: int, sweep: bool) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd.csvm import MI355CSVM
    from plssvm_amd.datagen import make_blobs_multiclass
    from plssvm_amd.multiclass import one_vs_all_targets
    from plssvm_amd.parameter import Parameter

    new = which == "new"
    assert new == hasattr(_capi.lib, "lssvm_mi355_problem_solve_lockstep"), "the parent's library must not have the lockstep entry point, this build's must"
    out = {}

    def pass_ms(prob, B):
        """kernel time of one Gram pass: two-vector (this build, two lanes) or single-vector (the parent), every pass of the run of that kind"""
        if new:
            _, _, infos, passes = prob.solve_lockstep(B[:2], 1e-30, PASS_ITERS)
            assert passes == (1 + PASS_ITERS, 0), passes
            return infos[0]["matvec_kernel_ms"]
        prob.cg_begin(B[0], 1e-30)
        prob.cg_step(PASS_ITERS)
        return prob.cg_finish()[2]["matvec_kernel_ms"]

    def parent_solve_systems(prm, X, B):
        """what MI355CSVM.solve_systems_of_linear_equations was before the lockstep solve"""
        with backend.ResidentProblem(prm, X, devices=[0]) as prob:
            for b in B:
                prob.cg_begin(b, EPS)
                prob.cg_step(X.shape[0])
                prob.cg_finish()

    for shape in SHAPES:
        X, y = make_blobs_multiclass(shape["n"], shape["d"], max(shape["ks"]), seed=42, dtype=np.float64)
        prm = Parameter(kernel_type=shape["kernel"], degree=3, gamma=1.0 / shape["d"], coef0=0.0, cost=1.0)
        with backend.ResidentProblem(prm, X, devices=[0]) as prob:
            B = one_vs_all_targets(np.arange(2), y, np.float64)
            for keep in [False] + [True] * reps:
                ms = pass_ms(prob, B)
                if keep:
                    out.setdefault(f"pass_{shape['name']}", []).append(ms)
        for k in shape["ks"]:
            B = one_vs_all_targets(np.arange(k), y % k, np.float64)
            for keep in [False] + [True] * reps:
                t0 = time.perf_counter()
                if new:
                    MI355CSVM(params=prm).solve_systems_of_linear_equations(prm, X, B, EPS, shape["n"])
                else:
                    parent_solve_systems(prm, X, B)
                if keep:
                    out.setdefault(f"solve_{shape['name']}_k{k}", []).append(1e3 * (time.perf_counter() - t0))
    if sweep:
        rng = np.random.default_rng(1)
        B = rng.choice([-1.0, 1.0], size=(2, SWEEP_POINTS))
        for chunks in CHUNKS:
            X = rng.uniform(-1, 1, size=(SWEEP_POINTS, 16 * chunks))
            for name, (kernel, degree) in SWEEP_KERNELS.items():
                prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / (16 * chunks), coef0=0.0, cost=1.0)
                with backend.ResidentProblem(prm, X, devices=[0]) as prob:
                    for keep in [False] + [True] * reps:
                        ms = pass_ms(prob, B)
                        if keep:
                            out.setdefault(f"sweep_{name}_nkc{chunks}", []).append(ms)
    print("RESULT " + json.dumps(out), flush=True)


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def pass_record(new, parent):
    ratio = new["median"] / (2.0 * parent["median"])
    return {"two_vector_pass_ms": new["median"], "parent_single_pass_ms": parent["median"], "ratio_to_two_parent_passes": ratio, "parent_spread": parent["spread"],
            "routed": ratio + parent["spread"] < 1.0}


def kernel_resources(asm_dir):
    """VGPRs, AGPRs, scratch and occupancy of every NV = 2 instantiation from the build's resource-usage files (make -C plssvm_amd/csrc writes them beside the ISA)"""
    rows = {}
    for unit in ("tile_launch_f64_sym2a", "tile_launch_f64_sym2b"):
        text = open(os.path.join(asm_dir, f"resource_usage_{unit}.txt")).read()
        for block in text.split("Function Name: ")[1:]:
            m = re.match(r"_ZN5lssvm18tile_matvec_f64_v2ILi(\d+)ELi(\d+)ELb1ELi2EEE", block)
            if not m:
                continue
            def field(label):
                return int(re.search(label + r": (\d+)", block).group(1))
            name = {0: "linear", 1: "poly", 3: "poly2", 4: "poly3", 2: "rbf"}[int(m.group(1))]
            rows[f"{name}_nkc{m.group(2)}"] = {"vgprs": field("VGPRs"), "agprs": field("AGPRs"), "scratch_bytes": field(r"ScratchSize \[bytes/lane\]"),
                                              "waves_per_simd": field(r"Occupancy \[waves/SIMD\]"), "workgroups_per_cu_by_launch_bounds": 2 if int(m.group(2)) <= 4 else 1,
                                              "lds_bytes": 50176}
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--resources", help="plssvm_amd/lib/asm of this build: only add the compiler's figures to --out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=280, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lockstep_f64.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps, not args.no_sweep)
        return 0
    if args.resources:
        res = json.load(open(args.out)) if os.path.isfile(args.out) else {}
        res["kernels"] = kernel_resources(args.resources)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    samples = {"parent": {}, "new": {}}
    for rnd in range(args.rounds):
        for which in ("parent", "new"):
            env = dict(os.environ)
            if which == "parent":
                env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("PLSSVM_AMD_LIBRARY", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(args.reps)] + (["--no-sweep"] if args.no_sweep else [])
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
    res = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    res["shapes"] = {}
    for shape in SHAPES:
        rec = {"pass": pass_record(new[f"pass_{shape['name']}"], parent[f"pass_{shape['name']}"]), "solve": {}}
        for k in shape["ks"]:
            a, b = new[f"solve_{shape['name']}_k{k}"], parent[f"solve_{shape['name']}_k{k}"]
            rec["solve"][f"k{k}"] = {"lockstep_ms": a["median"], "parent_ms": b["median"], "ratio": a["median"] / b["median"], "parent_spread": b["spread"], "lockstep_spread": a["spread"]}
        res["shapes"][shape["name"]] = rec
    res["instantiations"] = {name[len("sweep_"):]: pass_record(new[name], parent[name]) for name in sorted(new) if name.startswith("sweep_")}
    res["method"] = (f"{args.rounds} alternating child processes per library, {args.reps} timed repetitions after a warm-up; pass: lssvm_cg_info.matvec_kernel_ms (HIP events around the "
                     f"tile-kernel launches) of {PASS_ITERS} iterations; solve: host wall clock of the whole call, eps {EPS}; instantiations: the pass comparison at {SWEEP_POINTS} points, "
                     "16 features per chunk; routed: ratio + parent_spread < 1")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"shapes": res["shapes"], "not_routed": [k for k, v in res["instantiations"].items() if not v["routed"]]}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
