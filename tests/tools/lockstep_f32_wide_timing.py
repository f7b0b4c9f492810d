#!/usr/bin/env python3
"""What two right-hand sides per symmetric Gram pass save in fp32 on 129 ... 512 features, against a library built from the PARENT commit.

usage: lockstep_f32_wide_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 5] [--rounds 2] [--out profiles/lockstep_f32_wide.json]
       lockstep_f32_wide_timing.py --resources <plssvm_amd/lib/asm> [--out profiles/lockstep_f32_wide.json]     (no device: adds the compiler's figures to the file)

Per instantiation of the symmetric two-vector split kernels (tile_launch_f32v2ws.hip: plane kind x kernel function x 64-feature chunks, 38 of them) at 30 000 points
of uniform(-1, 1) data this records
  pass      ONE two-vector Gram pass of this build -- the pass lssvm_mi355_problem_matvec_pair and the lockstep CG run -- against TWO single-vector passes of the
            parent, by HIP events around the tile-kernel launches (lssvm_cg_info.matvec_kernel_ms of a two-lane lockstep solve / of a single solve, both stopped by
            max_iter so that every pass is of the kind measured),
and at the call level, at 30 000 x 256 rbf (f16x3 planes) and 30 000 x 512 polynomial of degree 3 on make_blobs_multiclass data, for k = 2, 4, 10 right-hand sides of two
kinds -- `ova`: the one-vs-all targets at cost 1 (well separated blobs: a few iterations, the call is mostly upload and preparation); `rand`: random +-1 labels at cost
100 (many iterations: the call is mostly Gram passes) --,
  solve     MI355CSVM.solve_systems_of_linear_equations of this build (the lockstep on lanes) against the parent's (the same call: there the right-hand sides one after
            the other on one resident problem), host wall clock of the whole call, the upload and preparation of the data included.
Child processes alternate between the two libraries (PLSSVM_AMD_LIBRARY), `--rounds` children per library, each with a warm-up of every shape and `--reps` timed
repetitions: medians of rounds x reps samples, and the parent's own run-to-run spread (max - min) / median.

Condition for routing an instantiation through the two-vector kernel (the project's rule): ratio + spread < 1, ratio = pair pass / (2 x parent pass).  The file lists
every instantiation with `routed`; one that fails is named in sym_pair_routed (lssvm_problem.hip) and takes two single passes.
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
POINTS = 30_000
SHAPES = [dict(name="30000x256_rbf", d=256, kernel="rbf", ks=(2, 4, 10)), dict(name="30000x512_poly3", d=512, kernel="polynomial", ks=(2, 4, 10))]
SWEEP_KERNELS = {"poly": ("polynomial", 4), "poly2": ("polynomial", 2), "poly3": ("polynomial", 3), "rbf": ("rbf", 3)}
PLANES = {"f16x3": None, "bf16x6": 1}  # Options.gram_mode
EPS, PASS_ITERS = 1e-3, 8
RHS_KINDS = {"ova": 1.0, "rand": 100.0}  # right-hand sides of the call-level shapes: kind -> cost
SOLVE_MAX_ITER = 200  # (both libraries alike: bounds a child's time whatever the conditioning)


def instantiations():
    for planes in PLANES:
        for name in SWEEP_KERNELS:
            for nk64 in range(3, (8 if planes == "f16x3" and name != "rbf" else 6) + 1):
                yield planes, name, nk64


def child(which: str, reps: int, sweep: bool) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd.csvm import MI355CSVM
    from plssvm_amd.datagen import make_blobs_multiclass
    from plssvm_amd.multiclass import one_vs_all_targets
    from plssvm_amd.parameter import Parameter

    new = which == "new"
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

    for shape in SHAPES:
        X, y = make_blobs_multiclass(POINTS, shape["d"], max(shape["ks"]), seed=42, dtype=np.float32)
        labels = np.random.default_rng(2).choice([-1.0, 1.0], size=(max(shape["ks"]), POINTS)).astype(np.float32)
        for kind, cost in RHS_KINDS.items():
            prm = Parameter(kernel_type=shape["kernel"], degree=3, gamma=1.0 / shape["d"], coef0=0.0, cost=cost)
            for k in shape["ks"]:
                B = one_vs_all_targets(np.arange(k), y % k, np.float32) if kind == "ova" else labels[:k]
                for keep in [False] + [True] * reps:
                    t0 = time.perf_counter()
                    _, _, infos = MI355CSVM(params=prm).solve_systems_of_linear_equations(prm, X, B, EPS, SOLVE_MAX_ITER)
                    if keep:
                        out.setdefault(f"solve_{shape['name']}_{kind}_k{k}", []).append(1e3 * (time.perf_counter() - t0))
                        out.setdefault(f"its_{shape['name']}_{kind}_k{k}", []).append(float(sum(info["iterations"] for info in infos)))
    if sweep:
        rng = np.random.default_rng(1)
        B = rng.choice([-1.0, 1.0], size=(2, POINTS)).astype(np.float32)
        for planes, name, nk64 in instantiations():
            kernel, degree = SWEEP_KERNELS[name]
            X = rng.uniform(-1, 1, size=(POINTS, 64 * nk64)).astype(np.float32)
            prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / (64 * nk64), coef0=0.0, cost=1.0)
            options = _capi.Options(gram_mode=PLANES[planes]) if PLANES[planes] is not None else None
            with backend.ResidentProblem(prm, X, devices=[0], options=options) as prob:
                for keep in [False] + [True] * reps:
                    ms = pass_ms(prob, B)
                    if keep:
                        out.setdefault(f"sweep_{planes}_{name}_nk{nk64}", []).append(ms)
    print("RESULT " + json.dumps(out), flush=True)


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def pass_record(new, parent):
    ratio = new["median"] / (2.0 * parent["median"])
    return {"two_vector_pass_ms": new["median"], "parent_single_pass_ms": parent["median"], "ratio_to_two_parent_passes": ratio, "parent_spread": parent["spread"],
            "two_vector_spread": new["spread"], "samples": new["n"], "routed": ratio + parent["spread"] < 1.0}


def kernel_resources(asm_dir):
    """VGPRs, AGPRs, scratch and occupancy of every instantiation from the build's resource-usage files (make -C plssvm_amd/csrc writes them beside the ISA)"""
    rows = {}
    names = {1: "poly", 3: "poly2", 4: "poly3", 5: "rbf"}
    for unit, planes in (("tile_launch_f32v2ws_f16", "f16x3"), ("tile_launch_f32v2ws_bf16", "bf16x6")):
        text = open(os.path.join(asm_dir, f"resource_usage_{unit}.txt")).read()
        for block in text.split("Function Name: ")[1:]:
            m = re.match(r"_ZN5lssvm\d+tile_matvec_f32_(?:f3w|s6w)_nv2sILi(\d+)ELi(\d+)EEE", block)
            if not m:
                continue

            def field(label):
                return int(re.search(label + r": (\d+)", block).group(1))

            rows[f"{planes}_{names[int(m.group(1))]}_nk{m.group(2)}"] = {"vgprs": field("VGPRs"), "agprs": field("AGPRs"), "scratch_bytes": field(r"ScratchSize \[bytes/lane\]"),
                                                                        "waves_per_simd": field(r"Occupancy \[waves/SIMD\]"), "vgpr_spills": field("VGPRs Spill"), "lds_bytes": 81408}
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--resources", help="plssvm_amd/lib/asm of this build: only add the compiler's figures to --out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=400, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lockstep_f32_wide.json"))
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
        rec = {}
        for kind in RHS_KINDS:
            for k in shape["ks"]:
                key = f"{shape['name']}_{kind}_k{k}"
                a, b = new[f"solve_{key}"], parent[f"solve_{key}"]
                rec[f"{kind}_k{k}"] = {"lockstep_ms": a["median"], "parent_ms": b["median"], "ratio": a["median"] / b["median"], "parent_spread": b["spread"], "lockstep_spread": a["spread"],
                                       "iterations_of_all_columns": new[f"its_{key}"]["median"], "parent_iterations_of_all_columns": parent[f"its_{key}"]["median"]}
        res["shapes"][shape["name"]] = {"solve": rec}
    res["instantiations"] = {name[len("sweep_"):]: pass_record(new[name], parent[name]) for name in sorted(new) if name.startswith("sweep_")}
    res["method"] = (f"{args.rounds} alternating child processes per library, {args.reps} timed repetitions after a warm-up; pass: lssvm_cg_info.matvec_kernel_ms (HIP events around the "
                     f"tile-kernel launches) of {PASS_ITERS} iterations at {POINTS} points, 64 features per chunk, float32; solve: host wall clock of the whole call, eps {EPS}, at most {SOLVE_MAX_ITER} iterations; "
                     "routed: ratio + parent_spread < 1")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"shapes": res["shapes"], "not_routed": [k for k, v in res["instantiations"].items() if not v["routed"]]}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
