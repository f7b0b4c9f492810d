#!/usr/bin/env python3
"""What two right-hand sides per symmetric Gram pass save BEYOND the one-pass kernels (the panel kernels), against a library built from the PARENT commit.

usage: lockstep_panels_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 10] [--solve-reps 3] [--rounds 1] [--out profiles/lockstep_panels.json]
       lockstep_panels_timing.py --resources <plssvm_amd/lib/asm> [--out profiles/lockstep_panels.json]     (no device: adds the compiler's figures to the file)

Per instantiation of the symmetric two-vector panel kernels (tile_launch_f32xv2s.hip: f16x3 / bf16x6 planes x polynomial of a run-time degree, degree 2, degree 3, folded
rbf, at 640 and 784 features; tile_launch_f64xv2s.hip: rbf and the three polynomial forms at 320 and 784) at 30 000 points of uniform(-1, 1) data this records
  pass      ONE two-vector Gram pass of this build -- the pass lssvm_mi355_problem_matvec_pair_panels and the lockstep CG run -- against TWO single-vector passes of the
            parent, by HIP events around the tile-kernel launches (lssvm_cg_info.matvec_kernel_ms of a two-lane lockstep solve / of a single solve, both stopped by
            max_iter so that every pass is of the kind measured); `dispatched`: whether this build's sym_panel_pair_routed sent the pair through the two-vector kernel,
and at the call level, at 30 000 x 784 rbf in float32 and float64 on make_blobs_multiclass data, for k = 2, 4, 10 one-vs-all right-hand sides,
  solve     MI355CSVM.solve_systems_of_linear_equations of this build (the lockstep on lanes, panels entry point) against the parent's (the same call: there the
            right-hand sides one after the other on one resident problem), host wall clock of the whole call, the upload and preparation of the data included.
One child process per library and round (PLSSVM_AMD_LIBRARY), alternating, each with a warm-up of every shape: medians, and the parent's own run-to-run spread
(max - min) / median.  Every timed shape's result (alpha of the first right-hand side / all alphas of the call) is hashed in both children and compared bit for bit.

Condition for routing an instantiation through the two-vector kernel (the project's rule): ratio + spread < 1, ratio = pair pass / (2 x parent pass).  The file lists
every instantiation with `routed` (the measurement) and `dispatched` (the library); one that fails is named in sym_panel_pair_routed (lssvm_problem.hip).
Every child runs under a time limit of its own; a child that fails ends the run: nothing more is started on the device.
"""

import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
POINTS = 30_000
SWEEP_KERNELS = {"poly": ("polynomial", 4), "poly2": ("polynomial", 2), "poly3": ("polynomial", 3), "rbf": ("rbf", 3)}
PLANES = {"f16x3": ("float32", None, (640, 784)), "bf16x6": ("float32", 1, (640, 784)), "fp64": ("float64", None, (320, 784))}  # dtype, Options.gram_mode, features
SOLVE = {"30000x784_rbf_f32": "float32", "30000x784_rbf_f64": "float64"}
KS = (2, 4, 10)
EPS, PASS_ITERS, SOLVE_MAX_ITER = 1e-3, 8, 200


def child(which: str, reps: int, solve_reps: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd.csvm import MI355CSVM
    from plssvm_amd.datagen import make_blobs_multiclass
    from plssvm_amd.multiclass import one_vs_all_targets
    from plssvm_amd.parameter import Parameter

    new = which == "new"
    if not new:  # (the parent's library has no _panels entry points: the same Python calls its solve_lockstep)
        plain = backend.ResidentProblem.solve_lockstep
        backend.ResidentProblem.solve_lockstep = lambda self, B, eps, max_iter, panels=False: plain(self, B, eps, max_iter)
    out, bits = {}, {}

    def digest(a):
        return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]

    rng = np.random.default_rng(1)
    for planes, (dtype, gram_mode, features) in PLANES.items():
        B = rng.choice([-1.0, 1.0], size=(2, POINTS)).astype(dtype)
        for d in features:
            X = rng.uniform(-1, 1, size=(POINTS, d)).astype(dtype)
            for name, (kernel, degree) in SWEEP_KERNELS.items():
                prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=0.0, cost=1.0)
                key = f"{planes}_{name}_{d}"
                with backend.ResidentProblem(prm, X, devices=[0], options=_capi.Options(gram_mode=gram_mode) if gram_mode is not None else None) as prob:
                    for keep in [False] + [True] * reps:
                        if new:  # kernel time of one Gram pass of the pair
                            alphas, _, infos, passes = prob.solve_lockstep(B, 1e-30, PASS_ITERS, panels=True)
                            out[f"dispatched_{key}"] = [float(passes[0] == 1 + PASS_ITERS and passes[1] == 0)]
                            ms, alpha = infos[0]["matvec_kernel_ms"], alphas[0]
                        else:  # ... of a single-vector pass
                            prob.cg_begin(B[0], 1e-30)
                            prob.cg_step(PASS_ITERS)
                            alpha, _, info = prob.cg_finish()
                            ms = info["matvec_kernel_ms"]
                        if keep:
                            out.setdefault(f"sweep_{key}", []).append(ms)
                    bits[f"sweep_{key}"] = digest(alpha)
    for shape, dtype in SOLVE.items():
        X, y = make_blobs_multiclass(POINTS, 784, max(KS), seed=42, dtype=np.dtype(dtype).type)
        prm = Parameter(kernel_type="rbf", gamma=1.0 / 784, cost=1.0)
        for k in KS:
            Bk = one_vs_all_targets(np.arange(k), y % k, np.dtype(dtype).type)
            for keep in [False] + [True] * solve_reps:
                t0 = time.perf_counter()
                alphas, _, infos = MI355CSVM(params=prm).solve_systems_of_linear_equations(prm, X, Bk, EPS, SOLVE_MAX_ITER)
                if keep:
                    out.setdefault(f"solve_{shape}_k{k}", []).append(1e3 * (time.perf_counter() - t0))
                    out.setdefault(f"its_{shape}_k{k}", []).append(float(sum(info["iterations"] for info in infos)))
            bits[f"solve_{shape}_k{k}"] = digest(alphas)
    print("RESULT " + json.dumps({"samples": out, "bits": bits}), flush=True)


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def kernel_resources(asm_dir):
    """VGPRs, scratch, occupancy and LDS bytes of every instantiation from the build's resource-usage files (make -C plssvm_amd/csrc writes them beside the ISA)"""
    rows = {}
    names = {1: "poly", 2: "rbf", 3: "poly2", 4: "poly3", 5: "rbf"}
    for unit, pattern, lds in (("tile_launch_f32xv2s", r"_ZN5lssvm\d+tile_matvec_f32_wide_nv2sILi(\d+)ELi(\d+)EEE", 81408), ("tile_launch_f64xv2s", r"_ZN5lssvm\d+tile_matvec_f64_wideILi(\d+)ELb1ELi(2)EEE", 50176)):
        text = open(os.path.join(asm_dir, f"resource_usage_{unit}.txt")).read()
        for block in text.split("Function Name: ")[1:]:
            m = re.match(pattern, block)
            if not m:
                continue

            def field(label):
                return int(re.search(label + r": (\d+)", block).group(1))

            planes = "fp64" if unit.endswith("f64xv2s") else {2: "f16x3", 3: "bf16x6"}[int(m.group(2))]
            rows[f"{planes}_{names[int(m.group(1))]}"] = {"vgprs": field("VGPRs"), "agprs": field("AGPRs"), "scratch_bytes": field(r"ScratchSize \[bytes/lane\]"),
                                                         "waves_per_simd": field(r"Occupancy \[waves/SIMD\]"), "vgpr_spills": field("VGPRs Spill"), "lds_bytes": lds}
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--resources", help="plssvm_amd/lib/asm of this build: only add the compiler's figures to --out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--solve-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--child-timeout", type=int, default=500, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lockstep_panels.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps, args.solve_reps)
        return 0
    res = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    if args.resources:
        res["kernels"] = kernel_resources(args.resources)
    else:
        if not args.parent_lib or not os.path.isfile(args.parent_lib):
            ap.error("--parent-lib must name the library built from the parent commit")
        samples, bits = {"parent": {}, "new": {}}, {"parent": {}, "new": {}}
        for rnd in range(args.rounds):
            for which in ("parent", "new"):
                env = dict(os.environ)
                env.pop("PLSSVM_AMD_LIBRARY", None)
                if which == "parent":
                    env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(args.reps), "--solve-reps", str(args.solve_reps)]
                try:
                    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
                except subprocess.TimeoutExpired:
                    print(f"round {rnd}, {which}: child exceeded {args.child_timeout} s; stopping", file=sys.stderr)
                    return 1
                line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
                if proc.returncode != 0 or line is None:
                    print(f"round {rnd}, {which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}", file=sys.stderr)
                    return 1
                got = json.loads(line[len("RESULT "):])
                for name, vals in got["samples"].items():
                    samples[which].setdefault(name, []).extend(vals)
                bits[which].update(got["bits"])
                print(f"round {rnd}, {which}: done", flush=True)
        new = {name: summary(v) for name, v in samples["new"].items()}
        parent = {name: summary(v) for name, v in samples["parent"].items()}
        res["instantiations"] = {}
        for name in sorted(n for n in new if n.startswith("sweep_")):
            a, b = new[name], parent[name]
            ratio = a["median"] / (2.0 * b["median"])
            res["instantiations"][name[len("sweep_"):]] = {"two_vector_pass_ms": a["median"], "parent_single_pass_ms": b["median"], "ratio_to_two_parent_passes": ratio, "parent_spread": b["spread"],
                                                          "two_vector_spread": a["spread"], "samples": a["n"], "routed": ratio + b["spread"] < 1.0,
                                                          "dispatched": bool(new["dispatched_" + name[len("sweep_"):]]["median"]), "same_bits_as_parent": bits["new"][name] == bits["parent"][name]}
        res["shapes"] = {}
        for shape in SOLVE:
            for k in KS:
                key = f"solve_{shape}_k{k}"
                a, b = new[key], parent[key]
                res["shapes"].setdefault(shape, {})[f"k{k}"] = {"lockstep_ms": a["median"], "parent_ms": b["median"], "ratio": a["median"] / b["median"], "parent_spread": b["spread"], "lockstep_spread": a["spread"],
                                                               "iterations_of_all_columns": new[f"its_{shape}_k{k}"]["median"], "same_bits_as_parent": bits["new"][key] == bits["parent"][key]}
        res["method"] = (f"{args.rounds} alternating child process(es) per library, {args.reps} timed repetitions after a warm-up (solve: {args.solve_reps}); pass: lssvm_cg_info.matvec_kernel_ms (HIP events "
                         f"around the tile-kernel launches) of {PASS_ITERS} iterations at {POINTS} points; solve: host wall clock of the whole call, one-vs-all targets, eps {EPS}, at most {SOLVE_MAX_ITER} "
                         "iterations; routed: ratio + parent_spread < 1; same_bits_as_parent: sha256 of the results of both libraries")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "method"}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
