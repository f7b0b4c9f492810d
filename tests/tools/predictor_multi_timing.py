#!/usr/bin/env python3
"""What the resident predictor of a one-vs-all model saves, against a library built from the PARENT commit.

usage: predictor_multi_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 5] [--rounds 2] [--out profiles/predictor_multi.json]

rbf, fp32, 50 000 support vectors x 128 features, k = 2, 4, 10 weight vectors, batches of 1 000, 4 096 and 200 000 points.  Per (k, batch) this times
  resident_multi       lssvm_mi355_predictor_predict_multi of this build (the model created once per child process, outside the timed calls),
  parent_one_shot      predict_values_multi of the parent's library (what multiclass.decision_values called before),
  parent_k_singles     k single-vector resident predictors of the parent's library, one call each, summed (what a caller could build from the parent's entry points),
and, at 4 096 points, ONE launch of the 128-row two-vector kernel (resident_multi with k = 2: kernel_ms) against ONE single-vector launch of the parent (one of
parent_k_singles).  Child processes alternate between the two libraries (PLSSVM_AMD_LIBRARY; two copies of one library in one process would resolve each other's
symbols), `--rounds` children per library, each with a warm-up call of every shape and `--reps` timed calls per shape, the shapes of a child in turn.  It reads
lssvm_predict_info (kernel_ms: HIP events around the product launches, summed; total_ms: the call's host wall clock) and writes medians and the spread.

Condition for shipping the 128-row two-vector instantiations: their launch takes less than two single-vector launches of the parent by more than the parent's own
run-to-run spread (ratios.two_vector_launch_over_two_parent_launches + ratios.parent_launch_spread < 1).
Every child runs under a time limit of its own; a child that fails ends the run: nothing more is started on the device.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPE = dict(num_sv=50_000, d=128, seed=42)
KS = (2, 4, 10)
BATCHES = (1_000, 4_096, 200_000)
KEYS = ("kernel_ms", "total_ms")


def child(which: str, reps: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    num_sv, d, seed = SHAPE["num_sv"], SHAPE["d"], SHAPE["seed"]
    X, _ = make_blobs_pm1(num_sv + max(BATCHES), d, seed=seed + 1, dtype=np.float32)  # (bench.py's predict leg)
    sv, pool = np.ascontiguousarray(X[:num_sv]), np.ascontiguousarray(X[num_sv:])
    alpha = np.random.default_rng(seed).standard_normal((max(KS), num_sv)).astype(np.float32)
    rho = (0.25 * (1 + np.arange(max(KS)))).astype(np.float32)
    prm = Parameter(kernel_type="rbf", gamma=None, cost=1.0)
    out = {}

    def record(name, infos):
        out.setdefault(name, []).append({key: sum(i[key] for i in infos) for key in KEYS})

    if which == "new":
        preds = {k: backend.Predictor(prm, sv, alpha[:k], rho[:k].astype(np.float64)) for k in KS}

        def run(k, n, keep):
            info = {}
            preds[k].predict(pool[:n], info_out=info)
            assert info["resident"] == 1 and info["vectors_per_launch"] == 2, info
            if keep:
                record(f"resident_multi_k{k}_n{n}", [info])
    else:
        singles = [backend.Predictor(prm, sv, alpha[v], float(rho[v])) for v in range(max(KS))]

        def run(k, n, keep):
            info = {}
            backend.predict_values_multi(prm, sv, alpha[:k], rho[:k], None, pool[:n], info_out=info)
            infos = []
            for v in range(k):
                infos.append({})
                singles[v].predict(pool[:n], info_out=infos[-1])
                assert infos[-1]["resident"] == 1, infos[-1]
            if keep:
                record(f"parent_one_shot_k{k}_n{n}", [info])
                record(f"parent_k_singles_k{k}_n{n}", infos)
                if k == KS[0]:
                    record(f"parent_single_launch_n{n}", infos[:1])

    for keep in [False] + [True] * reps:  # (a warm-up of every shape: code-object load, first allocations)
        for n in BATCHES:
            for k in KS:
                run(k, n, keep)
    print("RESULT " + json.dumps(out), flush=True)


def summary(samples):
    res = {}
    for key in KEYS:
        v = [s[key] for s in samples]
        med = statistics.median(v)
        res[key] = {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_multi.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps)
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    samples = {}
    for rnd in range(args.rounds):
        for which in ("parent", "new"):
            env = dict(os.environ)
            if which == "parent":
                env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("PLSSVM_AMD_LIBRARY", None)
            try:
                proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(args.reps)], env=env, capture_output=True, text=True,
                                      timeout=args.child_timeout)
            except subprocess.TimeoutExpired:
                print(f"round {rnd}, {which}: child exceeded {args.child_timeout} s; stopping", file=sys.stderr)
                return 1
            line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if proc.returncode != 0 or line is None:
                print(f"round {rnd}, {which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}", file=sys.stderr)
                return 1
            for name, vals in json.loads(line[len("RESULT "):]).items():
                samples.setdefault(name, []).extend(vals)
            print(f"round {rnd}, {which}: done", flush=True)
    res = {name: summary(v) for name, v in sorted(samples.items())}
    ratios = {}
    for k in KS:
        for n in BATCHES:
            new = res[f"resident_multi_k{k}_n{n}"]
            for base in ("parent_one_shot", "parent_k_singles"):
                for key in KEYS:
                    ratios[f"resident_multi_over_{base}_{key}_k{k}_n{n}"] = new[key]["median"] / res[f"{base}_k{k}_n{n}"][key]["median"]
    n = 4_096
    one = res[f"parent_single_launch_n{n}"]["kernel_ms"]
    ratios["two_vector_launch_ms"] = res[f"resident_multi_k2_n{n}"]["kernel_ms"]["median"]
    ratios["parent_single_launch_ms"] = one["median"]
    ratios["two_vector_launch_over_two_parent_launches"] = res[f"resident_multi_k2_n{n}"]["kernel_ms"]["median"] / (2 * one["median"])
    ratios["parent_launch_spread"] = one["spread"]
    res["ratios"] = ratios
    res["workload"] = f"rbf, fp32, {SHAPE['num_sv']} support vectors x {SHAPE['d']} features (bench.py's predict leg's data), k in {list(KS)}, batches of {list(BATCHES)} points"
    res["method"] = (f"{args.rounds} alternating child processes per library, {args.reps} timed calls per shape after a warm-up of every shape; kernel_ms = HIP events around the product "
                     "launches, summed over a call's launches; parent_k_singles: the sum over k single-vector calls; the 128-row two-vector launch: resident_multi_k2 at 4 096 points")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(ratios, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
