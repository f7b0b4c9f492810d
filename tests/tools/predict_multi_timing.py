#!/usr/bin/env python3
"""What a second weight vector costs in one pass of the rectangular 256-row kernel, against a library built from the PARENT commit.

usage: predict_multi_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 5] [--rounds 2] [--out profiles/predict_multi.json]

At the benchmark's predict shape (bench.py's predict leg: 200 000 points x 50 000 support vectors x 128 features, rbf, fp32, its seeds) this times
  parent_single   the single-vector predict_values of the parent's library (the baseline is the parent's CODE, not this build),
  new_single      the same call of this build (the NV = 1 instantiation: must not be slower),
  multi_k2 / k4   predict_values_multi of this build with 2 and 4 weight vectors (one and two launches of the two-vector kernel),
in ONE command: child processes that alternate between the two libraries (PLSSVM_AMD_LIBRARY; two copies of one library in one process would resolve each
other's symbols), `--rounds` children per library, each with a warm-up call of every shape and `--reps` timed calls per shape, the shapes of a child in turn.
It reads lssvm_predict_info (kernel_ms: HIP events around the product launches; total_ms: the call's host wall clock) and writes medians and the spread.

Condition of usefulness: multi_k2.kernel_ms < 2 x parent_single.kernel_ms by more than the baseline's own spread in this run.
A child that fails ends the run: nothing more is started on the device.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPE = dict(num_sv=50_000, num_points=200_000, d=128, seed=42)


def child(which: str, reps: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    num_sv, d, seed = SHAPE["num_sv"], SHAPE["d"], SHAPE["seed"]
    X, _ = make_blobs_pm1(num_sv + SHAPE["num_points"], d, seed=seed + 1, dtype=np.float32)  # (bench.py, predict_leg)
    sv, pts = np.ascontiguousarray(X[:num_sv]), np.ascontiguousarray(X[num_sv:])
    alpha = np.random.default_rng(seed).standard_normal((4, num_sv)).astype(np.float32)  # (row 0 = the predict leg's alpha)
    rho = np.array([0.25, 0.5, 0.75, 1.0], dtype=np.float32)
    prm = Parameter(kernel_type="rbf", gamma=None, cost=1.0)

    def single():
        info = {}
        backend.predict_values(prm, sv, alpha[0], 0.25, None, pts, info_out=info)
        return info

    def multi(k):
        info = {}
        backend.predict_values_multi(prm, sv, alpha[:k], rho[:k], None, pts, info_out=info)
        assert info["vectors_per_launch"] == 2, info
        return info

    shapes = {"single": single} if which == "parent" else {"single": single, "multi_k2": lambda: multi(2), "multi_k4": lambda: multi(4)}
    for fn in shapes.values():
        fn()  # warm-up: code-object load, first allocations
    out = {name: [] for name in shapes}
    for _ in range(reps):
        for name, fn in shapes.items():
            info = fn()
            out[name].append({"kernel_ms": info["kernel_ms"], "total_ms": info["total_ms"], "setup_ms": info["setup_ms"]})
    print("RESULT " + json.dumps(out), flush=True)


def summary(samples):
    res = {}
    for key in ("kernel_ms", "total_ms", "setup_ms"):
        v = [s[key] for s in samples]
        med = statistics.median(v)
        res[key] = {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_multi.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps)
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    samples = {"parent_single": [], "new_single": [], "multi_k2": [], "multi_k4": []}
    for rnd in range(args.rounds):
        for which in ("parent", "new"):
            env = dict(os.environ)
            if which == "parent":
                env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("PLSSVM_AMD_LIBRARY", None)
            proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=240)
            line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if proc.returncode != 0 or line is None:
                print(f"round {rnd}, {which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}", file=sys.stderr)
                return 1
            got = json.loads(line[len("RESULT "):])
            for name, vals in got.items():
                samples[("parent_" if which == "parent" else "new_") + name if name == "single" else name] += vals
            print(f"round {rnd}, {which}: " + ", ".join(f"{n} kernel {statistics.median(s['kernel_ms'] for s in v):.3f} ms" for n, v in got.items()), flush=True)
    res = {name: summary(v) for name, v in samples.items()}
    base_k, base_t = res["parent_single"]["kernel_ms"]["median"], res["parent_single"]["total_ms"]["median"]
    res["ratios"] = {
        "multi_k2_kernel_over_one_parent_launch": res["multi_k2"]["kernel_ms"]["median"] / base_k,
        "multi_k2_kernel_over_two_parent_launches": res["multi_k2"]["kernel_ms"]["median"] / (2 * base_k),
        "multi_k4_kernel_over_four_parent_launches": res["multi_k4"]["kernel_ms"]["median"] / (4 * base_k),
        "multi_k2_total_over_two_parent_calls": res["multi_k2"]["total_ms"]["median"] / (2 * base_t),
        "multi_k4_total_over_four_parent_calls": res["multi_k4"]["total_ms"]["median"] / (4 * base_t),
        "new_single_kernel_over_parent": res["new_single"]["kernel_ms"]["median"] / base_k,
        "new_single_total_over_parent": res["new_single"]["total_ms"]["median"] / base_t,
        "parent_kernel_spread": res["parent_single"]["kernel_ms"]["spread"],
    }
    res["workload"] = f"predict_values: {SHAPE['num_points']} points x {SHAPE['num_sv']} support vectors x {SHAPE['d']} features, rbf, fp32 (bench.py's predict leg)"
    res["method"] = f"{args.rounds} alternating child processes per library, {args.reps} timed calls per shape after a warm-up of every shape; kernel_ms = HIP events around the product launches"
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res["ratios"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
