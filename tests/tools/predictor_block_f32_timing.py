#!/usr/bin/env python3
"""What sixteen fp32 weight vectors per pass (lssvm_mi355_predictor_create_block32, tile_matvec_f32_blk) cost and save, against a library built from the PARENT commit.

usage: predictor_block_f32_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 10] [--phases launch,call] [--out profiles/predictor_block_f32.json]

launch level   For EVERY (kernel function, chunk count, plane kind) instantiation -- polynomial of a run-time degree, degree 2, degree 3 and folded rbf on 32, 64 and 128
               features, f16x3 (the default planes) and bf16x6 (gram_mode = 1) -- at 4 096 points x 30 000 support vectors: kernel_ms of ONE sixteen-vector launch of this
               build (a block32 handle of sixteen vectors) over kernel_ms of ONE single-vector launch of the parent's lssvm_mi355_predict_values_f32, and over the EIGHT pair
               launches of the parent's lssvm_mi355_predictor_create_resident handle of the same sixteen vectors; the parent's run-to-run spread, (max - min) / median,
               beside every ratio.
call level     50 000 x 128 rbf and 100 000 x 64 polynomial (degree 3), k = 1, 2, 4, 10, 16 weight vectors, batches of 1 000, 4 096 and 200 000 points: total_ms (the call's
               host wall clock) and kernel_ms of lssvm_mi355_predictor_predict_multi on the block32 handle against the parent's create_resident handle (which takes the
               rectangular 256-row kernel from 64 row blocks on).
One child process per library and part (PLSSVM_AMD_LIBRARY; two copies of one library in one process would resolve each other's symbols), each with a warm-up call of
every shape and `--reps` timed calls per shape: medians, and the spread.  Ratios are reported as measured, the losses included; nothing is routed on them.
Every child runs under a time limit of its own; a child that fails ends the run: nothing more is started on the device.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LAUNCH_POINTS, LAUNCH_SV, LAUNCH_K = 4_096, 30_000, 16
LAUNCH_KERNELS = {"poly": ("polynomial", 5), "poly2": ("polynomial", 2), "poly3": ("polynomial", 3), "rbf": ("rbf", 3)}
FEATURES = (32, 64, 128)
PLANES = {"f16x3": 0, "bf16x6": 1}  # option gram_mode (0 here: the default left alone, f16 planes on this data)
MODELS = {"50000x128_rbf": dict(num_sv=50_000, d=128, kernel="rbf", degree=3), "100000x64_poly3": dict(num_sv=100_000, d=64, kernel="polynomial", degree=3)}
KS = (1, 2, 4, 10, 16)
BATCHES = (1_000, 4_096, 200_000)
KEYS = ("kernel_ms", "total_ms")
COEF0 = 0.5
EXPECTED_BLOCK_OVER_SINGLE_128_F16X3 = 1.7  # 192 16x16x32 MFMAs + 64 16x16x4 fp32 MFMAs of about twice the length, per wave and tile: an instruction count, not a measurement


def child(which: str, part: str, reps: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd._capi import Options
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    new = which == "new"
    assert new == hasattr(_capi.lib, "lssvm_mi355_predictor_create_block32"), "the parent's library must not have the new entry point, this build's must"
    form = dict(block32=True) if new else dict(every_form=True)
    per_launch = 16 if new else 2
    out = {}

    def timed(name, pred, pts, want_launch, want_mode=None):
        for keep in [False] + [True] * reps:
            info = {}
            pred.predict(pts, info_out=info)
            assert info["resident"] == 1 and info["vectors_per_launch"] in (want_launch, 0) and want_mode in (None, info["gram_mode"]), info
            if keep:
                out.setdefault(name, []).append({key: info[key] for key in KEYS})

    if part == "launch":
        X, _ = make_blobs_pm1(LAUNCH_SV + LAUNCH_POINTS, max(FEATURES), seed=7, dtype=np.float32)
        alpha = np.random.default_rng(3).standard_normal((LAUNCH_K, LAUNCH_SV)).astype(np.float32)
        rho = 0.25 * (1 + np.arange(LAUNCH_K))
        for d in FEATURES:
            sv, pts = np.ascontiguousarray(X[:LAUNCH_SV, :d]), np.ascontiguousarray(X[LAUNCH_SV:, :d])
            for plane, gm in PLANES.items():
                opts = Options(gram_mode=gm) if gm else Options()
                for name, (kernel, degree) in LAUNCH_KERNELS.items():
                    tag = f"{name}_d{d}_{plane}"
                    prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=COEF0)
                    with backend.Predictor(prm, sv, alpha, rho, options=opts, **form) as pred:
                        timed(f"{'block_launch' if new else 'eight_pair_launches'}_{tag}", pred, pts, per_launch, 2 if plane == "f16x3" else 1)
                    if not new:
                        for keep in [False] + [True] * reps:
                            info = {}
                            backend.predict_values(prm, sv, alpha[0], float(rho[0]), None, pts, options=opts, info_out=info)
                            if keep:
                                out.setdefault(f"single_launch_{tag}", []).append({key: info[key] for key in KEYS})
    else:
        m = MODELS[part]
        X, _ = make_blobs_pm1(m["num_sv"] + max(BATCHES), m["d"], seed=43, dtype=np.float32)
        sv, pool = np.ascontiguousarray(X[:m["num_sv"]]), np.ascontiguousarray(X[m["num_sv"]:])
        alpha = np.random.default_rng(42).standard_normal((max(KS), m["num_sv"])).astype(np.float32)
        rho = 0.25 * (1 + np.arange(max(KS)))
        prm = Parameter(kernel_type=m["kernel"], degree=m["degree"], gamma=1.0 / m["d"], coef0=COEF0)
        for k in KS:
            with backend.Predictor(prm, sv, alpha[:k], rho[:k], **form) as pred:
                for n in BATCHES:
                    timed(f"{'block' if new else 'parent_resident'}_{part}_k{k}_n{n}", pred, pool[:n], per_launch if (new or k >= 2) else 1)
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--phases", default="launch,call")
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_block_f32.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    ap.add_argument("--part")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.part, args.reps)
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    phases = args.phases.split(",")
    parts = (["launch"] if "launch" in phases else []) + (list(MODELS) if "call" in phases else [])
    samples = {}
    for part in parts:
        for which in ("parent", "new"):
            env = dict(os.environ)
            if which == "parent":
                env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("PLSSVM_AMD_LIBRARY", None)
            try:
                proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--part", part, "--reps", str(args.reps)], env=env, capture_output=True, text=True,
                                      timeout=args.child_timeout)
            except subprocess.TimeoutExpired:
                print(f"{part}, {which}: child exceeded {args.child_timeout} s; stopping", file=sys.stderr)
                return 1
            line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if proc.returncode != 0 or line is None:
                print(f"{part}, {which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}", file=sys.stderr)
                return 1
            samples.update(json.loads(line[len("RESULT "):]))
            print(f"{part}, {which}: done", flush=True)
    res = {name: summary(v) for name, v in sorted(samples.items())}
    report = {"expected_block_over_one_single_128_features_f16x3": EXPECTED_BLOCK_OVER_SINGLE_128_F16X3}
    if "launch" in phases:
        launch = {}
        for name in LAUNCH_KERNELS:
            for d in FEATURES:
                for plane in PLANES:
                    tag = f"{name}_d{d}_{plane}"
                    blk, one, eight = (res[f"{n}_{tag}"]["kernel_ms"] for n in ("block_launch", "single_launch", "eight_pair_launches"))
                    launch[tag] = {"block_launch_ms": blk["median"], "parent_single_launch_ms": one["median"], "parent_eight_pair_launches_ms": eight["median"],
                                   "block_over_one_single": blk["median"] / one["median"], "block_over_eight_pairs": blk["median"] / eight["median"],
                                   "parent_single_spread": one["spread"], "parent_eight_pairs_spread": eight["spread"], "block_spread": blk["spread"]}
        report["launch_level"] = launch
        print(json.dumps({t: [round(v["block_over_one_single"], 3), round(v["block_over_eight_pairs"], 3), round(v["parent_eight_pairs_spread"], 3)] for t, v in launch.items()}))
    if "call" in phases:
        call = {}
        for part in MODELS:
            for k in KS:
                for n in BATCHES:
                    tag = f"{part}_k{k}_n{n}"
                    new, old = res[f"block_{tag}"], res[f"parent_resident_{tag}"]
                    call[tag] = {f"{w}_{key}": r[key]["median"] for w, r in (("block", new), ("parent_resident", old)) for key in KEYS}
                    call[tag].update({"block_over_parent_total": new["total_ms"]["median"] / old["total_ms"]["median"], "block_over_parent_kernel": new["kernel_ms"]["median"] / old["kernel_ms"]["median"],
                                      "parent_total_spread": old["total_ms"]["spread"], "parent_kernel_spread": old["kernel_ms"]["spread"]})
        report["call_level"] = call
        print(json.dumps({t: [round(v["block_over_parent_kernel"], 3), round(v["parent_kernel_spread"], 3)] for t, v in call.items()}))
    report["samples"] = res
    report["workload"] = (f"fp32; launch level: {LAUNCH_POINTS} points x {LAUNCH_SV} support vectors, {LAUNCH_K} vectors, {list(LAUNCH_KERNELS)} x {list(FEATURES)} features x {list(PLANES)}; call "
                          f"level: {list(MODELS)}, k in {list(KS)}, batches of {list(BATCHES)} points (make_blobs_pm1, gamma = 1 / d, coef0 = {COEF0})")
    report["method"] = (f"one child process per library and part, {args.reps} timed calls per shape after a warm-up of every shape: medians of {args.reps}; kernel_ms = HIP events around "
                        "the product launches, summed over a call's launches; total_ms = the call's host wall clock; spread = (max - min) / median; ratios below 1: the block form is faster")
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
