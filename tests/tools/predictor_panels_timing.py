#!/usr/bin/env python3
"""What the resident predictor beyond the one-pass kernels and the two-vector panel kernels save, against a library built from the PARENT commit.

usage: predictor_panels_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 5] [--rounds 2] [--phases launch,call] [--models a,b] [--out profiles/predictor_panels.json]

launch level   For EVERY instantiation of the two-vector panel kernels -- fp32 (plssvm_amd/csrc/tile_launch_f32xv2.hip): f16x3 and bf16x6 (gram_mode = 1) planes x polynomial
               of a run-time degree, degree 2, degree 3 and folded rbf, at 5 panels of 128 features (640) and at the panel count of 784 features (7); fp64
               (tile_launch_f64xv2.hip): rbf and the three polynomial forms at 5 panels of 64 features (320) and 13 (784) -- at 4 096 points x 30 000 support vectors:
               kernel_ms of ONE two-vector launch of this build (a panels predictor of two vectors) against kernel_ms of ONE single-vector launch of the parent's
               lssvm_mi355_predict_values_* at that width and with those options.
               Routing condition (the project's): the two-vector launch takes less than two single launches by more than the parent's own run-to-run spread
               (ratio + spread < 1, ratio = pair launch / (2 x parent launch), spread = (max - min) / median of the parent's launch).  The file lists every
               instantiation with `condition_met`; one that fails is to be named in panel_pair_routed (lssvm_problem.hip) and is then served by single-vector
               launches on the resident data.
call level     50 000 x 784 rbf fp32, 50 000 x 640 polynomial (degree 3) fp32 and 30 000 x 320 rbf fp64 with k = 1, 4, 10 weight vectors on batches of 1 000, 4 096 and
               200 000 points: total_ms (the call's host wall clock) and kernel_ms of lssvm_mi355_predictor_predict_multi on a handle of
               lssvm_mi355_predictor_create_panels (made once per child process, outside the timed calls) against the parent's lssvm_mi355_predict_values_multi_* and
               against the parent's lssvm_mi355_predictor_create_resident handle (which declines these widths and runs the one-shot call inside).
Child processes alternate between the two libraries (PLSSVM_AMD_LIBRARY; two copies of one library in one process would resolve each other's symbols), `--rounds`
children per library and part, each with a warm-up call of every shape and `--reps` timed calls per shape: medians of rounds x reps, and the spread.  Every child also
reports a SHA-256 of the values of every shape.  fp64 and fp32 rbf values of this build must be the parent's, bit for bit, or the run fails; fp32 polynomial values may
differ in their last bits (the planes' power-of-two scale comes from the support vectors alone in the resident form, from both sides in the one-shot call) and the file
says where they did.  A run of one phase alone keeps the other phase's sections of an existing --out file.  Every child runs under a time limit of its own; a child that fails ends the run: nothing more is started on the device.
"""

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LAUNCH_POINTS, LAUNCH_SV = 4_096, 30_000
LAUNCH_KERNELS = {"poly": ("polynomial", 5), "poly2": ("polynomial", 2), "poly3": ("polynomial", 3), "rbf": ("rbf", 3)}
PLANES = {"f16x3": ("float32", {}, 2, (640, 784)), "bf16x6": ("float32", {"gram_mode": 1}, 1, (640, 784)), "f64": ("float64", {}, 0, (320, 784))}  # dtype, options, gram_mode, widths
MODELS = {"50000x784_rbf_f32": dict(dtype="float32", num_sv=50_000, d=784, kernel="rbf", degree=3),
          "50000x640_poly3_f32": dict(dtype="float32", num_sv=50_000, d=640, kernel="polynomial", degree=3),
          "30000x320_rbf_f64": dict(dtype="float64", num_sv=30_000, d=320, kernel="rbf", degree=3)}
KS, BATCHES = (1, 4, 10), (1_000, 4_096, 200_000)
KEYS = ("kernel_ms", "total_ms")
COEF0 = 0.5


def instantiations():
    """(plane kind, kernel name, features) of the 12 two-vector panel kernels at two panel counts each"""
    return [(planes, name, d) for planes in PLANES for name in LAUNCH_KERNELS for d in PLANES[planes][3]]


def digest(a) -> str:
    import numpy as np

    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def child(which: str, part: str, reps: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd._capi import Options
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    new = which == "new"
    wanted = os.environ.get("PLSSVM_AMD_LIBRARY")
    assert new == (wanted is None) and (new or os.path.samefile(_capi.LIB_PATH, wanted)), (which, wanted, _capi.LIB_PATH)
    out, hashes, pair_launches = {}, {}, {}

    def record(name, infos):
        out.setdefault(name, []).append({key: sum(i[key] for i in infos) for key in KEYS})

    if part.startswith("launch_"):
        planes = part[len("launch_"):]
        dtype_name, opts, mode, widths = PLANES[planes]
        dtype = np.dtype(dtype_name).type
        X, _ = make_blobs_pm1(LAUNCH_SV + LAUNCH_POINTS, max(widths), seed=7, dtype=dtype)
        alpha = np.random.default_rng(3).standard_normal((2, LAUNCH_SV)).astype(dtype)
        rho = np.array([0.25, 0.5])
        for name in LAUNCH_KERNELS:
            for d in widths:
                kernel, degree = LAUNCH_KERNELS[name]
                sv, pts = np.ascontiguousarray(X[:LAUNCH_SV, :d]), np.ascontiguousarray(X[LAUNCH_SV:, :d])
                prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=COEF0)
                tag = f"{planes}_{name}_d{d}"
                if new:
                    with backend.Predictor(prm, sv, alpha, rho, options=Options(**opts), panels=True) as pred:
                        for keep in [False] + [True] * reps:
                            info = {}
                            values = pred.predict(pts, info_out=info)
                            assert info["resident"] == 1 and info["gram_mode"] == mode, (tag, info)
                            if keep:
                                record(f"pair_launch_{tag}", [info])
                        pair_launches[tag] = info["vectors_per_launch"] == 2  # (what was timed is a pair launch)
                    hashes[f"launch_{tag}_v0"], hashes[f"launch_{tag}_v1"] = digest(values[:, 0]), digest(values[:, 1])
                else:
                    for keep in [False] + [True] * reps:
                        info = {}
                        v0, _ = backend.predict_values(prm, sv, alpha[0], float(rho[0]), None, pts, options=Options(**opts), info_out=info)
                        assert info["gram_mode"] == mode, (tag, info)
                        if keep:
                            record(f"single_launch_{tag}", [info])
                    v1, _ = backend.predict_values(prm, sv, alpha[1], float(rho[1]), None, pts, options=Options(**opts))
                    hashes[f"launch_{tag}_v0"], hashes[f"launch_{tag}_v1"] = digest(v0), digest(v1)
    else:
        m = MODELS[part]
        dtype = np.dtype(m["dtype"]).type
        num_sv, d = m["num_sv"], m["d"]
        X, _ = make_blobs_pm1(num_sv + max(BATCHES), d, seed=43, dtype=dtype)
        sv, pool = np.ascontiguousarray(X[:num_sv]), np.ascontiguousarray(X[num_sv:])
        alpha = np.random.default_rng(42).standard_normal((max(KS), num_sv)).astype(dtype)
        rho = 0.25 * (1 + np.arange(max(KS)))
        prm = Parameter(kernel_type=m["kernel"], degree=m["degree"], gamma=1.0 / d, coef0=COEF0)
        preds = {k: (backend.Predictor(prm, sv, alpha[:k], rho[:k], panels=True) if new else backend.Predictor(prm, sv, alpha[:k], rho[:k], every_form=True)) for k in KS}
        for keep in [False] + [True] * reps:  # (a warm-up of every shape: code-object load, first allocations)
            for n in BATCHES:
                for k in KS:
                    tag = f"{part}_k{k}_n{n}"
                    info = {}
                    values = preds[k].predict(pool[:n], info_out=info)
                    assert info["resident"] == (1 if new else 0), info
                    if keep:
                        record(f"{'panels' if new else 'parent_every_form'}_{tag}", [info])
                    if not new:
                        info = {}
                        one, _ = backend.predict_values_multi(prm, sv, alpha[:k], rho[:k].astype(dtype), None, pool[:n], info_out=info)
                        assert np.array_equal(one, values), tag
                        if keep:
                            record(f"parent_one_shot_{tag}", [info])
                    hashes[f"call_{tag}"] = digest(values)
        for p in preds.values():
            p.close()
    print("RESULT " + json.dumps({"samples": out, "hashes": hashes, "pair_launches": pair_launches}), flush=True)


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
    ap.add_argument("--phases", default="launch,call")
    ap.add_argument("--models", default=",".join(MODELS), help="the call-level models to run")
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_panels.json"))
    ap.add_argument("--child", choices=["parent", "new"])
    ap.add_argument("--part")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.part, args.reps)
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    phases = args.phases.split(",")
    models = [m for m in args.models.split(",") if m] if "call" in phases else []
    parts = ([f"launch_{p}" for p in PLANES] if "launch" in phases else []) + models
    samples, hashes, pair_launches = {}, {"parent": {}, "new": {}}, {}
    for rnd in range(args.rounds):
        for part in parts:
            for which in ("parent", "new"):
                env = dict(os.environ)
                if which == "parent":
                    env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(args.parent_lib)
                else:
                    env.pop("PLSSVM_AMD_LIBRARY", None)
                try:
                    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--part", part, "--reps", str(args.reps)], env=env, capture_output=True,
                                          text=True, timeout=args.child_timeout)
                except subprocess.TimeoutExpired:
                    print(f"round {rnd}, {part}, {which}: child exceeded {args.child_timeout} s; stopping", file=sys.stderr)
                    return 1
                line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
                if proc.returncode != 0 or line is None:
                    print(f"round {rnd}, {part}, {which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}", file=sys.stderr)
                    return 1
                got = json.loads(line[len("RESULT "):])
                for name, vals in got["samples"].items():
                    samples.setdefault(name, []).extend(vals)
                pair_launches.update(got["pair_launches"])
                for name, h in got["hashes"].items():
                    if hashes[which].setdefault(name, h) != h:
                        print(f"round {rnd}, {part}, {which}: the values of {name} differ between two runs of one library", file=sys.stderr)
                        return 1
                print(f"round {rnd}, {part}, {which}: done", flush=True)
    if set(hashes["new"]) != set(hashes["parent"]):
        print("the two libraries did not compute the same shapes", file=sys.stderr)
        return 1
    differ = sorted(name for name, h in hashes["new"].items() if hashes["parent"][name] != h)
    must_equal = [n for n in differ if "rbf" in n or "f64" in n]
    if must_equal:
        print(f"the fp64 / rbf values of this build are not the parent's at: {must_equal}", file=sys.stderr)
        return 1
    res = {name: summary(v) for name, v in sorted(samples.items())}
    report = {"bits_equal_parent": {"shapes_compared": len(hashes["new"]), "fp64_and_rbf_all_equal": True, "fp32_polynomial_shapes_that_differ": differ}}
    if "launch" in phases:
        launch, not_routed = {}, []
        for planes, name, d in instantiations():
            tag = f"{planes}_{name}_d{d}"
            pair, one = res[f"pair_launch_{tag}"]["kernel_ms"], res[f"single_launch_{tag}"]["kernel_ms"]
            ratio = pair["median"] / (2 * one["median"])
            routed = ratio + one["spread"] < 1
            launch[tag] = {"pair_launch_ms": pair["median"], "parent_single_launch_ms": one["median"], "pair_over_two_singles": ratio, "parent_launch_spread": one["spread"],
                           "pair_launch_spread": pair["spread"], "condition_met": routed, "measured_with_pair_launch": bool(pair_launches[tag])}
            if not routed:
                not_routed.append(tag)
        report["launch_level"] = launch
        report["launch_level_condition_not_met"] = not_routed
        print(json.dumps({t: [round(v["pair_over_two_singles"], 3), round(v["parent_launch_spread"], 3)] for t, v in launch.items()}))
        print("condition not met:", not_routed)
    if models:
        call = {}
        for part in models:
            for k in KS:
                for n in BATCHES:
                    tag = f"{part}_k{k}_n{n}"
                    new = res[f"panels_{tag}"]
                    entry = {"panels_total_ms": new["total_ms"]["median"], "panels_total_min_ms": new["total_ms"]["min"], "panels_total_spread": new["total_ms"]["spread"],
                             "panels_kernel_ms": new["kernel_ms"]["median"]}
                    for base in ("parent_one_shot", "parent_every_form"):
                        b = res[f"{base}_{tag}"]
                        entry[f"{base}_total_ms"] = b["total_ms"]["median"]
                        entry[f"{base}_kernel_ms"] = b["kernel_ms"]["median"]
                        entry[f"{base}_total_spread"] = b["total_ms"]["spread"]
                        entry[f"factor_total_over_{base}"] = b["total_ms"]["median"] / new["total_ms"]["median"]
                        entry[f"factor_kernel_over_{base}"] = b["kernel_ms"]["median"] / new["kernel_ms"]["median"]
                    call[tag] = entry
        report["call_level"] = call
        print(json.dumps({t: [round(v["panels_total_ms"], 2), round(v["parent_one_shot_total_ms"], 2), round(v["factor_total_over_parent_one_shot"], 2)] for t, v in call.items()}))
    report["samples"] = res
    report["workload"] = (f"launch level: {LAUNCH_POINTS} points x {LAUNCH_SV} support vectors, {list(PLANES)} x {list(LAUNCH_KERNELS)} at the widths "
                          f"{ {p: v[3] for p, v in PLANES.items()} }; call level: {models}, k = {KS}, batches of {BATCHES} points (make_blobs_pm1, gamma = 1 / d, coef0 = {COEF0})")
    report["method"] = (f"{args.rounds} alternating child processes per library and part, {args.reps} timed calls per shape after a warm-up of every shape: medians of "
                        f"{args.rounds * args.reps}; kernel_ms = HIP events around the product launches, summed over a call's launches; total_ms = the call's host wall clock; "
                        "spread = (max - min) / median")
    if os.path.isfile(args.out) and set(phases) != {"launch", "call"}:  # a run of one phase keeps what an earlier run of the other phase wrote
        with open(args.out) as f:
            old = json.load(f)
        for key, value in old.items():
            if key in ("samples", "bits_equal_parent"):
                report[key] = {**value, **report[key]} if key == "samples" else {"earlier_run": value, **report[key]}
            elif key in ("workload", "method"):
                report[key] = value if value == report[key] else f"{value} || {report[key]}"
            else:
                report.setdefault(key, value)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
