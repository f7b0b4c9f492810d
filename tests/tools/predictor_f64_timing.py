#!/usr/bin/env python3
"""What the resident fp64 predictor and its two-vector full-square kernel save, against a library built from the PARENT commit.

usage: predictor_f64_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 5] [--rounds 2] [--phases launch,call] [--out profiles/predictor_f64.json]

launch level   For EVERY (kernel function, chunk count) instantiation of tile_matvec_f64_v2<KT, NKC, false, 2> -- polynomial of a run-time degree, degree 2, degree 3
               and rbf on 1 ... 8, 10, 12, 14, 16 chunks of 16 features -- at 4 096 points x 30 000 support vectors: kernel_ms of ONE two-vector launch of this build
               (a resident predictor of two vectors) against kernel_ms of ONE single-vector launch of the parent's lssvm_mi355_predict_values_f64.
               Routing condition: the two-vector launch takes less than two single launches by more than the parent's own run-to-run spread
               (ratio + spread < 1, ratio = pair launch / (2 x parent launch), spread = (max - min) / median of the parent's launch).  The file lists every
               instantiation with `condition_met` (all 48 meet it; one that failed would have to be served with single-vector launches on the resident data).
call level     50 000 x 128 rbf and 100 000 x 64 polynomial (degree 3), k = 1, 4, 10 weight vectors, batches of 1 000, 4 096 and 200 000 points: total_ms (the call's host
               wall clock) and kernel_ms of lssvm_mi355_predictor_predict_multi on a handle of lssvm_mi355_predictor_create_resident (made once per child process,
               outside the timed calls) against the parent's lssvm_mi355_predict_values_multi_f64 and against k calls of its lssvm_mi355_predict_values_f64, summed.
Child processes alternate between the two libraries (PLSSVM_AMD_LIBRARY; two copies of one library in one process would resolve each other's symbols), `--rounds`
children per library and part, each with a warm-up call of every shape and `--reps` timed calls per shape: medians of rounds x reps, and the spread.  Every child also
reports a SHA-256 of the values of every shape; the values of this build must be those of the parent, bit for bit, or the run fails.
Every child runs under a time limit of its own; a child that fails ends the run: nothing more is started on the device.
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
CHUNKS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16)  # of 16 features
MODELS = {"50000x128_rbf": dict(num_sv=50_000, d=128, kernel="rbf", degree=3), "100000x64_poly3": dict(num_sv=100_000, d=64, kernel="polynomial", degree=3)}
KS = (1, 4, 10)
BATCHES = (1_000, 4_096, 200_000)
KEYS = ("kernel_ms", "total_ms")
COEF0 = 0.5


def digest(a) -> str:
    import numpy as np

    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def child(which: str, part: str, reps: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import _capi, backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    new = which == "new"
    assert new == hasattr(_capi.lib, "lssvm_mi355_predictor_create_resident"), "the parent's library must not have the new entry point, this build's must"
    out, hashes, pair_launches = {}, {}, {}

    def record(name, infos):
        out.setdefault(name, []).append({key: sum(i[key] for i in infos) for key in KEYS})

    if part == "launch":
        X, _ = make_blobs_pm1(LAUNCH_SV + LAUNCH_POINTS, 16 * max(CHUNKS), seed=7, dtype=np.float64)
        alpha = np.random.default_rng(3).standard_normal((2, LAUNCH_SV))
        rho = np.array([0.25, 0.5])
        for nkc in CHUNKS:
            d = 16 * nkc
            sv, pts = np.ascontiguousarray(X[:LAUNCH_SV, :d]), np.ascontiguousarray(X[LAUNCH_SV:, :d])
            for name, (kernel, degree) in LAUNCH_KERNELS.items():
                prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=COEF0)
                tag = f"{name}_c{nkc}"
                if new:
                    with backend.Predictor(prm, sv, alpha, rho, every_form=True) as pred:
                        for keep in [False] + [True] * reps:
                            info = {}
                            values = pred.predict(pts, info_out=info)
                            assert info["resident"] == 1, info
                            if keep:
                                record(f"pair_launch_{tag}", [info])
                        pair_launches[tag] = info["vectors_per_launch"] == 2  # (what was timed is a pair launch)
                    hashes[f"launch_{tag}_v0"], hashes[f"launch_{tag}_v1"] = digest(values[:, 0]), digest(values[:, 1])
                else:
                    for keep in [False] + [True] * reps:
                        info = {}
                        v0, _ = backend.predict_values(prm, sv, alpha[0], float(rho[0]), None, pts, info_out=info)
                        if keep:
                            record(f"single_launch_{tag}", [info])
                    v1, _ = backend.predict_values(prm, sv, alpha[1], float(rho[1]), None, pts)
                    hashes[f"launch_{tag}_v0"], hashes[f"launch_{tag}_v1"] = digest(v0), digest(v1)
    else:
        m = MODELS[part]
        num_sv, d = m["num_sv"], m["d"]
        X, _ = make_blobs_pm1(num_sv + max(BATCHES), d, seed=43, dtype=np.float64)
        sv, pool = np.ascontiguousarray(X[:num_sv]), np.ascontiguousarray(X[num_sv:])
        alpha = np.random.default_rng(42).standard_normal((max(KS), num_sv))
        rho = 0.25 * (1 + np.arange(max(KS)))
        prm = Parameter(kernel_type=m["kernel"], degree=m["degree"], gamma=1.0 / d, coef0=COEF0)
        preds = {k: backend.Predictor(prm, sv, alpha[:k], rho[:k], every_form=True) for k in KS} if new else {}
        for keep in [False] + [True] * reps:  # (a warm-up of every shape: code-object load, first allocations)
            for n in BATCHES:
                for k in KS:
                    tag = f"{part}_k{k}_n{n}"
                    if new:
                        info = {}
                        values = preds[k].predict(pool[:n], info_out=info)
                        assert info["resident"] == 1, info
                        if keep:
                            record(f"resident_{tag}", [info])
                    else:
                        info = {}
                        values, _ = backend.predict_values_multi(prm, sv, alpha[:k], rho[:k], None, pool[:n], info_out=info)
                        infos = []
                        for v in range(k):
                            infos.append({})
                            single, _ = backend.predict_values(prm, sv, alpha[v], float(rho[v]), None, pool[:n], info_out=infos[-1])
                            assert np.array_equal(single, values[:, v]), (tag, v)
                        if keep:
                            record(f"parent_one_shot_{tag}", [info])
                            record(f"parent_k_singles_{tag}", infos)
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
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_f64.json"))
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
    differ = sorted(name for name, h in hashes["new"].items() if hashes["parent"].get(name) != h)
    if differ or set(hashes["new"]) != set(hashes["parent"]):
        print(f"the values of this build are not the parent's at: {differ}", file=sys.stderr)
        return 1
    res = {name: summary(v) for name, v in sorted(samples.items())}
    report = {"bits_equal_parent": {"shapes_compared": len(hashes["new"]), "all_equal": True}}
    if "launch" in phases:
        launch, not_routed = {}, []
        for name in LAUNCH_KERNELS:
            for nkc in CHUNKS:
                tag = f"{name}_c{nkc}"
                pair, one = res[f"pair_launch_{tag}"]["kernel_ms"], res[f"single_launch_{tag}"]["kernel_ms"]
                ratio = pair["median"] / (2 * one["median"])
                ran_pair = bool(pair_launches[tag])
                routed = ratio + one["spread"] < 1
                launch[tag] = {"pair_launch_ms": pair["median"], "parent_single_launch_ms": one["median"], "pair_over_two_singles": ratio, "parent_launch_spread": one["spread"],
                               "pair_launch_spread": pair["spread"], "condition_met": routed, "measured_with_pair_launch": ran_pair}
                if not routed:
                    not_routed.append(tag)
        report["launch_level"] = launch
        report["launch_level_condition_not_met"] = not_routed
        print(json.dumps({t: round(v["pair_over_two_singles"], 3) for t, v in launch.items()}))
        print("condition not met:", not_routed)
    if "call" in phases:
        call = {}
        for part in MODELS:
            for k in KS:
                for n in BATCHES:
                    tag = f"{part}_k{k}_n{n}"
                    new = res[f"resident_{tag}"]
                    entry = {"resident_total_ms": new["total_ms"]["median"], "resident_kernel_ms": new["kernel_ms"]["median"]}
                    for base in ("parent_one_shot", "parent_k_singles"):
                        b = res[f"{base}_{tag}"]
                        entry[f"{base}_total_ms"] = b["total_ms"]["median"]
                        entry[f"{base}_kernel_ms"] = b["kernel_ms"]["median"]
                        entry[f"{base}_total_spread"] = b["total_ms"]["spread"]
                        entry[f"factor_total_over_{base}"] = b["total_ms"]["median"] / new["total_ms"]["median"]
                        entry[f"factor_kernel_over_{base}"] = b["kernel_ms"]["median"] / new["kernel_ms"]["median"]
                    call[tag] = entry
        report["call_level"] = call
        print(json.dumps({t: round(v["factor_total_over_parent_one_shot"], 2) for t, v in call.items()}))
    report["samples"] = res
    report["workload"] = (f"fp64; launch level: {LAUNCH_POINTS} points x {LAUNCH_SV} support vectors, {list(LAUNCH_KERNELS)} x {list(CHUNKS)} chunks of 16 features; call level: "
                          f"{list(MODELS)}, k in {list(KS)}, batches of {list(BATCHES)} points (make_blobs_pm1, gamma = 1 / d, coef0 = {COEF0})")
    report["method"] = (f"{args.rounds} alternating child processes per library and part, {args.reps} timed calls per shape after a warm-up of every shape: medians of "
                        f"{args.rounds * args.reps}; kernel_ms = HIP events around the product launches, summed over a call's launches; total_ms = the call's host wall clock; "
                        "parent_k_singles: the sum over k single-vector one-shot calls; spread = (max - min) / median")
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
