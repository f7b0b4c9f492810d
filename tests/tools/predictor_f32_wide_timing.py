#!/usr/bin/env python3
"""What the resident fp32 predictor beyond 128 features and its wide two-vector kernels save, against a library built from the PARENT commit.

usage: predictor_f32_wide_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--reps 5] [--rounds 2] [--phases launch,call] [--out profiles/predictor_f32_wide.json]

launch level   For EVERY instantiation of the wide two-vector kernels (plssvm_amd/csrc/tile_launch_f32v2w.hip) -- f16x3 planes: polynomial of a run-time degree, degree 2
               and degree 3 on 3 ... 8 chunks of 64 features, folded rbf on 3 ... 6; bf16x6 planes (gram_mode = 1): all four on 3 ... 6; 38 in all -- at 4 096 points x
               30 000 support vectors: kernel_ms of ONE two-vector launch of this build (a resident predictor of two vectors) against kernel_ms of ONE single-vector
               launch of the parent's lssvm_mi355_predict_values_f32 at that width and with those options.
               Routing condition (the project's): the two-vector launch takes less than two single launches by more than the parent's own run-to-run spread
               (ratio + spread < 1, ratio = pair launch / (2 x parent launch), spread = (max - min) / median of the parent's launch).  The file lists every
               instantiation with `condition_met`; one that fails is to be named in wide_pair_routed (lssvm_problem.hip) and is then served by single-vector
               launches on the resident data.
call level     50 000 x 256 rbf with k = 1, 4, 10 weight vectors on batches of 1 000, 4 096 and 200 000 points, and 50 000 x 512 polynomial (degree 3) with k = 4 on
               1 000 points: total_ms (the call's host wall clock) and kernel_ms of lssvm_mi355_predictor_predict_multi on a handle of
               lssvm_mi355_predictor_create_resident (made once per child process, outside the timed calls) against the parent's lssvm_mi355_predict_values_multi_f32
               and against k calls of its lssvm_mi355_predict_values_f32, summed.
Child processes alternate between the two libraries (PLSSVM_AMD_LIBRARY; two copies of one library in one process would resolve each other's symbols), `--rounds`
children per library and part, each with a warm-up call of every shape and `--reps` timed calls per shape: medians of rounds x reps, and the spread.  Every child also
reports a SHA-256 of the values of every shape.  rbf values of this build must be the parent's, bit for bit, or the run fails; polynomial values may differ in their last
bits (the planes' power-of-two scale comes from the support vectors alone in the resident form, from both sides in the one-shot call) and the file says where they did.
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
PLANES = {"f16x3": {}, "bf16x6": {"gram_mode": 1}}  # (plane kind: the options that select it on this data)
MODELS = {"50000x256_rbf": dict(num_sv=50_000, d=256, kernel="rbf", degree=3, ks=(1, 4, 10), batches=(1_000, 4_096, 200_000)),
          "50000x512_poly3": dict(num_sv=50_000, d=512, kernel="polynomial", degree=3, ks=(4,), batches=(1_000,))}
KEYS = ("kernel_ms", "total_ms")
COEF0 = 0.5


def instantiations():
    """(plane kind, kernel name, 64-feature chunks) of the 38 wide two-vector kernels"""
    return [(planes, name, n) for planes in PLANES for name in LAUNCH_KERNELS for n in range(3, (8 if planes == "f16x3" and name != "rbf" else 6) + 1)]


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

    if part == "launch":
        X, _ = make_blobs_pm1(LAUNCH_SV + LAUNCH_POINTS, 512, seed=7, dtype=np.float32)
        alpha = np.random.default_rng(3).standard_normal((2, LAUNCH_SV)).astype(np.float32)
        rho = np.array([0.25, 0.5])
        for planes, name, nk64 in instantiations():
            d = 64 * nk64
            kernel, degree = LAUNCH_KERNELS[name]
            sv, pts = np.ascontiguousarray(X[:LAUNCH_SV, :d]), np.ascontiguousarray(X[LAUNCH_SV:, :d])
            prm = Parameter(kernel_type=kernel, degree=degree, gamma=1.0 / d, coef0=COEF0)
            tag = f"{planes}_{name}_c{nk64}"
            mode = 2 if planes == "f16x3" else 1
            if new:
                with backend.Predictor(prm, sv, alpha, rho, options=Options(**PLANES[planes]), every_form=True) as pred:
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
                    v0, _ = backend.predict_values(prm, sv, alpha[0], float(rho[0]), None, pts, options=Options(**PLANES[planes]), info_out=info)
                    assert info["gram_mode"] == mode, (tag, info)
                    if keep:
                        record(f"single_launch_{tag}", [info])
                v1, _ = backend.predict_values(prm, sv, alpha[1], float(rho[1]), None, pts, options=Options(**PLANES[planes]))
                hashes[f"launch_{tag}_v0"], hashes[f"launch_{tag}_v1"] = digest(v0), digest(v1)
    else:
        m = MODELS[part]
        num_sv, d, ks, batches = m["num_sv"], m["d"], m["ks"], m["batches"]
        X, _ = make_blobs_pm1(num_sv + max(batches), d, seed=43, dtype=np.float32)
        sv, pool = np.ascontiguousarray(X[:num_sv]), np.ascontiguousarray(X[num_sv:])
        alpha = np.random.default_rng(42).standard_normal((max(ks), num_sv)).astype(np.float32)
        rho = 0.25 * (1 + np.arange(max(ks)))
        prm = Parameter(kernel_type=m["kernel"], degree=m["degree"], gamma=1.0 / d, coef0=COEF0)
        preds = {k: backend.Predictor(prm, sv, alpha[:k], rho[:k], every_form=True) for k in ks} if new else {}
        for keep in [False] + [True] * reps:  # (a warm-up of every shape: code-object load, first allocations)
            for n in batches:
                for k in ks:
                    tag = f"{part}_k{k}_n{n}"
                    if new:
                        info = {}
                        values = preds[k].predict(pool[:n], info_out=info)
                        assert info["resident"] == 1, info
                        if keep:
                            record(f"resident_{tag}", [info])
                    else:
                        info = {}
                        values, _ = backend.predict_values_multi(prm, sv, alpha[:k], rho[:k].astype(np.float32), None, pool[:n], info_out=info)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_f32_wide.json"))
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
    if set(hashes["new"]) != set(hashes["parent"]):
        print("the two libraries did not compute the same shapes", file=sys.stderr)
        return 1
    differ = sorted(name for name, h in hashes["new"].items() if hashes["parent"][name] != h)
    if any("rbf" in name for name in differ):
        print(f"the rbf values of this build are not the parent's at: {[n for n in differ if 'rbf' in n]}", file=sys.stderr)
        return 1
    res = {name: summary(v) for name, v in sorted(samples.items())}
    report = {"bits_equal_parent": {"shapes_compared": len(hashes["new"]), "rbf_all_equal": True, "polynomial_shapes_that_differ": differ}}
    if "launch" in phases:
        launch, not_routed = {}, []
        for planes, name, nk64 in instantiations():
            tag = f"{planes}_{name}_c{nk64}"
            pair, one = res[f"pair_launch_{tag}"]["kernel_ms"], res[f"single_launch_{tag}"]["kernel_ms"]
            ratio = pair["median"] / (2 * one["median"])
            routed = ratio + one["spread"] < 1
            launch[tag] = {"pair_launch_ms": pair["median"], "parent_single_launch_ms": one["median"], "pair_over_two_singles": ratio, "parent_launch_spread": one["spread"],
                           "pair_launch_spread": pair["spread"], "condition_met": routed, "measured_with_pair_launch": bool(pair_launches[tag])}
            if not routed:
                not_routed.append(tag)
        report["launch_level"] = launch
        report["launch_level_condition_not_met"] = not_routed
        print(json.dumps({t: round(v["pair_over_two_singles"], 3) for t, v in launch.items()}))
        print("condition not met:", not_routed)
    if "call" in phases:
        call = {}
        for part, m in MODELS.items():
            for k in m["ks"]:
                for n in m["batches"]:
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
    report["workload"] = (f"fp32; launch level: {LAUNCH_POINTS} points x {LAUNCH_SV} support vectors, the {len(instantiations())} instantiations {list(PLANES)} x {list(LAUNCH_KERNELS)} x "
                          f"3 ... 8 / 3 ... 6 chunks of 64 features; call level: {list(MODELS)} (make_blobs_pm1, gamma = 1 / d, coef0 = {COEF0})")
    report["method"] = (f"{args.rounds} alternating child processes per library and part, {args.reps} timed calls per shape after a warm-up of every shape: medians of "
                        f"{args.rounds * args.reps}; kernel_ms = HIP events around the product launches, summed over a call's launches; total_ms = the call's host wall clock; "
                        "parent_k_singles: the sum over k single-vector one-shot calls; spread = (max - min) / median")
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
