#!/usr/bin/env python3
"""What the fixed-size logistic regression costs against the same IRLS driven from Python.  Reported, not asserted; no ratio is fixed in advance.

usage: reduced_logistic_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--rows a,b] [--ranks 64,256,1024] [--ks 1,4] [--reps 10] [--factor host]
                                  [--out profiles/reduced_logistic.json]

Per row (the shapes of profiles/reduced.json), rank and number of classes k, on a resident problem with the library's own landmarks:

  library     this build, ResidentProblem.fit_reduced_logistic(Y, rank, tol=1e-8)                      (lssvm_mi355_problem_fit_reduced_logistic)
  baseline    the PARENT commit's library, the same Newton iteration with the same number of passes per class driven from Python: per pass a resident predictor of the
              current coefficients evaluates eta for all N points (the data stays on the device; ONE download of k x N values), numpy forms v and z in the library's
              cancellation-free forms, and per class fit_reduced(Y = z, sample_weight = v) solves the step (TWO uploads of N-sized arrays per class; Phi is evaluated
              once by the predictor and once by the fit)                                                 (one child process per library: PLSSVM_AMD_LIBRARY)

Call time: medians of `reps` calls after a warm-up (3 at a million points), spread = (max - min) / median; library / baseline is reported with the baseline's spread
beside it.  `agreement`: the largest |eta_library - eta_baseline| over the training points relative to the largest |eta| (the baseline's eta and z pass through the
problem's data type, so a float32 row agrees to float32 roundings only).  Per pass of the library: step_ms against landmark_ms and gram_ms, and the step kernel's bytes
(rank x the slabs' rows x 8 per launch, one launch per slab and pass up to four classes) over its time as a fraction of the 6.3 TB/s a copy achieves on an MI355X.
A child that fails ends the run and nothing more is started on the device.  A run adds its cells to an existing --out file."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# name -> (N, d, kernel, dtype, cost)
ROWS = {
    "rbf50k_f32": (50_000, 128, "rbf", "float32", 100.0),
    "rbf50k_f64": (50_000, 128, "rbf", "float64", 100.0),
    "poly100k_f64": (100_000, 64, "polynomial", "float64", 10.0),
    "rbf1m_f32": (1_000_000, 128, "rbf", "float32", 100.0),
}
COPY_BYTES_PER_S = 6.3e12
DELTA = 2.0 ** -32
SLAB_ROWS = 65536


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def labels_of(y, k, np):
    """k label vectors: y itself, then copies of it with a tenth of the labels flipped (overlapping classes, as a one-vs-all call on noisy labels sees them)."""
    rng = np.random.default_rng(31)
    return np.stack([y] + [np.where(rng.random(y.size) < 0.1, -y, y) for _ in range(k - 1)]).astype(y.dtype)


def row_quantities(np, y, eta):
    s = y * eta
    e = np.exp(-np.abs(s))
    ope = 1.0 + e
    mu = np.maximum(e / (ope * ope), DELTA)
    g = y * np.where(s >= 0.0, e / ope, 1.0 / ope)
    return mu, eta + g / mu


def baseline_call(np, torch, backend, prob, params, X, X_dev, Y, lm, passes, factor):
    """The Newton iteration from Python on the weighted fit and a resident predictor; class c takes passes[c] evaluations, the last of them without a solve."""
    k, N = Y.shape
    m = len(lm)
    sv = np.ascontiguousarray(X[lm.astype(np.int64)])
    betas, rhos = np.zeros((k, m)), np.zeros(k)
    out_dev = torch.empty((N, k), dtype=X_dev.dtype, device=X_dev.device)
    eta = np.zeros((k, N))
    for t in range(max(passes)):
        active = [c for c in range(k) if t < passes[c]]
        if t == 0:
            eta[:] = 0.0
        else:
            with backend.Predictor(params, sv, betas.astype(X.dtype), rhos, every_form=True) as pred:
                pred.predict_device(X_dev.data_ptr(), N, out_dev.data_ptr())
            eta[:] = out_dev.cpu().numpy().astype(np.float64).T
        for c in active:
            if t + 1 >= passes[c]:
                continue  # (the pass that found the class converged: evaluated, not solved)
            v, z = row_quantities(np, Y[c].astype(np.float64), eta[c])
            betas[c], rhos[c], _, _ = prob.fit_reduced(z.astype(X.dtype), m, landmarks=lm, sample_weight=v, factor=factor)
    return betas, rhos, eta


def child(args):
    """One library (this process was started with or without PLSSVM_AMD_LIBRARY), one row, all ranks and k: a JSON line."""
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    N, d, kernel, dtype, cost = ROWS[args.child]
    X, y = make_blobs_pm1(N, d, seed=42, dtype=np.dtype(dtype))
    reps = args.reps if N < 1_000_000 else min(args.reps, 3)
    params = Parameter(kernel_type=kernel, cost=cost)
    plan = json.load(open(args.plan)) if args.plan else {}  # (a file: the coefficients of rank 1 024 do not fit a command line)
    result = {}
    if args.parent:
        import torch
        X_dev = torch.from_numpy(X).to("cuda:0")
    with backend.ResidentProblem(params, X) as prob:
        resolved = prob.params
        for rank in (int(r) for r in args.ranks.split(",")):
            for k in (int(v) for v in args.ks.split(",")):
                Y = labels_of(y, k, np)
                cell = f"{rank}/{k}"
                if not args.parent:
                    times, info, out = [], None, None
                    for rep in range(reps + 1):
                        t0 = time.perf_counter()
                        out = prob.fit_reduced_logistic(Y, rank, factor=args.factor)
                        if rep:
                            times.append((time.perf_counter() - t0) * 1e3)
                    infos = out[3]
                    slabs = (N + SLAB_ROWS - 1) // SLAB_ROWS
                    rows256 = (slabs - 1) * SLAB_ROWS + -(-(N - (slabs - 1) * SLAB_ROWS) // 256) * 256
                    most = max(infos, key=lambda i: i["passes"])  # (the class that took part in every pass: its device times are the call's)
                    step_bytes = most["passes"] * rank * rows256 * 8
                    result[cell] = {"call_ms": summary(times), "passes": [i["passes"] for i in infos], "halvings": [i["halvings"] for i in infos],
                                    "converged": [i["converged"] for i in infos], "landmark_ms": most["landmark_ms"], "step_ms": most["step_ms"], "gram_ms": most["gram_ms"],
                                    "host_ms": sum(i["host_ms"] for i in infos), "step_bytes": step_bytes,
                                    "step_fraction_of_copy": step_bytes / (most["step_ms"] * 1e-3) / COPY_BYTES_PER_S,
                                    "landmarks": [int(v) for v in out[2]], "betas": np.asarray(out[0]).tolist(), "rhos": np.asarray(out[1]).tolist()}
                else:
                    p = plan[cell]
                    lm, passes = np.array(p["landmarks"], dtype=np.uint64), p["passes"]
                    times, got = [], None
                    for rep in range(reps + 1):
                        t0 = time.perf_counter()
                        got = baseline_call(np, torch, backend, prob, resolved, X, X_dev, Y, lm, passes, args.factor)
                        if rep:
                            times.append((time.perf_counter() - t0) * 1e3)
                    # agreement on the training points: both sets of coefficients through ONE predictor form
                    etas = []
                    for b, r in ((np.array(p["betas"]).reshape(k, rank), np.array(p["rhos"]).reshape(k)), (got[0], got[1])):
                        with backend.Predictor(resolved, np.ascontiguousarray(X[lm.astype(np.int64)]), b.astype(X.dtype), r, every_form=True) as pred:
                            etas.append(np.asarray(pred.predict(X), dtype=np.float64))
                    result[cell] = {"call_ms": summary(times), "agreement": float(np.max(np.abs(etas[0] - etas[1])) / np.max(np.abs(etas[0])))}
    print(json.dumps(result))


def run_child(name, args, parent, plan=None):
    env = dict(os.environ)
    env.pop("PLSSVM_AMD_LIBRARY", None)
    if parent:
        env["PLSSVM_AMD_LIBRARY"] = args.parent_lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps), "--ranks", args.ranks, "--ks", args.ks, "--factor", args.factor]
    with tempfile.TemporaryDirectory() as tmp:
        if parent:
            with open(os.path.join(tmp, "plan.json"), "w") as f:
                json.dump(plan, f)
            cmd += ["--parent", "--plan", os.path.join(tmp, "plan.json")]
        done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if done.returncode != 0:
        print(done.stdout + done.stderr)
        sys.exit(f"{name}: the child of {'the parent library' if parent else 'this build'} failed ({done.returncode}); nothing more is started")
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--ranks", default="64,256,1024")
    ap.add_argument("--ks", default="1,4")
    ap.add_argument("--factor", default="host", choices=["host", "device"])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduced_logistic.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--plan", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        sys.exit("--parent-lib: the parent commit's libplssvm_amd.so is the yardstick; without it nothing is measured")
    out = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    out["method"] = ("fit_reduced_logistic on a resident problem at tol 1e-8, the library's landmarks, against the same Newton iteration with the same passes per class driven "
                     "from Python on the PARENT commit's library (fit_reduced with Y = z and sample_weight = v per class, a resident predictor for eta, the data kept on the "
                     "device); one child process per library and row; wall-clock medians after a warm-up, spread = (max - min) / median; step_fraction_of_copy = the step "
                     "kernel's bytes over its device time, over 6.3 TB/s")
    out.setdefault("rows", {})
    for name in args.rows.split(","):
        N, d, kernel, dtype, cost = ROWS[name]
        this = run_child(name, args, False)
        parent = run_child(name, args, True, {cell: {key: c[key] for key in ("landmarks", "passes", "betas", "rhos")} for cell, c in this.items()})
        row = out["rows"].setdefault(name, {"N": N, "d": d, "kernel": kernel, "dtype": dtype, "cost": cost, "cells": {}})
        for cell, c in this.items():
            b = parent[cell]
            r = {key: value for key, value in c.items() if key not in ("landmarks", "betas", "rhos")}
            r.update(factor=args.factor, baseline_call_ms=b["call_ms"], agreement=b["agreement"], call_over_baseline=c["call_ms"]["median"] / b["call_ms"]["median"],
                     baseline_spread=b["call_ms"]["spread"])
            r["verdict"] = "gain" if r["call_over_baseline"] < 1.0 - r["baseline_spread"] else ("loss" if r["call_over_baseline"] > 1.0 + r["baseline_spread"] else "tie")
            row["cells"][f"{cell}/{args.factor}"] = r
            print(f"{name} rank/k {cell} {args.factor}: passes {r['passes']}, call {c['call_ms']['median']:.2f} ms against {b['call_ms']['median']:.2f} ms = x{r['call_over_baseline']:.3f} "
                  f"(baseline spread {r['baseline_spread']:.3f}: {r['verdict']}), agreement {r['agreement']:.1e}; landmark / step / gram / host ms {r['landmark_ms']:.2f} / "
                  f"{r['step_ms']:.2f} / {r['gram_ms']:.2f} / {r['host_ms']:.2f}, step kernel at {100 * r['step_fraction_of_copy']:.1f} % of a copy", flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
