#!/usr/bin/env python3
"""What the landmark selection costs and gives.  Reported, not asserted.

usage: landmark_select_timing.py [--reps 10] [--rows a,b] [--ranks 64,256,1024] [--parts select,pcg,reduced] [--parent-lib <libplssvm_amd.so of the parent commit>]
                                 [--budget-s S] [--out profiles/landmark_select.json]

(a) select   per row, rule and rank: select_ms (the whole call on a resident problem: allocation, 2 rank + 2 launches, one read-back; medians of `reps` after a warm-up)
             beside the step model's streamed bytes, sum over j of (n ldx sizeof(T) + 8 j n + 24 n) -- the candidates' rows of X_, j rows of F, and F[j], d read and
             written -- as achieved bytes per second and as the fraction of the 8 TB/s of HBM3E.
(b) pcg      select + build + solve against the fixed rule's build + solve on the same resident problem at the same eps (eps 1e-3 fp32, 1e-8 fp64; rank 256, make_blobs
             data): iterations and milliseconds of both sides.  The entry points that consume landmarks are those of the parent commit, so the fixed rule's side IS the
             parent's computation; with --parent-lib the parent's one-shot solve_pcg is timed as well, in a child process of its own (PLSSVM_AMD_LIBRARY).
(c) reduced  fit_reduced with selected against fixed landmarks: held-out accuracy on 20 000 fresh points, and the relative rms difference of the decision values there
             to the full model solved to eps 1e-8 (rows of at most 100 000 points; one more solve, not timed).
Rows where selection only adds its own time are printed like the others; on make_blobs data ties are expected.  A part that fails ends the run and nothing more is
started on the device.  A run adds its rows to an existing --out file."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_BYTES_PER_S = 8.0e12
HELD_OUT = 20_000
# name -> (N, d, kernel, degree, dtype, cost, pool)
ROWS = {
    "rbf50k_f32": (50_000, 128, "rbf", 3, "float32", 100.0, 0),
    "rbf50k_f64": (50_000, 128, "rbf", 3, "float64", 100.0, 0),
    "poly100k_f64": (100_000, 64, "polynomial", 3, "float64", 10.0, 0),
    "rbf1m_f32_pool64k": (1_000_000, 128, "rbf", 3, "float32", 100.0, 65_536),
    "rbf1m_f32": (1_000_000, 128, "rbf", 3, "float32", 100.0, 0),
}
EPS = {"float32": 1e-3, "float64": 1e-8}
RULES = ("greedy", "rpcholesky")


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def step_model_bytes(n, ldx, size, rank):
    return sum(n * ldx * size + 8 * j * n + 24 * n for j in range(rank))


def parent_child(args):
    """The parent library's one-shot solve_pcg with the fixed rule (this process was started with PLSSVM_AMD_LIBRARY set)."""
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    N, d, kernel, degree, dtype, cost, _ = ROWS[args.child]
    X, y = make_blobs_pm1(N, d, seed=42, dtype=np.dtype(dtype))
    prm = Parameter(kernel_type=kernel, degree=degree, cost=cost)
    ms, its = [], 0
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        _, _, info = backend.solve_pcg(prm, X, y, EPS[dtype], 2000, rank=256)
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
        its = info["iterations"]
    print(json.dumps({"parent_one_shot_ms": summary(ms), "iterations": its}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--ranks", default="64,256,1024")
    ap.add_argument("--parts", default="select,pcg,reduced")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--budget-s", type=float, default=1e9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmark_select.json"))
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return parent_child(args)
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    started = time.perf_counter()
    ranks = [int(r) for r in args.ranks.split(",")]
    parts = args.parts.split(",")
    out = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    out.setdefault("rows", {})

    def flush():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")

    for name in args.rows.split(","):
        N, d, kernel, degree, dtype, cost, pool = ROWS[name]
        if time.perf_counter() - started > args.budget_s:
            print(f"{name}: skipped, the budget of {args.budget_s:.0f} s is spent")
            continue
        X, y = make_blobs_pm1(N + HELD_OUT, d, seed=42, dtype=np.dtype(dtype))
        X, y, Xv, yv = X[:N], y[:N], X[N:], y[N:]
        prm = Parameter(kernel_type=kernel, degree=degree, cost=cost)
        size = np.dtype(dtype).itemsize
        n = pool if pool else N
        row = out["rows"].setdefault(name, {"N": N, "d": d, "kernel": kernel, "dtype": dtype, "cost": cost, "pool": pool})
        with backend.ResidentProblem(prm, X) as prob:
            ldx = -(-d // (32 if dtype == "float32" else 16)) * (32 if dtype == "float32" else 16)
            if "select" in parts:
                for rule in RULES:
                    for rank in ranks:
                        if time.perf_counter() - started > args.budget_s:
                            continue
                        reps = args.reps if N * rank <= 100_000 * 1024 else max(2, args.reps // 4)
                        ms, info = [], None
                        for rep in range(reps + 1):
                            info = prob.select_landmarks(rank, method=rule, pool=pool, seed=rep)[3]
                            if rep:
                                ms.append(info["select_ms"])
                        s = summary(ms)
                        nbytes = step_model_bytes(n, ldx, size, int(info["rank_found"]))
                        rate = nbytes / (s["median"] * 1e-3)
                        row.setdefault("select", {})[f"{rule}_rank{rank}"] = {
                            "select_ms": s, "rank_found": info["rank_found"], "trace0": info["trace0"], "trace": info["trace"], "device_bytes": info["device_bytes"],
                            "step_model_bytes": nbytes, "achieved_bytes_per_s": rate, "fraction_of_hbm": rate / HBM_BYTES_PER_S}
                        print(f"{name} select {rule} rank {rank}: {s['median']:.2f} ms (spread {s['spread']:.2f}), model {nbytes / 1e9:.2f} GB -> {rate / 1e12:.3f} TB/s "
                              f"= {rate / HBM_BYTES_PER_S:.3f} of HBM; trace {info['trace0']:.4g} -> {info['trace']:.4g}", flush=True)
                        flush()
            if "pcg" in parts and N <= 100_000 and time.perf_counter() - started <= args.budget_s:
                rank, eps = 256, EPS[dtype]
                for rule in (None,) + RULES:
                    ms, sel_ms, info = [], [], None
                    for rep in range(args.reps + 1):
                        t0 = time.perf_counter()
                        lm = None
                        if rule is not None:
                            lm, _, _, sinfo = prob.select_landmarks(rank, method=rule, pool=pool)
                        built = prob.build_preconditioner(rank, landmarks=lm)
                        _, _, info = prob.solve_pcg(y, eps, 2000)
                        if rep:
                            ms.append(1e3 * (time.perf_counter() - t0))
                            sel_ms.append(sinfo["select_ms"] if rule is not None else 0.0)
                    row.setdefault("pcg", {})[rule or "fixed"] = {"eps": eps, "rank": rank, "iterations": info["iterations"], "converged": info["converged"],
                                                                   "select_build_solve_ms": summary(ms), "select_ms": summary(sel_ms), "build_ms": built["build_ms"]}
                    print(f"{name} pcg {rule or 'fixed'}: {info['iterations']} iterations, select + build + solve {statistics.median(ms):.1f} ms (select {statistics.median(sel_ms):.1f})", flush=True)
                    flush()
            if "reduced" in parts and N <= 100_000 and time.perf_counter() - started <= args.budget_s:
                rank = 256
                kw = dict(gamma=prob.params.gamma, coef0=prob.params.coef0, degree=prob.params.degree)
                prob.cg_begin(y, 1e-8)
                prob.cg_step(5000)
                alpha, rho, full_info = prob.cg_finish()
                full = backend.predict_values(prm, X, alpha, float(rho), None, Xv)[0].astype(np.float64)
                for rule in (None,) + RULES:
                    betas, rho_r, used, rinfo = prob.fit_reduced(y, rank, landmarks=rule)
                    f = backend.predict_values(prm, X[used.astype(np.int64)], betas.astype(X.dtype), float(rho_r), None, Xv)[0].astype(np.float64)
                    row.setdefault("reduced", {})[rule or "fixed"] = {
                        "rank": int(rinfo["rank"]), "held_out_accuracy": float(np.mean(np.sign(f) == yv)), "full_model_accuracy": float(np.mean(np.sign(full) == yv)),
                        "relative_rms_to_full": float(np.sqrt(np.mean((f - full) ** 2) / np.mean(full ** 2))), "full_model_iterations": full_info["iterations"], "kernel": kw}
                    print(f"{name} reduced {rule or 'fixed'}: held-out accuracy {row['reduced'][rule or 'fixed']['held_out_accuracy']:.4f} (full {row['reduced'][rule or 'fixed']['full_model_accuracy']:.4f}), "
                          f"relative rms to the full model {row['reduced'][rule or 'fixed']['relative_rms_to_full']:.3e}", flush=True)
                    flush()
        if args.parent_lib and "pcg" in parts and N <= 100_000:
            env = dict(os.environ, PLSSVM_AMD_LIBRARY=args.parent_lib)
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=900)
            if done.returncode != 0:
                print(done.stdout + done.stderr)
                sys.exit(f"{name}: the parent library's child failed ({done.returncode}); nothing more is started")
            row["pcg"]["parent_one_shot"] = json.loads(done.stdout.strip().splitlines()[-1])
            print(f"{name} parent one-shot solve_pcg: {row['pcg']['parent_one_shot']}", flush=True)
            flush()
    flush()


if __name__ == "__main__":
    main()
