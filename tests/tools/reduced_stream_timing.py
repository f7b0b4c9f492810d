#!/usr/bin/env python3
"""What the fixed-size LS-SVM from a stream of chunks costs against the one-shot calls on data held at once.  Reported, not asserted; no ratio is
fixed in advance.  The baselines of (b) come from the PARENT commit's library, never from the build under test.

usage: reduced_stream_timing.py --parent-lib <libplssvm_amd.so of the parent commit> [--rows a,b] [--reps 10] [--skip-out-of-core] [--out profiles/reduced_stream.json]

One child process per library and row (PLSSVM_AMD_LIBRARY selects the library):

  (a) kernel   k_cross_product on 65 536 rows against k_landmark_product at the same shape (lssvm_mi355_reduced_stream_time_kernels: both in THIS build -- the parent has no
               entry that times its kernel alone, and the build's comparison of the generated code shows k_landmark_product instruction for instruction the parent's), 128
               features float32 and 64 features float64, rank 64 / 256 / 1 024, rbf.  ratio = cross / landmark, spread = the sibling's (max - min) / median.  A tie is the
               expectation.
  (b) call     wall clock: create a stream, update from host memory in chunks of 65 536 rows, solve at one cost -- against the parent's one-shot fit_reduced on the same
               rows, rank 64 / 256 / 1 024, both factors; and the two-pass walk with 8 costs (update, solve, loo per chunk) against the parent's fit_reduced_loo at rank 256.
               A cell is a GAIN or a LOSS only where |1 - ratio| exceeds the parent's spread.
  (c) out of core   8 000 000 x 128 float32 rows generated chunk by chunk and never held at once, rank 256: rows / s of the updates alone and with the generation.  No
               baseline: the parent cannot run it.

Medians of `reps` repeats after a warm-up (3 at a million points).  A child that fails ends the run and nothing more is started on the device.  A run adds its rows to an
existing --out file; what was not run is listed under `not_measured`."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# name -> (N, d, kernel, dtype): the four shapes of profiles/reduced.json
ROWS = {
    "rbf50k_f32": (50_000, 128, "rbf", "float32"),
    "rbf50k_f64": (50_000, 128, "rbf", "float64"),
    "poly100k_f64": (100_000, 64, "polynomial", "float64"),
    "rbf1m_f32": (1_000_000, 128, "rbf", "float32"),
}
KERNEL_SHAPES = {"f32_128": (128, "float32"), "f64_64": (64, "float64")}
RANKS = (64, 256, 1024)
FACTORS = ("host", "device")
CHUNK = 65_536
LOO_COSTS = (0.01, 0.1, 1.0, 10.0, 100.0, 1e3, 1e4, 1e5)
LOO_RANK = 256
OUT_OF_CORE = (8_000_000, 128, 256)


def summary(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med if med > 0 else 0.0, "n": len(v)}


def timed(reps, call):
    call()  # the warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return summary(out)


def parameter(kernel, d, cost=10.0):
    from plssvm_amd.parameter import Parameter
    return Parameter(kernel_type=kernel, cost=cost, gamma=1.0 / d, coef0=1.0, degree=3)


def chunks_of(X, y):
    return [(X[a:a + CHUNK], y[a:a + CHUNK].reshape(1, -1)) for a in range(0, X.shape[0], CHUNK)]


def child(args):
    """One library, one row: a JSON line."""
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1

    out = {}
    if args.child.startswith("kernel:"):
        d, dtype = KERNEL_SHAPES[args.child.split(":")[1]]
        X, _ = make_blobs_pm1(CHUNK + 1, d, seed=5, dtype=np.dtype(dtype))
        X = X[:CHUNK]
        for rank in RANKS:
            with backend.ReducedStream(parameter("rbf", d), X[:rank]) as stream:
                cross, landmark = stream.time_kernels(X, args.reps)
            out[str(rank)] = {"cross_ms": summary(cross.tolist()), "landmark_ms": summary(landmark.tolist())}
    elif args.child == "out_of_core":
        N, d, rank = OUT_OF_CORE
        base, yb = make_blobs_pm1(CHUNK + 1, d, seed=7, dtype=np.float32)
        base, yb = base[:CHUNK], yb[:CHUNK].reshape(1, -1)
        t0 = time.perf_counter()
        in_update = 0.0
        with backend.ReducedStream(parameter("rbf", d), base[:rank]) as stream:
            done = 0
            while done < N:
                n = min(CHUNK, N - done)
                X = base[:n] + np.float32(1e-3 * (done // CHUNK))  # a fresh chunk every time: the rows are never held at once
                t1 = time.perf_counter()
                stream.update(X, yb[:, :n])
                in_update += time.perf_counter() - t1
                done += n
            t1 = time.perf_counter()
            stream.solve([10.0])
            solve_s = time.perf_counter() - t1
            assert stream.num_points == N
        wall = time.perf_counter() - t0
        out = {"rows": N, "features": d, "rank": rank, "rows_per_s_updates": N / in_update, "rows_per_s_with_generation": N / wall, "solve_ms": solve_s * 1e3, "wall_s": wall}
    else:
        N, d, kernel, dtype = ROWS[args.child]
        reps = 3 if N >= 1_000_000 else args.reps
        X, y = make_blobs_pm1(N + 1, d, seed=5, dtype=np.dtype(dtype))
        X, y = X[:N], y[:N]
        prm = parameter(kernel, d)
        lms = np.sort(np.random.default_rng(3).choice(N, size=max(RANKS), replace=False)).astype(np.uint64)
        pieces = chunks_of(X, y)
        for rank in RANKS:
            at = lms[:rank]
            XL = np.ascontiguousarray(X[at.astype(np.int64)])
            for factor in FACTORS:
                cell = {}
                if args.role == "parent":
                    cell["fit_ms"] = timed(reps, lambda: backend.fit_reduced(prm, X, y, rank, landmarks=at, factor=factor))
                else:
                    def run():
                        with backend.ReducedStream(prm, XL) as stream:
                            for Xc, Yc in pieces:
                                stream.update(Xc, Yc)
                            stream.solve([10.0], factor=factor)
                    cell["fit_ms"] = timed(reps, run)
                out[f"{rank}/{factor}"] = cell
        at = lms[:LOO_RANK]
        XL = np.ascontiguousarray(X[at.astype(np.int64)])
        for factor in FACTORS:
            if args.role == "parent":
                cell = timed(reps, lambda: backend.fit_reduced_loo(prm, X, y, LOO_RANK, LOO_COSTS, landmarks=at, factor=factor))
            else:
                cell = timed(reps, lambda: backend.fit_reduced_stream(prm, XL, [(Xc, Yc, None) for Xc, Yc in pieces], LOO_COSTS, factor=factor, loo=True))
            out[f"loo8/{factor}"] = {"fit_ms": cell}
    print(json.dumps(out))


def run_child(lib, name, role, reps):
    env = dict(os.environ, PLSSVM_AMD_LIBRARY=lib)
    print(f"[{time.strftime('%H:%M:%S')}] {name} ({role})", file=sys.stderr, flush=True)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--role", role, "--reps", str(reps)], env=env, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        raise SystemExit(f"child {name} ({role}) failed with {res.returncode}: nothing more is started")
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-out-of-core", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduced_stream.json"))
    ap.add_argument("--child")
    ap.add_argument("--role", default="build")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        raise SystemExit("--parent-lib must name the parent commit's libplssvm_amd.so")
    own = os.path.join(ROOT, "plssvm_amd", "lib", "libplssvm_amd.so")
    result = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    result["method"] = ("one child process per library and row; medians of the repeats after a warm-up (3 at a million points); spread = (max - min) / median; (a) device time "
                        "between events, both kernels in this build; (b) wall clock of the whole call, the stream fed from host memory in chunks of 65 536 rows; a gain or a loss "
                        "counts only beyond the parent's spread")
    kernel = result.setdefault("kernel", {})
    for name in KERNEL_SHAPES:
        cells = run_child(own, f"kernel:{name}", "build", args.reps)
        for cell in cells.values():
            cell["ratio"] = cell["cross_ms"]["median"] / cell["landmark_ms"]["median"]
            cell["baseline_spread"] = cell["landmark_ms"]["spread"]
            cell["tie"] = abs(1.0 - cell["ratio"]) <= cell["baseline_spread"]
        kernel[name] = cells
    rows = result.setdefault("rows", {})
    for name in [r for r in args.rows.split(",") if r]:
        parent = run_child(args.parent_lib, name, "parent", args.reps)
        build = run_child(own, name, "build", args.reps)
        cells = {}
        for key in parent:
            p, b = parent[key]["fit_ms"], build[key]["fit_ms"]
            ratio = b["median"] / p["median"]
            cells[key] = {"parent_ms": p, "stream_ms": b, "ratio": ratio, "parent_spread": p["spread"],
                          "verdict": "gain" if 1.0 - ratio > p["spread"] else "loss" if ratio - 1.0 > p["spread"] else "within the spread"}
        rows[name] = cells
    if not args.skip_out_of_core:
        result["out_of_core"] = run_child(own, "out_of_core", "build", args.reps)
    result["not_measured"] = [r for r in ROWS if r not in rows] + ([] if "out_of_core" in result else ["out_of_core"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "method"}, indent=1, sort_keys=True)[:6000])


if __name__ == "__main__":
    main()
