#!/usr/bin/env python3
"""The predict paths of this build against a library built from the PARENT commit: the same bits (default) and the same time (--timing).

usage: predict_bits_ab.py --parent-lib <libplssvm_amd.so of the parent commit> [--out profiles/predict_stage_bits.json]
       predict_bits_ab.py --parent-lib <...> --timing [--rounds 4] [--reps 7] [--new-lib <...>] [--out profiles/predict_stage_bits.json]

Written for a change that moves host code of the predict paths (the one-shot call and both resident predictors on one product stage) without touching arithmetic or
the order of the stream: every value of every entry point must be bit-equal, so the condition is equality of SHA-256 digests with no tolerance, and the time of a call
must be the parent's within the parent's own spread.

Bits.  A case is one call of one entry point; its record is the SHA-256 digest of the returned values and of the two reals of `lssvm_predict_info` that belong to the
path (rbf_exponent_scale, f16_row_rel_error), followed by its four integers: g = gram_mode, d = rbf_direct, r = resident, v = vectors_per_launch.  All of it must be
equal (--out lists both digests of every case, and the integers once where they agree).  300 support vectors (three column tiles) unless said otherwise, batches of 300
and 8 000 points (8 000 pads to 64 row blocks: the 256-row kernel) through predict_values / predict_values_multi and a handle of predictor_create / _create_multi /
_create_resident, the 300-point batch in host memory and in HBM.  rbf and polynomial degree 3 with 1, 2 and 3 weight vectors and, at the first width, j_chunk_tiles 0
and 1 (three column chunks); the other kernels with 1 and 3 vectors:
  fp32  linear, rbf, polynomial degree 2, 3, 5 and -2 on 48 and 128 features; rbf and polynomial degree 3 on 192 features (one pass, resident only through
        _create_resident); rbf on 600 features (feature panels, one-shot); gram_mode 0 and 1; rbf_form 1, 2 and 3; rbf_form 2 at exponent scales 48 / 128 / 400 (pair,
        folded and unfolded records); 1 200 support vectors in ten chunks at 8 000 points (320 work items: a persistent launch, whose counters alternate between the
        launches of a call), once more under LSSVM_MI355_PREDICT_REPEAT=4; a resident handle that serves a batch, declines a far one, serves again, and one that declines
        a batch on the f16 check after a resident call
  fp64  linear, rbf, polynomial degree 3 and -2 on 40 and 136 features (resident through _create_resident), rbf on 300 features (feature panels, one-shot)
Timing (--timing).  Host wall clock of the whole call and `kernel_ms`, medians over rounds x reps samples per library and the parent's spread (max - min) / median, each
resident call with the one-shot call beside it, against 30 000 support vectors:
  fp32 rbf 128 features, fp64 rbf 64 features: 100 points (the host's share dominates) and 4 096 points; fp32 polynomial degree 3 on 192 features with three weight
  vectors (_create_resident): 4 096 points
Condition per shape and clock: median(new) <= median(parent) * (1 + spread(parent)).  `total_ms` and `setup_ms` of the same calls are listed beside them without a condition:
they say where a difference in the wall clock lies.  --new-lib with the parent's library once more compares the parent with itself: the noise of the comparison.
Child processes alternate between the two libraries (PLSSVM_AMD_LIBRARY); in --timing the first of a round is the parent's and this build's in turn.  Every child runs
under a time limit of its own; a child that fails ends the run: nothing more is started on the device.  The tool exits non-zero on any difference / any shape over its bound, after it has written --out.
"""

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LOG2E = 1.4426950408889634
INFO_FIELDS = ("gram_mode", "rbf_direct", "resident", "vectors_per_launch")
# kernel name -> (kernel_type, degree)
KERNELS32 = {"linear": ("linear", 3), "rbf": ("rbf", 3), "poly2": ("polynomial", 2), "poly3": ("polynomial", 3), "poly5": ("polynomial", 5), "poly-2": ("polynomial", -2)}
KERNELS64 = {"linear": ("linear", 3), "rbf": ("rbf", 3), "poly3": ("polynomial", 3), "poly-2": ("polynomial", -2)}
BATCHES = (300, 8000)
NVECS = (1, 2, 3)


def record(values, info) -> str:
    import numpy as np

    a = np.ascontiguousarray(values)
    reals = np.array([info["rbf_exponent_scale"], info["f16_row_rel_error"]], dtype=np.float64)  # (hashed with the values; the four integers stay readable)
    h = hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes() + reals.tobytes()).hexdigest()
    return h + " " + " ".join(f"{short}{info[k]}" for short, k in zip("gdrv", INFO_FIELDS))


def bits_child() -> None:
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from plssvm_amd import backend
    from plssvm_amd._capi import Options
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    out = {}

    def model(kernel, nsv, npts, d, dt, seed):
        """support vectors, points, three weight vectors and their rho; a negative degree needs data away from zero (tests/test_gpu_predict_edges.py)"""
        rng = np.random.default_rng(seed)
        name, degree = kernel
        if degree < 0:
            X = rng.uniform(0.5, 1.5, size=(nsv + npts, d)).astype(dt)
        else:
            X, _ = make_blobs_pm1(nsv + npts, d, seed=seed, dtype=dt)
        alphas = rng.standard_normal((3, nsv)).astype(dt)
        prm = Parameter(kernel_type=name, degree=degree, gamma=1.0 / d, coef0=(0.5 if name == "polynomial" and degree > 0 else 0.0))
        return prm, X[:nsv], X[nsv:], alphas, np.array([0.25, -0.5, 0.0])

    def one_shot(key, prm, sv, alphas, rhos, k, pts, options=None):
        info = {}
        if k == 1:
            vals, _ = backend.predict_values(prm, sv, alphas[0], float(rhos[0]), None, pts, options=options, info_out=info)
            out[f"{key}: predict_values"] = record(vals, info)
        else:
            vals, _ = backend.predict_values_multi(prm, sv, alphas[:k], rhos[:k], None, pts, options=options, info_out=info)
            out[f"{key}: predict_values_multi"] = record(vals, info)

    def predictor(prm, sv, alphas, rhos, k, options, every_form):
        if k == 1:
            return backend.Predictor(prm, sv, alphas[0], float(rhos[0]), options=options, every_form=every_form)
        return backend.Predictor(prm, sv, alphas[:k], rhos[:k], options=options, every_form=every_form)

    def handle_calls(key, pred, pts, k, hbm):
        info = {}
        out[f"{key}, host batch"] = record(pred.predict(pts, info_out=info), info)
        if hbm:
            Pd = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
            Od = torch.full((pts.shape[0],) if k == 1 else (pts.shape[0], k), float("nan"), dtype=Pd.dtype, device="cuda")
            torch.cuda.synchronize()
            info = {}
            pred.predict_device(Pd.data_ptr(), pts.shape[0], Od.data_ptr(), info_out=info)
            out[f"{key}, HBM batch"] = record(Od.cpu().numpy(), info)

    def every_entry(key, prm, sv, alphas, rhos, k, pts, options=None, resident_forms=(False, True)):
        """the one-shot call and a handle of each form; the HBM batch beside the host batch at the small batch size (the same path, another copy kind)"""
        one_shot(key, prm, sv, alphas, rhos, k, pts, options)
        for every_form in resident_forms:
            create = "predictor_create_resident" if every_form else ("predictor_create" if k == 1 else "predictor_create_multi")
            with predictor(prm, sv, alphas, rhos, k, options, every_form) as pred:
                handle_calls(f"{key}: {create}", pred, pts, k, hbm=pts.shape[0] <= 300)

    def sweep(tag, dt, kernels, widths, resident_forms, nsv=300):
        """rbf and polynomial degree 3: 1, 2 and 3 weight vectors, and three column chunks at the first width; the other kernels: 1 and 3 vectors"""
        for kname, kernel in kernels.items():
            full = kname in ("rbf", "poly3")
            for d in widths:
                for npts in BATCHES:
                    prm, sv, pts, alphas, rhos = model(kernel, nsv, npts, d, dt, seed=1000 * d + npts)
                    for jc in ((0, 1) if full and d == widths[0] else (0,)):
                        opts = Options(j_chunk_tiles=jc) if jc else None
                        for k in (NVECS if full else (1, 3)):
                            every_entry(f"{tag} {kname} {d} features, {nsv} x {npts}, nvec {k}, j_chunk_tiles {jc}", prm, sv, alphas, rhos.astype(dt), k, pts, opts, resident_forms)

    f32, f64 = np.float32, np.float64
    sweep("fp32", f32, KERNELS32, (48, 128), (False,))
    sweep("fp32", f32, {"rbf": KERNELS32["rbf"], "poly3": KERNELS32["poly3"]}, (192,), (False, True))
    sweep("fp64", f64, KERNELS64, (40, 136), (True,))
    # feature panels: one-shot, also inside a handle made by _create_resident
    for tag, dt, d in (("fp32", f32, 600), ("fp64", f64, 300)):
        prm, sv, pts, alphas, rhos = model(KERNELS32["rbf"], 300, 300, d, dt, seed=d)
        for k in (1, 2):
            every_entry(f"{tag} rbf {d} features (feature panels), 300 x 300, nvec {k}", prm, sv, alphas, rhos.astype(dt), k, pts, resident_forms=(True,))
    # fp32 options
    for kname in ("rbf", "poly3"):
        prm, sv, pts, alphas, rhos = model(KERNELS32[kname], 300, 8000, 48, f32, seed=5)
        for gm in (0, 1):
            for k in (1, 2):
                every_entry(f"fp32 {kname} 48 features, 300 x 8000, nvec {k}, gram_mode {gm}", prm, sv, alphas, rhos.astype(f32), k, pts, Options(gram_mode=gm), resident_forms=(False,))
    for npts in BATCHES:
        prm, sv, pts, alphas, rhos = model(KERNELS32["rbf"], 300, npts, 64, f32, seed=64 + npts)
        for form in (1, 2, 3):
            for k in (1, 2):
                every_entry(f"fp32 rbf 64 features, 300 x {npts}, nvec {k}, rbf_form {form}", prm, sv, alphas, rhos.astype(f32), k, pts, Options(rbf_form=form), resident_forms=(False,))
        # (tests/test_gpu_predict_edges.py: gamma that puts the exponent scale 2 gamma log2(e) max |x - mean|^2 of both sides at r2)
        mean = (sv.astype(f64).sum(axis=0) / sv.shape[0]).astype(f32).astype(f64)
        sq = max(float(np.max(np.sum((M.astype(f64) - mean) ** 2, axis=1))) for M in (sv, pts))
        for r2 in (48.0, 128.0, 400.0):
            prm2 = Parameter(kernel_type="rbf", gamma=float(np.float32(r2 / (2.0 * LOG2E * sq))))
            for k in NVECS:
                every_entry(f"fp32 rbf 64 features, 300 x {npts}, nvec {k}, rbf_form 2 at exponent scale {r2:.0f}", prm2, sv, alphas, rhos.astype(f32), k, pts, Options(rbf_form=2),
                            resident_forms=(False,))
    # a persistent launch: 32 row pairs x 10 column chunks = 320 work items, more than the device has CUs
    for kname in ("rbf", "poly3"):
        prm, sv, pts, alphas, rhos = model(KERNELS32[kname], 1200, 8000, 48, f32, seed=12)
        for k in NVECS:
            every_entry(f"fp32 {kname} 48 features, 1200 x 8000, nvec {k}, j_chunk_tiles 1 (persistent launch)", prm, sv, alphas, rhos.astype(f32), k, pts, Options(j_chunk_tiles=1),
                        resident_forms=(False,))
        os.environ["LSSVM_MI355_PREDICT_REPEAT"] = "4"
        try:
            one_shot(f"fp32 {kname} 48 features, 1200 x 8000, nvec 1, j_chunk_tiles 1, LSSVM_MI355_PREDICT_REPEAT=4", prm, sv, alphas, rhos.astype(f32), 1, pts, Options(j_chunk_tiles=1))
        finally:
            del os.environ["LSSVM_MI355_PREDICT_REPEAT"]
    # declines of a resident fp32 handle, after a resident call on the same handle
    prm, sv, pts, alphas, rhos = model(KERNELS32["rbf"], 300, 300, 48, f32, seed=77)
    far = (pts * 12.0).astype(f32)  # (beyond the norm expansion's range around the support vectors' centre)
    for k in (1, 3):
        with predictor(prm, sv, alphas, rhos, k, None, False) as pred:
            for step, batch in enumerate((pts, far, pts[:77])):
                handle_calls(f"fp32 rbf 48 features, nvec {k}, one handle, call {step} ({'far batch' if batch is far else 'near batch'})", pred, batch, k, hbm=(step == 1))

    def shell(rng, n, d, norm):
        u = rng.standard_normal((n, d))
        return (u / np.linalg.norm(u, axis=1, keepdims=True) * norm).astype(f32)

    # (tests/test_gpu_predict_edges.py, _cross_term_data(reverse=True): the support vectors alone pass the f16 check, together with this batch they do not)
    rng = np.random.default_rng(32)
    large = shell(rng, 150, 64, 4.0)
    sv, batch = np.concatenate([large, -large]), np.concatenate([shell(rng, 150, 64, 0.5), shell(rng, 2, 64, 2.0 ** -10)])
    prm = Parameter(kernel_type="rbf", gamma=float(np.float32(0.5 / LOG2E)))
    alphas = rng.standard_normal((3, sv.shape[0])).astype(f32)
    calm = shell(np.random.default_rng(3), 100, 64, 0.5)
    for k in (1, 2):
        with predictor(prm, sv, alphas, rhos, k, None, False) as pred:
            for step, (what, b) in enumerate((("batch that passes", calm), ("batch that fails the f16 check", batch), ("batch that passes", calm[:50]))):
                handle_calls(f"fp32 rbf 64 features, nvec {k}, f16 check over both sides, call {step} ({what})", pred, b, k, hbm=(step == 1))
    print("RESULT " + json.dumps(out), flush=True)


def timing_child(reps: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np

    from plssvm_amd import backend
    from plssvm_amd.datagen import make_blobs_pm1
    from plssvm_amd.parameter import Parameter

    out = {}

    def timed(name, call):
        for keep in [False, False] + [True] * reps:
            info = {}
            t0 = time.perf_counter()
            call(info)
            wall = 1e3 * (time.perf_counter() - t0)
            if keep:
                out.setdefault(name + " wall_ms", []).append(wall)
                for clock in ("kernel_ms", "total_ms", "setup_ms"):
                    out.setdefault(f"{name} {clock}", []).append(info[clock])

    def shape(tag, prm, dt, d, sizes, k=1, every_form=False):
        X, _ = make_blobs_pm1(30_000 + max(sizes), d, seed=42, dtype=dt)
        sv, pts = X[:30_000], X[30_000:]
        rng = np.random.default_rng(1)
        alpha = rng.standard_normal((k, 30_000)).astype(dt)
        rho = np.linspace(0.25, 0.75, k)
        with (backend.Predictor(prm, sv, alpha[0], 0.25, every_form=every_form) if k == 1 else backend.Predictor(prm, sv, alpha, rho, every_form=every_form)) as pred:
            for n in sizes:
                batch = np.ascontiguousarray(pts[:n])
                timed(f"{tag}, {n} points: resident", lambda info: pred.predict(batch, info_out=info))
                if k == 1:
                    timed(f"{tag}, {n} points: one-shot", lambda info: backend.predict_values(prm, sv, alpha[0], 0.25, None, batch, info_out=info))
                else:
                    timed(f"{tag}, {n} points: one-shot", lambda info: backend.predict_values_multi(prm, sv, alpha, rho.astype(dt), None, batch, info_out=info))

    shape("fp32 rbf 30000 x 128", Parameter(kernel_type="rbf", gamma=1.0 / 128), np.float32, 128, (100, 4096))
    shape("fp64 rbf 30000 x 64", Parameter(kernel_type="rbf", gamma=1.0 / 64), np.float64, 64, (100, 4096), every_form=True)
    shape("fp32 poly3 30000 x 192 nvec 3", Parameter(kernel_type="polynomial", degree=3, gamma=1.0 / 192, coef0=0.5), np.float32, 192, (4096,), k=3, every_form=True)
    print("RESULT " + json.dumps(out), flush=True)


def run_child(which, libs, mode, reps, limit):
    env = dict(os.environ)
    if libs[which]:
        env["PLSSVM_AMD_LIBRARY"] = os.path.abspath(libs[which])
    else:
        env.pop("PLSSVM_AMD_LIBRARY", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(reps)]
    try:
        proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"{which}: child exceeded {limit} s; stopping", file=sys.stderr)
        return None
    line = next((ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if proc.returncode != 0 or line is None:
        print(f"{which}: child failed with status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}", file=sys.stderr)
        return None
    return json.loads(line[len("RESULT "):])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--new-lib", default=None, help="the library under test (default: this build's); the parent's once more gives the run-to-run noise of the comparison itself")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_stage_bits.json"))
    ap.add_argument("--child", choices=["bits", "timing"])
    args = ap.parse_args()
    if args.child:
        bits_child() if args.child == "bits" else timing_child(args.reps)
        return 0
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        ap.error("--parent-lib must name the library built from the parent commit")
    libs = {"parent": args.parent_lib, "new": args.new_lib}
    res = json.load(open(args.out)) if os.path.isfile(args.out) else {}
    failed = []
    if args.timing:
        samples = {"parent": {}, "new": {}}
        for rnd in range(args.rounds):
            for which in (("parent", "new") if rnd % 2 == 0 else ("new", "parent")):  # (neither library is always the first of a round)
                got = run_child(which, libs, "timing", args.reps, args.child_timeout)
                if got is None:
                    return 1
                for name, vals in got.items():
                    samples[which].setdefault(name, []).extend(vals)
                print(f"round {rnd}, {which}: done", flush=True)
        res["timing"] = {}
        for name in sorted(samples["new"]):
            a, b = samples["new"][name], samples["parent"][name]
            med_a, med_b = statistics.median(a), statistics.median(b)
            spread = (max(b) - min(b)) / med_b
            ok = med_a <= med_b * (1.0 + spread)
            checked = name.endswith((" wall_ms", " kernel_ms"))  # (total_ms and setup_ms, the call's own clocks, say where a difference lies)
            res["timing"][name] = {"new_median_ms": round(med_a, 5), "parent_median_ms": round(med_b, 5), "ratio": round(med_a / med_b, 4), "parent_spread": round(spread, 4),
                                   "new_spread": round((max(a) - min(a)) / med_a, 4), "samples_per_library": len(b), "within_parent_spread": ok, "condition": checked}
            if checked and not ok:
                failed.append(name)
        res["timing_method"] = (f"{args.rounds} child processes per library, alternating, the first of a round the parent's and this build's in turn; {args.reps} timed repetitions "
                                "each after two warm-up calls; wall_ms: host wall clock of the whole call, kernel_ms / total_ms / setup_ms: the call's own report; condition on "
                                "wall_ms and kernel_ms: new median <= parent median * (1 + parent spread), spread = (max - min) / median")
        res["timing_failed"] = failed
        print(json.dumps(res["timing"], indent=1))
    else:
        got = {}
        for which in ("parent", "new"):
            got[which] = run_child(which, libs, "bits", args.reps, args.child_timeout)
            if got[which] is None:
                return 1
            print(f"{which}: {len(got[which])} cases", flush=True)
        res["bits"] = {}
        for name in sorted(set(got["parent"]) | set(got["new"])):
            (sha_p, _, info_p), (sha_n, _, info_n) = (got[which].get(name, "missing").partition(" ") for which in ("parent", "new"))
            res["bits"][name] = {"parent": sha_p, "new": sha_n, "info": info_p if info_p == info_n else {"parent": info_p, "new": info_n}}  # (the fields once where they agree)
        failed = [name for name, d in res["bits"].items() if d["parent"] != d["new"] or isinstance(d["info"], dict)]
        res["bits_summary"] = {"cases": len(res["bits"]), "equal": len(res["bits"]) - len(failed), "different": failed}
        print(json.dumps(res["bits_summary"], indent=1))
    with open(args.out, "w") as f:  # (one line per case and per timed shape)
        parts = []
        for key in sorted(res):
            if isinstance(res[key], dict) and key in ("bits", "timing"):
                rows = ",\n".join(f"  {json.dumps(name)}: {json.dumps(res[key][name], sort_keys=True)}" for name in sorted(res[key]))
                parts.append(f" {json.dumps(key)}: {{\n{rows}\n }}")
            else:
                parts.append(f" {json.dumps(key)}: {json.dumps(res[key], sort_keys=True)}")
        f.write("{\n" + ",\n".join(parts) + "\n}\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
