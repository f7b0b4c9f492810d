#!/usr/bin/env python3
"""The reference library's answers behind tests/test_oracle_golden.py::test_oracle_vs_live_reference, stored so that the test runs where oracle/_ref
cannot be built: on the test's own seeded 151 x 23 inputs, for every kernel in fp32 and fp64, the reference's q, ONE implicit matvec, a 5-step CG solve
(plus, for fp32, the float64 solve of the same data: the yardstick of the reference's own fp32 rounding) and predict_values.  The inputs are stored beside
them, so that a change of numpy's generator shows as such.

Run in the build container only (needs oracle/_ref):   make -C oracle ref && python tests/golden/make_golden_live_ref.py"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as ol  # noqa: E402

KERNELS = ["linear", "polynomial", "rbf"]
KW = dict(degree=3, gamma=1.0 / 23, coef0=0.5)


def inputs(dt):
    """The test's inputs, drawn in the test's order."""
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, size=(151, 23)).astype(dt)
    y = np.where(rng.uniform(size=151) > 0.5, 1, -1).astype(dt)
    rhs = rng.uniform(1, 2, size=150).astype(dt)
    return X, y, rhs


def main():
    if not ol.have_ref():
        raise SystemExit("oracle/_ref/liblssvm_ref.so is missing: make -C oracle ref")
    ref = ol.ref()
    out = {}
    for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
        X, y, rhs = inputs(dt)
        out[f"{tag}/X"], out[f"{tag}/y"], out[f"{tag}/rhs"] = X, y, rhs
        for kernel in KERNELS:
            key = f"{kernel}/{tag}"
            q = ref.q(kernel, X, **KW)
            out[key + "/q"] = q
            out[key + "/matvec"] = ref.matvec(kernel, X, q, rhs, np.zeros(150, dt), 2.0, 1.0, 1.0, **KW)
            alpha, _, info = ref.solve(kernel, X, y, 1e-30, 5, cost=1.0, **KW)
            out[key + "/solve_alpha"], out[key + "/solve_iterations"] = alpha, np.int64(info["iterations"])
            if dt == np.float32:
                out[key + "/solve_alpha_f64"] = ref.solve(kernel, X.astype(np.float64), y.astype(np.float64), 1e-30, 5, cost=1.0, **KW)[0]
            out[key + "/predict"] = ref.predict_values(kernel, X[:50], rhs[:50], 0.25, X[100:120], **KW)[0]
    path = os.path.join(HERE, "live_ref_151x23.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays")


if __name__ == "__main__":
    main()
