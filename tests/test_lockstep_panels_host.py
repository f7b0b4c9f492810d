"""Host side of the lockstep CG on the panel kernels (no GPU): the two _panels entry points are declared and exported, and the measured routing of
profiles/lockstep_panels.json (tests/tools/lockstep_panels_timing.py) is the routing of sym_panel_pair_routed -- an instantiation the library dispatched took less than two
single-vector passes of the parent by more than the parent's own run-to-run spread, one that did not is not dispatched."""

import json
import os

import pytest

from plssvm_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "profiles", "lockstep_panels.json")) as f:
    PROFILE = json.load(f)
WANT = ([f"{planes}_{kernel}_{d}" for planes in ("f16x3", "bf16x6") for kernel in ("poly", "poly2", "poly3", "rbf") for d in (640, 784)]
        + [f"fp64_{kernel}_{d}" for kernel in ("poly", "poly2", "poly3", "rbf") for d in (320, 784)])


def test_the_entry_points_are_exported():
    for name in ("lssvm_mi355_problem_matvec_pair_panels", "lssvm_mi355_problem_solve_lockstep_panels"):
        assert name in _capi.EXPORTED_SYMBOLS and getattr(_capi.lib, name) is not None


def test_every_instantiation_was_measured():
    assert sorted(PROFILE["instantiations"]) == sorted(WANT)
    assert len(PROFILE["kernels"]) == 12 and all(k["scratch_bytes"] == 0 and k["vgpr_spills"] == 0 for k in PROFILE["kernels"].values())


@pytest.mark.parametrize("name", WANT)
def test_dispatch_follows_the_measurement(name):
    rec = PROFILE["instantiations"][name]
    assert rec["samples"] >= 10 and rec["same_bits_as_parent"]
    pays = rec["ratio_to_two_parent_passes"] + rec["parent_spread"] < 1.0
    assert rec["dispatched"] == pays, (name, rec)
