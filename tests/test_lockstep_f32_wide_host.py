"""Host side of the fp32 lockstep CG on 129 ... 512 features (no GPU): the translation units of the symmetric two-vector split kernels
(plssvm_amd/csrc/tile_launch_f32v2ws.hip, built as its _f16 and _bf16 halves) hold exactly the instantiations sym_pair_routed of lssvm_problem.hip may dispatch --
f16x3 planes: the polynomial forms on 3 ... 8 chunks of 64 features, folded rbf on 3 ... 6; bf16x6 planes: all four on 3 ... 6; 38 kernels --, every one without
scratch and without spills at one wave per SIMD.  Read from the resource-usage files the build leaves beside the ISA of the library that ships."""

import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE = os.path.join(ROOT, "plssvm_amd", "lib", "asm", "resource_usage_tile_launch_f32v2ws*.txt")
KT_POLY, KT_POLY2, KT_POLY3, KT_RBFF = 1, 3, 4, 5  # (lssvm_types.hpp)


def expected_kernels():
    """(wrapper, kernel type, 64-feature chunks) of every instantiation sym_pair_routed dispatches"""
    want = set()
    for kt in (KT_POLY, KT_POLY2, KT_POLY3, KT_RBFF):
        want.update(("f3w_nv2s", kt, n) for n in range(3, (6 if kt == KT_RBFF else 8) + 1))
        want.update(("s6w_nv2s", kt, n) for n in range(3, 7))
    return want


def test_the_symmetric_two_vector_units_hold_the_routed_kernels_without_scratch_at_one_wave_per_simd():
    files = sorted(glob.glob(USAGE))
    if not files:
        pytest.skip("no build tree here")
    lib = os.path.join(ROOT, "plssvm_amd", "lib", "libplssvm_amd.so")
    found = {}
    for path in files:
        assert os.path.getmtime(path) <= os.path.getmtime(lib) + 1, "lib/asm is newer than the library: run make"
        name = None
        with open(path) as f:
            for line in f:
                m = re.search(r"Function Name: (\S+)", line)
                if m:
                    name = m.group(1)
                    assert name not in found, f"instantiated twice: {name}"
                    found[name] = {}
                    continue
                m = re.search(r"remark: \S+\s+(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
                if m and name is not None:
                    found[name][m.group(1).split()[0]] = int(m.group(2))
    kernels = {}
    for name, usage in found.items():
        m = re.fullmatch(r"_ZN5lssvm\d+tile_matvec_f32_(f3w_nv2s|s6w_nv2s)ILi(\d+)ELi(\d+)EEEvNS_8TileArgsIfEE", name)
        assert m, f"a kernel that is no symmetric two-vector instantiation: {name}"
        kernels[(m.group(1), int(m.group(2)), int(m.group(3)))] = usage
    assert set(kernels) == expected_kernels() and len(kernels) == 38, sorted(set(kernels) ^ expected_kernels())
    for key, usage in sorted(kernels.items()):
        assert usage == {"ScratchSize": 0, "Occupancy": 1, "SGPRs": 0, "VGPRs": 0}, (key, usage)
