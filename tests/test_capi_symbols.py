"""CPU: libplssvm_amd.so loads without a GPU, exports every symbol include/plssvm_amd.h declares, validates arguments
before touching a device, and FAILS LOUDLY (LSSVM_ERR_NO_DEVICE) instead of falling back to a CPU path."""

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from plssvm_amd import _capi, backend
from plssvm_amd.exceptions import BackendError, InvalidParameterError
from plssvm_amd.parameter import Parameter

HEADER = os.path.join(ROOT, "include", "plssvm_amd.h")                   # the boundary a PLSSVM maintainer binds
TESTING_HEADER = os.path.join(ROOT, "include", "plssvm_amd_testing.h")   # measurement / test aids of bench.py and tests/ (same library)


def declared_symbols(headers=(HEADER, TESTING_HEADER)):
    found = set()
    for header in headers:
        text = open(header).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        found.update(re.findall(r"\b(lssvm_mi355_\w+)\s*\(", text))
    return sorted(found)


def test_header_and_binding_agree():
    assert declared_symbols() == sorted(_capi.EXPORTED_SYMBOLS)
    # the public header carries no measurement / test entry point and documents no test knob
    assert "lssvm_mi355_measure_bf16_mfma_ceiling" not in declared_symbols((HEADER,))
    public = open(HEADER).read()
    for knob in ("debug_ablate", "pair_lag", "skip_collective", "force_collective"):
        assert knob not in public, knob
    # thirteen documented options + two testing aids + one experimental option (the testing header) = the sixteen the library accepts (+ those of development builds)
    documented = re.findall(r'^ \*   "(\w+)"', public, flags=re.M)
    assert sorted(documented + ["force_collective", "skip_collective", "rebalance_after"]) == sorted(_capi.OPTION_NAMES) and len(_capi.OPTION_NAMES) == 16
    # the speculative multi-device surface of round 5 is not part of the boundary a maintainer binds: testing header only
    testing = open(TESTING_HEADER).read()
    for name in ("lssvm_mi355_set_shard_weights", "lssvm_mi355_problem_rebalance", "rebalance_after"):
        assert name not in public and name in testing, name
    for name in _capi.OPTION_NAMES + _capi.DEV_OPTION_NAMES:
        _capi.get_option(name)
    for retired in ("xcd_map", "lds_extra_kb", "item_order", "linear_panel_features", "check_shards", "rbf_direct_above"):
        with pytest.raises(InvalidParameterError):
            _capi.get_option(retired)


def test_library_exports_every_declared_symbol():
    for name in declared_symbols():
        assert hasattr(_capi.lib, name), f"{name} is declared in include/plssvm_amd.h but not exported"
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lssvm_mi355_\w+)", out))
    assert exported == set(declared_symbols())


def test_no_oracle_or_torch_in_the_product_library():
    """The product path must not route through the oracle or any CPU fallback."""
    out = subprocess.run(["ldd", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "lssvm_oracle" not in out and "lssvm_ref" not in out and "torch" not in out
    assert "libamdhip64" in out
    pkg = os.path.join(ROOT, "plssvm_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oracle_lib" not in text and "liblssvm_oracle" not in text, f"{f} references the oracle"


def test_abi_version_and_struct_layout():
    assert _capi.lib.lssvm_mi355_abi_version() == _capi.ABI_VERSION
    assert C.sizeof(_capi.LssvmParams) == 32
    assert C.sizeof(_capi.LssvmShard) == 8
    assert C.sizeof(_capi.LssvmCgInfo) == 168  # ABI 4 (static_assert in capi.hip)
    assert C.sizeof(_capi.LssvmPredictInfo) == 56 and C.sizeof(_capi.LssvmModelInfo) == 80


has_gpu = _capi.device_count() > 0


def test_argument_validation_happens_without_a_device():
    X = np.ones((4, 3))
    y = np.array([1.0, -1, 1, -1])
    with pytest.raises(InvalidParameterError, match="stopping criterion"):   # csvm.cpp:77
        backend.solve_system_of_linear_equations(Parameter(), X, y, 0.0, 4)
    with pytest.raises(InvalidParameterError, match="CG iterations"):        # csvm.cpp:78
        backend.solve_system_of_linear_equations(Parameter(), X, y, 1e-3, 0)
    with pytest.raises(InvalidParameterError, match="right hand side"):      # csvm.cpp:76
        backend.solve_system_of_linear_equations(Parameter(), X, y[:3], 1e-3, 4)
    with pytest.raises(InvalidParameterError, match="gamma"):                # svm_kernel.cpp:68
        ps = _capi.LssvmParams(2, 3, -1.0, 0.0, 1.0)
        _capi.check(_capi.lib.lssvm_mi355_generate_q_f64(C.byref(ps), _capi.ptr(X), C.c_size_t(4), C.c_size_t(3), _capi.ptr(np.zeros(3)), None))
    with pytest.raises(InvalidParameterError, match="cost"):                 # svm_kernel.cpp:27
        ps = _capi.LssvmParams(0, 3, 1.0, 0.0, 0.0)
        _capi.check(_capi.lib.lssvm_mi355_generate_q_f64(C.byref(ps), _capi.ptr(X), C.c_size_t(4), C.c_size_t(3), _capi.ptr(np.zeros(3)), None))
    with pytest.raises(InvalidParameterError, match="unknown option"):
        _capi.set_option("no_such_option", 1)
    assert _capi.get_option("rbf_form") == 0 and _capi.get_option("j_chunk_tiles") == 0
    # the IPC entry points of the one-process-per-GPU mode: NULL handles and bad options are refused before anything touches a device
    blob = (C.c_ubyte * _capi.LSSVM_IPC_BLOB_BYTES)()
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(_capi.lib.lssvm_mi355_problem_ipc_export(None, blob, C.c_size_t(_capi.LSSVM_IPC_BLOB_BYTES)))
    with pytest.raises(InvalidParameterError, match="handle"):
        _capi.check(_capi.lib.lssvm_mi355_problem_ipc_connect(None, blob, C.c_size_t(_capi.LSSVM_IPC_BLOB_BYTES)))
    with pytest.raises(InvalidParameterError, match="ipc_timeout_s"):
        _capi.set_option("ipc_timeout_s", 0)
    assert _capi.get_option("ipc_timeout_s") == 600 and _capi.get_option("enqueue_ahead_below_us") == 5000


@pytest.mark.skipif(has_gpu, reason="only meaningful on a box without a GPU")
def test_no_device_is_a_loud_error_not_a_fallback():
    assert _capi.device_count() == 0
    X = np.ones((4, 3))
    y = np.array([1.0, -1, 1, -1])
    with pytest.raises(BackendError, match="no HIP capable devices"):        # csvm.hip.cpp:70-72
        backend.solve_system_of_linear_equations(Parameter(), X, y, 1e-3, 4)
    with pytest.raises(BackendError, match="no HIP capable devices"):
        backend.generate_q(Parameter(kernel_type="rbf"), X)
    with pytest.raises(BackendError, match="no HIP capable devices"):
        backend.predict_values(Parameter(), X, y, 0.0, None, X)
    with pytest.raises(BackendError, match="no HIP capable devices"):
        backend.ResidentProblem(Parameter(), X)


def test_cpp_adaptor_factory_and_loud_failure_without_gpu():
    """tests/cpp/test_csvm --no-gpu: make_csvm / exception behaviour of include/plssvm_amd/csvm.hpp (reads like the reference's
    tests/csvm_factory.cpp); on a box without a GPU the backend constructor must throw mi355::backend_exception."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_csvm")
    if not os.path.isfile(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True)
    if has_gpu:
        pytest.skip("covered by the -m gpu run of the full driver")
    out = subprocess.run([exe, "--no-gpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_generated_code_of_the_shipped_library_passes_the_audit():
    """The library is linked only if tests/tools/audit_hand_asm.py passes on the ISA its objects were assembled from (plssvm_amd/csrc/Makefile keeps it
    under lib/asm): compiler code must stay out of the hand-scheduled kernels' private registers and away from accumulators in flight, must not touch
    M0 where inline asm owns it, and no load may write the C operand of an in-flight v_mfma_f64 (gfx950 hazard without a compiler rule,
    tests/tools/repro/dgemm_srcc_war.hip).  Re-run here so that the check is part of every test run where the build tree is present."""
    import glob
    import subprocess
    import sys

    asm = sorted(glob.glob(os.path.join(ROOT, "plssvm_amd", "lib", "asm", "*.s")))
    if not asm:
        pytest.skip("no build tree here (the ISA dumps do not travel to the GPU box)")
    lib = os.path.join(ROOT, "plssvm_amd", "lib", "libplssvm_amd.so")
    assert all(os.path.getmtime(a) <= os.path.getmtime(lib) + 1 for a in asm), "lib/asm is newer than the library: run make"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "audit_hand_asm.py")] + asm, capture_output=True, text=True)
    last = res.stdout.strip().splitlines()[-1]
    assert res.returncode == 0 and last.endswith(" 0 broken"), res.stdout[-2000:]
    assert int(last.split()[0]) >= 40, last  # the hand-scheduled instantiations were found at all


@pytest.mark.parametrize("exe_name, args", [("test_reader_sanitized", []), ("test_arff_reader_sanitized", []), ("test_model_io_sanitized", []), ("test_csvm_sanitized", ["--no-gpu"]), ("test_geometry_sanitized", [])])
def test_host_side_under_address_and_undefined_behaviour_sanitizers(exe_name, args):
    """CPU build only (GPU sanitizers are not available on this pool): the native LIBSVM reader on the shapes of the reference's
    invalid fixtures, every truncation and single-byte corruption of a valid file, overflowing indices, CR / CRLF, NUL bytes ... and the host side of
    the C++ adaptor (factory, named parameters, exceptions), both compiled with -fsanitize=address,undefined -fno-sanitize-recover.  The reader must
    refuse what is not well formed without ever touching memory it does not own (/root/reference/include/plssvm/detail/io/libsvm_parsing.hpp:118-229
    is the rule book; the reference-exact diagnosis stays with plssvm_amd/io_libsvm.py).  Round 5: the native ARFF reader likewise (arff_parsing.hpp:57-372)."""
    exe = os.path.join(ROOT, "tests", "cpp", exe_name)
    if not os.path.isfile(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe), exe_name], check=True, capture_output=True)
    if exe_name == "test_csvm_sanitized" and has_gpu:
        pytest.skip("the --no-gpu subset is for boxes without a device")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")  # (leak checking: the HIP runtime's own start-up allocations)
    out = subprocess.run([exe] + args, capture_output=True, text=True, env=env)
    assert out.returncode == 0 and "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stdout[-1500:] + out.stderr[-3000:]


FAKE_RCCL = os.path.join(ROOT, "tests", "tools", "fake_rccl", "librccl.so.1")


def test_rccl_stand_in_exports_what_the_product_binds_and_is_unknown_to_the_product():
    """tests/tools/fake_rccl/librccl.so.1 (test infrastructure for tests/test_gpu_fake_rccl.py) must offer every RCCL entry point the product resolves
    with dlsym -- and the product must not know about it: no file of the package or of include/ and no string of the shipped library names it."""
    src = open(os.path.join(ROOT, "plssvm_amd", "csrc", "lssvm_exchange.hip")).read()
    bound = set(re.findall(r'dlsym\(lib, "(nccl\w+)"\)', src))
    assert {"ncclAllReduce", "ncclAllGather", "ncclCommInitRank", "ncclCommInitAll", "ncclGroupStart", "ncclGroupEnd", "ncclCommCount"} <= bound
    assert os.path.isfile(FAKE_RCCL), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    out = subprocess.run(["nm", "-D", "--defined-only", FAKE_RCCL], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    assert bound <= exported and "fake_rccl_marker" in exported
    soname = subprocess.run(["readelf", "-d", FAKE_RCCL], capture_output=True, text=True, check=True).stdout
    assert "librccl.so.1" in soname
    for base in (os.path.join(ROOT, "plssvm_amd"), os.path.join(ROOT, "include")):
        for dirpath, _, files in os.walk(base):
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp", ".inc", "Makefile")):
                    assert "fake_rccl" not in open(os.path.join(dirpath, f), errors="replace").read(), f"{f} names the RCCL stand-in"
    assert b"fake_rccl" not in open(_capi.LIB_PATH, "rb").read()
    # the only libraries the product ever dlopens are RCCL's own names
    assert set(re.findall(r'"((?:/opt/rocm/lib/)?librccl[^"]*)"', src)) == {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}


def test_rccl_stand_in_wins_the_soname_lookup_only_when_a_harness_loads_it_first():
    """How the stand-in reaches a process: a harness loads it BEFORE anything else; the product's dlopen("librccl.so.1") then returns the already-loaded
    object with that SONAME.  In a process that did not do so, the same dlopen finds a real RCCL (checked in a child: no GPU is touched)."""
    code = ("import ctypes, os, sys\n"
            "if len(sys.argv) > 1:\n"
            "    sys.path.insert(0, os.path.dirname(sys.argv[1]))\n"
            "    import preload\n"
            "    first = preload.load(sys.argv[1])\n"
            "import torch\n"
            "h = ctypes.CDLL('librccl.so.1')\n"
            "hip = [l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l]\n"
            "print('stand-in' if hasattr(h, 'fake_rccl_marker') else 'real', torch.cuda.nccl.version()[0], len(set(hip)))\n")
    with_it = subprocess.run([sys.executable, "-c", code, FAKE_RCCL], capture_output=True, text=True, check=True).stdout.split()
    without = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout.split()
    assert with_it[0] == "stand-in" and without[0] == "real"
    assert with_it[1] == without[1] == "2"  # torch keeps its own RCCL either way (the stand-in reports version 0)
    assert with_it[2] == without[2] == "1"  # ONE HIP runtime in the process (a second one finds no device)
