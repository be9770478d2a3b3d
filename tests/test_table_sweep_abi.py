"""CPU-side checks of the table-sweep entry points: the header declares them, the library exports them with the
signatures engine.py binds, both engines carry the Python methods, null handles are refused, and the idle predicates
(sentinel_amd/csrc/table_sweep.h) pass their stand-alone program tests/cpp/test_table_sweep_host.cpp, built by
tests/cpp/table_sweep_host.mk with the address and undefined-behaviour sanitizers. No compute calls (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sentinel_gpu.h")
BIN = os.path.join(ROOT, "build", "tests", "test_table_sweep_host")

NAMES = ("sg_param_sweep", "sg_cparam_sweep", "sg_node_param_sweep", "sg_node_cparam_sweep")


def test_header_declares_the_sweep_entry_points():
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"^int %s\(\w+\* \w+, int64_t now_ms, sg_sweep_stats\* out\);" % name, text, re.M), name
    m = re.search(r"typedef struct sg_sweep_stats \{(.*?)\} sg_sweep_stats;", text, re.S)
    assert m, "sg_sweep_stats"
    assert re.findall(r"uint64_t (\w+);", m.group(1)) == ["values_removed", "claims_dropped", "threads_removed",
                                                         "values_kept"]


def test_library_exports_them_with_the_bound_signatures():
    from sentinel_amd import abi
    from sentinel_amd.engine import LIB_PATH, load_library
    assert os.path.exists(LIB_PATH), "build with make -C sentinel_amd/csrc"
    L = load_library()
    assert C.sizeof(abi.sg_sweep_stats) == 32
    assert [n for n, _ in abi.sg_sweep_stats._fields_] == ["values_removed", "claims_dropped", "threads_removed",
                                                          "values_kept"]
    for name in NAMES:
        f = getattr(L, name)
        assert f.restype is C.c_int, name
        assert list(f.argtypes) == [C.c_void_p, C.c_int64, C.POINTER(abi.sg_sweep_stats)], name


def test_engines_carry_the_methods():
    from sentinel_amd.engine import FlowEngine, NodeEngine
    for cls in (FlowEngine, NodeEngine):
        for m in ("param_sweep", "cparam_sweep"):
            assert callable(getattr(cls, m)), (cls.__name__, m)


def test_null_handles_are_refused():
    from sentinel_amd import abi
    from sentinel_amd.engine import load_library
    L = load_library()
    st = abi.sg_sweep_stats()
    for name in NAMES:
        assert getattr(L, name)(None, 0, None) == abi.SG_E_INVAL, name
        assert getattr(L, name)(None, 0, C.byref(st)) == abi.SG_E_INVAL, name


def test_idle_predicates_on_the_host():
    assert os.path.exists(BIN), (f"{BIN} is missing: build it with `make -C tests/cpp -f table_sweep_host.mk` "
                                 "(or __graft_entry__.build())")
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "table sweep host ok" in p.stdout
