"""CPU-side checks of the table-growth entry points: the library exports them with the signatures engine.py binds,
both engines carry the Python methods, and the host-only size arithmetic and refusal order
(sentinel_amd/csrc/table_grow.h) pass their stand-alone program tests/cpp/test_table_grow_host.cpp, built by
tests/cpp/table_grow_host.mk with the address and undefined-behaviour sanitizers. No compute calls (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sentinel_gpu.h")
BIN = os.path.join(ROOT, "build", "tests", "test_table_grow_host")

USED = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
ENTRY_POINTS = {
    "sg_param_resize": [C.c_void_p, C.c_void_p, C.c_uint32],
    "sg_param_table_used": USED,
    "sg_cparam_resize": [C.c_void_p, C.c_int32],
    "sg_cparam_table_used": USED,
    "sg_vdict_grow": [C.c_void_p, C.c_int32, C.c_uint64],
    "sg_node_param_resize": [C.c_void_p, C.c_void_p, C.c_uint32],
    "sg_node_param_table_used": USED,
    "sg_node_cparam_resize": [C.c_void_p, C.c_int32],
    "sg_node_cparam_table_used": USED,
}


def test_header_declares_the_growth_entry_points():
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    assert "growing a dictionary after sg_vdict_init" not in text   # no longer among the things not covered


def test_library_exports_them_with_the_bound_signatures():
    from sentinel_amd.engine import LIB_PATH, load_library
    assert os.path.exists(LIB_PATH), "build with make -C sentinel_amd/csrc"
    L = load_library()
    for name, args in ENTRY_POINTS.items():
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == args, name


def test_engines_carry_the_methods():
    from sentinel_amd.engine import FlowEngine, NodeEngine
    for m in ("param_resize", "param_table_used", "cparam_resize", "cparam_table_used", "vdict_grow"):
        assert callable(getattr(FlowEngine, m)), m
    for m in ("param_resize", "param_table_used", "cparam_resize", "cparam_table_used"):
        assert callable(getattr(NodeEngine, m)), m


def test_null_handles_are_refused():
    from sentinel_amd import abi
    from sentinel_amd.engine import load_library
    L = load_library()
    assert L.sg_param_resize(None, None, 0) == abi.SG_E_INVAL
    assert L.sg_param_table_used(None, 0, None, None, None) == abi.SG_E_INVAL
    assert L.sg_cparam_resize(None, 4) == abi.SG_E_INVAL
    assert L.sg_cparam_table_used(None, 0, None, None, None) == abi.SG_E_INVAL
    assert L.sg_vdict_grow(None, 4, 0) == abi.SG_E_INVAL
    assert L.sg_node_param_resize(None, None, 0) == abi.SG_E_INVAL
    assert L.sg_node_param_table_used(None, 0, None, None, None) == abi.SG_E_INVAL
    assert L.sg_node_cparam_resize(None, 4) == abi.SG_E_INVAL
    assert L.sg_node_cparam_table_used(None, 0, None, None, None) == abi.SG_E_INVAL


def test_growth_plans_on_the_host():
    assert os.path.exists(BIN), (f"{BIN} is missing: build it with `make -C tests/cpp -f table_grow_host.mk` "
                                 "(or __graft_entry__.build())")
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "table grow host ok" in p.stdout
