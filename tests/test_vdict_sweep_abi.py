"""CPU-side checks of sg_vdict_sweep's ABI: the header's sg_vdict_sweep_stats against sentinel_amd/abi.py field by
field (a compiled probe), the declaration, the export with the signature engine.py binds, the Python method, and the
refusal of a null handle. No compute calls (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

from sentinel_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sentinel_gpu.h")
FIELDS = ["live", "removed", "free_ids", "high", "arena_before", "arena_after"]


def test_stats_layout_matches_header(tmp_path):
    prints = ['printf("%zu\\n", sizeof(sg_vdict_sweep_stats));']
    prints += [f'printf("%zu\\n", offsetof(sg_vdict_sweep_stats, {f}));' for f in FIELDS]
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\n'
                   f'int main(void) {{ {" ".join(prints)} return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    st = abi.sg_vdict_sweep_stats
    assert [n for n, _ in st._fields_] == FIELDS
    assert got == [C.sizeof(st)] + [getattr(st, f).offset for f in FIELDS]
    assert got == [48, 0, 8, 16, 24, 32, 40]


def test_header_declares_the_entry_point():
    text = open(HEADER).read()
    assert re.search(r"^int sg_vdict_sweep\(sg_handle\* h, const uint64_t\* keep_ids, uint64_t n_keep, "
                     r"sg_vdict_sweep_stats\* out\);", text, re.M)
    m = re.search(r"typedef struct sg_vdict_sweep_stats \{(.*?)\} sg_vdict_sweep_stats;", text, re.S)
    assert m and re.findall(r"uint64_t (\w+);", m.group(1)) == FIELDS


def test_library_exports_it_with_the_bound_signature():
    from sentinel_amd.engine import EXPORTS, LIB_PATH, load_library
    assert os.path.exists(LIB_PATH), "build with make -C sentinel_amd/csrc"
    L = load_library()
    assert "sg_vdict_sweep" in EXPORTS
    f = L.sg_vdict_sweep
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(abi.sg_vdict_sweep_stats)]


def test_engine_carries_the_method():
    from sentinel_amd.engine import FlowEngine
    assert callable(FlowEngine.vdict_sweep)


def test_null_handle_is_refused():
    from sentinel_amd.engine import load_library
    L = load_library()
    st = abi.sg_vdict_sweep_stats()
    assert L.sg_vdict_sweep(None, None, 0, None) == abi.SG_E_INVAL
    assert L.sg_vdict_sweep(None, None, 0, C.byref(st)) == abi.SG_E_INVAL
