"""CPU-side checks of the gateway ABI (sg_gateway_*): the header's struct layouts against sentinel_amd/abi.py, field by
field, and the C conversion (sentinel_amd/csrc/gateway_rules.h gw_convert, the function sg_gateway_load_rules runs)
against tests/gateway_ref.py over random rule sets. sg_gateway_load_rules itself needs a device, so the conversion is
reached through the host program build/tests/test_gateway_host (`convert` mode, sanitizer build); the device tests
compare sg_gateway_converted with the same reference."""
import os
import subprocess

import numpy as np
import pytest

from gateway_ref import Manager, random_rules, rules_to_abi
from sentinel_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sentinel_gpu.h")
BIN = os.path.join(ROOT, "build", "tests", "test_gateway_host")
STRUCTS = [("sg_gateway_rule", abi.GATEWAY_RULE_DTYPE), ("sg_gateway_req", abi.GATEWAY_REQ_DTYPE),
           ("sg_gateway_item", abi.GATEWAY_ITEM_DTYPE)]
RES_DTYPE = np.dtype([("rule_begin", "<u4"), ("n_items", "<u4"), ("has_item_less", "<u4"), ("reserved", "<u4")])
ITEM_RULE_DTYPE = np.dtype([("resource_mode", "<i4"), ("parse_strategy", "<i4"), ("match_strategy", "<i4"),
                            ("pat_off", "<u4"), ("pat_len", "<u4")])


def test_struct_layouts_match_header(tmp_path):
    prints = []
    for name, dt in STRUCTS:
        prints.append(f'printf("%zu\\n", sizeof({name}));')
        prints += [f'printf("%zu\\n", offsetof({name}, {f}));' for f in dt.names]
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\n'
                   f'int main(void) {{ {" ".join(prints)} return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = []
    for _, dt in STRUCTS:
        want += [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    assert got == want


def test_constants_match_header():
    text = open(HEADER).read()
    for name, value in [("SG_GW_PARSE_COOKIE", abi.GW_PARSE_COOKIE), ("SG_GW_MATCH_CONTAINS", abi.GW_MATCH_CONTAINS),
                        ("SG_GW_MATCH_REGEX", abi.GW_MATCH_REGEX), ("SG_GW_ITEM_NULL", abi.GW_ITEM_NULL),
                        ("SG_GW_ITEM_REGEX_MATCH", abi.GW_ITEM_REGEX_MATCH), ("SG_GW_NM_THRESHOLD", abi.GW_NM_THRESHOLD)]:
        assert f"#define {name}" in text
        assert int(text.split(f"#define {name}")[1].split()[0].rstrip("u")) == value


def test_library_exports_the_gateway_entry_points():
    from sentinel_amd.engine import EXPORTS, load_library
    L = load_library()
    for name in ("sg_gateway_load_rules", "sg_gateway_converted", "sg_gateway_param_rule_count",
                 "sg_gateway_parse_batch"):
        assert name in EXPORTS and hasattr(L, name)


def _convert_c(rules_abi, n_resources, nm_id, tmp_path):
    assert os.path.exists(BIN), (f"{BIN} is missing: build it with `make -C tests/cpp -f gateway_host.mk` "
                                 "(or __graft_entry__.build())")
    src, dst = tmp_path / "rules.bin", tmp_path / "converted.bin"
    src.write_bytes(rules_abi.tobytes())
    p = subprocess.run([BIN, "convert", str(src), str(n_resources), str(nm_id), str(dst)], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = dst.read_bytes()
    n_rules, n_hot, n_res, n_items = np.frombuffer(raw, np.uint32, 4)
    out, at = [], 16
    for dt, n in [(abi.PSLOT_RULE_DTYPE, n_rules), (abi.PARAM_HOT_DTYPE, n_hot), (np.dtype("<u4"), n_rules),
                  (RES_DTYPE, n_res), (ITEM_RULE_DTYPE, n_items)]:
        out.append(np.frombuffer(raw, dt, int(n), at))
        at += int(n) * dt.itemsize
    assert at == len(raw)
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_c_conversion_matches_reference(seed, tmp_path):
    rng = np.random.default_rng(seed)
    n_res = 60
    rules = random_rules(rng, n_res)
    rules_abi, blob = rules_to_abi(rules)
    conv, hot, source, res, item_rules = _convert_c(rules_abi, n_res + 2, 41, tmp_path)
    mgr = Manager(rules)
    want, want_hot, want_source = mgr.pslot_rules(41)
    assert np.array_equal(conv, want) and np.array_equal(hot, want_hot)
    assert np.array_equal(source.astype(np.int64), want_source)
    assert len(res) == n_res + 2
    for r in range(n_res + 2):
        assert (int(res[r]["n_items"]), bool(res[r]["has_item_less"])) == (mgr.n_item_rules(r), mgr.has_item_less(r))
        kept = [rule for _, rule in mgr.by_resource.get(r, []) if rule.item is not None]
        for rule in kept:
            t = item_rules[int(res[r]["rule_begin"]) + rule.item.index]
            pat = blob[int(t["pat_off"]):int(t["pat_off"]) + int(t["pat_len"])]
            assert (int(t["resource_mode"]), int(t["parse_strategy"]), int(t["match_strategy"]), pat) == \
                   (rule.resource_mode, rule.item.parse_strategy, rule.item.match_strategy, rule.item.pattern or b"")
    assert len(want) > 100 and len(want_hot) > 30 and len(want) < sum(1 for r in rules)   # collapses and drops occurred


def test_c_conversion_of_nothing(tmp_path):
    conv, hot, source, res, item_rules = _convert_c(np.zeros(0, abi.GATEWAY_RULE_DTYPE), 3, 1, tmp_path)
    assert len(conv) == len(hot) == len(source) == len(item_rules) == 0 and not res["n_items"].any()
