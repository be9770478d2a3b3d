"""CPU-side checks of the gateway API ABI (sg_gateway_load_apis, sg_gateway_verdict_ids, sg_gateway_set_item_fields,
sg_gateway_expand_batch): the header's struct layouts against sentinel_amd/abi.py, field by field, its constants, and
the library's exports."""
import os
import subprocess

from sentinel_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sentinel_gpu.h")
STRUCTS = [("sg_gateway_api", abi.GATEWAY_API_DTYPE), ("sg_gateway_api_pred", abi.GATEWAY_API_PRED_DTYPE),
           ("sg_gateway_http_req", abi.GATEWAY_HTTP_REQ_DTYPE), ("sg_gateway_field", abi.GATEWAY_FIELD_DTYPE)]


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
    assert [dt.itemsize for _, dt in STRUCTS] == [16, 16, 48, 16]


def test_constants_match_header():
    text = open(HEADER).read()
    for name, value in [("SG_GW_URL_MATCH_EXACT", abi.GW_URL_MATCH_EXACT), ("SG_GW_URL_MATCH_PREFIX", abi.GW_URL_MATCH_PREFIX),
                        ("SG_GW_URL_MATCH_REGEX", abi.GW_URL_MATCH_REGEX), ("SG_GW_API_NAME_BLANK", abi.GW_API_NAME_BLANK),
                        ("SG_GW_API_PREDS_NULL", abi.GW_API_PREDS_NULL), ("SG_GW_PRED_PATTERN_NULL", abi.GW_PRED_PATTERN_NULL),
                        ("SG_GW_PRED_NOT_PATH", abi.GW_PRED_NOT_PATH), ("SG_GW_PRED_REGEX_INVALID", abi.GW_PRED_REGEX_INVALID),
                        ("SG_GW_NO_ROUTE", abi.GW_NO_ROUTE)]:
        assert f"#define {name} " in text
        assert int(text.split(f"#define {name} ")[1].split()[0].rstrip("u"), 0) == value


def test_library_exports_the_gateway_api_entry_points():
    from sentinel_amd.engine import EXPORTS, load_library
    L = load_library()
    for name in ("sg_gateway_load_apis", "sg_gateway_verdict_ids", "sg_gateway_set_item_fields",
                 "sg_gateway_expand_batch"):
        assert name in EXPORTS and hasattr(L, name)
