"""The gateway API definitions' host side and the matcher host and device share (sentinel_amd/csrc/gateway_api.h) on
the CPU: the stand-alone program tests/cpp/test_gateway_api_host.cpp, built by tests/cpp/gateway_api_host.mk with the
address and undefined-behaviour sanitizers. Its own run holds the known answers, classification, the lookup tables and
the verdict ids; its `match` mode classifies and matches a file of definitions and paths, compared here with
tests/gateway_api_ref.py over random definitions."""
import os
import subprocess

import numpy as np
import pytest

from gateway_api_ref import HOST, Definitions, apis_to_abi, random_apis, random_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "tests", "test_gateway_api_host")
MISSING = (f"{BIN} is missing: build it with `make -C tests/cpp -f gateway_api_host.mk` "
           "(or __graft_entry__.build())")


def test_gateway_api_header():
    assert os.path.exists(BIN), MISSING
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "gateway api host ok" in p.stdout


def _hex(b):
    return b.hex() if b else "-"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_c_matching_equals_reference(seed, tmp_path):
    assert os.path.exists(BIN), MISSING
    rng = np.random.default_rng(seed)
    apis = random_apis(rng, 80, 50)
    d = Definitions(apis)
    a, preds, blob = apis_to_abi(apis)
    queries = []
    for _ in range(1500):
        path = random_path(rng) if rng.random() < 0.9 else b"a/" + random_path(rng)[1:]
        verdicts = tuple(v for v in range(len(d.vid_pred)) if rng.random() < 0.05)
        queries.append((path, verdicts))
    queries += [(b"", ()), (b"/", ()), (b"//", ()), (b"a", ())]
    lines = [f"P {p['match_strategy']} {p['flags']} {_hex(blob[p['pattern_off']:p['pattern_off'] + p['pattern_len']])}"
             for p in preds]
    lines += [f"A {x['resource']} {x['pred_begin']} {x['pred_count']} {x['flags']}" for x in a]
    lines += [f"Q {_hex(path)} {','.join(map(str, v)) if v else '-'}" for path, v in queries]
    src = tmp_path / "defs.txt"
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run([BIN, "match", str(src)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout.splitlines()
    assert [int(x) for x in out[0].split()[1:]] == d.cls
    assert [int(x) for x in out[1].split()[1:]] == d.vid_pred
    got = [[int(x) for x in line.split()[1:]] for line in out[2:]]
    want = [d.match(path, v) for path, v in queries]
    assert len(got) == len(want)
    for (path, v), g, w in zip(queries, got, want):
        assert g == w, (path, v, g, w)
    # the run holds what it is meant to hold
    assert sum(1 for w in want if len(w) > 1) > 50 and sum(1 for w in want if not w) > 50
    assert 0 < d.cls.count(HOST) <= 0.1 * len(d.cls)
