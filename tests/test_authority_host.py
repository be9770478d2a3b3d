"""The host-only compiler of AuthoritySlot's rule table (sentinel_amd/csrc/authority_rules.h) on the CPU: the
stand-alone program tests/cpp/test_authority_host.cpp, built by tests/cpp/authority_host.mk with the address and
undefined-behaviour sanitizers (validity, first rule wins, ids above 64 in the sorted tail, duplicates, refused loads).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "tests", "test_authority_host")


def test_authority_rule_compiler():
    assert os.path.exists(BIN), (f"{BIN} is missing: build it with `make -C tests/cpp -f authority_host.mk` "
                                 "(or __graft_entry__.build())")
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "authority host ok" in p.stdout
