"""The host-only part of SystemSlot (sentinel_amd/csrc/system_rules.h) on the CPU: the stand-alone program
tests/cpp/test_system_host.cpp, built by tests/cpp/system_host.mk with the address and undefined-behaviour sanitizers
(the merge of loadSystemConf: defaults, minimum of duplicates, cpu > 1, the last rule's status; the key groups of the
system image).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "tests", "test_system_host")


def test_system_rule_merge_and_groups():
    assert os.path.exists(BIN), (f"{BIN} is missing: build it with `make -C tests/cpp -f system_host.mk` "
                                 "(or __graft_entry__.build())")
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "system host ok" in p.stdout
