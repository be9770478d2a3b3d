"""The host-only arithmetic of the token server stat log (sentinel_amd/csrc/serverlog_rules.h) on the CPU: the
stand-alone program tests/cpp/test_serverlog_host.cpp, built by tests/cpp/serverlog_host.mk with the address and
undefined-behaviour sanitizers (the expansion of a slot's counters into rows, the merge of equal keys, the row order,
the capacity arithmetic at 2^4 and 2^24, the answer to a cap that is too small).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "tests", "test_serverlog_host")


def test_serverlog_expand_merge_sort_capacity():
    assert os.path.exists(BIN), (f"{BIN} is missing: build it with `make -C tests/cpp -f serverlog_host.mk` "
                                 "(or __graft_entry__.build())")
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "serverlog host ok" in p.stdout
