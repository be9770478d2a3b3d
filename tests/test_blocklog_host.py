"""The host-only per-resource limitApp table of LogSlot's rollup (sentinel_amd/csrc/blocklog_rules.h) on the CPU: the
stand-alone program tests/cpp/test_blocklog_host.cpp, built by tests/cpp/blocklog_host.mk with the address and
undefined-behaviour sanitizers (no rules, one rule, equal and mixed limitApps, rules dropped at load, cluster-mode
rules, a resource index at K - 1).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "tests", "test_blocklog_host")


def test_blocklog_limit_app_table():
    assert os.path.exists(BIN), (f"{BIN} is missing: build it with `make -C tests/cpp -f blocklog_host.mk` "
                                 "(or __graft_entry__.build())")
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "blocklog host ok" in p.stdout
