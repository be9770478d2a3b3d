"""GatewayFlowSlot's host side (sentinel_amd/csrc/gateway_rules.h) on the CPU: the stand-alone program
tests/cpp/test_gateway_host.cpp, built by tests/cpp/gateway_host.mk with the address and undefined-behaviour
sanitizers (every validity branch of isValidRule, the conversion with its indices, hot items and the collapse of equal
item-less rules, gw_match's edges, and the adapter's parser expectations over the converted tables).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "tests", "test_gateway_host")


def test_gateway_rules_header():
    assert os.path.exists(BIN), (f"{BIN} is missing: build it with `make -C tests/cpp -f gateway_host.mk` "
                                 "(or __graft_entry__.build())")
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "gateway host ok" in p.stdout
