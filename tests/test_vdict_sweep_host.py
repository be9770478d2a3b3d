"""The host-side rules of sg_vdict_sweep (sentinel_amd/csrc/vdict_sweep.h: refusal order, the id rule, the post-batch
bookkeeping and the liveness predicates shared with the kernels) pass their stand-alone program
tests/cpp/test_vdict_sweep_host.cpp, built by tests/cpp/vdict_sweep_host.mk with the address and undefined-behaviour
sanitizers. Runs on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "tests", "test_vdict_sweep_host")


def test_vdict_sweep_rules_on_the_host():
    assert os.path.exists(BIN), (f"{BIN} is missing: build it with `make -C tests/cpp -f vdict_sweep_host.mk` "
                                 "(or __graft_entry__.build())")
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "vdict sweep host ok" in p.stdout
