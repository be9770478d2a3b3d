"""The Java numeric conversions and the mixing hash of sentinel_amd/csrc/java_num.h, the one copy the kernels and the
host side share, on the CPU: the stand-alone program tests/cpp/test_java_num_host.cpp (built by
tests/cpp/java_num_host.mk with the address and undefined-behaviour sanitizers) checks the known answers of
Math.round, (int) and (long); its mix64 and table_home are compared here with the project's Python mirrors. No GPU."""
import os
import subprocess

import numpy as np

from sentinel_amd import cluster, param_wire
from tests import value_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "tests", "test_java_num_host")

M64 = (1 << 64) - 1
INPUTS = [0, 1, 2, 63, 64, 12345, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 1 << 32, (1 << 63) - 1, 1 << 63, M64 - 1, M64,
          0x9E3779B97F4A7C15, 0x61C8864680B583EB, 0xDEADBEEFCAFEF00D]


def run(*args):
    assert os.path.exists(BIN), (f"{BIN} is missing: build it with `make -C tests/cpp -f java_num_host.mk` "
                                 "(or __graft_entry__.build())")
    p = subprocess.run([BIN, *[str(a) for a in args]], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def hashes(mask, xs):
    """[(x, mix64(x), mix64_final(x), table_home(x, mask))] as the program computes them."""
    rows = [tuple(int(w, 16) for w in line.split()) for line in run(hex(mask), *[hex(x) for x in xs]).splitlines()]
    assert [r[0] for r in rows] == list(xs)
    return rows


def test_known_answers_on_the_host():
    assert "java num host ok" in run()


def test_mix64_is_the_shard_hash():
    rows = hashes(0, INPUTS)
    want = cluster.splitmix64(np.array(INPUTS, dtype=np.uint64))
    assert [r[1] for r in rows] == [int(w) for w in want]
    for world in (1, 2, 3, 8):
        own = cluster.owner_of(np.array(INPUTS, dtype=np.uint64), world)
        assert [r[1] % world for r in rows] == [int(o) for o in own]


def test_mix64_chains_to_the_value_hash():
    # (type tag, canonical payload) of at most 8 bytes: the hash is mix64(mix64(type | length << 8) ^ payload)
    keys = [(0, (7).to_bytes(4, "big")), (1, b""), (2, b"\x01"), (3, bytes(range(8))), (5, b"\xff" * 8), (6, b"abc")]
    seeds = hashes(0, [t | (len(p) << 8) for t, p in keys])
    second = hashes(0, [s[1] ^ int.from_bytes(p, "little") for s, (t, p) in zip(seeds, keys)])
    for (t, p), r in zip(keys, second):
        assert r[1] == param_wire.value_hash(t, p), (t, p)


def test_mix64_final_is_mix64_without_the_offset():
    rows = hashes(0, INPUTS)
    shifted = hashes(0, [(x + 0x9E3779B97F4A7C15) & M64 for x in INPUTS])
    assert [r[1] for r in rows] == [s[2] for s in shifted]


def test_table_home_is_the_value_tables_home_slot():
    for mask in (0, 1, 63, 1023, (1 << 20) - 1, (1 << 40) - 1):
        for x, _, _, home in hashes(mask, INPUTS):
            assert home == value_tables.home(x, mask), (x, mask)
