#!/usr/bin/env python3
"""Times sg_vdict_sweep on one MI355X against the closest full pass the dictionary had before it, sg_vdict_grow to the
next size (entries copy plus rehash) — DESIGN.md §8, "Sweeping the value dictionary". No oracle:
tests/test_vdict_sweep_gpu.py checks the results.

Two dictionaries, each exactly full:
  (a) ip      2^24 strings of 11 bytes, the size of a client IP (they live in the arena: longer than 8 bytes)
  (b) str40   2^22 strings of 40 bytes
Half of the values (the odd ids) are named by one hot-parameter rule's PSlot table, which is half full with them; the
others are named by nothing, so the sweep frees half of the ids and compacts half of the arena.

Every repetition builds a fresh engine and times one call by the host clock; both calls end with a device synchronise,
so the time covers the allocations, the kernels and the release of the old arrays. --grow-only times the growth alone:
run it with SG_LIB_PATH pointing at a library built from the parent commit to get the parent's figure on the same
dictionary. Writes fastest, median and slowest of each as one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sentinel_amd import abi  # noqa: E402
from sentinel_amd.engine import FlowEngine  # noqa: E402

T0 = 1_700_000_000_000
CHUNK = 1 << 20
HEX = np.frombuffer(b"0123456789abcdef", np.uint8)


def _stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(min(xs)), "max_ms": float(max(xs)), "reps": len(xs)}


def _strings(lo, n, width):
    """n distinct strings of `width` bytes: eight hex digits of the index behind a fixed prefix."""
    idx = np.arange(lo, lo + n, dtype=np.uint64)
    out = np.full((n, width), ord("."), np.uint8)
    for d in range(8):
        out[:, width - 1 - d] = HEX[((idx >> np.uint64(4 * d)) & np.uint64(15)).astype(np.int64)]
    return out.reshape(-1)


def build(lg, width, dev):
    """A dictionary of 2^lg strings, exactly full, and a PSlot table that names its odd ids."""
    n = 1 << lg
    eng = FlowEngine(device=0, max_batch=1 << 23)
    eng.vdict_init(lg, n * width, CHUNK)
    types = np.full(CHUNK, abi.PARAM_TYPE_STRING, np.uint8)
    offsets = (np.arange(CHUNK + 1, dtype=np.uint64) * width).astype(np.uint32)
    ids = np.zeros(CHUNK, np.uint64)
    for lo in range(0, n, CHUNK):
        data = _strings(lo, CHUNK, width)
        eng._check(eng._L.sg_vdict_intern(eng.h, abi.ptr(types), abi.ptr(offsets), abi.ptr(data), CHUNK, abi.ptr(ids)))
        assert ids[0] == lo + 1 and ids[-1] == lo + CHUNK
    assert eng.vdict_size() == (n, n * width)
    rule = np.zeros(1, abi.PARAM_RULE_DTYPE)
    rule["count"], rule["duration_sec"], rule["capacity_log2"] = 5, 1, lg
    eng.param_load_rules(rule)
    half = n // 2
    for lo in range(0, half, 1 << 23):
        m = min(1 << 23, half - lo)
        w = torch.zeros((m, 3), dtype=torch.int64, device=dev)
        w[:, 0] = T0
        w[:, 1] = (torch.arange(lo, lo + m, device=dev) << 1) + 1       # the odd ids
        w[:, 2] = 1 << 32                                               # rule 0, acquireCount 1
        out = torch.empty(m, dtype=torch.int32, device=dev)
        eng.param_decide_device(w.data_ptr(), m, out.data_ptr())
        torch.cuda.synchronize()
        del w, out
    assert eng.param_table_used(0)[0] == half
    torch.cuda.empty_cache()
    return eng, n


def _timed(call):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = call()
    return (time.perf_counter() - t) * 1e3, out


def time_grow(lg, width, dev):
    eng, n = build(lg, width, dev)
    ms, _ = _timed(lambda: eng.vdict_grow(lg + 1, 2 * n * width))
    assert eng.vdict_size() == (n, n * width)
    eng.close()
    return ms


def time_sweep(lg, width, dev):
    eng, n = build(lg, width, dev)
    ms, st = _timed(lambda: eng.vdict_sweep())
    assert st == {"live": n // 2, "removed": n // 2, "free_ids": n // 2, "high": n, "arena_before": n * width,
                  "arena_after": n // 2 * width}, st
    assert eng.vdict_lookup([n - 1])[0][1] == _strings(n - 2, 1, width).tobytes()
    eng.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grow-only", action="store_true", help="time sg_vdict_grow alone (a parent library has no sweep)")
    ap.add_argument("--label", default="this commit", help="which library the figures belong to")
    ap.add_argument("--out", default="profiles/vdict_sweep_time.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "library": args.label}
    for name, lg, width in (("ip", 24, 11), ("str40", 22, 40)):
        row = {"values": 1 << lg, "string_bytes": width}
        time_grow(lg, width, dev)                                           # warm-up: loads the kernels
        row["grow_to_next_size"] = _stat([time_grow(lg, width, dev) for _ in range(args.reps)])
        if not args.grow_only:
            time_sweep(lg, width, dev)
            row["sweep"] = _stat([time_sweep(lg, width, dev) for _ in range(args.reps)])
            row["sweep_over_grow_fastest"] = row["sweep"]["min_ms"] / row["grow_to_next_size"]["min_ms"]
            row["sweep_over_grow_median"] = row["sweep"]["median_ms"] / row["grow_to_next_size"]["median_ms"]
        res[name] = row
        print(name, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
