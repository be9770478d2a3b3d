#!/usr/bin/env python3
"""Times the in-place growth of the value tables on one MI355X ("Growing the value tables").
No oracle: tests/test_table_grow_gpu.py checks the results.

  (a) cparam_resize  the rules and capacity of `bench_configs.py --workload cparam` (1000 rules, 2^16 slots each,
                     10 buckets per slot), every rule's table half full of live values, one bit up
  (b) param_resize   1000 hot-parameter rules of 2^16 slots, half full, one bit up
  (c) vdict_grow     a dictionary of 2^20 values (half of them strings of 12 bytes) to 2^21
  (d) the yardstick  one device-to-device hipMemcpyAsync of the bytes of the old tables of (a), (b) and (c)

Each call is timed by the host clock: the calls end with a device synchronise, so the time covers the allocation of
the new tables, the clear, the rehash kernels and the release of the old tables. The copy is timed by HIP events
around the memcpy alone, after one untimed copy. Every repetition builds its engine again (a resize can be measured
once per table). Writes the medians and ranges as one JSON object."""
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
R = 1000
MAX_BATCH = 1 << 24


def _stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(min(xs)), "max_ms": float(max(xs)), "reps": len(xs)}


def _pairs(lg, dev):
    """Every rule with 2^(lg - 1) distinct values, rule-major: (rule i64, value i64) on the device."""
    k = 1 << (lg - 1)
    rule = torch.arange(R, device=dev).repeat_interleave(k)
    value = (torch.arange(k, device=dev).repeat(R) * 0x9E3779B1 + rule * 0x85EBCA77 + 11) & 0x7FFFFFFFFFFFFFFF
    return rule, value


def _copy_ms(nbytes, reps):
    """Device-to-device copy of nbytes (torch's same-device copy of contiguous bytes is one hipMemcpyAsync), HIP
    events around the copy."""
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src, non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        if i:
            out.append(a.elapsed_time(b))
    del src, dst
    torch.cuda.empty_cache()
    return out


def _timed(call):
    torch.cuda.synchronize()
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def time_cparam(lg, dev):
    rng = np.random.default_rng(7)
    rules = np.zeros(R, abi.CPARAM_RULE_DTYPE)
    rules["flow_id"] = np.arange(R) + 1
    rules["count"] = rng.integers(1, 41, R)
    rules["threshold_type"] = abi.THRESHOLD_GLOBAL
    rules["sample_count"], rules["window_interval_ms"] = 10, 1000
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"] = 1
    eng = FlowEngine(device=0, max_batch=MAX_BATCH)
    eng.set_namespaces(ns)
    eng.cparam_load_rules(rules, None, lg)
    rule, value = _pairs(lg, dev)
    for lo in range(0, len(rule), MAX_BATCH):   # one request per (rule, value): its first token, so the value is live
        r, v = rule[lo:lo + MAX_BATCH], value[lo:lo + MAX_BATCH].contiguous()
        n = len(r)
        w = torch.zeros((n, 3), dtype=torch.int64, device=dev)
        w[:, 0] = T0
        w[:, 1] = r | (1 << 32)                                  # key, acquireCount 1
        w[:, 2] = torch.arange(n, device=dev) | (1 << 32)        # value_begin, value_count 1
        out = torch.empty(n * abi.RES_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        eng.cparam_decide_device(w.data_ptr(), n, v.data_ptr(), n, out.data_ptr())
        torch.cuda.synchronize()
    used = eng.cparam_table_used(R - 1)
    assert used == (1 << (lg - 1), 1 << (lg - 1), 1 << lg), used
    del w, out, rule, value
    torch.cuda.empty_cache()
    ms = _timed(lambda: eng.cparam_resize(lg + 1))
    assert eng.cparam_table_used(R - 1) == (1 << (lg - 1), 1 << (lg - 1), 2 << lg)
    eng.close()
    return ms


def time_param(lg, dev):
    rng = np.random.default_rng(8)
    rules = np.zeros(R, abi.PARAM_RULE_DTYPE)
    rules["count"] = rng.integers(1, 41, R)
    rules["duration_sec"] = 1
    rules["capacity_log2"] = lg
    eng = FlowEngine(device=0, max_batch=MAX_BATCH)
    eng.param_load_rules(rules)
    rule, value = _pairs(lg, dev)
    for lo in range(0, len(rule), MAX_BATCH):
        r, v = rule[lo:lo + MAX_BATCH], value[lo:lo + MAX_BATCH]
        n = len(r)
        w = torch.zeros((n, 3), dtype=torch.int64, device=dev)
        w[:, 0] = T0
        w[:, 1] = v
        w[:, 2] = r | (1 << 32)                                  # rule, acquireCount 1
        out = torch.empty(n, dtype=torch.int32, device=dev)
        eng.param_decide_device(w.data_ptr(), n, out.data_ptr())
        torch.cuda.synchronize()
    assert eng.param_table_used(R - 1) == (1 << (lg - 1), 1 << (lg - 1), 1 << lg)
    del w, out, rule, value
    torch.cuda.empty_cache()
    ms = _timed(lambda: eng.param_resize([lg + 1] * R))
    assert eng.param_table_used(R - 1) == (1 << (lg - 1), 1 << (lg - 1), 2 << lg)
    eng.close()
    return ms


def time_vdict(lg):
    n = 1 << lg
    eng = FlowEngine(device=0, max_batch=1 << 16)
    eng.vdict_init(lg, 12 * (n // 2), n)
    idx = np.arange(n, dtype=np.int64)
    lens = np.where(idx % 2 == 1, 12, 8).astype(np.uint32)       # STRING of 12 bytes / LONG
    types = np.where(idx % 2 == 1, abi.PARAM_TYPE_STRING, abi.PARAM_TYPE_LONG).astype(np.uint8)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    wide = np.zeros((n, 12), np.uint8)
    wide[:, :8] = idx.astype(">i8").view(np.uint8).reshape(n, 8)
    wide[:, 8:] = 0x41
    data = np.ascontiguousarray(wide[np.arange(12)[None, :] < lens[:, None]])
    ids = np.zeros(n, np.uint64)
    eng._check(eng._L.sg_vdict_intern(eng.h, abi.ptr(types), abi.ptr(offsets), abi.ptr(data), n, abi.ptr(ids)))
    assert eng.vdict_size() == (n, 12 * (n // 2)) and ids[-1] == n
    ms = _timed(lambda: eng.vdict_grow(lg + 1, 24 * (n // 2)))
    assert eng.vdict_size() == (n, 12 * (n // 2))
    eng.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--capacity-log2", type=int, default=16, help="sub-table size before the growth (bench_configs cparam: 16)")
    ap.add_argument("--vdict-log2", type=int, default=20)
    ap.add_argument("--out", default="profiles/table_grow_time.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    dev = torch.device("cuda:0")
    lg, slots = args.capacity_log2, R * ((1 << args.capacity_log2) + 1)
    sizes = {
        "cparam": slots * (8 + 10 * 16),                                   # keys and 10 buckets of 16 bytes per slot
        "param": slots * 32,
        "vdict": (1 << args.vdict_log2) * (24 + 16) + 24 + 12 * (1 << (args.vdict_log2 - 1)),  # entries, table, arena
    }
    res = {"device": torch.cuda.get_device_name(0), "rules": R, "capacity_log2": lg, "vdict_log2": args.vdict_log2,
           "old_table_bytes": sizes}
    runs = {"cparam": lambda: time_cparam(lg, dev), "param": lambda: time_param(lg, dev),
            "vdict": lambda: time_vdict(args.vdict_log2)}
    for name, run in runs.items():
        run()                                                              # warm-up: loads every kernel
        grow = _stat([run() for _ in range(args.reps)])
        copy = _stat(_copy_ms(sizes[name], args.reps))
        res[name] = {"resize": grow, "d2d_copy": copy,
                     "resize_old_bytes_per_s": sizes[name] / (grow["median_ms"] * 1e-3),
                     "copy_bytes_per_s": sizes[name] / (copy["median_ms"] * 1e-3),
                     "resize_over_copy": grow["median_ms"] / copy["median_ms"]}
        print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
