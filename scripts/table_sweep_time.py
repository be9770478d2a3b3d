#!/usr/bin/env python3
"""Times the sweep of idle values on one MI355X against the rehash it is built on ("Sweeping the value
tables"). No oracle: tests/test_table_sweep_gpu.py checks the results.

The shapes are those of scripts/table_grow_time.py, every table half full, and half of those values idle at the sweep:

  (a) cparam   1000 rules of 2^16 slots, 10 buckets per slot: half the values were last added 5 s before the sweep
               (every bucket deprecated), half in the sweep's own window
  (b) param    1000 hot-parameter rules of 2^16 slots: half the values took their first token 5 durations before the
               sweep (refilled past the maximum), half at the sweep's own millisecond
  (c) pslot    (b) with the rules loaded through the ParamFlowSlot chain, so the sweep also rehashes the thread-count
               table (2^20 slots, empty here)
The value dictionary, the third shape of the growth script, has no sweep.

Every repetition builds its engine, then times on the same tables first sg_*_resize at the size in force — the
same-size rehash: the same clear, probe and move traffic with nothing left out — and then the sweep. Both calls end
with a device synchronise and are timed by the host clock, so the time covers the allocation of the new tables, the
clear, the kernels and the release of the old tables. Writes the medians and ranges as one JSON object."""
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
GAP = 5000
R = 1000
MAX_BATCH = 1 << 24


def _stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(min(xs)), "max_ms": float(max(xs)), "reps": len(xs)}


def _pairs(lg, dev, half):
    """Every rule with 2^(lg - 2) distinct values of half 0 or 1, rule-major: (rule i64, value i64) on the device."""
    k = 1 << (lg - 2)
    rule = torch.arange(R, device=dev).repeat_interleave(k)
    value = ((torch.arange(k, device=dev).repeat(R) * 2 + half) * 0x9E3779B1 + rule * 0x85EBCA77 + 11) & 0x7FFFFFFFFFFFFFFF
    return rule, value


def _timed(call):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = call()
    return (time.perf_counter() - t) * 1e3, out


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
    for half in (0, 1):   # one request per (rule, value): its first token, so the value is live at its time
        rule, value = _pairs(lg, dev, half)
        for lo in range(0, len(rule), MAX_BATCH):
            r, v = rule[lo:lo + MAX_BATCH], value[lo:lo + MAX_BATCH].contiguous()
            n = len(r)
            w = torch.zeros((n, 3), dtype=torch.int64, device=dev)
            w[:, 0] = T0 + half * GAP
            w[:, 1] = r | (1 << 32)                                  # key, acquireCount 1
            w[:, 2] = torch.arange(n, device=dev) | (1 << 32)        # value_begin, value_count 1
            out = torch.empty(n * abi.RES_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            eng.cparam_decide_device(w.data_ptr(), n, v.data_ptr(), n, out.data_ptr())
            torch.cuda.synchronize()
    half_full, quarter = 1 << (lg - 1), 1 << (lg - 2)
    assert eng.cparam_table_used(R - 1) == (half_full, half_full, 1 << lg)
    del w, out, rule, value
    torch.cuda.empty_cache()
    rehash, _ = _timed(lambda: eng.cparam_resize(lg))
    assert eng.cparam_table_used(R - 1) == (half_full, half_full, 1 << lg)
    sweep, st = _timed(lambda: eng.cparam_sweep(T0 + GAP))
    assert st == {"values_removed": R * quarter, "claims_dropped": 0, "threads_removed": 0, "values_kept": R * quarter}, st
    assert eng.cparam_table_used(R - 1) == (quarter, quarter, 1 << lg)
    eng.close()
    return rehash, sweep


def time_param(lg, dev, pslot=False):
    rng = np.random.default_rng(8)
    rules = np.zeros(R, abi.PSLOT_RULE_DTYPE if pslot else abi.PARAM_RULE_DTYPE)
    prm = rules["rule"] if pslot else rules
    prm["count"] = rng.integers(1, 41, R)
    prm["duration_sec"] = 1
    prm["capacity_log2"] = lg
    eng = FlowEngine(device=0, max_batch=MAX_BATCH)
    if pslot:
        rules["resource"], rules["grade"] = np.arange(R), 1
        eng.pslot_load_rules(rules, n_resources=R)
    else:
        eng.param_load_rules(rules)
    for half in (0, 1):
        rule, value = _pairs(lg, dev, half)
        for lo in range(0, len(rule), MAX_BATCH):
            r, v = rule[lo:lo + MAX_BATCH], value[lo:lo + MAX_BATCH]
            n = len(r)
            w = torch.zeros((n, 3), dtype=torch.int64, device=dev)
            w[:, 0] = T0 + half * GAP
            w[:, 1] = v
            w[:, 2] = r | (1 << 32)                                  # rule, acquireCount 1
            out = torch.empty(n, dtype=torch.int32, device=dev)
            eng.param_decide_device(w.data_ptr(), n, out.data_ptr())
            torch.cuda.synchronize()
    half_full, quarter = 1 << (lg - 1), 1 << (lg - 2)
    assert eng.param_table_used(R - 1) == (half_full, half_full, 1 << lg)
    del w, out, rule, value
    torch.cuda.empty_cache()
    rehash, _ = _timed(lambda: eng.param_resize([0] * R))
    assert eng.param_table_used(R - 1) == (half_full, half_full, 1 << lg)
    sweep, st = _timed(lambda: eng.param_sweep(T0 + GAP))
    assert st == {"values_removed": R * quarter, "claims_dropped": 0, "threads_removed": 0, "values_kept": R * quarter}, st
    assert eng.param_table_used(R - 1) == (quarter, quarter, 1 << lg)
    eng.close()
    return rehash, sweep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--capacity-log2", type=int, default=16, help="sub-table size (bench_configs cparam: 16)")
    ap.add_argument("--out", default="profiles/table_sweep_time.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    dev = torch.device("cuda:0")
    lg, slots = args.capacity_log2, R * ((1 << args.capacity_log2) + 1)
    sizes = {"cparam": slots * (8 + 10 * 16), "param": slots * 32, "pslot": slots * 32 + (32 << 20)}
    res = {"device": torch.cuda.get_device_name(0), "rules": R, "capacity_log2": lg, "table_bytes": sizes}
    runs = {"cparam": lambda: time_cparam(lg, dev), "param": lambda: time_param(lg, dev),
            "pslot": lambda: time_param(lg, dev, pslot=True)}
    for name, run in runs.items():
        run()                                                              # warm-up: loads every kernel
        got = [run() for _ in range(args.reps)]
        rehash, sweep = _stat([g[0] for g in got]), _stat([g[1] for g in got])
        # the fastest runs: a call that allocates gigabytes now and then takes a second, and a median can land on one
        res[name] = {"same_size_resize": rehash, "sweep": sweep,
                     "sweep_over_resize_fastest": sweep["min_ms"] / rehash["min_ms"]}
        print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
