#!/usr/bin/env python3
"""Times the node's metric-row merge and one node step of the local slot chain ("The local chain over the
node handle"). No oracle: the rows and the trace are synthetic.

  merge   raw rows of K resources over G shards (one row per resource and second, two seconds, plus the shards'
          ENTRY_NODE rows), laid out shard by shard as sg_node_local_metrics lays them out; on the same rows
            (a) cluster.DeviceLocalMetricRollup.merge   (torch sort / unique / searchsorted, two host round trips)
            (b) sg_node_local_merge_rows                (k_merge_*)
          HIP events around each repetition, medians.
  step    a trace of --events entries per second over the same resources (QPS rule + two breakers each);
            node    NodeEngine.local_decide_device + local_metrics_device (events and results in HBM)
            python  cluster.split_local_events on the host, G FlowEngines (slices uploaded, decided, raw rows fetched),
                    DeviceLocalMetricRollup.merge
          wall clock around each step with the device idle before and after, medians.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sentinel_amd import abi  # noqa: E402
from sentinel_amd.cluster import (ENTRY_NODE_RESOURCE, DeviceLocalMetricRollup, owner_of,  # noqa: E402
                                  split_local_events)
from sentinel_amd.engine import FlowEngine, NodeEngine  # noqa: E402

T0 = 1_700_000_000_000


def rules_of(K):
    r = np.zeros(K, abi.LOCAL_RULE_DTYPE)
    r["flow_count"], r["flow_grade"], r["n_breakers"] = 20.0, abi.FLOW_GRADE_QPS, 2
    b = np.zeros(2, abi.DEGRADE_RULE_DTYPE)
    b["grade"] = [abi.DEGRADE_RT, abi.DEGRADE_EXCEPTION_RATIO]
    b["count"] = [100, 0.5]
    b["time_window_sec"], b["min_request_amount"], b["stat_interval_ms"] = 10, 5, 1000
    b["slow_ratio_threshold"] = [0.5, 1.0]
    r["breakers"] = b
    return r


def raw_rows(K, G, owners, rng):
    parts = []
    for g in range(G):
        mine = np.nonzero(owners == g)[0]
        r = np.zeros(2 * len(mine) + 2, abi.METRIC_NODE_DTYPE)
        r["resource"][:-2] = np.repeat(mine, 2)
        r["timestamp"][:-2] = np.tile([T0, T0 + 1000], len(mine))
        r["resource"][-2:] = ENTRY_NODE_RESOURCE
        r["timestamp"][-2:] = [T0, T0 + 1000]
        for f in ("pass_qps", "block_qps", "success_qps", "exception_qps"):
            r[f] = rng.integers(0, 8, len(r))
        r["rt"] = rng.integers(0, 4000, len(r))
        parts.append(r)
    return np.concatenate(parts)


def spread(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4), "reps": len(ms)}


def timed_events(fn, reps, warmup):
    out = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", type=int, default=1_000_000)
    ap.add_argument("--shards", type=int, default=4)
    ap.add_argument("--events", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--merge-only", action="store_true", help="skip the node step")
    args = ap.parse_args()
    K, G = args.resources, args.shards
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    rules = rules_of(K)
    owners = owner_of(np.arange(K, dtype=np.uint64), G)
    node = NodeEngine([0] * G, max_batch=args.events)
    node.local_load_rules(rules, 2, 1000, 500)
    node.local_set_entry_types(np.ones(K, np.uint8))
    assert all(node.local_owner_of(r) == owners[r] for r in range(0, K, max(1, K // 1000)))

    # ---- merge
    rows = raw_rows(K, G, owners, rng)
    rows_t = torch.from_numpy(rows.view(np.int64).reshape(-1, 8).copy()).to(dev)
    out_t = torch.empty_like(rows_t)
    st = torch.cuda.current_stream().cuda_stream
    want = DeviceLocalMetricRollup.merge(rows_t)
    k = node.local_merge_rows(rows_t, out_t, st)
    assert k == want.shape[0] and bool((out_t[:k] == want).all()), "the two merges differ"
    res = {"resources": K, "shards": G, "rows": int(rows_t.shape[0]), "merged_rows": int(k)}
    res["merge_torch"] = spread(timed_events(lambda: DeviceLocalMetricRollup.merge(rows_t), args.reps, args.warmup))
    res["merge_node"] = spread(timed_events(lambda: node.local_merge_rows(rows_t, out_t, st), args.reps, args.warmup))

    if args.merge_only:
        print(json.dumps(res))
        return

    # ---- one step: the same entries every second (Zipf(1.0) popularity), no exits
    n = args.events
    w = 1.0 / (np.arange(K, dtype=np.float64) + 1.0)
    cdf = np.cumsum(w)
    cdf /= cdf[-1]
    perm = rng.permutation(K)
    ev = np.zeros(n, abi.LOCAL_EVENT_DTYPE)
    ev["ts_ms"] = T0 + np.sort(rng.integers(0, 1000, n))
    ev["resource"] = perm[np.minimum(np.searchsorted(cdf, rng.random(n), side="right"), K - 1)]
    ev["count"] = 1
    engs = []
    for _ in range(G):
        e = FlowEngine(device=0, max_batch=n)
        e.local_load_rules(rules, 2, 1000, 500)
        e.local_set_entry_types(np.ones(K, np.uint8))
        engs.append(e)
    cap = 4 * K + 64
    node_rows = torch.empty((cap, 8), dtype=torch.int64, device=dev)
    out_dev = torch.empty(n * abi.LOCAL_RES_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    bufs = [torch.empty((cap, 8), dtype=torch.int64, device=dev) for _ in range(G)]
    outs = [torch.empty(n * abi.LOCAL_RES_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in range(G)]
    t_node, t_py = [], []
    for s in range(args.warmup + args.reps):
        cur = ev.copy()
        cur["ts_ms"] += 1000 * s
        now = T0 + 1000 * (s + 1)
        ev_t = torch.from_numpy(cur.view(np.uint8)).to(dev)
        torch.cuda.synchronize()
        t = time.perf_counter()
        node.local_decide_device(ev_t.data_ptr(), n, out_dev.data_ptr(), st)
        kn = node.local_metrics_device(now, node_rows)
        torch.cuda.synchronize()
        t_node.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        parts = split_local_events(cur, owners, G)
        got = []
        for e, pos, buf, o in zip(engs, parts, bufs, outs):
            sl = torch.from_numpy(cur[pos].view(np.uint8)).to(dev)
            e.local_decide_device(sl.data_ptr(), len(pos), o.data_ptr(), st)
            got.append(buf[:e.local_metrics_raw_device(now, buf)])
        m = DeviceLocalMetricRollup.merge(torch.cat(got))
        torch.cuda.synchronize()
        t_py.append(1e3 * (time.perf_counter() - t))
        assert kn == m.shape[0] and bool((node_rows[:kn] == m).all()), f"step {s}: the two tables differ"
        node_res = out_dev.view(torch.int64)
        for pos, o in zip(parts, outs):
            idx = torch.from_numpy(pos).to(dev)
            assert bool((node_res[idx] == o.view(torch.int64)[:len(pos)]).all()), f"step {s}: decisions differ"
    res["events_per_step"] = n
    res["step_node"] = spread(t_node[args.warmup:])
    res["step_python"] = spread(t_py[args.warmup:])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
