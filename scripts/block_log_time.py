#!/usr/bin/env python3
"""Times LogSlot's rollup on the C2 shape of bench_configs.py (10k resources, Zipf(1.0), one second of entries per
batch, synchronous sg_local_decide_batch) — DESIGN.md §8 "LogSlot: what it costs". No oracle: the trace is synthetic.

For each case two handles decide the same batches, one with the block log on and one without, interleaved step by
step, HIP events around each batch:
  c2        the C2 rules as they are (count U{1..64}: with --events in the millions nearly every entry blocks already)
  overload  every count cut to 1
  mixed     every resource with the rules {"default" count c, "other" count c}: mixed limitApps, so with the log on
            the cx walkers give up their dead periods (no origin is declared, so "other" never applies and the
            decisions are those of one rule)
and per case the once-a-second fetch (sg_local_block_log, wall clock) and the host alternative the rollup replaces:
events and results copied to the host and grouped there with numpy by (second, resource, status). Last, the fetch of a
full table: 2^capacity_log2 keys, one blocked entry each.

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
from sentinel_amd.engine import FlowEngine  # noqa: E402
from bench_configs import T0, gpu_keys, zipf_cdf  # noqa: E402


def spread(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4), "reps": len(ms)}


def host_group_by(ev_t, out_t):
    """The shim's alternative: everything back to the host, one group-by there (FlowException rows only need the
    resource; the limitApp of a mixed resource cannot be had this way at all)."""
    ev = ev_t.cpu().numpy().view(abi.LOCAL_EVENT_DTYPE)
    out = out_t.cpu().numpy().view(abi.LOCAL_RES_DTYPE)
    blocked = np.nonzero((out["status"] != abi.LOCAL_PASS) & (out["status"] != abi.LOCAL_PASS_WAIT))[0]
    key = ((ev["ts_ms"][blocked] // 1000) << 34) | (ev["resource"][blocked].astype(np.int64) << 3) | out["status"][blocked]
    uniq, inv = np.unique(key, return_inverse=True)
    return uniq, np.bincount(inv, weights=ev["count"][blocked].astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=16_000_000)
    ap.add_argument("--resources", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--capacity-log2", type=int, default=16)
    ap.add_argument("--cases", default="c2,overload,mixed")
    args = ap.parse_args()
    K, n = args.resources, args.events
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2)
    counts = rng.integers(1, 65, K).astype(np.float64)
    cdf, perm = zipf_cdf(K, 1.0, 2)
    cdf_t, perm_t = torch.from_numpy(cdf).to(dev), torch.from_numpy(perm.astype(np.int64)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(2)
    steps = args.warmup + args.reps

    def batch(b):
        w = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        w[:, 0] = torch.sort(torch.randint(0, 1000, (n,), generator=gen, device=dev)).values + T0 + 1000 * b
        cnt = torch.where(torch.rand(n, generator=gen, device=dev) < 0.1,
                          torch.randint(2, 5, (n,), generator=gen, device=dev), torch.ones(n, dtype=torch.int64, device=dev))
        w[:, 2] = gpu_keys(cdf_t, perm_t, n, gen) | (cnt << 32)
        return w.view(torch.uint8).reshape(-1)

    batches = [batch(b) for b in range(steps)]
    out_t = [torch.empty(n * 8, dtype=torch.uint8, device=dev) for _ in range(2)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {"events": n, "resources": K, "capacity_log2": args.capacity_log2}

    def engine(case, log):
        eng = FlowEngine(device=0, max_batch=n)
        base = np.zeros(K, abi.LOCAL_RULE_DTYPE)
        base["flow_grade"] = abi.FLOW_GRADE_NONE if case == "mixed" else abi.FLOW_GRADE_QPS
        base["flow_count"] = 1.0 if case == "overload" else counts
        eng.local_load_rules(base, 2, 1000, 500)
        if case == "mixed":
            fr = np.zeros(2 * K, abi.LOCAL_FLOW_RULE_DTYPE)
            fr["resource"] = np.repeat(np.arange(K), 2)
            fr["grade"], fr["count"] = abi.FLOW_GRADE_QPS, np.repeat(counts, 2)
            fr["limit_app"] = np.tile([abi.LIMIT_APP_DEFAULT, abi.LIMIT_APP_OTHER], K)
            fr["warm_up_period_sec"], fr["max_queueing_ms"], fr["ref_resource"] = 10, 500, -1
            fr["cluster_key"] = abi.KEY_NO_RULE
            assert eng.local_load_flow_rules(fr, 0) == 2 * K
        if log:
            eng.block_log_enable(args.capacity_log2)
        return eng

    for case in args.cases.split(","):
        off, on = engine(case, False), engine(case, True)
        t_off, t_on, t_fetch, t_host, rows_n, lost = [], [], [], [], 0, 0
        for s in range(steps):
            ms = []
            for eng, o in ((off, out_t[0]), (on, out_t[1])):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                eng.local_decide_device(batches[s].data_ptr(), n, o.data_ptr(), stream)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            assert bool((out_t[0] == out_t[1]).all()), f"{case}: step {s}: the log changed a decision"
            t = time.perf_counter()
            rows, le, lc = on.block_log(T0 + 1000 * (s + 1))
            dt_fetch = 1e3 * (time.perf_counter() - t)
            t = time.perf_counter()
            uniq, sums = host_group_by(batches[s], out_t[1])
            dt_host = 1e3 * (time.perf_counter() - t)
            if case != "mixed":  # (a mixed resource's rows carry the failing rule's limitApp: still one per resource here)
                assert len(rows) == len(uniq) and int(rows["count"].sum()) + lc == int(sums.sum()), f"{case}: step {s}"
            if s >= args.warmup:
                t_off.append(ms[0])
                t_on.append(ms[1])
                t_fetch.append(dt_fetch)
                t_host.append(dt_host)
                rows_n, lost = len(rows), le
        blocked = int((out_t[1].view(torch.int32)[::2] != 0).sum())
        res[case] = {"log_off": spread(t_off), "log_on": spread(t_on),
                     "added_ms": round(float(np.median(t_on) - np.median(t_off)), 4), "fetch": spread(t_fetch),
                     "host_group_by": spread(t_host), "rows_per_fetch": rows_n, "lost_events": int(lost),
                     "blocked_share": round(blocked / n, 4)}
        off.close()
        on.close()
    # ---- the fetch of a full table: one blocked entry for each of 2^capacity_log2 keys, every slot taken
    slots = 1 << args.capacity_log2
    eng = FlowEngine(device=0, max_batch=slots)
    base = np.zeros(slots, abi.LOCAL_RULE_DTYPE)
    base["flow_grade"], base["flow_count"] = abi.FLOW_GRADE_QPS, 0.0
    eng.local_load_rules(base, 2, 1000, 500)
    eng.block_log_enable(args.capacity_log2)
    t_full, lost = [], 0
    for s in range(steps):
        ev = np.zeros(slots, abi.LOCAL_EVENT_DTYPE)
        ev["ts_ms"] = T0 + 1000 * s + np.arange(slots) * 1000 // slots
        ev["resource"], ev["count"] = rng.permutation(slots), 1
        eng.local_decide_host(ev)
        t = time.perf_counter()
        rows, le, lc = eng.block_log(T0 + 1000 * (s + 1))
        dt = 1e3 * (time.perf_counter() - t)
        assert len(rows) + le == slots and int(rows["count"].sum()) + lc == slots
        if s >= args.warmup:
            t_full.append(dt)
            lost = le
    res["full_table_fetch"] = dict(spread(t_full), rows=slots - int(lost), lost_events=int(lost))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
