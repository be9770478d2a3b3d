"""Secondary benchmarks: the other BASELINE.json configurations, on one GPU, with the same JSON contract as
bench.py (which measures the headline C3 workload).

  --workload c2  10k resources, QPS FlowRule each (count U{1..64}), DefaultController over each resource's
                 StatisticNode (second window S=2/1000 ms + minute window), 16M entries per 1000 ms batch,
                 Zipf(1.0) resources, acquire 1 (10 % U{2..4}), no prioritized requests, no exits.
  --workload c4  one ParamFlowRule (count 5, durationInSec 1, DEFAULT token bucket) over 10M distinct u64
                 values, Zipf(1.1), 16M requests per 1000 ms batch, exact HBM table (2^25 slots).
  --workload c5  1M resources, each a QPS FlowRule + RT breaker (100 ms, slow ratio 0.5) + exception-ratio
                 breaker (0.5); statIntervalMs 1000, minRequestAmount 5, timeWindow 10 s; 16M entries per
                 1000 ms batch plus the exits of the passed ones (rt ~ lognormal, median 12 ms; 5 % errors).
                 The event stream depends on the decisions (only passed entries exit), so it is produced by
                 the CPU oracle's client model (oracle.binding.LocalTraceGen) before the timed region.
  --workload cparam  cluster hot-parameter tokens: 1000 ClusterParamFlowRules, 50k values each Zipf(1.1), 16M
                 requests per batch, 10 % with 2-3 values (the fixed-point path).
  --workload slot  the whole slot chain at C5 size with 10 % of the resources carrying an origin-limitApp rule, a
                 WarmUp rule or a ParamFlowRule (the cx walker's share); every batch checked against the oracle.
  --workload node  the C3 workload through the node handle (G same-device shards, --shards), pipelined.
  --workload gateway  GatewayFlowSlot: --resources routes with 3 item rules (client IP, EXACT header, CONTAINS URL
                  parameter) and an item-less rule each; times sg_gateway_parse_batch alone and parse + the slot chain.
  --workload gateway_api  the gateway workload behind its front: --resources routes plus --resources / 4 custom APIs (half
                  exact paths, half /x…/** definitions, a URL-parameter rule and an item-less rule each); HTTP requests
                  with a path and three fields; times sg_gateway_expand_batch alone and expand + parse + the slot chain.
  --workload pace  1M resources, each a FlowRule with CONTROL_BEHAVIOR_RATE_LIMITER (RateLimiterController,
                 count U{1..64}, maxQueueingTimeMs 500), 16M canPass calls per 1000 ms batch, Zipf(1.0),
                 acquire 1 (10 % U{2..4}).

Inputs are resident in HBM before the timed region; one step = one batch. cpu_baseline = the oracle
(sequential C restatement, 1 thread) on the first batch of the same workload.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from sentinel_amd import abi  # noqa: E402
from sentinel_amd.engine import FlowEngine  # noqa: E402

HBM_PEAK_GBS = 8000.0
T0 = 1_700_000_000_000


def zipf_cdf(n, s, seed):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    w = 1.0 / np.power(np.arange(1, n + 1, dtype=np.float64), s)
    cdf = np.cumsum(w)
    return cdf / cdf[-1], perm


def gpu_keys(cdf_t, perm_t, n, gen):
    u = torch.rand(n, generator=gen, device=cdf_t.device, dtype=torch.float64)
    r = torch.searchsorted(cdf_t, u, right=True).clamp_(max=len(cdf_t) - 1)
    return perm_t[r]


def timed(step, warmup, steps):
    for b in range(warmup):
        step(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(warmup, warmup + steps):
        step(b)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def local_timed(eng, batches, sizes, args, dev, stream):
    """C2 / C5 steps through sg_local_enqueue (the pipelined local path: a batch's front half — validation, sort by
    resource, segment and exit lists — beside the previous batch's walkers): at most two batches in flight (the two
    workspaces), each ticket collected two batches later, two out buffers alternating. --local-sync: the synchronous
    sg_local_decide_batch, one batch at a time."""
    outs = [torch.empty(max(sizes) * 8, dtype=torch.uint8, device=dev) for _ in range(2)]
    if args.local_sync:
        return timed(lambda b: eng.local_decide_device(batches[b].data_ptr(), sizes[b], outs[0].data_ptr(), stream),
                     args.warmup, args.steps)
    tickets = []

    def step(b):
        if len(tickets) >= 2:
            eng.local_wait(tickets.pop(0))
        tickets.append(eng.local_enqueue(batches[b].data_ptr(), sizes[b], outs[b % 2].data_ptr()))

    torch.cuda.synchronize()  # the batches were generated on torch's stream
    el = timed(step, args.warmup, args.steps)
    for t in tickets:
        eng.local_wait(t)
    return el


def c2(args, dev):
    K, n = 10_000, args.events
    rng = np.random.default_rng(2)
    rules = np.zeros(K, abi.LOCAL_RULE_DTYPE)
    rules["flow_count"] = rng.integers(1, 65, K).astype(np.float64)
    rules["flow_grade"] = abi.FLOW_GRADE_QPS
    cdf, perm = zipf_cdf(K, 1.0, 2)
    cdf_t, perm_t = torch.from_numpy(cdf).to(dev), torch.from_numpy(perm.astype(np.int64)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(2)

    def batch(b):
        w = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        w[:, 0] = torch.sort(torch.randint(0, 1000, (n,), generator=gen, device=dev)).values + T0 + 1000 * b
        cnt = torch.where(torch.rand(n, generator=gen, device=dev) < 0.1,
                          torch.randint(2, 5, (n,), generator=gen, device=dev), torch.ones(n, dtype=torch.int64, device=dev))
        w[:, 2] = gpu_keys(cdf_t, perm_t, n, gen) | (cnt << 32)   # resource | count << 32; kind = 0 (entry)
        return w.view(torch.uint8).reshape(-1)

    eng = FlowEngine(device=0, max_batch=n)
    eng.local_load_rules(rules, 2, 1000, 500)
    batches = [batch(b) for b in range(args.warmup + args.steps)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    el = local_timed(eng, batches, [n] * len(batches), args, dev, stream)
    touched = int(torch.unique(batches[-1].view(torch.int64).reshape(-1, 4)[:, 2] & 0xFFFFFFFF).numel())
    # per event: 32 B sg_local_event in + 8 B result out; per touched resource: second window 2x64 B read +
    # write, one minute bucket read + write, curThreadNum/breaker head 2x16 B, rule 16 B
    b_alg = n * (32 + 8) + touched * (2 * 128 + 2 * 64 + 2 * 16 + 16)
    base = None
    if not args.no_cpu_baseline:
        from oracle.binding import LocalChain
        ev = batches[0].view(torch.int64).reshape(-1, 4)[: args.cpu_events].cpu().numpy().copy().view(abi.LOCAL_EVENT_DTYPE).reshape(-1)
        ora = LocalChain(2, 1000, 500)
        ora.load_rules(rules)
        t = time.perf_counter()
        ora.decide(ev)
        dt = time.perf_counter() - t
        base = {"value": len(ev) / dt, "unit": "decisions/s", "cores": 1, "kind": "port",
                "sample": f"first {len(ev)} events of batch 0 through oracle LocalChain (1 thread), {dt:.1f} s"}
    return {"metric": "local flow decisions/sec (DefaultController over StatisticNode), 10k resources",
            "workload": "C2: 10k resources x QPS FlowRule, S=2/1000 ms second window + minute window, 16M entries/batch",
            "value": n * args.steps / el, "el": el, "n": n, "b_alg": b_alg, "touched": touched, "cpu": base,
            "data": "synthetic (GPU-generated, seeded): Zipf(1.0) resources, counts U{1..64}, 10% acquire U{2..4}"}


def c4(args, dev):
    n, V = args.events, 10_000_000
    rules = np.zeros(1, abi.PARAM_RULE_DTYPE)
    rules["count"], rules["duration_sec"], rules["behavior"], rules["capacity_log2"] = 5, 1, abi.BEHAVIOR_DEFAULT, 25
    cdf, perm = zipf_cdf(V, 1.1, 4)
    cdf_t, perm_t = torch.from_numpy(cdf).to(dev), torch.from_numpy(perm.astype(np.int64)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(4)

    def batch(b):
        w = torch.zeros((n, 3), dtype=torch.int64, device=dev)
        w[:, 0] = torch.sort(torch.randint(0, 1000, (n,), generator=gen, device=dev)).values + T0 + 1000 * b
        w[:, 1] = gpu_keys(cdf_t, perm_t, n, gen) * 0x9E3779B1 + 17     # distinct u64 values
        w[:, 2] = 1 << 32                                                # rule 0, acquireCount 1
        return w.view(torch.uint8).reshape(-1)

    eng = FlowEngine(device=0, max_batch=n)
    eng.param_load_rules(rules)
    batches = [batch(b) for b in range(args.warmup + args.steps)]
    out = torch.empty(n * 4, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    el = timed(lambda b: eng.param_decide_device(batches[b].data_ptr(), n, out.data_ptr(), stream), args.warmup, args.steps)
    touched = int(torch.unique(batches[-1].view(torch.int64).reshape(-1, 3)[:, 1]).numel())
    b_alg = n * (24 + 4) + touched * (2 * 32)   # request in, pass bit out; per value slot 32 B read + write
    base = None
    if not args.no_cpu_baseline:
        from oracle.binding import ParamFlowChecker
        req = batches[0].view(torch.int64).reshape(-1, 3)[: args.cpu_events].cpu().numpy().copy().view(abi.PARAM_REQ_DTYPE).reshape(-1)
        ora = ParamFlowChecker()
        ora.load_rules(rules)
        t = time.perf_counter()
        ora.decide(req)
        dt = time.perf_counter() - t
        base = {"value": len(req) / dt, "unit": "decisions/s", "cores": 1, "kind": "port",
                "sample": f"first {len(req)} requests of batch 0 through oracle ParamFlowChecker (1 thread), {dt:.1f} s"}
    return {"metric": "hot-parameter decisions/sec (ParamFlowChecker token bucket), 10M values",
            "workload": "C4: 1 ParamFlowRule count=5/1 s, 10M distinct values Zipf(1.1), 16M requests/batch",
            "value": n * args.steps / el, "el": el, "n": n, "b_alg": b_alg, "touched": touched, "cpu": base,
            "data": "synthetic (GPU-generated, seeded)"}


def c5(args, dev):
    from oracle.binding import LocalChain, LocalTraceGen, degrade_rule, local_rule
    K, n = args.resources, args.events
    rng = np.random.default_rng(5)
    rules = np.zeros(K, abi.LOCAL_RULE_DTYPE)
    rules["flow_count"] = rng.integers(1, 65, K).astype(np.float64)
    rules["flow_grade"] = abi.FLOW_GRADE_QPS
    rules["n_breakers"] = 2
    b = np.zeros(2, abi.DEGRADE_RULE_DTYPE)
    b[0] = degrade_rule(abi.DEGRADE_RT, 100, 10, 5, 1000, 0.5)
    b[1] = degrade_rule(abi.DEGRADE_EXCEPTION_RATIO, 0.5, 10, 5, 1000)
    rules["breakers"] = b
    cdf, perm = zipf_cdf(K, 1.0, 5)
    ora = LocalChain(2, 1000, 500)
    ora.load_rules(rules)
    gen = LocalTraceGen(ora)
    t_gen = time.time()
    host = []
    gen_s = 0.0
    for bt in range(args.warmup + args.steps):
        ent = np.zeros(n, abi.LOCAL_EVENT_DTYPE)
        ent["ts_ms"] = T0 + 1000 * bt + np.sort(rng.integers(0, 1000, n))
        ent["resource"] = perm[np.minimum(np.searchsorted(cdf, rng.random(n), side="right"), K - 1)]
        ent["count"] = 1
        rt = np.minimum(np.round(np.exp(rng.normal(2.5, 0.8, n))), 10_000).astype(np.int32)
        err = (rng.random(n) < 0.05).astype(np.uint8)
        t = time.perf_counter()
        ev, _ = gen.run(ent, rt, err, T0 + 1000 * (bt + 1))
        gen_s += time.perf_counter() - t
        host.append(ev)
    print(f"# c5 trace: {sum(len(e) for e in host)} events generated by the oracle client model in "
          f"{time.time() - t_gen:.1f} s", file=sys.stderr)
    eng = FlowEngine(device=0, max_batch=max(len(e) for e in host))
    eng.local_load_rules(rules, 2, 1000, 500)
    batches = [torch.from_numpy(e.view(np.uint8).copy()).to(dev) for e in host]
    stream = torch.cuda.current_stream(dev).cuda_stream
    sizes = [len(e) for e in host]
    el = local_timed(eng, batches, sizes, args, dev, stream)
    decided = sum(sizes[args.warmup:])
    touched = int(np.unique(host[-1]["resource"] & 0x7FFFFFFF).size)
    # per event 32 B in + 8 B out; per touched resource: second window 2x128 B, two minute buckets 2x2x64 B,
    # head (threads + two breakers) 2x128 B, rule 80 B
    b_alg = sizes[-1] * (32 + 8) + touched * (2 * 128 + 2 * 2 * 64 + 2 * 128 + 80)
    base = {"value": sum(sizes) / gen_s, "unit": "decisions/s", "cores": 1, "kind": "port",
            "sample": f"the oracle replaying all {sum(sizes)} events while generating them (client model, 1 thread), "
                      f"{gen_s:.1f} s"}
    return {"metric": "local flow + circuit-breaker decisions/sec (entries + exits), 1M resources",
            "workload": "C5: 1M resources x (QPS FlowRule + RT breaker + exception-ratio breaker), minute window, "
                        "16M entries/batch + exits of passed entries",
            "value": decided / el, "el": el, "n": decided // args.steps, "b_alg": b_alg, "touched": touched,
            "cpu": base, "data": "synthetic (seeded): Zipf(1.0) resources, rt lognormal(2.5, 0.8) ms, 5% errors; "
                                 "exits generated by the oracle client model"}


def slot(args, dev):
    """The whole slot chain at C5 size (sg_slot_decide_batch: ParamFlowSlot -> FlowSlot -> DegradeSlot inside
    StatisticSlot), with 10 % of the 1M resources off the fast walkers' single-DefaultController shape: a third carry an
    origin-limitApp rule beside their default rule (their callers pass an origin: 70 % of their entries, U{1..4}), a
    third a WarmUp rule (warmUpPeriodSec 10, coldFactor 3), a third a ParamFlowRule on argument 0 (QPS, count U{5..20},
    1 s; the argument one of 1000 values, Zipf 1.1). Every resource keeps C5's RT and exception-ratio breakers. Those
    resources go through the cx walker (k_lwalk_cx); with Zipf(1.0) popularity some of the hottest are among them.
    Entries + the exits of passed entries (the oracle's client model, as C5); the batches are synchronous (origin
    nodes are created with a host round trip). Every timed batch's results are checked against the oracle."""
    from oracle.binding import LocalChain, LocalTraceGen, ParamFlowSlot, degrade_rule
    K, n = args.resources, args.events
    rng = np.random.default_rng(7)
    base = np.zeros(K, abi.LOCAL_RULE_DTYPE)
    base["flow_grade"] = abi.FLOW_GRADE_NONE
    base["n_breakers"] = 2
    b = np.zeros(2, abi.DEGRADE_RULE_DTYPE)
    b[0] = degrade_rule(abi.DEGRADE_RT, 100, 10, 5, 1000, 0.5)
    b[1] = degrade_rule(abi.DEGRADE_EXCEPTION_RATIO, 0.5, 10, 5, 1000)
    base["breakers"] = b
    kind = np.zeros(K, np.int64)  # 0 plain, 1 origin-limitApp, 2 WarmUp, 3 param rule
    cx = rng.random(K) < 0.10
    kind[cx] = rng.integers(1, 4, int(cx.sum()))
    n_org = int((kind == 1).sum())
    fr = np.zeros(K + n_org, abi.LOCAL_FLOW_RULE_DTYPE)
    fr["resource"][:K] = np.arange(K)
    fr["grade"] = abi.FLOW_GRADE_QPS
    fr["count"][:K] = rng.integers(1, 65, K)
    fr["control_behavior"][:K] = np.where(kind == 2, abi.CONTROL_WARM_UP, abi.CONTROL_DEFAULT)
    fr["limit_app"] = abi.LIMIT_APP_DEFAULT
    fr["strategy"] = abi.STRATEGY_DIRECT
    fr["warm_up_period_sec"] = 10
    fr["max_queueing_ms"] = 500
    fr["ref_resource"] = -1
    fr["cluster_key"] = abi.KEY_NO_RULE
    org_res = np.nonzero(kind == 1)[0]
    fr["resource"][K:] = org_res
    fr["count"][K:] = rng.integers(1, 17, n_org)
    fr["limit_app"][K:] = rng.integers(1, 5, n_org)
    par_res = np.nonzero(kind == 3)[0]
    params = np.zeros(len(par_res), abi.PSLOT_RULE_DTYPE)
    params["resource"] = par_res
    params["param_idx"] = 0
    params["grade"] = abi.FLOW_GRADE_QPS
    params["rule"]["count"] = rng.integers(5, 21, len(par_res))
    params["rule"]["duration_sec"] = 1
    params["rule"]["capacity_log2"] = 11  # exact value table of 2048 slots per rule (1000 values)
    n_vals = 1000
    pargs = np.zeros(n_vals, abi.PSLOT_ARG_DTYPE)
    pargs["value_begin"] = np.arange(n_vals)
    pargs["value_count"] = 1
    pargs["kind"] = abi.ARG_VALUE
    values = np.arange(1, n_vals + 1, dtype=np.uint64)
    vcdf, _ = zipf_cdf(n_vals, 1.1, 8)
    cdf, perm = zipf_cdf(K, 1.0, 7)
    ora = LocalChain(2, 1000, 500)
    ora.load_rules(base)
    kept = ora.load_flow_rules(fr, 4, 0)
    ps = ParamFlowSlot(params, n_resources=K)
    ora.attach_params(ps)
    gen = LocalTraceGen(ora)
    host, wants = [], []
    gen_s = 0.0
    for bt in range(args.warmup + args.steps):
        ent = np.zeros(n, abi.LOCAL_EVENT_DTYPE)
        ent["ts_ms"] = T0 + 1000 * bt + np.sort(rng.integers(0, 1000, n))
        res = perm[np.minimum(np.searchsorted(cdf, rng.random(n), side="right"), K - 1)]
        ent["resource"] = res
        ent["count"] = 1
        og = rng.integers(1, 5, n).astype(np.int32)
        og[(kind[res] != 1) | (rng.random(n) < 0.3)] = 0
        ent["origin"] = og
        ext = np.zeros(n, abi.SLOT_EXT_DTYPE)
        ext["args_null"] = (kind[res] != 3).astype(np.int32)
        ext["arg_begin"] = np.minimum(np.searchsorted(vcdf, rng.random(n), side="right"), n_vals - 1)
        ext["arg_count"] = 1
        rt = np.minimum(np.round(np.exp(rng.normal(2.5, 0.8, n))), 10_000).astype(np.int32)
        err = (rng.random(n) < 0.05).astype(np.uint8)
        t = time.perf_counter()
        ev, xo, want = gen.run_ext(ent, ext, rt, err, T0 + 1000 * (bt + 1), pargs, values)
        gen_s += time.perf_counter() - t
        host.append((ev, xo))
        wants.append(want)
        print(f"# slot trace batch {bt}: {len(ev)} events, {gen_s:.1f} s so far", file=sys.stderr, flush=True)
    print(f"# slot trace: {sum(len(e) for e, _ in host)} events generated by the oracle client model in {gen_s:.1f} s",
          file=sys.stderr)
    eng = FlowEngine(device=0, max_batch=max(len(e) for e, _ in host))
    eng.local_load_rules(base, 2, 1000, 500)
    assert eng.local_load_flow_rules(fr, 4, 0) == kept
    eng.pslot_load_rules(params, n_resources=K)
    d_args = torch.from_numpy(pargs.view(np.uint8).copy()).to(dev)
    d_vals = torch.from_numpy(values.view(np.uint8).copy()).to(dev)
    evs = [torch.from_numpy(e.view(np.uint8).copy()).to(dev) for e, _ in host]
    exs = [torch.from_numpy(x.view(np.uint8).copy()).to(dev) for _, x in host]
    sizes = [len(e) for e, _ in host]
    outs = [torch.empty(sz * 8, dtype=torch.uint8, device=dev) for sz in sizes]
    stream = torch.cuda.current_stream(dev).cuda_stream
    el = timed(lambda i: eng.slot_decide_device(evs[i].data_ptr(), exs[i].data_ptr(), sizes[i], d_args.data_ptr(),
                                                n_vals, d_vals.data_ptr(), n_vals, outs[i].data_ptr(), stream),
               args.warmup, args.steps)
    if int(os.environ.get("SG_DEBUG", "0")) & 64:  # the cx wave walker's counters (local.hip cx_wave), per batch
        d = eng.debug_copy(5, np.uint64, 128).astype(np.int64)
        nb = len(sizes)
        print("# cxw per batch: segments %.0f, wave-ms sum %.2f max %.2f, dead chunks %.0f, general chunks %.0f, "
              "serial entries %.0f exits %.0f, dead-chunk ms %.2f, serial ms %.2f" % (
                  d[20] / nb, d[21] / nb / 1e5, d[22] / 1e5, d[23] / nb, d[24] / nb, d[25] / nb, d[26] / nb,
                  d[27] / nb / 1e5, d[28] / nb / 1e5), file=sys.stderr, flush=True)
        print("# cxw dead-chunk head ms per batch: %.2f" % (d[17] / nb / 1e5), file=sys.stderr, flush=True)
        print("# cxw param dead loop phases ms per batch: prefetch+fixup %.2f, chains %.2f, stores %.2f" % (
            d[12] / nb / 1e5, d[13] / nb / 1e5, d[14] / nb / 1e5), file=sys.stderr, flush=True)
        print("# cxw segments over 5 ms per batch: %.1f; their serial steps %.0f (%.2f ms), dead chunks %.0f" % (
            d[19] / nb, d[29] / nb, d[30] / nb / 1e5, d[31] / nb), file=sys.stderr, flush=True)
        for sl in range(min(12, int(d[18]))):
            o = d[32 + 8 * sl: 40 + 8 * sl]
            print("#   segment: resource %d records %d wave-ms %.2f dead-ms %.2f dead chunks %d serial %d (%.2f ms) "
                  "param rule %d" % (o[0], o[1], o[2] / 1e5, o[3] / 1e5, o[4], o[5], o[6] / 1e5, o[7]),
                  file=sys.stderr, flush=True)
    for i in range(len(sizes)):  # full-size parity of every batch
        got = outs[i].cpu().numpy().view(abi.LOCAL_RES_DTYPE)
        if not np.array_equal(got, wants[i]):
            bad = np.nonzero(got != wants[i])[0]
            raise AssertionError(f"slot batch {i}: {len(bad)} results differ from the oracle (first at {bad[0]})")
    decided = sum(sizes[args.warmup:])
    last = host[-1][0]
    touched = int(np.unique(last["resource"] & 0x7FFFFFFF).size)
    hot = perm[:1000]
    b_alg = sizes[-1] * (32 + 16 + 8) + touched * (2 * 128 + 2 * 2 * 64 + 2 * 128 + 80)  # C5's bytes + the ext
    base_cpu = {"value": sum(sizes) / gen_s, "unit": "decisions/s", "cores": 1, "kind": "port",
                "sample": f"the oracle replaying all {sum(sizes)} events while generating them (client model, 1 thread), "
                          f"{gen_s:.1f} s"}
    return {"metric": "slot-chain decisions/sec (entries + exits), 1M resources, 10 % origin / WarmUp / param rules",
            "workload": "slot: C5 (1M resources, QPS FlowRule + RT + exception-ratio breakers, 16M entries/batch + exits) "
                        "with 10 % of resources carrying an origin-limitApp rule, a WarmUp rule or a ParamFlowRule",
            "value": decided / el, "el": el, "n": decided // args.steps, "b_alg": b_alg, "touched": touched,
            "cpu": base_cpu,
            "extra": {"cx_resources": int(cx.sum()), "cx_among_hottest_1000": int(cx[hot].sum()),
                      "cx_share_of_entries": float(np.isin(last["resource"] & 0x7FFFFFFF,
                                                            np.nonzero(cx)[0])[last["kind"] == 0].mean()),
                      "parity": "every batch equal to the oracle"},
            "data": "synthetic (seeded): Zipf(1.0) resources, rt lognormal(2.5, 0.8) ms, 5% errors; exits generated by "
                    "the oracle client model"}


def codec(args, dev):
    """Token-server step from the wire: 16M MSG_TYPE_FLOW frames (the C3 traffic, 1M flowIds, Zipf 1.0)
    → sg_codec_decode_flow → sg_flow_decide_batch → sg_codec_encode_flow, all resident in HBM."""
    import bench
    from sentinel_amd.engine import FlowEngine
    n = args.events
    wl = bench.ShardWorkload(args.resources, n, 0, 1, dev)
    fid_t = torch.from_numpy(wl.rules["flow_id"].astype(np.int64)).to(dev)
    FB = 18  # [i32 xid][u8 type][i64 flowId][i32 count][bool prio]

    def be(x, nbytes):  # int64 tensor → big-endian bytes [n, nbytes]
        return torch.stack([(x >> (8 * (nbytes - 1 - j))) & 0xFF for j in range(nbytes)], dim=1).to(torch.uint8)

    def frames(b):
        req = wl.batch(b).view(torch.int64).reshape(-1, 2)
        ts, kw = req[:, 0].contiguous(), req[:, 1]
        key, acq = kw & 0x7FFFFFFF, (kw >> 32) & 0xFFFFFFFF
        prio = (kw >> 31) & 1
        xid = torch.arange(n, device=dev, dtype=torch.int64) + b * n
        pay = torch.cat([be(xid, 4), torch.ones((n, 1), dtype=torch.uint8, device=dev), be(fid_t[key], 8),
                         be(acq, 4), prio.to(torch.uint8).reshape(-1, 1)], dim=1).reshape(-1).contiguous()
        return pay, ts

    eng = FlowEngine(device=0, max_batch=n)
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"] = 1
    ns["max_allowed_qps"] = 30000
    eng.set_namespaces(ns)
    eng.load_rules(wl.rules)
    batches = [frames(b) for b in range(args.warmup + args.steps)]
    offsets = (torch.arange(n + 1, device=dev, dtype=torch.int64) * FB).to(torch.int32)
    req = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    xid = torch.empty(n * 4, dtype=torch.uint8, device=dev)
    kind = torch.empty(n, dtype=torch.uint8, device=dev)
    res = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    out = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_codec = [0.0, 0.0]

    def step(b, timed_codec=False):
        pay, ts = batches[b]
        ev[0].record(stream)
        eng.codec_decode(pay.data_ptr(), offsets.data_ptr(), ts.data_ptr(), n, req.data_ptr(), xid.data_ptr(),
                         kind.data_ptr(), s)
        ev[1].record(stream)
        eng.decide_device(req.data_ptr(), n, res.data_ptr(), s)
        ev[2].record(stream)
        eng.codec_encode(xid.data_ptr(), kind.data_ptr(), res.data_ptr(), n, out.data_ptr(), s)
        ev[3].record(stream)
        if timed_codec:
            ev[3].synchronize()
            t_codec[0] += ev[0].elapsed_time(ev[1])
            t_codec[1] += ev[2].elapsed_time(ev[3])

    el = timed(lambda b: step(b, b >= args.warmup), args.warmup, args.steps)
    dec_ms, enc_ms = t_codec[0] / args.steps, t_codec[1] / args.steps
    dec_b, enc_b = n * (FB + 4 + 8 + 16 + 4 + 1), n * (4 + 1 + 12 + 16)
    touched = int(torch.unique(batches[-1][0].reshape(-1, FB)[:, 5:13].contiguous().view(torch.int64)).numel())
    b_alg = n * (FB + 4 + 16) + touched * (bench.STATE_B + bench.RULE_B)  # frames in/out + the C3 state
    base = None
    if not args.no_cpu_baseline:
        from oracle import binding
        from oracle.binding import ClusterTokenService
        m = min(args.cpu_events, n)
        pay, ts = batches[0]
        pay_h = pay[: m * FB].cpu().numpy()
        off_h = np.arange(m + 1, dtype=np.uint32) * FB
        ts_h = ts[:m].cpu().numpy()
        ora = ClusterTokenService()
        ora.set_namespaces(ns)
        ora.load_rules(wl.rules)
        t = time.perf_counter()
        r_h, x_h, k_h = binding.codec_decode_flow(pay_h, off_h, ts_h, wl.rules["flow_id"])
        binding.codec_encode_flow(x_h, k_h, ora.decide(r_h))
        dt = time.perf_counter() - t
        base = {"value": m / dt, "unit": "frames/s", "cores": 1, "kind": "port",
                "sample": f"first {m} frames of batch 0 through the oracle codec + ClusterTokenService (1 thread), {dt:.1f} s"}
    return {"metric": "token-server frames/sec (decode + decide + encode), 1M flowIds",
            "workload": "C3 traffic as MSG_TYPE_FLOW frames: sg_codec_decode_flow -> sg_flow_decide_batch -> "
                        "sg_codec_encode_flow, 16M frames per 1000 ms batch",
            "value": n * args.steps / el, "el": el, "n": n, "b_alg": b_alg, "touched": touched, "cpu": base,
            "unit": "frames/s", "dtype": "u8",
            "extra": {"codec_kernels": {"decode_ms": dec_ms, "encode_ms": enc_ms,
                                        "decode_gbs": dec_b / dec_ms / 1e6, "encode_gbs": enc_b / enc_ms / 1e6,
                                        "decode_frac": dec_b / dec_ms / 1e6 / HBM_PEAK_GBS,
                                        "encode_frac": enc_b / enc_ms / 1e6 / HBM_PEAK_GBS,
                                        "bytes_per_frame": {"decode": dec_b // n, "encode": enc_b // n}}},
            "data": "synthetic (GPU-generated, seeded): the bench.py C3 trace encoded as big-endian flow frames"}


def pace(args, dev):
    K, n = args.resources, args.events
    rng = np.random.default_rng(6)
    rules = np.zeros(K, abi.PACE_RULE_DTYPE)
    rules["count"] = rng.integers(1, 65, K).astype(np.float64)
    rules["max_queueing_ms"] = 500
    cdf, perm = zipf_cdf(K, 1.0, 6)
    cdf_t, perm_t = torch.from_numpy(cdf).to(dev), torch.from_numpy(perm.astype(np.int64)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(6)

    def batch(b):
        w = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        w[:, 0] = torch.sort(torch.randint(0, 1000, (n,), generator=gen, device=dev)).values + T0 + 1000 * b
        acq = torch.where(torch.rand(n, generator=gen, device=dev) < 0.1,
                          torch.randint(2, 5, (n,), generator=gen, device=dev), torch.ones(n, dtype=torch.int64, device=dev))
        w[:, 1] = gpu_keys(cdf_t, perm_t, n, gen) | (acq << 32)       # rule | acquireCount << 32
        return w.view(torch.uint8).reshape(-1)

    eng = FlowEngine(device=0, max_batch=n)
    eng.pace_load_rules(rules)
    batches = [batch(b) for b in range(args.warmup + args.steps)]
    out = torch.empty(n * 4, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    el = timed(lambda b: eng.pace_decide_device(batches[b].data_ptr(), n, out.data_ptr(), stream), args.warmup, args.steps)
    touched = int(torch.unique(batches[-1].view(torch.int64).reshape(-1, 2)[:, 1] & 0xFFFFFFFF).numel())
    b_alg = n * (16 + 4) + touched * (16 + 2 * 8)   # request in, wait out; per rule: rule 16 B, latest read + write
    base = None
    if not args.no_cpu_baseline:
        from oracle.binding import RateLimiterController
        req = batches[0].view(torch.int64).reshape(-1, 2)[: args.cpu_events].cpu().numpy().copy().view(abi.PACE_REQ_DTYPE).reshape(-1)
        ora = RateLimiterController(rules)
        t = time.perf_counter()
        ora.decide(req)
        dt = time.perf_counter() - t
        base = {"value": len(req) / dt, "unit": "decisions/s", "cores": 1, "kind": "port",
                "sample": f"first {len(req)} requests of batch 0 through oracle RateLimiterController (1 thread), {dt:.1f} s"}
    return {"metric": "pace decisions/sec (RateLimiterController.canPass), 1M rate-limited resources",
            "workload": "pace: 1M RATE_LIMITER FlowRules count U{1..64} maxQueueing 500 ms, 16M canPass/batch",
            "value": n * args.steps / el, "el": el, "n": n, "b_alg": b_alg, "touched": touched, "cpu": base,
            "data": "synthetic (GPU-generated, seeded): Zipf(1.0) resources, 10% acquire U{2..4}"}


def cparam(args, dev):
    """Cluster hot-parameter tokens: 1000 ClusterParamFlowRules (GLOBAL, count U{1..40}, S=10 / 1000 ms), rules
    Zipf(1.0), each rule's values Zipf(1.1) over 50k distinct u64, 16M requests per 1000 ms batch, 10 % of them
    carrying 2-3 values (all-or-nothing)."""
    R, n, V = 1000, args.events, 50_000
    rng = np.random.default_rng(7)
    rules = np.zeros(R, abi.CPARAM_RULE_DTYPE)
    rules["flow_id"] = np.arange(R) + 1
    rules["count"] = rng.integers(1, 41, R)
    rules["threshold_type"] = abi.THRESHOLD_GLOBAL
    rules["sample_count"], rules["window_interval_ms"] = 10, 1000
    if args.chain:
        rules["count"][0] = 1
    rcdf, rperm = zipf_cdf(R, 1.0, 7)
    vcdf, vperm = zipf_cdf(V, 1.1, 8)
    rcdf_t, rperm_t = torch.from_numpy(rcdf).to(dev), torch.from_numpy(rperm.astype(np.int64)).to(dev)
    vcdf_t, vperm_t = torch.from_numpy(vcdf).to(dev), torch.from_numpy(vperm.astype(np.int64)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(7)

    def batch(b):
        w = torch.zeros((n, 3), dtype=torch.int64, device=dev)
        w[:, 0] = torch.sort(torch.randint(0, 1000, (n,), generator=gen, device=dev)).values + T0 + 1000 * b
        key = gpu_keys(rcdf_t, rperm_t, n, gen)
        cnt = torch.where(torch.rand(n, generator=gen, device=dev) < 0.1,
                          torch.randint(2, 4, (n,), generator=gen, device=dev), torch.ones(n, dtype=torch.int64, device=dev))
        if args.chain:  # chain link k at request k * n / L: rule 0 (threshold 1), values (c_k, c_k+1)
            ci = torch.arange(args.chain, device=dev) * (n // args.chain)
            key[ci] = 0
            cnt[ci] = 2
        begin = torch.cumsum(cnt, 0) - cnt
        w[:, 1] = key | (1 << 32)                     # key, acquireCount 1
        w[:, 2] = begin | (cnt << 32)                 # value_begin, value_count
        nv = int(cnt.sum())
        owner = torch.repeat_interleave(key, cnt)
        vals = gpu_keys(vcdf_t, vperm_t, nv, gen) * 0x9E3779B1 + owner * 0x85EBCA77 + 11
        if args.chain:
            c = (0x5C4A << 48) + b * (args.chain + 1) + torch.arange(args.chain + 1, device=dev)
            vals[begin[ci]] = c[:-1]
            vals[begin[ci] + 1] = c[1:]
        return w.view(torch.uint8).reshape(-1), vals, nv

    batches = [batch(b) for b in range(args.warmup + args.steps)]
    max_nv = max(x[2] for x in batches)
    G = args.shards  # --shards G: the node handle's sharded param path (sg_node_cparam_*), G shards on this GPU
    if G:
        from sentinel_amd.engine import NodeEngine
        eng = NodeEngine([0] * G, max_batch=max(n, max_nv))
    else:
        eng = FlowEngine(device=0, max_batch=max(n, max_nv))
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"] = 1
    eng.set_namespaces(ns)
    eng.cparam_load_rules(rules, None, 17)
    out = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rounds = []

    def step(b):
        req, vals, nv = batches[b]
        eng.cparam_decide_device(req.data_ptr(), n, vals.data_ptr(), nv, out.data_ptr(), stream)
        if not G:
            rounds.append(eng.cparam_last_rounds())

    el = timed(step, args.warmup, args.steps)
    req_l, vals_l, nv_l = batches[-1]
    keys_l = torch.repeat_interleave(req_l.view(torch.int64).reshape(-1, 3)[:, 1] & 0xFFFFFFFF,
                                     (req_l.view(torch.int64).reshape(-1, 3)[:, 2] >> 32))
    touched = int(torch.unique(keys_l * 1_000_003 + vals_l).numel())
    # per request 24 B in + 12 B out; per value 8 B; per touched (rule, value) slot: key 8 B + ring S x 16 B read
    # and written once
    b_alg = n * (24 + 12) + nv_l * 8 + touched * (8 + 2 * 10 * 16)
    base = None
    if not args.no_cpu_baseline:
        from oracle.binding import ClusterTokenService
        m = min(args.cpu_events, n)
        req0, vals0, _ = batches[0]
        req_h = req0.view(torch.int64).reshape(-1, 3)[:m].cpu().numpy().copy().view(abi.CPARAM_REQ_DTYPE).reshape(-1)
        end = int(req_h["value_begin"][-1]) + int(req_h["value_count"][-1])
        vals_h = vals0[:end].cpu().numpy().astype(np.uint64)
        ora = ClusterTokenService()
        ora.set_namespaces(ns)
        ora.load_param_rules(rules)
        t = time.perf_counter()
        ora.decide_param(req_h, vals_h)
        dt = time.perf_counter() - t
        base = {"value": m / dt, "unit": "decisions/s", "cores": 1, "kind": "port",
                "sample": f"first {m} requests of batch 0 through oracle ClusterTokenService.decide_param (1 thread), "
                          f"{dt:.1f} s"}
    return {"metric": "cluster hot-parameter token decisions/sec (ClusterParamFlowChecker), 1000 param rules"
                      + (f", node handle with {G} shards on one GPU (routing inside)" if G else ""),
            "workload": "cparam: 1000 ClusterParamFlowRules x 50k values Zipf(1.1), 16M requests/batch, 10% multi-value"
                        + (f", a {args.chain}-deep two-value dependency chain per batch (rule 0, threshold 1)" if args.chain else "")
                        + (f", sg_node_cparam_decide_batch over {G} same-device shards" if G else ""),
            "value": n * args.steps / el, "el": el, "n": n, "b_alg": b_alg, "touched": touched, "cpu": base,
            "extra": {"fixed_point_rounds": rounds[args.warmup:], "values_per_step": nv_l, "shards": G},
            "data": "synthetic (GPU-generated, seeded): rules Zipf(1.0), values Zipf(1.1) per rule, 10% 2-3 values"}


def node(args, dev):
    """The node handle (sg_node_*) on one GPU: the C3 workload (1M flowIds, 16M requests per 1000 ms batch) decided
    by G same-device shard handles with the routing inside the library — validation and the namespace limiters on the
    front handle, the stable multisplit by splitmix64(flowId) mod G, every shard's sort and walkers — through the node
    pipeline (sg_node_flow_enqueue: the front's part of batch i+1 and the shards' sorts beside the shards' walkers of
    batch i, at most two batches in flight), against one handle's pipeline (sg_flow_enqueue) on the same batches;
    --local-sync: both synchronous (sg_node_flow_decide_batch / sg_flow_decide_batch)."""
    import bench
    from sentinel_amd.engine import NodeEngine
    G = args.shards or 2
    wl = bench.ShardWorkload(1_000_000, args.events, 0, 1, dev)
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"] = 1
    nd = NodeEngine([0] * G, max_batch=args.events)
    nd.set_namespaces(ns)
    nd.load_rules(wl.rules)
    one = FlowEngine(device=0, max_batch=args.events)
    one.set_namespaces(ns)
    one.load_rules(wl.rules)
    batches = [wl.batch(b) for b in range(args.warmup + args.steps)]
    outs = [torch.empty(args.events * 12, dtype=torch.uint8, device=dev) for _ in range(2)]
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run(eng, bs, sync):
        if sync:
            return timed(lambda b: eng.decide_device(bs[b].data_ptr(), args.events, outs[0].data_ptr(), stream),
                         args.warmup, args.steps)
        tickets = []

        def step(b):
            if len(tickets) >= 2:
                eng.wait(tickets.pop(0))
            tickets.append(eng.enqueue_device(bs[b].data_ptr(), args.events, outs[b % 2].data_ptr()))
        torch.cuda.synchronize()
        el = timed(step, args.warmup, args.steps)
        for t in tickets:
            eng.wait(t)
        return el

    el = run(nd, batches, args.local_sync)
    # the single handle on the same batches, later in time (each batch shifted past the node's last)
    later = [b.clone() for b in batches]
    for x in later:
        x.view(torch.int64).view(-1, 2)[:, 0] += 1000 * (args.warmup + args.steps)
    el1 = run(one, later, args.local_sync)
    n = args.events
    keys = batches[-1].view(torch.int64).view(-1, 2)[:, 1] & 0x7FFFFFFF
    touched = int(torch.unique(keys).numel())
    b_alg = n * (bench.REQ_B + bench.RES_B) + touched * (bench.STATE_B + bench.RULE_B)  # bench.py's C3 bytes
    mode = "synchronous" if args.local_sync else "pipelined"
    return {"metric": f"flow decisions/sec through the node handle, {G} shards on one GPU (routing inside)",
            "workload": f"C3 workload (1M flowIds, 16M requests/batch, Zipf 1.0) on sg_node with {G} same-device "
                        f"shards, {mode} node batches",
            "value": n * args.steps / el, "el": el, "n": n, "b_alg": b_alg, "touched": touched, "cpu": None,
            "extra": {"shards": G, "mode": mode, "single_handle_ms_per_step": el1 / args.steps * 1e3,
                      "single_handle_decisions_per_s": n * args.steps / el1,
                      "node_over_single": el / el1},
            "data": "synthetic (GPU-generated, seeded): bench.py's C3 batches"}


def gateway(args, dev):
    """GatewayFlowSlot from the adapter's side: --resources routes, each with 3 item rules (client IP with no pattern, a
    header with an EXACT pattern, a URL parameter with a CONTAINS pattern) and one item-less rule; --events requests per
    1000 ms batch with Zipf(1.0) routes and Zipf(1.1) client IPs. Timed: sg_gateway_parse_batch alone, and parse +
    sg_slot_decide_batch over the arg spans the parser wrote into the ext records."""
    K, n = args.resources, args.events
    n_clients = min(1 << 20, max(1024, n // 4))
    L = (12, 8, 12)                   # bytes of the client IP, the header value and the URL parameter
    stride = sum(L)
    g = np.zeros(4 * K, abi.GATEWAY_RULE_DTYPE)
    g["resource"] = np.repeat(np.arange(K, dtype=np.uint32), 4)
    g["grade"], g["interval_sec"], g["max_queueing_timeout_ms"], g["pattern_null"] = 1, 1, 500, 1
    g["capacity_log2"] = 10
    res_cdf, res_perm = zipf_cdf(K, 1.0, 31)
    # the client-IP rule's table holds every client the route sees: sized from the route's share of the traffic
    share = np.diff(res_cdf, prepend=0.0)
    seen = np.minimum(n_clients, share * n * (args.warmup + args.steps) * 2.0)
    cap = np.zeros(K, np.int32)
    cap[res_perm] = np.maximum(10, np.ceil(np.log2(np.maximum(seen, 1.0))).astype(np.int32) + 1)
    pat = b"tier-vipid=7"
    ip, hdr, url, dflt = g[0::4], g[1::4], g[2::4], g[3::4]
    ip["has_item"], ip["parse_strategy"], ip["count"] = 1, abi.GW_PARSE_CLIENT_IP, 5
    ip["capacity_log2"] = cap
    hdr["has_item"], hdr["parse_strategy"], hdr["match_strategy"], hdr["count"] = 1, abi.GW_PARSE_HEADER, abi.GW_MATCH_EXACT, 50
    hdr["pattern_null"], hdr["pattern_off"], hdr["pattern_len"] = 0, 0, 8
    url["has_item"], url["parse_strategy"], url["match_strategy"], url["count"] = 1, abi.GW_PARSE_URL_PARAM, abi.GW_MATCH_CONTAINS, 20
    url["pattern_null"], url["pattern_off"], url["pattern_len"] = 0, 8, 4
    dflt["count"] = 200
    eng = FlowEngine(device=0, max_batch=2 * n)
    eng.vdict_init(max(12, int(np.ceil(np.log2(n_clients + 4096))) + 1), max(64 << 20, n_clients * 24), 8 * n)
    eng.local_load_rules(_gateway_local_rules(K), 2, 1000, 500)
    eng.gateway_load_rules(g, pat, K)
    ip_cdf, ip_perm = zipf_cdf(n_clients, 1.1, 32)
    res_cdf_t, res_perm_t = torch.from_numpy(res_cdf).to(dev), torch.from_numpy(res_perm).to(dev)
    ip_cdf_t, ip_perm_t = torch.from_numpy(ip_cdf).to(dev), torch.from_numpy(ip_perm).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(33)
    hexd = torch.tensor(list(b"0123456789abcdef"), dtype=torch.uint8, device=dev)

    def text(prefix, x, digits):      # prefix + `digits` hex digits of x, [n, len(prefix) + digits] bytes
        cols = [torch.full((n,), c, dtype=torch.uint8, device=dev) for c in prefix]
        cols += [hexd[(x >> (4 * (digits - 1 - j))) & 15] for j in range(digits)]
        return torch.stack(cols, dim=1)

    def entries(b):                   # (route, [n, stride] string bytes, sorted arrival ms)
        route = gpu_keys(res_cdf_t, res_perm_t, n, gen)
        client = gpu_keys(ip_cdf_t, ip_perm_t, n, gen)
        u = torch.rand(n, generator=gen, device=dev)
        tier = torch.where(u < 0.2, torch.zeros_like(route), 1 + (u * 64).long() % 5)
        v = torch.randint(0, 16, (n,), generator=gen, device=dev)
        hdr_b = text(b"tier-", tier + 0xAAA, 3)
        hdr_b[tier == 0] = torch.tensor(list(b"tier-vip"), dtype=torch.uint8, device=dev)
        rows = torch.cat([text(b"10.c", client, 8), hdr_b, text(b"a=1&id=", (((v & 3) + 5) << 16) | v, 5)], dim=1)
        ts = T0 + b * 1000 + torch.sort(torch.randint(0, 1000, (n,), generator=gen, device=dev)).values
        return route, rows.contiguous(), ts

    def records(route, m):            # sg_gateway_req[m]: request i owns items [3i, 3i + 3)
        req = torch.zeros((m, 4), dtype=torch.int32, device=dev)
        req[:, 0], req[:, 2], req[:, 3] = route.int(), torch.arange(m, device=dev, dtype=torch.int32) * 3, 3
        return req.reshape(-1).contiguous()

    N2 = 2 * n                        # a step of the chain: the exits of the last step's passed entries, then n entries
    off = torch.arange(N2, device=dev, dtype=torch.int64) * stride
    items = torch.zeros((N2, 3, 4), dtype=torch.int32, device=dev)
    items[:, 0, 0], items[:, 1, 0], items[:, 2, 0] = off.int(), (off + L[0]).int(), (off + L[0] + L[1]).int()
    items[:, 0, 1], items[:, 1, 1], items[:, 2, 1] = L
    items = items.reshape(-1).contiguous()
    batches = [entries(b) for b in range(args.warmup + args.steps)]
    reqs = [records(route, n) for route, _, _ in batches]
    a_t = torch.empty(4 * N2 * 16, dtype=torch.uint8, device=dev)
    v_t = torch.empty(4 * N2 * 8, dtype=torch.uint8, device=dev)
    ext = torch.zeros(N2 * 16, dtype=torch.uint8, device=dev)
    out = torch.empty(N2 * 8, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def parse(req, rows, m):
        return eng.gateway_parse_device(req.data_ptr(), m, items.data_ptr(), 3 * m, rows.data_ptr(), stride * m,
                                        a_t.data_ptr(), 4 * N2, v_t.data_ptr(), 4 * N2, ext.data_ptr(), 0, s)

    # the parse step alone over every batch first: it fills the dictionary as the timed steps then find it (steady state:
    # known clients; the first sight of a client is the dedupe / commit passes' work)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(args.warmup + args.steps):
        n_args, n_values = parse(reqs[b], batches[b][1], n)
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1000.0 / (args.warmup + args.steps)
    el_parse = timed(lambda b: parse(reqs[b], batches[b][1], n), args.warmup, args.steps)
    strings, _ = eng.vdict_size()

    # parse + the slot chain: every step parses and decides the exits of the last step's passed entries (an exit carries
    # its entry's request: ParamFlowStatisticExitCallback lowers the thread counts of the same args) and nc new entries.
    # The chain's thread-count table has 2^20 slots for every (route, paramIdx, value) in flight, so a step takes at
    # most 2^18 entries, and the counts that returned to 0 are swept between the steps (outside the timed region).
    nc = min(n, 1 << 18)
    chain = {"ms": None, "requests_per_step": None, "error": None}
    try:
        el, served, prev = 0.0, 0, None
        for b in range(args.warmup + args.steps):
            route, rows, ts = batches[b][0][:nc], batches[b][1][:nc], batches[b][2][:nc]
            entry_route, entry_rows = route, rows
            x = 0 if prev is None else len(prev[0])
            if x:
                eng.param_sweep(T0 + b * 1000)
                route, rows = torch.cat([prev[0], route]), torch.cat([prev[1], rows]).contiguous()
            m = x + nc
            ev = torch.zeros((m, 4), dtype=torch.int64, device=dev)   # sg_local_event: ts, create_ts, resource | count, kind | origin
            ev[:, 2] = route | (1 << 32)
            ev[x:, 0] = ts
            if x:
                ev[:x, 0], ev[:x, 1], ev[:x, 3] = T0 + b * 1000, prev[2], abi.LOCAL_EXIT
            req = records(route, m)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            na, nv = parse(req, rows, m)
            eng.slot_decide_device(ev.data_ptr(), ext.data_ptr(), m, a_t.data_ptr(), na, v_t.data_ptr(), nv,
                                   out.data_ptr(), s)
            torch.cuda.synchronize()
            if b >= args.warmup:
                el += time.perf_counter() - t0
                served += m
            status = out[: m * 8].view(torch.int32)[0::2][x:]
            ok = (status == abi.LOCAL_PASS) | (status == abi.LOCAL_PASS_WAIT)
            prev = (entry_route[ok], entry_rows[ok], ts[ok])
        chain = {"ms": el * 1000.0 / args.steps, "requests_per_step": served / args.steps, "error": None}
    except Exception as e:  # the parse figures stand on their own
        chain["error"] = str(e)
        el, served = el_parse, n * args.steps
    b_alg = n * 16 + 3 * n * 16 + stride * n + n_args * 16 + n_values * 8 + n * 16
    return {"metric": "gateway requests/sec (GatewayParamParser on the device + the whole slot chain)",
            "workload": f"gateway: {K} routes x (client IP, EXACT header, CONTAINS URL parameter, item-less) rules, "
                        f"{n} requests per parse batch; chain steps of {nc} entries plus the exits of the passed ones, "
                        f"Zipf(1.0) routes, "
                        f"Zipf(1.1) over {n_clients} client IPs",
            "value": served / el, "el": el, "n": n, "b_alg": b_alg, "touched": strings, "cpu": None,
            "unit": "requests/s", "dtype": "u8",
            "extra": {"gateway": {"parse_ms": el_parse * 1000.0 / args.steps, "parse_first_sight_ms": first_ms,
                                  "parse_requests_per_s": n * args.steps / el_parse,
                                  "parse_items_per_s": 3 * n * args.steps / el_parse,
                                  "parse_decide_ms": chain["ms"], "parse_decide_requests_per_step": chain["requests_per_step"],
                                  "parse_decide_requests_per_s": served / el if chain["ms"] else None,
                                  "parse_decide_error": chain["error"],
                                  "algorithmic_bytes": {"requests": n * 16, "items": 3 * n * 16, "strings": stride * n,
                                                        "args": n_args * 16, "values": n_values * 8, "ext": n * 16},
                                  "dictionary_strings": strings}},
            "data": "synthetic (GPU-generated, seeded): fixed-width client IP, header and URL parameter strings"}


def gateway_api(args, dev):
    """The gateway workload from the HTTP request on: --resources routes with the gateway workload's four rules each, and
    A = max(16, --resources / 4) custom APIs, even ones defined by an exact path, odd ones by /x<id>/**, each with a
    URL-parameter rule and an item-less rule. A request has a route (Zipf 1.0), a 16-byte path (40 % the exact path of a
    Zipf(1.0) API, 40 % under an Ant API's prefix, 20 % matching nothing) and three fields (client IP, header, URL
    parameter). Timed: sg_gateway_expand_batch alone; sg_gateway_parse_batch alone over the expansion; and expand + parse
    + sg_slot_decide_batch on steps of at most 2^16 requests (entries only: no exits, so the step stays small)."""
    K, n = args.resources, args.events
    A = max(16, K // 4)
    n_clients = min(1 << 20, max(1024, n // 4))
    L = (12, 8, 12)                   # bytes of the client IP, the header value and the URL parameter
    stride, P = sum(L), 16            # field bytes and path bytes per request
    HDR, UID = 1, 2                   # the caller's field name ids
    g = np.zeros(4 * K + 2 * A, abi.GATEWAY_RULE_DTYPE)
    g["grade"], g["interval_sec"], g["max_queueing_timeout_ms"], g["pattern_null"] = 1, 1, 500, 1
    g["capacity_log2"] = 10
    g["resource"][:4 * K] = np.repeat(np.arange(K, dtype=np.uint32), 4)
    g["resource"][4 * K:] = K + np.repeat(np.arange(A, dtype=np.uint32), 2)
    field_id = np.zeros(len(g), np.uint32)
    pat = b"tier-vipid=7"
    r4 = g[:4 * K]
    ip, hdr, url, dflt = r4[0::4], r4[1::4], r4[2::4], r4[3::4]
    ip["has_item"], ip["parse_strategy"], ip["count"] = 1, abi.GW_PARSE_CLIENT_IP, 5
    # the client-IP rule's table holds every client the route sees in the chain steps
    res_cdf, res_perm = zipf_cdf(K, 1.0, 31)
    nc = min(n, 1 << 16)
    seen = np.minimum(n_clients, np.diff(res_cdf, prepend=0.0) * nc * (args.warmup + args.steps) * 2.0)
    cap = np.zeros(K, np.int32)
    cap[res_perm] = np.maximum(10, np.ceil(np.log2(np.maximum(seen, 1.0))).astype(np.int32) + 1)
    ip["capacity_log2"] = cap
    hdr["has_item"], hdr["parse_strategy"], hdr["match_strategy"], hdr["count"] = 1, abi.GW_PARSE_HEADER, abi.GW_MATCH_EXACT, 50
    hdr["pattern_null"], hdr["pattern_off"], hdr["pattern_len"] = 0, 0, 8
    url["has_item"], url["parse_strategy"], url["match_strategy"], url["count"] = 1, abi.GW_PARSE_URL_PARAM, abi.GW_MATCH_CONTAINS, 20
    url["pattern_null"], url["pattern_off"], url["pattern_len"] = 0, 8, 4
    dflt["count"] = 200
    field_id[1:4 * K:4], field_id[2:4 * K:4] = HDR, UID
    a_url, a_dflt = g[4 * K::2], g[4 * K + 1::2]
    a_url["resource_mode"], a_dflt["resource_mode"] = 1, 1
    a_url["has_item"], a_url["parse_strategy"], a_url["count"] = 1, abi.GW_PARSE_URL_PARAM, 30
    a_dflt["count"] = 400
    field_id[4 * K::2] = UID
    # definitions: API a is resource K + a; one predicate each, the pattern 16 bytes
    apis = np.zeros(A, abi.GATEWAY_API_DTYPE)
    apis["resource"], apis["pred_begin"], apis["pred_count"] = K + np.arange(A), np.arange(A), 1
    preds = np.zeros(A, abi.GATEWAY_API_PRED_DTYPE)
    names = [b"/exact/%09x" % a if a % 2 == 0 else b"/x%08x/**" % a for a in range(A)]
    preds["match_strategy"] = [abi.GW_URL_MATCH_EXACT if a % 2 == 0 else abi.GW_URL_MATCH_PREFIX for a in range(A)]
    preds["pattern_len"] = [len(x) for x in names]
    preds["pattern_off"] = np.concatenate([[0], np.cumsum(preds["pattern_len"])[:-1]])
    R = K + A
    eng = FlowEngine(device=0, max_batch=2 * n)
    eng.vdict_init(max(12, int(np.ceil(np.log2(n_clients + 4096))) + 1), max(64 << 20, n_clients * 24), 8 * n)
    eng.local_load_rules(_gateway_local_rules(R), 2, 1000, 500)
    eng.gateway_load_apis(apis, preds, b"".join(names), R, 0)
    eng.gateway_load_rules(g, pat, R)
    eng.gateway_set_item_fields(field_id)
    api_cdf, api_perm = zipf_cdf(A // 2, 1.0, 34)
    ip_cdf, ip_perm = zipf_cdf(n_clients, 1.1, 32)
    to = lambda x: torch.from_numpy(x).to(dev)
    res_cdf_t, res_perm_t, api_cdf_t, api_perm_t = to(res_cdf), to(res_perm), to(api_cdf), to(api_perm)
    ip_cdf_t, ip_perm_t = to(ip_cdf), to(ip_perm)
    gen = torch.Generator(device=dev)
    gen.manual_seed(35)
    hexd = torch.tensor(list(b"0123456789abcdef"), dtype=torch.uint8, device=dev)

    def text(prefix, x, digits, suffix=b""):
        cols = [torch.full((n,), c, dtype=torch.uint8, device=dev) for c in prefix]
        cols += [hexd[(x >> (4 * (digits - 1 - j))) & 15] for j in range(digits)]
        cols += [torch.full((n,), c, dtype=torch.uint8, device=dev) for c in suffix]
        return torch.stack(cols, dim=1)

    fields = torch.zeros((n, 3, 4), dtype=torch.int32, device=dev)      # sg_gateway_field: kind, name_id, off, len
    base = (n * P + torch.arange(n, device=dev, dtype=torch.int64) * stride)
    fields[:, 0, 0], fields[:, 1, 0], fields[:, 2, 0] = abi.GW_PARSE_CLIENT_IP, abi.GW_PARSE_HEADER, abi.GW_PARSE_URL_PARAM
    fields[:, 1, 1], fields[:, 2, 1] = HDR, UID
    fields[:, 0, 2], fields[:, 1, 2], fields[:, 2, 2] = base.int(), (base + L[0]).int(), (base + L[0] + L[1]).int()
    fields[:, 0, 3], fields[:, 1, 3], fields[:, 2, 3] = L
    fields = fields.reshape(-1).contiguous()

    def batch(b):                     # (sg_gateway_http_req[n] as int32 words, the blob: n paths then n field rows)
        route = gpu_keys(res_cdf_t, res_perm_t, n, gen)
        api = gpu_keys(api_cdf_t, api_perm_t, n, gen)
        client = gpu_keys(ip_cdf_t, ip_perm_t, n, gen)
        u = torch.rand(n, generator=gen, device=dev)
        w = torch.rand(n, generator=gen, device=dev)
        tier = torch.where(u < 0.2, torch.zeros_like(route), 1 + (u * 64).long() % 5)
        v = torch.randint(0, 16, (n,), generator=gen, device=dev)
        hdr_b = text(b"tier-", tier + 0xAAA, 3)
        hdr_b[tier == 0] = torch.tensor(list(b"tier-vip"), dtype=torch.uint8, device=dev)
        rows = torch.cat([text(b"10.c", client, 8), hdr_b, text(b"a=1&id=", (((v & 3) + 5) << 16) | v, 5)], dim=1)
        path = text(b"/none/", client, 10)
        path = torch.where((w < 0.4)[:, None], text(b"/exact/", 2 * api, 9), path)
        path = torch.where(((w >= 0.4) & (w < 0.8))[:, None], text(b"/x", 2 * api + 1, 8, b"/items"), path)
        blob = torch.cat([path.reshape(-1), rows.reshape(-1)]).contiguous()
        ts = T0 + b * 1000 + torch.sort(torch.randint(0, 1000, (n,), generator=gen, device=dev)).values
        q = torch.zeros((n, 12), dtype=torch.int32, device=dev)
        q[:, 0:2] = ts.view(torch.int32).view(n, 2)
        q[:, 2] = route.int()
        i = torch.arange(n, device=dev, dtype=torch.int32)
        q[:, 5], q[:, 6], q[:, 7], q[:, 8] = i * P, P, i * 3, 3
        return q.reshape(-1).contiguous(), blob

    batches = [batch(b) for b in range(args.warmup + args.steps)]
    nbytes = n * (P + stride)
    verd = torch.zeros(4, dtype=torch.int32, device=dev)
    E, I = 2 * n, 4 * n                # a request makes at most two entries: three route items and one API item
    req_o = torch.empty(E * 16, dtype=torch.uint8, device=dev)
    items_o = torch.empty(I * 16, dtype=torch.uint8, device=dev)
    src_o = torch.empty(E * 4, dtype=torch.uint8, device=dev)
    ev_o = torch.empty(E * 32, dtype=torch.uint8, device=dev)
    ext_o = torch.zeros(E * 16, dtype=torch.uint8, device=dev)
    a_t = torch.empty((I + E) * 16, dtype=torch.uint8, device=dev)
    v_t = torch.empty((I + E) * 8, dtype=torch.uint8, device=dev)
    out = torch.empty(E * 8, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def expand(b, m):                 # the first m requests of batch b
        q, blob = batches[b]
        return eng.gateway_expand_device(q.data_ptr(), m, fields.data_ptr(), 3 * n, verd.data_ptr(), 0, blob.data_ptr(),
                                         nbytes, req_o.data_ptr(), E, items_o.data_ptr(), I, src_o.data_ptr(),
                                         ev_o.data_ptr(), ext_o.data_ptr(), s)

    def parse(b, ne, ni):
        return eng.gateway_parse_device(req_o.data_ptr(), ne, items_o.data_ptr(), ni, batches[b][1].data_ptr(), nbytes,
                                        a_t.data_ptr(), I + E, v_t.data_ptr(), I + E, ext_o.data_ptr(), 0, s)

    el_expand = timed(lambda b: expand(b, n), args.warmup, args.steps)
    ne, ni = expand(0, n)
    for b in range(args.warmup + args.steps):      # the dictionary sees every client once before the parse is timed
        parse(b, *expand(b, n))
    counts = [expand(b, n) for b in range(args.warmup + args.steps)]
    last = args.warmup + args.steps - 1            # req_o / items_o now hold the last batch's expansion
    t_parse = timed(lambda b: parse(last, *counts[last]), args.warmup, args.steps)
    strings, _ = eng.vdict_size()
    chain = {"ms": None, "entries_per_step": None, "error": None}
    try:
        el, served = 0.0, 0
        for b in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            me, mi = expand(b, nc)
            na, nv = parse(b, me, mi)
            eng.slot_decide_device(ev_o.data_ptr(), ext_o.data_ptr(), me, a_t.data_ptr(), na, v_t.data_ptr(), nv,
                                   out.data_ptr(), s)
            torch.cuda.synchronize()
            if b >= args.warmup:
                el += time.perf_counter() - t0
                served += nc
        chain = {"ms": el * 1000.0 / args.steps, "entries_per_step": me, "error": None}
    except Exception as e:  # the expand figures stand on their own
        chain["error"] = str(e)
        el, served = el_expand, n * args.steps
    b_alg = n * 48 + 3 * n * 16 + n * P + ne * (16 + 4 + 32 + 4) + ni * 16
    return {"metric": "gateway HTTP requests/sec (API matching and expansion on the device + parser + the whole slot chain)",
            "workload": f"gateway_api: {K} routes x 4 rules, {A} custom APIs (half exact, half /x../**) x 2 rules, {n} "
                        f"requests per expand batch (16-byte paths, 3 fields); chain steps of {nc} requests, entries only, "
                        f"Zipf(1.0) routes and APIs, Zipf(1.1) over {n_clients} client IPs",
            "value": served / el, "el": el, "n": n, "b_alg": b_alg, "touched": strings, "cpu": None,
            "unit": "requests/s", "dtype": "u8",
            "extra": {"gateway_api": {"expand_ms": el_expand * 1000.0 / args.steps,
                                      "expand_requests_per_s": n * args.steps / el_expand,
                                      "entries_per_batch": ne, "items_per_batch": ni,
                                      "parse_ms": t_parse * 1000.0 / args.steps,
                                      "expand_parse_decide_ms": chain["ms"],
                                      "expand_parse_decide_requests_per_step": nc,
                                      "expand_parse_decide_entries_per_step": chain["entries_per_step"],
                                      "expand_parse_decide_requests_per_s": served / el if chain["ms"] else None,
                                      "expand_parse_decide_error": chain["error"],
                                      "algorithmic_bytes": {"requests": n * 48, "fields": 3 * n * 16, "paths": n * P,
                                                            "entries": ne * 56, "items": ni * 16},
                                      "dictionary_strings": strings}},
            "data": "synthetic (GPU-generated, seeded): fixed-width paths, client IP, header and URL parameter strings"}


def _gateway_local_rules(K):
    r = np.zeros(K, abi.LOCAL_RULE_DTYPE)
    r["flow_grade"] = abi.FLOW_GRADE_NONE
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c2", "c4", "c5", "codec", "pace", "cparam", "node", "slot", "gateway",
                                              "gateway_api"],
                    default="c2")
    ap.add_argument("--shards", type=int, default=0,
                    help="node: shard handles on the one GPU (default 2); cparam: decide through the node handle "
                         "with this many shards (default: one handle)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--events", type=int, default=16_000_000)
    ap.add_argument("--resources", type=int, default=1_000_000)
    ap.add_argument("--cpu-events", type=int, default=4_000_000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--local-sync", action="store_true",
                    help="c2 / c5: time the synchronous sg_local_decide_batch instead of the sg_local_enqueue pipeline")
    ap.add_argument("--chain", type=int, default=0,
                    help="cparam: embed a chain of this many two-value requests per batch, each sharing a value with "
                         "the next under a threshold of one (adversarial: one link per fixed-point round)")
    ap.add_argument("--pmc-summary", default=None,
                    help="scripts/pmc_summary.py output of this workload's FETCH_SIZE / WRITE_SIZE passes (roofline traffic)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    r = {"c2": c2, "c4": c4, "c5": c5, "codec": codec, "pace": pace, "cparam": cparam, "node": node,
         "slot": slot, "gateway": gateway, "gateway_api": gateway_api}[args.workload](args, dev)
    ms = r["el"] * 1000.0 / args.steps
    gbs = r["b_alg"] / (ms / 1000.0) / 1e9
    res = {"metric": r["metric"], "value": r["value"], "unit": r.get("unit", "decisions/s"), "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": r.get("dtype", "int64"), "data": r["data"],
           "config": {"workload": r["workload"], "decisions_per_step": r["n"], "touched_keys": r["touched"]},
           "roofline": {"bound": "hbm", "kernel": "whole batch pipeline, wall time per step", "achieved": gbs,
                        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS, "traffic": None,
                        "algorithmic_bytes_per_step": r["b_alg"]}}
    if args.pmc_summary and os.path.exists(args.pmc_summary):
        res["roofline"]["traffic"] = json.load(open(args.pmc_summary)).get("pipeline_bytes_per_step")
        res["roofline"]["traffic_source"] = args.pmc_summary
    res.update(r.get("extra", {}))
    if r["cpu"] is not None:
        res["cpu_baseline"] = r["cpu"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
