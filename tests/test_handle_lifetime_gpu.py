"""Lifetime of the handles: one FlowEngine, and one two-shard NodeEngine, driven through every path that allocates
device memory lazily (both flow workspaces, the host-path staging of every entry point, the cparam save area, the
local chain, the concurrent tokens, the ParamFlowSlot chain, the value dictionary, the node's slices, snapshot and
metric rows), every result compared with the oracle as the neighbouring tests do, then destroyed. Creating, using
and destroying the same handle again and again must not lose device memory: the free memory reported after cycles 2,
3 and 4 (the first is warm-up) may fall by no more than it fell on the commit before the handles owned their memory
through DevBuf / PinnedBuf (csrc/devmem.h)."""
import functools
import gc

import numpy as np
import pytest

from sentinel_amd import abi
from sentinel_amd.param_wire import canonical_key

pytestmark = pytest.mark.gpu

MAX_BATCH = 4096
N_FLOWS = 64
T0 = 1_700_000_000_000

# Free-memory drift over cycles 2 -> 4, in bytes, measured with this file on the parent commit (raw pointers and the
# hand-kept free lists in sg_destroy / sg_node_destroy): single handle 0, node 0. The margin is the parent's own drift
# and nothing more: the point is "no new leak", not a property of the runtime's allocator.
PARENT_DRIFT_SINGLE = 0
PARENT_DRIFT_NODE = 0


def _ns():
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"] = 1
    ns["max_allowed_qps"] = 30000
    return ns


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {len(bad)} differ; first {bad[0]}: oracle={want[bad[0]]} gpu={got[bad[0]]}")


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _single_case():
    """Inputs and oracle results of one cycle of the single handle (computed once, never modified)."""
    from oracle.binding import (ClusterTokenService, ConcurrentTokenService, LocalChain, LocalTraceGen, ParamFlowChecker,
                                ParamFlowSlot, RateLimiterController)
    from sentinel_amd.workload import ClusterWorkload
    from tests import test_conc_gpu, test_cparam_gpu, test_local_gpu, test_pace_gpu, test_param_gpu, test_pslot_gpu
    c = {}
    # flow: device batch, host batch, three submits, then (after the cparam batch) one more host batch
    wl = ClusterWorkload(n_flows=N_FLOWS, n_requests=MAX_BATCH, seed=31, prio_frac=0.05)
    rng = np.random.default_rng(5)
    c["flow_rules"] = wl.rules()
    c["cp_rules"] = test_cparam_gpu._rules(6, rng)
    ora = ClusterTokenService()
    ora.set_namespaces(_ns())
    ora.load_rules(c["flow_rules"])
    ora.load_param_rules(c["cp_rules"], None)
    c["flow_req"] = [wl.requests(b) for b in range(6)]
    c["flow_want"] = [ora.decide(r) for r in c["flow_req"]]
    # cparam with multi-value requests (the ring save area), after flow batch 4 in wall order but on its own clock
    c["cp_req"], c["cp_vals"] = test_cparam_gpu._trace(rng, 3000, 6, 40, T0 + 500, 1500, multi=0.05, bad=0.01)
    c["cp_want"] = ora.decide_param(c["cp_req"], c["cp_vals"])
    assert (c["cp_req"]["value_count"] > 1).any()
    # hot-parameter flow control
    c["p_rules"] = test_param_gpu._rules([{"count": 5}, {"count": 2, "burst": 1}, {"count": 9, "duration": 2}])
    c["p_req"] = test_param_gpu._trace(rng, 3000, 3, 50, T0, 1500)
    po = ParamFlowChecker()
    po.load_rules(c["p_rules"], None)
    c["p_want"] = po.decide(c["p_req"])
    # pace controller
    c["pace_rules"] = test_pace_gpu._rules(rng, 20)
    c["pace_req"] = test_pace_gpu._trace(rng, 3000, 20, T0, 1500)
    c["pace_want"] = RateLimiterController(c["pace_rules"]).decide(c["pace_req"])
    # local slot chain
    c["l_rules"] = test_local_gpu._rules(16, rng)
    lo = LocalChain(2, 1000, 500)
    lo.load_rules(c["l_rules"])
    ent = test_local_gpu._entries(rng, 1500, 16, T0, 1000)
    c["l_ev"], c["l_want"] = LocalTraceGen(lo).run(ent, rng.integers(0, 41, 1500).astype(np.int32),
                                                  (rng.random(1500) < 0.05).astype(np.uint8), T0 + 1000)
    assert len(c["l_ev"]) <= MAX_BATCH
    # concurrent tokens over the handle's flow rules
    co = ConcurrentTokenService()
    co.set_namespaces(_ns())
    co.load_rules(c["flow_rules"])
    c["c_req"] = test_conc_gpu.Trace(7, N_FLOWS).batch(2000, 700)
    c["c_want"] = co.decide(c["c_req"])
    # ParamFlowSlot chain
    c["ps_rules"], c["ps_hot"] = test_pslot_gpu._rules(np.random.default_rng(2), 12)
    c["ps_ev"], c["ps_args"], c["ps_vals"], _ = test_pslot_gpu.Gen(2, 12).batch(2000, 1500)
    c["ps_want"] = ParamFlowSlot(c["ps_rules"], c["ps_hot"], n_resources=12).decide(c["ps_ev"], c["ps_args"],
                                                                                   c["ps_vals"])
    for v in c.values():
        _frozen(*(v if isinstance(v, list) else [v]))
    return c


def _single_cycle(c):
    import torch
    from sentinel_amd.engine import FlowEngine
    eng = FlowEngine(device=0, max_batch=MAX_BATCH)
    try:
        eng.set_namespaces(_ns())
        eng.load_rules(c["flow_rules"])
        eng.cparam_load_rules(c["cp_rules"], None, 12)
        req, want = c["flow_req"], c["flow_want"]
        # synchronous device batch
        req_t = torch.from_numpy(req[0].view(np.uint8).copy()).cuda()
        out_t = torch.empty(len(req[0]) * abi.RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        eng.decide_device(req_t.data_ptr(), len(req[0]), out_t.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _same(out_t.cpu().numpy().view(abi.RES_DTYPE), want[0], "device batch")
        # host batch, then three submits (the second allocates workspace 1)
        _same(eng.decide_host(req[1]), want[1], "host batch")
        outs = [np.zeros(len(req[b]), abi.RES_DTYPE) for b in (2, 3, 4)]
        tickets = [eng.submit(req[b], o) for b, o in zip((2, 3, 4), outs)]
        for tk in tickets:
            eng.wait(tk)
        for b, o in zip((2, 3, 4), outs):
            _same(o, want[b], f"submitted batch {b}")
        # the shared host-path staging: flow (above), cparam, flow again
        _same(eng.cparam_decide_host(c["cp_req"], c["cp_vals"]), c["cp_want"], "cparam host batch")
        _same(eng.decide_host(req[5]), want[5], "host batch after the cparam batch")
        eng.param_load_rules(c["p_rules"], None)
        _same(eng.param_decide_host(c["p_req"]), c["p_want"], "param host batch")
        eng.pace_load_rules(c["pace_rules"])
        _same(eng.pace_decide_host(c["pace_req"]), c["pace_want"], "pace host batch")
        eng.local_load_rules(c["l_rules"], 2, 1000, 500)
        _same(eng.local_decide_host(c["l_ev"]), c["l_want"], "local host batch")
        _same(eng.conc_decide_host(c["c_req"]), c["c_want"], "conc host batch")
        eng.pslot_load_rules(c["ps_rules"], c["ps_hot"], n_resources=12)
        _same(eng.pslot_decide_host(c["ps_ev"], c["ps_args"], c["ps_vals"]), c["ps_want"], "pslot host batch")
        eng.vdict_init(8, 1 << 12, 64)
        keys = [canonical_key(5, "int"), canonical_key("5"), canonical_key(5, "int")]
        assert list(eng.vdict_intern(keys)) == [1, 2, 1]
        assert eng.vdict_lookup([2, 1]) == [(int(t), bytes(p)) for t, p in (keys[1], keys[0])]
    finally:
        eng.close()


def _free_after(cycle, n=4):
    """Free device memory after each of n create / use / destroy cycles."""
    import torch
    free = []
    for _ in range(n):
        cycle()
        gc.collect()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    return free


def _assert_no_drift(free, parent_drift, what):
    print(f"{what}: free device memory after cycles 1..4: {free}; drift over cycles 2 -> 4: {free[1] - free[3]} B "
          f"(parent: {parent_drift} B)")
    assert free[1] - free[2] <= parent_drift and free[1] - free[3] <= parent_drift, \
        f"{what}: free device memory fell over cycles 2..4: {free[1:]} (allowed: {parent_drift} B)"


def test_single_handle_results_and_no_memory_drift():
    c = _single_case()
    free = _free_after(lambda: _single_cycle(c))
    _assert_no_drift(free, PARENT_DRIFT_SINGLE, "single handle")


# ---- the node handle


def _node_rules(K):
    r = np.zeros(K, abi.RULE_DTYPE)
    r["flow_id"] = 1000 + 7 * np.arange(K)
    r["count"] = 1 + np.arange(K) % 23
    r["threshold_type"] = abi.THRESHOLD_GLOBAL
    r["sample_count"] = 10
    r["window_interval_ms"] = 1000
    return r


def _node_batch(rng, n, K, t):
    from sentinel_amd.workload import zipf_keys
    req = np.zeros(n, abi.REQ_DTYPE)
    req["ts_ms"] = t + np.sort(rng.integers(0, 900, n))
    req["key"] = zipf_keys(rng, K, n, 1.0, perm_seed=3).astype(np.uint32)
    req["acquire"] = 1
    return req


@functools.lru_cache(maxsize=None)
def _node_case():
    from oracle.binding import ClusterTokenService
    from tests import test_node_tokens_gpu
    from tests.test_local_shard import N_ORIGINS, node_setup, node_trace
    c = {}
    rng = np.random.default_rng(9)
    c["rules"] = [_node_rules(16), _node_rules(64)]       # the reload gives every shard four times the rules
    c["req"] = [_node_batch(rng, 3000, 16, T0), _node_batch(rng, 3000, 64, T0 + 1000)]
    ora = ClusterTokenService()
    ora.set_namespaces(_ns())
    c["want"] = []
    for rules, req in zip(c["rules"], c["req"]):
        ora.load_rules(rules)
        c["want"].append(ora.decide(req))
    c["cp_rules"] = test_node_tokens_gpu._prules(rng, 8)
    c["cp_rules"]["namespace_id"] = 0
    c["cp_req"], c["cp_vals"] = test_node_tokens_gpu._ptrace(rng, 3000, 8, 60, T0, 1500, multi=0.1)
    ora.load_param_rules(c["cp_rules"], None)
    c["cp_want"] = ora.decide_param(c["cp_req"], c["cp_vals"])
    base, frules, _, inbound = node_setup()
    (ev, res, now, rows), = node_trace(base, frules, inbound, n_batches=1, n=1500)
    assert len(ev) <= MAX_BATCH
    c.update(l_base=base, l_frules=frules, l_inbound=inbound, l_origins=N_ORIGINS, l_ev=ev, l_want=res, l_now=now,
             l_rows=rows)
    for v in c.values():
        _frozen(*(v if isinstance(v, list) else [v]))
    return c


def _node_cycle(c, devices=(0, 0)):
    from sentinel_amd.engine import FlowEngine, NodeEngine
    node = NodeEngine(list(devices), max_batch=MAX_BATCH)
    single = FlowEngine(device=devices[0], max_batch=MAX_BATCH)
    try:
        for e in (node, single):
            e.set_namespaces(_ns())
        for b, (rules, req, want) in enumerate(zip(c["rules"], c["req"], c["want"])):
            K = len(rules)
            for e in (node, single):
                e.load_rules(rules)
            _same(node.decide_host(req), want, f"node flow batch {b}")
            _same(single.decide_host(req), want, f"single flow batch {b}")
            now = int(req["ts_ms"][-1]) + 5
            assert np.array_equal(node.snapshot(now, K), single.snapshot(now, K).reshape(K, 2)), f"snapshot {b}"
        node.cparam_load_rules(c["cp_rules"], None, 12)
        _same(node.cparam_decide_host(c["cp_req"], c["cp_vals"]), c["cp_want"], "node cparam batch")
        node.local_load_rules(c["l_base"], 2, 1000, 500)
        node.local_load_flow_rules(c["l_frules"], c["l_origins"], 0)
        node.local_set_entry_types(c["l_inbound"])
        _same(node.local_decide_host(c["l_ev"]), c["l_want"], "node local batch")
        assert np.array_equal(node.local_metrics(c["l_now"]), c["l_rows"])
    finally:
        single.close()
        node.__del__()


def test_node_results_and_no_memory_drift():
    c = _node_case()
    free = _free_after(lambda: _node_cycle(c))
    _assert_no_drift(free, PARENT_DRIFT_NODE, "two-shard node")


def test_node_snapshot_regrows_remote_part_after_reload():
    """Shards on two devices: a shard's part of the node snapshot is computed in a buffer on its own device. A reload
    that gives the shard more rules (8 -> 64 over the node) must regrow that buffer; both snapshots equal a single
    handle's."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices: the remote snapshot part exists only for a shard off the front's device")
    from sentinel_amd.engine import FlowEngine, NodeEngine
    rng = np.random.default_rng(4)
    node = NodeEngine([0, 1], max_batch=MAX_BATCH)
    single = FlowEngine(device=0, max_batch=MAX_BATCH)
    try:
        for e in (node, single):
            e.set_namespaces(_ns())
        t = T0
        for K in (8, 64):
            rules = _node_rules(K)
            req = _node_batch(rng, 3000, K, t)
            for e in (node, single):
                e.load_rules(rules)
            assert np.array_equal(node.decide_host(req), single.decide_host(req))
            t += 1000
            assert np.array_equal(node.snapshot(t, K), single.snapshot(t, K).reshape(K, 2)), f"snapshot at {K} rules"
    finally:
        single.close()
        node.__del__()
