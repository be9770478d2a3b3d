"""The two logs over the node handle: sg_node_server_log_enable / sg_node_server_log (the token server's stat log of the
front and every shard, equal keys summed) and sg_node_local_block_log_enable / sg_node_local_block_log (the shards'
LogSlot rows, one owner per resource). Server log rows equal the model of tests/serverlog_ref.py fed with one sequential
oracle's results over the whole node's rules, exactly; block log rows equal those of one handle that decided the same
node trace (tests/test_blocklog_gpu.py holds that handle's rows against the LogSlot model)."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import ClusterTokenService
from sentinel_amd import abi
from tests.serverlog_ref import T0, ServerLog
from tests.test_node_gpu import _batch, _ns, _rules

pytestmark = pytest.mark.gpu
NO_ROWS = np.zeros(0, abi.SERVER_ROW_DTYPE)


def _same(got, want, what="rows"):
    assert got.dtype == want.dtype and len(got) == len(want) and np.array_equal(got, want), \
        f"{what}: device\n{got}\nmodel\n{want}"


def _node(G, rules, ns, max_batch=1 << 15, log2=14):
    from sentinel_amd.engine import NodeEngine
    node = NodeEngine([0] * G, max_batch=max_batch)
    node.set_namespaces(ns)
    node.load_rules(rules)
    if log2:
        node.server_log_enable(log2)
    cts = ClusterTokenService()
    cts.set_namespaces(ns)
    cts.load_rules(rules)
    return node, cts


@pytest.mark.parametrize("G,lim_qps,pipelined", [(1, 0.0, False), (1, 0.0, True), (3, 0.0, False), (3, 3000.0, False),
                                                 (3, 0.0, True), (2, 3000.0, True)])
def test_node_flow_rows_equal_one_token_service(G, lim_qps, pipelined):
    """sg_node_flow_decide_batch_host and sg_node_flow_enqueue (4 batches, 2 in flight, the last ones drained by the
    fetch): every shard adds its slice's logged decisions behind its walkers; G = 1 takes the front's records as they
    are, G > 1 the routed slices (node request indices, shard-local rule indices), with and without namespace limiters."""
    import torch
    rng = np.random.default_rng(100 * G + int(lim_qps > 0) + 10 * pipelined)
    K, n = 300, 20_000
    rules = _rules(rng, K)
    rules["count"] = rng.integers(0, 12, K)
    node, cts = _node(G, rules, _ns(lim_qps), max_batch=n)
    log = ServerLog()
    t, reqs = T0 + 9, []
    for _ in range(4):
        reqs.append(_batch(rng, n, K, t, 900))
        t = int(reqs[-1]["ts_ms"][-1]) + 5
    want = [cts.decide(r) for r in reqs]
    seen = set()
    for r, w in zip(reqs, want):
        log.flow_batch(rules, r, w)
        seen |= set(int(s) for s in w["status"])
    assert {abi.OK, abi.BLOCKED, abi.SHOULD_WAIT, abi.NO_RULE_EXISTS, abi.BAD_REQUEST} <= seen
    assert (abi.TOO_MANY_REQUEST in seen) == (lim_qps > 0)
    if pipelined:
        dev = torch.device("cuda:0")
        ins = [torch.from_numpy(r.view(np.uint8).copy()).to(dev) for r in reqs]
        outs = [torch.empty(n * abi.RES_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in reqs]
        torch.cuda.synchronize()
        tickets = []
        for b in range(4):
            if b >= 2:
                node.wait(tickets[b - 2])
            tickets.append(node.enqueue_device(ins[b].data_ptr(), n, outs[b].data_ptr()))
    else:
        got = [node.decide_host(r) for r in reqs]
    rows = log.take(t + 2000)
    assert len(rows) > 100
    got_rows, le, lc = node.server_log(t + 2000)
    _same(got_rows, rows)
    assert (le, lc) == (0, 0)
    if pipelined:
        for tk in tickets[-2:]:
            node.wait(tk)
        got = [o.cpu().numpy().view(abi.RES_DTYPE) for o in outs]
    for b in range(4):
        _same(np.asarray(got[b]), want[b], f"results of batch {b}")
    _same(node.server_log(t + 9000)[0], NO_ROWS)


def test_node_concurrent_and_param_tokens_log_on_their_shards():
    """sg_node_conc_* and sg_node_cparam_* reach the shards' own entry points: rows of both families, merged and sorted
    with the flow rows of the same node."""
    from oracle.binding import ConcurrentTokenService
    from tests.serverlog_ref import ParamChecker
    from tests.test_node_tokens_gpu import NodeTrace
    from tests.test_cparam_gpu import _rules as prules
    from tests.test_cparam_gpu import _trace as ptrace
    rng = np.random.default_rng(5)
    K = 40
    rules = _rules(rng, K)
    rules["count"] = rng.integers(1, 10, K)
    ns = _ns(0.0)
    node, cts = _node(3, rules, ns)
    pr = prules(6, rng)
    pr["count"] = rng.integers(1, 6, 6)
    node.cparam_load_rules(pr, None, 12)
    cts.load_param_rules(pr)
    conc = ConcurrentTokenService()
    conc.set_namespaces(ns)
    conc.load_rules(rules)
    log, tr = ServerLog(), NodeTrace(5, K)      # the node mints its own token ids: a release names the same token in each
    tr.t = T0 + 100
    for _ in range(2):
        q, qn = tr.batch(3000, 700)
        want = conc.decide(q)
        got = node.conc_decide_host(qn)
        _same(got["status"], want["status"], "concurrent statuses")
        log.conc_batch(rules, q, want)
        tr.absorb(q, want, got)
    req, vals = ptrace(rng, 3000, 6, 20, T0 + 200, 1500, multi=0.3, zipf=1.2)
    want, blocks = ParamChecker(cts, pr, ns).decide(req, vals)
    _same(node.cparam_decide_host(req, vals), want, "param results")
    log.param_batch(pr, req, want, blocks)
    f = _batch(rng, 4000, K, T0 + 300, 1200)
    wf = cts.decide(f)
    _same(node.decide_host(f), wf, "flow results")
    log.flow_batch(rules, f, wf)
    rows = log.take(T0 + 9000)
    events = {int(e) for e in rows["event"]}
    assert {abi.SLOG_CONC_PASS, abi.SLOG_CONC_BLOCK, abi.SLOG_CONC_RELEASE, abi.SLOG_PARAM_PASS, abi.SLOG_PARAM_BLOCK,
            abi.SLOG_FLOW_BLOCK, abi.SLOG_FLOW_BLOCK_REQUEST} <= events
    got, le, lc = node.server_log(T0 + 9000)
    _same(got, rows)
    assert (le, lc) == (0, 0)


def _raw(node, fn, dtype, now, cap):
    out = np.zeros(max(1, cap), dtype)
    n, le, lc = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = fn(node.h, now, abi.ptr(out), cap, C.byref(n), C.byref(le), C.byref(lc))
    return rc, out, n.value, le.value, lc.value


def test_node_server_log_contract_full_tables_and_a_cap_too_small():
    """Before the enable SG_E_INVAL; the same capacity again nothing, another SG_E_INVAL; a cap below the sum of the
    parts' rows SG_E_CAPACITY with that sum and nothing changed; with 16 slots a shard and 60 flowIds blocked in one
    second every returned row equals the model's and the lost totals are exactly the rest, summed over the shards."""
    from sentinel_amd.engine import EngineError
    rng = np.random.default_rng(8)
    K = 60
    rules = _rules(rng, K)
    rules["count"] = 0                                    # every request is BLOCKED
    node, cts = _node(3, rules, _ns(0.0), log2=0)
    with pytest.raises(EngineError) as ei:
        node.server_log(T0)
    assert ei.value.code == abi.SG_E_INVAL
    node.server_log_enable(4)
    node.server_log_enable(4)
    with pytest.raises(EngineError) as ei:
        node.server_log_enable(5)
    assert ei.value.code == abi.SG_E_INVAL
    n = 6000
    req = np.zeros(n, abi.REQ_DTYPE)
    req["ts_ms"], req["key"], req["acquire"] = T0 + np.arange(n) * 999 // n, np.arange(n) % K, 1 + np.arange(n) % 3
    want = cts.decide(req)
    assert (want["status"] == abi.BLOCKED).all()
    _same(node.decide_host(req), want, "results")         # decisions untouched by the full tables
    log = ServerLog()
    log.flow_batch(rules, req, want)
    model = log.take(T0 + 1000)
    fn = node._L.sg_node_server_log
    rc, _, need, le, lc = _raw(node, fn, abi.SERVER_ROW_DTYPE, T0 + 1000, 3)
    assert rc == abi.SG_E_CAPACITY and need > 3 and (le, lc) == (0, 0)
    rc, out, m, le, lc = _raw(node, fn, abi.SERVER_ROW_DTYPE, T0 + 1000, need)
    assert rc == 0 and m == need                          # distinct flowIds: nothing merged
    rows = out[:m]
    ids = sorted(set(int(f) for f in rows["flow_id"]))
    shards = [node.shard_of(k)[0] for k in range(K)]
    fit = sum(min(16, shards.count(g)) for g in range(3))
    assert len(ids) == fit and fit < K                    # every shard's table filled or took all its flowIds
    _same(rows, model[np.isin(model["flow_id"], ids)])
    rest = model[~np.isin(model["flow_id"], ids)]
    assert le == int(rest["count"][rest["event"] == abi.SLOG_FLOW_BLOCK_REQUEST].sum())
    assert lc == int(rest["count"][rest["event"] == abi.SLOG_FLOW_BLOCK].sum()) and le > 0
    got, le, lc = node.server_log(T0 + 1000)
    assert len(got) == 0 and (le, lc) == (0, 0)


@pytest.mark.parametrize("G", [1, 3, 5])
def test_node_block_log_equals_one_handle(G):
    """The node's three-batch reference trace (48 resources, RELATE groups, origin rules, breakers): the node's block
    log rows equal one handle's, fetched between the batches and at the end; keys are unique (a resource has one
    owner: the call itself refuses a key that comes from two shards); a cap below the sum changes nothing."""
    from sentinel_amd.engine import EngineError, FlowEngine
    from tests.test_local_shard import N_ORIGINS
    from tests.test_node_local_gpu import MAX_BATCH, _node, _node_case
    base, frules, relate, inbound, trace = _node_case()
    nd = _node(G, base, frules, inbound)
    with pytest.raises(EngineError) as ei:
        nd.block_log(T0)
    assert ei.value.code == abi.SG_E_INVAL
    nd.block_log_enable(12)
    nd.block_log_enable(12)
    with pytest.raises(EngineError) as ei:
        nd.block_log_enable(13)
    assert ei.value.code == abi.SG_E_INVAL
    one = FlowEngine(device=0, max_batch=MAX_BATCH)
    one.local_load_rules(base, 2, 1000, 500)
    one.local_load_flow_rules(frules, N_ORIGINS, 0)
    one.local_set_entry_types(inbound)
    one.block_log_enable(12)
    total = 0
    for b, (ev, want, now, _) in enumerate(trace):
        assert np.array_equal(nd.local_decide_host(ev), want) and np.array_equal(one.local_decide_host(ev), want)
        fetch_at = now if b < len(trace) - 1 else now + 5000
        ref, rle, rlc = one.block_log(fetch_at)
        if len(ref) > 1:
            rc, _, need, _, _ = _raw(nd, nd._L.sg_node_local_block_log, abi.BLOCK_ROW_DTYPE, fetch_at, len(ref) - 1)
            assert rc == abi.SG_E_CAPACITY and need == len(ref)
        rows, le, lc = nd.block_log(fetch_at)
        _same(rows, ref, f"block log rows after batch {b}")
        assert (le, lc) == (rle, rlc) == (0, 0)
        fields = ("timestamp", "resource", "status", "app_kind", "app", "origin")
        assert len(set(zip(*(rows[f].tolist() for f in fields)))) == len(rows)
        total += len(rows)
    assert total > 20
