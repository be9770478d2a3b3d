"""The local slot chain over the node handle (sg_node_local_*): G shards of one GPU standing for G GPUs of a node, the
events routed by resource owner inside the library (the stable multisplit k_lroute_*) and the node's metric rows merged
on the device (k_merge_*). Every decision and every metrics.log row must equal one sequential replay of the whole node
trace by the oracle (tests/test_local_shard.py: 48 resources, RELATE groups, origin rules, WarmUp, thread grade,
breakers); a refused call leaves no trace; the merge kernel alone equals cluster.merge_metric_rows on synthetic rows."""
import functools

import numpy as np
import pytest

from sentinel_amd import abi
from sentinel_amd.cluster import ENTRY_NODE_RESOURCE, local_owners, merge_metric_rows
from tests.test_local_shard import N_ORIGINS, N_RES, T0, node_setup, node_trace

pytestmark = pytest.mark.gpu

ROUTE_TILE = 4096        # events per tile of the multisplit (node.hip kRouteTile)
MERGE_PASS_WORDS = 512   # bitmap words one pass of the merge's word scan covers (node.hip kMergeScanPass)
MAX_BATCH = 1 << 14


@functools.lru_cache(maxsize=None)
def _node_case():
    """The node's rules and its three-batch reference trace (computed once, never modified)."""
    base, frules, relate, inbound = node_setup()
    trace = node_trace(base, frules, inbound)
    for ev, res, _, rows in trace:
        for a in (ev, res, rows):
            a.setflags(write=False)
    return base, frules, relate, inbound, trace


def _node(G, base, frules, inbound, flow_rules=True, cold_factor=3):
    from sentinel_amd.engine import NodeEngine
    nd = NodeEngine([0] * G, max_batch=MAX_BATCH)
    nd.local_load_rules(base, 2, 1000, 500, cold_factor=cold_factor)
    if flow_rules:
        nd.local_load_flow_rules(frules, N_ORIGINS, 0)
    nd.local_set_entry_types(inbound)
    return nd


def _code(call, *args):
    from sentinel_amd.engine import EngineError
    with pytest.raises(EngineError) as e:
        call(*args)
    return e.value.code


class _Replay:
    """One sequential oracle chain with its client model: batches of entries become (events, reference results)."""

    def __init__(self, base, frules, inbound, seed):
        from oracle.binding import LocalChain, LocalTraceGen
        self.rng = np.random.default_rng(seed)
        self.chain = LocalChain(2, 1000, 500)
        self.chain.load_rules(base)
        self.chain.load_flow_rules(frules, N_ORIGINS, 0)
        self.chain.set_entry_types(inbound)
        self.gen = LocalTraceGen(self.chain)

    def batch(self, t, span, n, resource=None):
        from sentinel_amd.workload import zipf_keys
        rng = self.rng
        ent = np.zeros(n, abi.LOCAL_EVENT_DTYPE)
        ent["ts_ms"] = t + np.sort(rng.integers(0, span, n))
        ent["resource"] = zipf_keys(rng, N_RES, n, 1.0, perm_seed=7) if resource is None else resource
        ent["count"] = 1
        ent["origin"] = rng.integers(0, N_ORIGINS + 1, n)
        rt = rng.integers(0, 60, n).astype(np.int32)
        err = (rng.random(n) < 0.1).astype(np.uint8)
        ev, res = self.gen.run(ent, rt, err, t + span)
        return ev, res, t + span


@pytest.mark.parametrize("G,device", [(1, False), (2, False), (3, False), (5, False), (3, True)])
def test_node_equals_node_replay(G, device):
    from sentinel_amd.engine import FlowEngine
    base, frules, relate, inbound, trace = _node_case()
    nd = _node(G, base, frules, inbound)
    want_own = local_owners(N_RES, relate, G)
    assert [nd.local_owner_of(r) for r in range(N_RES)] == [int(x) for x in want_own]
    assert _code(nd.local_owner_of, N_RES) == abi.SG_E_INVAL
    one = FlowEngine(device=0, max_batch=MAX_BATCH)
    one.local_load_rules(base, 2, 1000, 500)
    one.local_load_flow_rules(frules, N_ORIGINS, 0)
    one.local_set_entry_types(inbound)
    statuses = set()
    for b, (ev, want, now, rows_want) in enumerate(trace):
        if device:
            import torch
            ev_t = torch.from_numpy(ev.view(np.uint8).copy()).cuda()
            out_t = torch.empty(len(ev) * abi.LOCAL_RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            nd.local_decide_device(ev_t.data_ptr(), len(ev), out_t.data_ptr(), torch.cuda.current_stream().cuda_stream)
            got = out_t.cpu().numpy().view(abi.LOCAL_RES_DTYPE)
            buf = torch.empty((4 * N_RES + 64, 8), dtype=torch.int64, device="cuda")
            k = nd.local_metrics_device(now, buf)
            rows = buf[:k].cpu().numpy().copy().view(abi.METRIC_NODE_DTYPE).reshape(-1)
        else:
            got = nd.local_decide_host(ev)
            rows = nd.local_metrics(now)
        assert np.array_equal(got, want), f"batch {b}: {(got != want).sum()} results differ"
        assert np.array_equal(rows, rows_want), f"batch {b}: metric rows differ ({len(rows)} vs {len(rows_want)})"
        assert (rows_want["resource"] == ENTRY_NODE_RESOURCE).any()
        statuses |= set(np.unique(want["status"][ev["kind"] == abi.LOCAL_ENTRY]).tolist())
        assert np.array_equal(one.local_decide_host(ev), want)
        assert np.array_equal(one.local_metrics(now), rows_want)
    assert statuses == {abi.LOCAL_PASS, abi.LOCAL_BLOCK_FLOW, abi.LOCAL_BLOCK_DEGRADE, abi.LOCAL_PASS_WAIT}
    assert len(np.unique(trace[1][3]["timestamp"])) == 2
    for r in (0, 3, 10, 21, 47):
        for a, w in zip(nd.local_state(r), one.local_state(r)):
            assert np.array_equal(a, w), f"resource {r}: state differs from one handle's"


def test_node_cold_factor_5():
    """sg_local_config.cold_factor reaches every shard: the node's trace replayed by the oracle with
    ColdFactorProperty.coldFactor 5 (other decisions than with 3), on two shards and on one handle."""
    from oracle.binding import LocalChain
    from sentinel_amd.engine import FlowEngine
    base, frules, relate, inbound, trace3 = _node_case()
    trace = node_trace(base, frules, inbound, cold_factor=5)
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(trace, trace3)), "the cold factor decides nothing here"
    nd = _node(2, base, frules, inbound, cold_factor=5)
    one = FlowEngine(device=0, max_batch=MAX_BATCH)
    one.local_load_rules(base, 2, 1000, 500, cold_factor=5)
    one.local_load_flow_rules(frules, N_ORIGINS, 0)
    one.local_set_entry_types(inbound)
    for b, (ev, want, now, rows_want) in enumerate(trace):
        assert np.array_equal(nd.local_decide_host(ev), want), f"batch {b}: the node's results differ"
        assert np.array_equal(one.local_decide_host(ev), want), f"batch {b}: one handle's results differ"
        assert np.array_equal(nd.local_metrics(now), rows_want) and np.array_equal(one.local_metrics(now), rows_want)
    ora = LocalChain(2, 1000, 500, cold_factor=5)   # the controllers after the last batch: the replay once more
    ora.load_rules(base)
    ora.load_flow_rules(frules, N_ORIGINS, 0)
    ora.set_entry_types(inbound)
    for ev, want, _, _ in trace:
        assert np.array_equal(ora.decide(ev), want)
    warm = np.nonzero(frules["control_behavior"] == abi.CONTROL_WARM_UP)[0]
    assert len(warm) == N_RES // 6
    for i in warm:
        assert np.array_equal(nd.local_controller(i), ora.controller(i)), f"rule {i}: the node's controller"
        assert np.array_equal(one.local_controller(i), ora.controller(i)), f"rule {i}: one handle's controller"
    for r in range(2, N_RES, 6):
        for a, w in zip(nd.local_state(r), one.local_state(r)):
            assert np.array_equal(a, w), f"resource {r}: state differs from one handle's"


def test_routing_shapes():
    """A batch over three tiles of the multisplit ending in a partial one, a batch naming one resource (every other
    shard's slice empty), a single event, and no event at all."""
    base, frules, relate, inbound, _ = _node_case()
    G = 3
    nd = _node(G, base, frules, inbound)
    ora = _Replay(base, frules, inbound, seed=11)
    ev, want, now = ora.batch(T0, 1500, 7600)
    assert len(ev) > 2 * ROUTE_TILE and len(ev) % ROUTE_TILE != 0 and len(ev) <= MAX_BATCH
    owners = local_owners(N_RES, relate, G)
    assert len(np.unique(owners[ev["resource"] & 0x7FFFFFFF])) == G
    assert np.array_equal(nd.local_decide_host(ev), want)
    assert np.array_equal(nd.local_metrics(now), ora.chain.metrics(now))
    # a second later every exit of that batch is due (rt < 60 ms, waits <= 500 ms): one entry drains them
    ev, want, now = ora.batch(now + 999, 1, 1, resource=5)
    assert np.array_equal(nd.local_decide_host(ev), want)
    ev, want, now = ora.batch(now, 300, 400, resource=5)
    assert len(ev) >= 400 and (ev["resource"] & 0x7FFFFFFF == 5).all()   # every other shard's slice is empty
    assert np.array_equal(nd.local_decide_host(ev), want)
    # the generator's pending exits, then one entry: the exits are one node batch, the single event another
    ev, want, now = ora.batch(now + 999, 1, 1, resource=9)
    keep = int(np.nonzero(ev["kind"] == abi.LOCAL_ENTRY)[0][-1])
    for lo, hi in ((0, keep), (keep, keep + 1), (keep + 1, len(ev))):
        assert np.array_equal(nd.local_decide_host(ev[lo:hi]), want[lo:hi])
    assert len(nd.local_decide_host(ev[:0])) == 0
    assert np.array_equal(nd.local_metrics(now + 1000), ora.chain.metrics(now + 1000))


def test_refusals_leave_no_trace():
    from sentinel_amd.engine import NodeEngine
    base, frules, relate, inbound, trace = _node_case()
    G = 3
    fresh = NodeEngine([0] * G, max_batch=MAX_BATCH)
    assert _code(fresh.local_decide_host, trace[0][0]) == abi.SG_E_INVAL  # decide before load
    nd = _node(G, base, frules, inbound)
    owners = local_owners(N_RES, relate, G)
    # two events of different owners, decreasing timestamps: each shard's slice alone is sorted
    a = 0
    b = next(r for r in range(N_RES) if owners[r] != owners[a])
    two = np.zeros(2, abi.LOCAL_EVENT_DTYPE)
    two["ts_ms"] = [T0 + 5, T0 + 4]
    two["resource"] = [a, b]
    two["count"] = 1
    assert _code(nd.local_decide_host, two) == abi.SG_E_TIME
    (ev0, want0, now0, rows0), (ev1, want1, now1, rows1), (ev2, want2, now2, rows2) = trace
    assert np.array_equal(nd.local_decide_host(ev0), want0)
    assert np.array_equal(nd.local_metrics(now0), rows0)
    assert _code(nd.local_decide_host, ev0) == abi.SG_E_TIME  # older than the previous batch
    bad = ev1.copy()
    bad["origin"][len(bad) // 2] = N_ORIGINS + 1
    assert _code(nd.local_decide_host, bad) == abi.SG_E_INVAL
    big = np.zeros(MAX_BATCH + 1, abi.LOCAL_EVENT_DTYPE)
    big["ts_ms"] = ev1["ts_ms"][0]
    big["count"] = 1
    assert _code(nd.local_decide_host, big) == abi.SG_E_CAPACITY
    assert np.array_equal(nd.local_decide_host(ev1), want1)
    assert np.array_equal(nd.local_metrics(now1), rows1)
    assert np.array_equal(nd.local_decide_host(ev2), want2)
    assert np.array_equal(nd.local_metrics(now2), rows2)


def _moving_pair(relate, G):
    """A RELATE pair (resource, ref) that gives some resource another owner at G shards."""
    old = local_owners(N_RES, relate, G)
    for a in range(N_RES):
        for b in range(N_RES):
            if a != b and not np.array_equal(local_owners(N_RES, list(relate) + [(a, b)], G), old):
                return a, b
    raise AssertionError("no RELATE pair moves an owner")


def test_reload_keeps_statistics_and_refuses_a_move():
    from oracle.binding import local_flow_rule
    base, frules, relate, inbound, _ = _node_case()
    G = 3
    nd = _node(G, base, frules, inbound)
    ora = _Replay(base, frules, inbound, seed=12)
    ev, want, now = ora.batch(T0, 1500, 3000)
    assert np.array_equal(nd.local_decide_host(ev), want)
    # the same key groups, other counts: the statistics stay, the oracle reloads at the same point
    frules2 = frules.copy()
    frules2["count"] = np.where(frules2["count"] > 4, frules2["count"] - 2, frules2["count"] + 3)
    kept = ora.chain.load_flow_rules(frules2, N_ORIGINS, 0)
    assert nd.local_load_flow_rules(frules2, N_ORIGINS, 0) == kept
    ev, want, now = ora.batch(now, 1500, 3000)
    assert np.array_equal(nd.local_decide_host(ev), want)
    # a RELATE pair that moves a resource to another shard: refused whole, the old rules stay in force
    a, b = _moving_pair(relate, G)
    frules3 = np.concatenate([frules2, np.array([local_flow_rule(a, 7.0, strategy=abi.STRATEGY_RELATE, ref=b)],
                                                abi.LOCAL_FLOW_RULE_DTYPE)])
    assert _code(nd.local_load_flow_rules, frules3, N_ORIGINS, 0) == abi.SG_E_UNSUPPORTED
    assert [nd.local_owner_of(r) for r in range(N_RES)] == [int(x) for x in local_owners(N_RES, relate, G)]
    ev, want, now = ora.batch(now, 1500, 3000)
    assert np.array_equal(nd.local_decide_host(ev), want)
    assert np.array_equal(nd.local_metrics(now), ora.chain.metrics(now))
    # before any batch the same reload is accepted, and the owners follow the new groups
    nd2 = _node(G, base, frules, inbound)
    nd2.local_load_flow_rules(frules3, N_ORIGINS, 0)
    want_own = local_owners(N_RES, list(relate) + [(a, b)], G)
    assert [nd2.local_owner_of(r) for r in range(N_RES)] == [int(x) for x in want_own]


def test_metrics_capacity_has_no_side_effect():
    import ctypes as C

    import torch
    base, frules, relate, inbound, trace = _node_case()
    nd = _node(5, base, frules, inbound)
    ev, want, now, rows_want = trace[0]
    assert np.array_equal(nd.local_decide_host(ev), want)
    n = C.c_uint64()
    assert nd._L.sg_node_local_metrics_device(nd.h, now, None, 0, C.byref(n)) == abi.SG_E_CAPACITY
    total = n.value  # the sum of the shards' row counts: ENTRY_NODE rows of one second not yet collapsed
    seconds = len(np.unique(rows_want["timestamp"]))
    assert len(rows_want) <= total <= len(rows_want) + 4 * seconds
    buf = torch.full((total, 8), -7, dtype=torch.int64, device="cuda")
    rc = nd._L.sg_node_local_metrics_device(nd.h, now, C.c_void_p(buf.data_ptr()), total - 1, C.byref(n))
    assert rc == abi.SG_E_CAPACITY and n.value == total
    assert bool((buf == -7).all())
    k = nd.local_metrics_device(now, buf)
    rows = buf[:k].cpu().numpy().copy().view(abi.METRIC_NODE_DTYPE).reshape(-1)
    assert np.array_equal(rows, rows_want)


# ---- the merge kernel alone ----

def _plain_node(K):
    from sentinel_amd.engine import NodeEngine
    rules = np.zeros(K, abi.LOCAL_RULE_DTYPE)
    rules["flow_grade"] = abi.FLOW_GRADE_NONE
    nd = NodeEngine([0], max_batch=1 << 10)
    nd.local_load_rules(rules, 2, 1000, 500)
    return nd


def _raw_parts(rng, K, sec0, seconds, p, forced, entry=True):
    """Raw rows of three "shards" (resource r on shard r % 3): each (second, resource) present with probability p,
    the `forced` resources in every second; ENTRY_NODE rows of the shards in overlapping seconds."""
    fields = ("pass_qps", "block_qps", "success_qps", "exception_qps", "occupied_pass_qps")
    parts = []
    for g in range(3):
        mine = np.arange(g, K, 3)
        take = rng.random((len(seconds), len(mine))) < p
        take[:, np.isin(mine, forced)] = True
        s_idx, r_idx = np.nonzero(take)
        r = np.zeros(len(s_idx), abi.METRIC_NODE_DTYPE)
        r["timestamp"] = 1000 * (sec0 + np.asarray(seconds)[s_idx])
        r["resource"] = mine[r_idx]
        for f in fields:
            r[f] = rng.integers(0, 4, len(r))
        r["rt"] = rng.integers(0, 500, len(r))
        if entry:
            lo, hi = [(0, 40), (20, 59), (10, 31)][g]
            es = [s for s in seconds if lo <= s < hi]
            e = np.zeros(len(es), abi.METRIC_NODE_DTYPE)
            e["timestamp"] = 1000 * (sec0 + np.asarray(es, dtype=np.int64))
            e["resource"] = ENTRY_NODE_RESOURCE
            for f in fields[:4]:
                e[f] = rng.integers(0, 4, len(e))
            e["rt"] = rng.integers(0, 500, len(e))
            for i, s in enumerate(es):
                if s in (5, 22):      # sums of nothing: no valid ENTRY_NODE row (one shard's; all three shards')
                    for f in fields[:4] + ("rt",):
                        e[f][i] = 0
                if s == 25:           # Σsuccess = 0 and Σrt > 0: a valid row carrying the raw rt sum
                    for f in fields[:4]:
                        e[f][i] = 0
                    e["rt"][i] = 17 + g
            r = np.concatenate([r, e])
        parts.append(r[rng.permutation(len(r))])
    return parts


def _merge(nd, rows, cap=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(rows).view(np.int64).reshape(-1, 8).copy()).cuda()
    out = torch.full((len(rows) if cap is None else cap, 8), -7, dtype=torch.int64, device="cuda")
    k = nd.local_merge_rows(t, out, torch.cuda.current_stream().cuda_stream)
    return out[:k].cpu().numpy().copy().view(abi.METRIC_NODE_DTYPE).reshape(-1), out


def test_merge_rows_three_words_ring_wraps():
    """K = 193: three bitmap words, the last one partial; all 59 seconds with the minute ring wrapping; ENTRY_NODE rows
    of three shards in overlapping seconds, two sums invalid, one with Σsuccess = 0 and Σrt > 0; rows in random order."""
    rng = np.random.default_rng(21)
    K = 193
    sec0 = (T0 // 1000) // 60 * 60 + 30   # slot 30 holds the oldest second: slot 0 lies in the middle of the table
    parts = _raw_parts(rng, K, sec0, list(range(59)), 0.3, [63, 64, 127, 128, 192])
    want = merge_metric_rows(parts)
    ent = want[want["resource"] == ENTRY_NODE_RESOURCE]
    ts = (ent["timestamp"] // 1000 - sec0).tolist()
    assert 5 not in ts and 22 not in ts and 25 in ts
    e25 = ent[ts.index(25)]
    assert e25["success_qps"] == 0 and e25["rt"] == 17 + 18 + 19
    assert {63, 64, 127, 128, 192} <= set(want["resource"].tolist())
    nd = _plain_node(K)
    rows = np.concatenate(parts)
    rows = rows[rng.permutation(len(rows))]
    got, _ = _merge(nd, rows)
    assert np.array_equal(got, want)
    got, _ = _merge(nd, rows[:0], cap=4)
    assert len(got) == 0

    # contract errors: SG_E_INVAL, the output untouched
    def refused(bad_rows):
        import torch

        from sentinel_amd.engine import EngineError
        t = torch.from_numpy(bad_rows.view(np.int64).reshape(-1, 8).copy()).cuda()
        out = torch.full((len(bad_rows), 8), -7, dtype=torch.int64, device="cuda")
        with pytest.raises(EngineError) as e:
            nd.local_merge_rows(t, out)
        assert e.value.code == abi.SG_E_INVAL
        assert bool((out == -7).all())

    res_at = np.nonzero(rows["resource"] != ENTRY_NODE_RESOURCE)[0]
    i = int(res_at[len(res_at) // 2])
    refused(np.concatenate([rows, rows[i:i + 1]]))                       # a duplicate far from its twin
    refused(np.concatenate([rows[:i + 1], rows[i:i + 1], rows[i + 1:]]))  # … and next to it
    for field, delta in (("timestamp", 1), ("timestamp", 60_000)):
        bad = rows.copy()
        bad[field][i] += delta
        refused(bad)
    bad = rows.copy()
    bad["resource"][i] = K
    refused(bad)
    got, _ = _merge(nd, rows)   # the scratch of a refused call is cleared by the next
    assert np.array_equal(got, want)
    # a table larger than the buffer: SG_E_CAPACITY with the rows needed, nothing written
    import torch

    from sentinel_amd.engine import EngineError
    t = torch.from_numpy(rows.view(np.int64).reshape(-1, 8).copy()).cuda()
    out = torch.full((len(want) - 1, 8), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(EngineError) as e:
        nd.local_merge_rows(t, out)
    assert e.value.code == abi.SG_E_CAPACITY and e.value.rows == len(want) and bool((out == -7).all())


@pytest.mark.parametrize("K,forced", [(4100, [4095, 4096, 4099]),
                                      (MERGE_PASS_WORDS * 64 + 65, [MERGE_PASS_WORDS * 64 - 1, MERGE_PASS_WORDS * 64,
                                                                    MERGE_PASS_WORDS * 64 + 64])])
def test_merge_rows_many_words(K, forced):
    """K = 4100: 65 words, one more than a wave; K past what one pass of the word scan covers (G = 1: the state of that
    many resources stays small)."""
    rng = np.random.default_rng(K)
    sec0 = (T0 // 1000) // 60 * 60 + 58
    parts = _raw_parts(rng, K, sec0, [0, 1, 3], 0.4, forced)   # slots 58, 59, 1
    want = merge_metric_rows(parts)
    nd = _plain_node(K)
    rows = np.concatenate(parts)
    got, _ = _merge(nd, rows[rng.permutation(len(rows))])
    assert np.array_equal(got, want)
    got, _ = _merge(nd, rows)   # shard by shard, as the node lays them out
    assert np.array_equal(got, want)
