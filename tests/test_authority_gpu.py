"""AuthoritySlot on the device (sg_local_load_authority_rules): every result and the whole chain state against the
oracle run that tests/test_authority_kat.py shows equivalent (count-0 origin flow rules standing for the black and
white lists, the two corrections applied to the oracle's copy of the trace only), hand-traced cases for what the
equivalence cannot show, the load contract, a refused batch, and the node handle."""
import functools

import numpy as np
import pytest

from oracle.binding import degrade_rule, local_flow_rule, local_rule
from sentinel_amd import abi
from sentinel_amd.cluster import ENTRY_NODE_RESOURCE
from tests.test_authority_kat import BLACK, MIXED, WHITE, AuthChecker, mixed_case, random_authority_rules, to_abi
from tests.test_oracle_pslot_kat import rule as prule
from tests.test_slot_chain_gpu import OTHER, RL, WU, Pool, _compare, _entries, _flow_rules

pytestmark = pytest.mark.gpu

AUTH = abi.LOCAL_BLOCK_AUTHORITY
T0 = 1_700_000_000_000
NO_PARAMS = np.zeros(0, abi.PSLOT_RULE_DTYPE)


def _engine(flags=0, max_batch=1 << 20):
    from sentinel_amd.engine import FlowEngine
    return FlowEngine(device=0, max_batch=max_batch, flags=flags)


def _code(call, *args):
    from sentinel_amd.engine import EngineError
    with pytest.raises(EngineError) as e:
        call(*args)
    return e.value.code


def _device(base, frules, params, auth, n_origins, n_ctx, flags=0, kept=None):
    eng = _engine(flags)
    eng.local_load_rules(base, 2, 1000, 500)
    k = eng.local_load_flow_rules(frules, n_origins, n_ctx)
    assert kept is None or k == kept
    if params is not None:
        eng.pslot_load_rules(params, n_resources=len(base))
    rules, ids = to_abi(auth)
    assert eng.local_load_authority_rules(rules, ids, n_origins) == len(auth)
    return eng


def _check_batches(eng, batches):
    for b, (ev, xo, args, values, want) in enumerate(batches):
        got = eng.slot_decide_host(ev, xo, args, values)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            i = bad[0]
            raise AssertionError(f"batch {b}: {len(bad)} results differ; first at {i}: ev={ev[i]} ext={xo[i]} "
                                 f"expected={want[i]} gpu={got[i]}")


def _check_state(eng, chk, n_res, n_origins, n_ctx, pool):
    # (the flow controllers apart: the oracle's indices are shifted by the rules the checker added)
    _compare(eng, chk.ora, chk.ps, chk.frules[:0], chk.params if chk.params is not None else NO_PARAMS, n_res,
             n_origins, n_ctx, pool)
    for i in range(len(chk.frules)):
        want = chk.ora.controller(i + chk.n_added)
        if want is not None:
            assert np.array_equal(want, eng.local_controller(i)), f"controller of rule {i}"


# ---- 1. the mixed chain

@pytest.mark.parametrize("flags", [0, abi.FLAG_SERIAL_ONLY, abi.FLAG_WAVE_ONLY])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mixed_chain_with_authority_rules(flags, seed):
    base, frules, params, auth, chk, batches, pool, n_rej = mixed_case(seed)
    assert n_rej > 1000
    eng = _device(base, frules, params, auth, MIXED["n_origins"], MIXED["n_ctx"], flags, kept=chk.kept)
    _check_batches(eng, batches)
    _check_state(eng, chk, MIXED["n_res"], MIXED["n_origins"], MIXED["n_ctx"], pool)


# ---- 2. dead periods

DEAD_AUTH = [(0, BLACK, [1]), (2, BLACK, [2]), (7, WHITE, [1, 2])]


@functools.lru_cache(maxsize=None)
def _dead_case():
    """test_slot_chain_gpu.test_dead_periods' rules, params and sizes with three authority rules: the reference of
    every env / flags variant (computed once, never modified)."""
    rng = np.random.default_rng(21)
    n_res, n_origins = 12, 3
    sets = [[local_flow_rule(0, 30.0), local_flow_rule(0, 6.0, limit_app=1)],
            [local_flow_rule(1, 25.0, behavior=WU, warm_up_sec=3)],
            [local_flow_rule(2, 40.0)],
            [local_flow_rule(3, 20.0), local_flow_rule(3, 4.0, limit_app=OTHER)],
            [local_flow_rule(4, 15.0)],
            [local_flow_rule(5, 12.0, behavior=WU, warm_up_sec=2)],
            [local_flow_rule(6, 50.0)],
            [local_flow_rule(7, 8.0), local_flow_rule(7, 2.0, limit_app=2)],
            [local_flow_rule(8, 5.0)], [local_flow_rule(9, 60.0)], [], [local_flow_rule(11, 3.0)]]
    params = np.array([prule(res=2, idx=0, count=8.0), prule(res=4, idx=0, count=3.0, dur=2),
                       prule(res=6, idx=0, count=20.0, behavior=abi.BEHAVIOR_RATE_LIMITER, max_q=50),
                       prule(res=9, idx=1, count=5.0), prule(res=10, idx=0, count=4.0)], abi.PSLOT_RULE_DTYPE)
    base = np.zeros(n_res, abi.LOCAL_RULE_DTYPE)
    for r in range(n_res):
        base[r] = local_rule(0.0, abi.FLOW_GRADE_NONE,
                             [degrade_rule(abi.DEGRADE_EXCEPTION_RATIO, 0.3, 1, 5, 1000)] if r % 4 == 0 else [])
    flat = [x for rs in sets for x in rs]
    rng.shuffle(flat)
    frules = np.array(flat, abi.LOCAL_FLOW_RULE_DTYPE)
    chk = AuthChecker(base, frules, params, DEAD_AUTH, n_res, n_origins, 0)
    rng = np.random.default_rng(21 + 1000)
    pool = Pool()
    t = T0 + int(rng.integers(0, 1000))
    batches, n_rej = [], 0
    for n, span in [(60_000, 3000), (60_000, 2500), (30_000, 4000)]:
        ent = _entries(rng, n, n_res, t, span, n_origins, zipf=1.2, prio=0.0)
        ext = pool.draw(rng, n)
        ext["context"] = 0
        args, values = pool.arrays()
        rt = rng.integers(0, 41, n).astype(np.int32)
        er = (rng.random(n) < 0.05).astype(np.uint8)
        ev, xo, want, k = chk.batch(ent, ext, rt, er, t + span, args, values)
        n_rej += k
        for a in (ev, xo, want, args, values):
            a.setflags(write=False)
        batches.append((ev, xo, args, values, want))
        t += span
    return base, frules, params, chk, batches, pool, n_rej


@pytest.mark.parametrize("env", [{}, {"SG_CXW_MIN": "17"}, {"SG_CXW": "0"}, {"SG_TEST_CXSIDE_POISON": "1"}],
                         ids=["default", "cxw17", "lanes", "cxside_poison"])
@pytest.mark.parametrize("flags", [0, abi.FLAG_SERIAL_ONLY, abi.FLAG_WAVE_ONLY])
def test_dead_periods_with_authority_rules(flags, env, monkeypatch):
    """Rejected entries inside the cx walkers' dead periods: they add BLOCK to the ClusterNode and their origin node
    and nothing else — resource 2's param table and token state (one QPS param rule) stay the oracle's — and keep
    prep's default result."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SG_DEBUG", "64")
    base, frules, params, chk, batches, pool, n_rej = _dead_case()
    assert n_rej > 5000
    eng = _device(base, frules, params, DEAD_AUTH, 3, 0, flags, kept=chk.kept)
    _check_batches(eng, batches)
    _check_state(eng, chk, 12, 3, 0, pool)
    if flags != abi.FLAG_SERIAL_ONLY and env.get("SG_CXW") != "0":  # the wave walker decided dead chunks
        d = eng.debug_copy(5, np.uint64, 32)
        assert d[20] > 0 and d[23] > 0, f"wave walker segments {d[20]}, dead chunks {d[23]}"


# ---- 3. hand-traced cases

def _events(rows):
    """rows: (ts offset, resource, count, origin[, prio])"""
    ev = np.zeros(len(rows), abi.LOCAL_EVENT_DTYPE)
    for i, r in enumerate(rows):
        ev[i]["ts_ms"], ev[i]["resource"], ev[i]["count"], ev[i]["origin"] = T0 + r[0], r[1], r[2], r[3]
        if len(r) > 4 and r[4]:
            ev[i]["resource"] |= abi.KEY_PRIO
    return ev


def _simple(frules, auth, n_res=1, n_origins=2):
    base = np.array([local_rule() for _ in range(n_res)], abi.LOCAL_RULE_DTYPE)
    fr = np.array(frules, abi.LOCAL_FLOW_RULE_DTYPE) if frules else np.zeros(0, abi.LOCAL_FLOW_RULE_DTYPE)
    return _device(base, fr, None, auth, n_origins, 0)


def test_prioritized_rejected_entry():
    """No PriorityWaitException for an AuthorityException: status 5, wait 0, no occupied window on the ClusterNode or
    the origin node, no thread count; BLOCK = count on both."""
    eng = _simple([local_flow_rule(0, 1.0)], [(0, BLACK, [1])])
    borrow0 = eng.local_state(0)[1].copy()
    got = eng.local_decide_host(_events([(0, 0, 1, 0), (1, 0, 3, 1, True)]))
    assert got.tolist() == [(abi.LOCAL_PASS, 0), (AUTH, 0)]
    sec, bor, mnt, head = eng.local_state(0)
    assert np.array_equal(bor, borrow0) and head[0] == 1              # (the passed entry's thread)
    assert sec[:, 2].sum() == 3 and mnt[:, 2].sum() == 3 and sec[:, 6].sum() == 0
    so, bo, mo, ho, exists = eng.local_origin_state(0, 1, with_exists=True)
    assert exists and np.array_equal(bo, borrow0) and ho[0] == 0
    assert so[:, 2].sum() == 3 and mo[:, 2].sum() == 3 and so[:, 1].sum() == 0


def test_rejected_entry_creates_the_nodes():
    """The first event ever of resource 1 is rejected: ClusterBuilderSlot has run, so its origin node exists with
    BLOCK = count, and resource 0's RELATE rule (count 0: it passes only while resource 1 has no ClusterNode) now
    reads a ClusterNode."""
    eng = _simple([local_flow_rule(0, 0.0, strategy=abi.STRATEGY_RELATE, ref=1)], [(1, BLACK, [1])], n_res=2)
    assert not eng.local_origin_state(1, 1, with_exists=True)[4]
    got = eng.local_decide_host(_events([(0, 0, 1, 0), (0, 1, 2, 1), (0, 0, 1, 0)]))
    assert got["status"].tolist() == [abi.LOCAL_PASS, AUTH, abi.LOCAL_BLOCK_FLOW]
    so, bo, mo, ho, exists = eng.local_origin_state(1, 1, with_exists=True)
    assert exists and so[:, 2].sum() == 2 and mo[:, 2].sum() == 2


def test_rejected_entry_leaves_the_rate_limiter():
    eng = _simple([local_flow_rule(0, 10.0, behavior=RL, max_queueing_ms=500)], [(0, BLACK, [2])])
    assert eng.local_decide_host(_events([(0, 0, 1, 1)]))["status"].tolist() == [abi.LOCAL_PASS]
    ctl = eng.local_controller(0).copy()
    assert ctl[2] == T0                                                # latestPassedTime
    got = eng.local_decide_host(_events([(700, 0, 1, 2), (700, 0, 1, 2)]))
    assert got.tolist() == [(AUTH, 0), (AUTH, 0)]
    assert np.array_equal(eng.local_controller(0), ctl)


def test_entry_node_counts_rejected_entries():
    eng = _simple([], [(0, BLACK, [1])])
    eng.local_set_entry_types(np.array([1], np.uint8))
    got = eng.local_decide_host(_events([(0, 0, 2, 1), (5, 0, 3, 1), (6, 0, 1, 2)]))
    assert got["status"].tolist() == [AUTH, AUTH, abi.LOCAL_PASS]
    rows = eng.local_metrics(T0 + 2000)
    total = rows[rows["resource"] == ENTRY_NODE_RESOURCE]
    assert len(total) == 1 and total["block_qps"][0] == 5 and total["pass_qps"][0] == 1
    own = rows[rows["resource"] == 0]
    assert len(own) == 1 and own["block_qps"][0] == 5


# ---- 4. the load contract

def test_reload_black_white_none_keeps_statistics():
    eng = _simple([], [(0, BLACK, [1])])
    ev = lambda dt: _events([(dt, 0, 1, 1), (dt, 0, 1, 2), (dt, 0, 1, 0)])  # noqa: E731
    assert eng.local_decide_host(ev(0))["status"].tolist() == [AUTH, abi.LOCAL_PASS, abi.LOCAL_PASS]
    rules, ids = to_abi([(0, WHITE, [1])])
    assert eng.local_load_authority_rules(rules, ids) == 1
    assert eng.local_decide_host(ev(10))["status"].tolist() == [abi.LOCAL_PASS, AUTH, abi.LOCAL_PASS]
    assert eng.local_load_authority_rules(rules[:0], ids[:0]) == 0
    assert eng.local_decide_host(ev(20))["status"].tolist() == [abi.LOCAL_PASS] * 3
    sec, bor, mnt, head = eng.local_state(0)
    assert mnt[:, 1].sum() == 7 and mnt[:, 2].sum() == 2 and head[0] == 7
    assert eng.local_origin_state(0, 1)[2][:, 2].sum() == 1 and eng.local_origin_state(0, 2)[2][:, 2].sum() == 1


def test_return_value_counts_the_kept_rules():
    eng = _simple([], [], n_res=3)
    rules, ids = to_abi([(0, BLACK, [1]), (0, WHITE, [1]), (1, -1, [1]), (1, 2, [1]), (1, BLACK, [1]), (2, BLACK, [])])
    assert eng.local_load_authority_rules(rules, ids, 2) == 2
    got = eng.local_decide_host(_events([(0, 0, 1, 1), (0, 1, 1, 1), (0, 2, 1, 1)]))
    assert got["status"].tolist() == [AUTH, abi.LOCAL_PASS, abi.LOCAL_PASS]   # strategy 2 shadows the black list


def test_invalid_loads():
    fresh = _engine()
    rules, ids = to_abi([(0, BLACK, [1])])
    assert _code(fresh.local_load_authority_rules, rules, ids, 1) == abi.SG_E_INVAL    # before sg_local_load_rules
    eng = _simple([], [(0, BLACK, [1])], n_res=2)
    for bad in ([(2, BLACK, [1])], [(0, BLACK, [0])], [(0, WHITE, [1, -4])]):
        r, o = to_abi(bad)
        assert _code(eng.local_load_authority_rules, r, o, 2) == abi.SG_E_INVAL
    r, o = to_abi([(0, BLACK, [1, 2])])
    assert _code(eng.local_load_authority_rules, r, o[:1], 2) == abi.SG_E_INVAL       # a range past n_origin_ids
    # a failed load leaves the previous rules in force
    assert eng.local_decide_host(_events([(0, 0, 1, 1), (0, 0, 1, 2)]))["status"].tolist() == [AUTH, abi.LOCAL_PASS]


def test_ids_above_64_use_the_sorted_tail():
    eng = _simple([], [(0, BLACK, [200, 3, 65]), (1, WHITE, [64, 65, 200])], n_res=2, n_origins=200)
    origins = [3, 64, 65, 66, 199, 200, 0]
    got = eng.local_decide_host(_events([(0, r, 1, o) for r in (0, 1) for o in origins]))
    black = [AUTH, 0, AUTH, 0, 0, AUTH, 0]
    white = [AUTH, 0, 0, AUTH, AUTH, 0, 0]
    assert got["status"].tolist()[:7] == black and got["status"].tolist()[7:] == white


def test_fresh_resources_drop_the_lists():
    eng = _simple([], [(0, BLACK, [1])])
    assert eng.local_decide_host(_events([(0, 0, 1, 1)]))["status"].tolist() == [AUTH]
    eng.local_load_rules(np.array([local_rule()], abi.LOCAL_RULE_DTYPE), 2, 1000, 500)
    assert eng.local_load_flow_rules(np.zeros(0, abi.LOCAL_FLOW_RULE_DTYPE), 2, 0) == 0
    assert eng.local_decide_host(_events([(0, 0, 1, 1)]))["status"].tolist() == [abi.LOCAL_PASS]


def test_authority_load_declares_origins():
    eng = _engine()
    eng.local_load_rules(np.array([local_rule()], abi.LOCAL_RULE_DTYPE), 2, 1000, 500)
    ev = _events([(0, 0, 1, 2)])
    assert _code(eng.local_decide_host, ev) == abi.SG_E_INVAL
    rules, ids = to_abi([(0, WHITE, [1])])
    assert eng.local_load_authority_rules(rules, ids, 2) == 1
    assert eng.local_decide_host(ev)["status"].tolist() == [AUTH]
    assert eng.local_load_authority_rules(rules, ids, 0) == 1                          # the count never shrinks
    assert eng.local_decide_host(_events([(1, 0, 1, 2), (1, 0, 1, 1)]))["status"].tolist() == [AUTH, abi.LOCAL_PASS]


# ---- 5. a refused batch

def test_refused_batch_changes_nothing():
    rng = np.random.default_rng(5)
    n_res, n_origins = 6, 3
    base = np.array([local_rule() for _ in range(n_res)], abi.LOCAL_RULE_DTYPE)
    frules = np.array([local_flow_rule(r, 20.0) for r in range(n_res)] + [local_flow_rule(1, 3.0, limit_app=2)],
                      abi.LOCAL_FLOW_RULE_DTYPE)
    auth = [(0, BLACK, [1]), (1, WHITE, [2]), (3, BLACK, [1, 2, 3])]
    chk = AuthChecker(base, frules, NO_PARAMS, auth, n_res, n_origins, 0)
    eng = _device(base, frules, NO_PARAMS, auth, n_origins, 0, kept=chk.kept)
    bad = _entries(rng, 3000, n_res, T0, 1000, n_origins, prio=0.0)
    assert chk.rejected(bad).sum() > 300
    bad["ts_ms"][2000] = bad["ts_ms"][1999] - 1
    assert _code(eng.local_decide_host, bad) == abi.SG_E_TIME
    for r in range(n_res):
        sec, bor, mnt, head = eng.local_state(r)
        assert sec[:, 1:7].sum() == 0 and mnt[:, 1:7].sum() == 0 and head[0] == 0
        assert not any(eng.local_origin_state(r, o, with_exists=True)[4] for o in range(1, n_origins + 1))
    pool = Pool()
    ent = _entries(rng, 4000, n_res, T0, 1500, n_origins)
    ext = np.zeros(len(ent), abi.SLOT_EXT_DTYPE)
    ext["args_null"] = 1
    args, values = pool.arrays()
    ev, xo, want, k = chk.batch(ent, ext, rng.integers(0, 41, len(ent)).astype(np.int32),
                                np.zeros(len(ent), np.uint8), T0 + 1500, args, values)
    assert k > 300
    assert np.array_equal(eng.local_decide_host(ev), want)
    _check_state(eng, chk, n_res, n_origins, 0, pool)


# ---- 6. the node handle

@pytest.mark.parametrize("G", [2, 3])
def test_node_equals_one_handle(G):
    from sentinel_amd.engine import NodeEngine
    rng = np.random.default_rng(60)
    n_res, n_origins, max_batch = 24, 3, 1 << 15
    base = np.zeros(n_res, abi.LOCAL_RULE_DTYPE)
    for r in range(n_res):
        base[r] = local_rule(0.0, abi.FLOW_GRADE_NONE,
                             [degrade_rule(abi.DEGRADE_EXCEPTION_RATIO, 0.3, 1, 5, 1000)] if r % 4 == 0 else [])
    flat = [x for r in range(n_res) for x in _flow_rules(rng, r, n_res, n_origins, 1)
            if x["strategy"] != abi.STRATEGY_CHAIN]          # (no contexts over the node)
    frules = np.array(flat, abi.LOCAL_FLOW_RULE_DTYPE)
    auth = random_authority_rules(rng, n_res)
    inbound = (np.arange(n_res) % 3 == 0).astype(np.uint8)
    chk = AuthChecker(base, frules, None, auth, n_res, n_origins, 0, inbound=inbound)
    ent = _entries(rng, 10_000, n_res, T0, 2000, n_origins)
    ext = np.zeros(len(ent), abi.SLOT_EXT_DTYPE)
    ext["args_null"] = 1
    ev, xo, want, k = chk.batch(ent, ext, rng.integers(0, 41, len(ent)).astype(np.int32),
                                (rng.random(len(ent)) < 0.05).astype(np.uint8), T0 + 2000,
                                np.zeros(1, abi.PSLOT_ARG_DTYPE), np.zeros(1, np.uint64))
    assert k > 500 and len(ev) > len(ent) and len(ev) <= max_batch
    rules, ids = to_abi(auth)
    one = _engine(max_batch=max_batch)
    nd = NodeEngine([0] * G, max_batch=max_batch)
    for e in (one, nd):
        e.local_load_rules(base, 2, 1000, 500)
        assert e.local_load_flow_rules(frules, n_origins, 0) == chk.kept
        assert e.local_load_authority_rules(rules, ids, n_origins) == len(auth)
        e.local_set_entry_types(inbound)
    assert len({nd.local_owner_of(r) for r in range(n_res)}) == G
    got_one, got_nd = one.local_decide_host(ev), nd.local_decide_host(ev)
    assert np.array_equal(got_one, want) and np.array_equal(got_nd, want)
    now = T0 + 3000
    rows = one.local_metrics(now)
    assert np.array_equal(nd.local_metrics(now), rows) and np.array_equal(rows, chk.ora.metrics(now))
    assert (rows["resource"] == ENTRY_NODE_RESOURCE).any()
    for r in range(n_res):
        for a, w in zip(nd.local_state(r), one.local_state(r)):
            assert np.array_equal(a, w), f"resource {r}: state differs from one handle's"
    r, o = to_abi([(n_res, BLACK, [1])])
    assert _code(nd.local_load_authority_rules, r, o, n_origins) == abi.SG_E_INVAL
    assert np.array_equal(nd.local_decide_host(ev[:0]), want[:0])
