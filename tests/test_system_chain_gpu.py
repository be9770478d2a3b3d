"""SystemSlot inside the whole slot chain on the device against the unmodified oracle.

The oracle has no SystemSlot, so SysChecker (in the manner of tests/test_authority_kat.py::AuthChecker) drives
LocalChain event by event: it generates the exits from the oracle's own passes, runs the Python checkSystem of
tests/system_ref.py on its ENTRY_NODE before every inbound entry, and rewrites a system-blocked entry — in the oracle's
copy only — so that a count-0 flow rule for a reserved origin rejects it (origin := the reserved id, PRIO bit cleared,
args_null = 1: no occupy path, ParamFlowSlot returns at once). The guard: the oracle answers {BLOCK_FLOW, 0} there.
StatisticSlot then counts the same BLOCK on the ClusterNode, the context's DefaultNode and (in the oracle) ENTRY_NODE;
the reserved origin's node is not compared. Inbound entries carry origin 0. The one authority rule (an outbound
resource) is stood for in the same way. Everything else — nodes, controllers, param tables, breakers, metric rows — is
compared as tests/test_slot_chain_gpu.py::_compare does."""
import functools
import heapq

import numpy as np
import pytest

from oracle.binding import LocalChain, ParamFlowSlot, degrade_rule, lib, local_flow_rule, local_rule
from sentinel_amd import abi
from tests.system_ref import EntryNode, SystemConf
from tests.test_authority_kat import BLACK, to_abi
from tests.test_oracle_pslot_kat import QPS, rule as prule

T0 = 1_700_000_000_000
N_RES, N_ORIGINS, N_CTX, RESERVED = 12, 2, 2, 3   # origin ids 1, 2 for the events; 3 only in the oracle
INBOUND = [1] * 7 + [0] * 5
AUTH = [(7, BLACK, [1])]
SYS, FLOW = abi.LOCAL_BLOCK_SYSTEM, abi.LOCAL_BLOCK_FLOW
WU, RL, RELATE = abi.CONTROL_WARM_UP, abi.CONTROL_RATE_LIMITER, abi.STRATEGY_RELATE
BATCHES = ((20_000, 6000), (20_000, 6000), (20_000, 6000))


def R(load=-1.0, cpu=-1.0, qps=-1.0, avg_rt=-1, max_thread=-1):
    return (load, cpu, qps, avg_rt, max_thread)


SYS_RULES = [[R(qps=1e9, max_thread=10 ** 9, avg_rt=10 ** 9)],          # far under: proven clear
             [R(qps=700.0, max_thread=60), R(avg_rt=22)],
             [R(qps=2000.0, max_thread=14, avg_rt=400), R(qps=520.0)]]


def _rules():
    brk = [degrade_rule(abi.DEGRADE_EXCEPTION_RATIO, 0.3, 1, 5, 1000)]
    base = np.array([local_rule(0.0, abi.FLOW_GRADE_NONE, brk if r in (0, 8) else []) for r in range(N_RES)])
    frules = np.array([
        local_flow_rule(0, 60.0),
        local_flow_rule(1, 80.0, behavior=WU, warm_up_sec=3),
        local_flow_rule(2, 100.0, behavior=RL, max_queueing_ms=200),
        local_flow_rule(3, 50.0, strategy=RELATE, ref=9),   # a RELATE pair: 3 is inbound, 9 is not
        local_flow_rule(7, 30.0),
        local_flow_rule(8, 60.0, behavior=RL, max_queueing_ms=100),
        local_flow_rule(9, 70.0),
    ], abi.LOCAL_FLOW_RULE_DTYPE)
    params = np.array([prule(res=4, idx=0, count=6.0, grade=QPS)], abi.PSLOT_RULE_DTYPE)
    return base, frules, params


class SysChecker:
    def __init__(self, base, frules, params):
        added = [local_flow_rule(r, 0.0, limit_app=RESERVED) for r in range(N_RES) if INBOUND[r]]
        added += [local_flow_rule(r, 0.0, limit_app=o) for r, _, ids in AUTH for o in ids]
        self.n_added = len(added)
        self.ora = LocalChain(2, 1000, 500)
        self.ora.load_rules(base)
        self.kept = self.ora.load_flow_rules(np.array(added + list(frules), abi.LOCAL_FLOW_RULE_DTYPE), RESERVED,
                                             N_CTX) - self.n_added
        self.ora.set_entry_types(INBOUND)
        self.ps = ParamFlowSlot(params, n_resources=N_RES)
        self.ora.attach_params(self.ps)
        self.node = EntryNode(2, 1000)
        self.conf = SystemConf()
        self.load = self.cpu = -1.0
        self.pending, self.seq = [], 0
        self.kinds = np.zeros(5, np.int64)
        self._e = np.zeros(1, abi.LOCAL_EVENT_DTYPE)
        self._x = np.zeros(1, abi.SLOT_EXT_DTYPE)
        self._o = np.zeros(1, abi.LOCAL_RES_DTYPE)

    def _oracle(self, e, x, args, values):
        self._e[0], self._x[0] = e, x
        rc = lib().or_local_decide_ext(self.ora.h, abi.ptr(self._e), abi.ptr(self._x), 1, abi.ptr(args),
                                       abi.ptr(values), abi.ptr(self._o))
        assert rc == 0
        return int(self._o[0]["status"]), int(self._o[0]["wait_ms"])

    def batch(self, ent, ext, rt, er, t_end, args, values):
        """Entries → (events, ext records, expected results) of the device."""
        ev, xo, want = [], [], []

        def exits_until(t):
            while self.pending and self.pending[0][0] <= t:
                te, _, e, x = heapq.heappop(self.pending)
                self._oracle(e, x, args, values)
                res = int(e[2])
                if INBOUND[res]:
                    self.node.on_exit(te, int(e[1]), int(e[3]), e[4] == abi.LOCAL_EXIT_ERROR)
                ev.append(e)
                xo.append(x)
                want.append((0, 0))

        for i in range(len(ent)):
            t, word, count, origin = int(ent["ts_ms"][i]), int(ent["resource"][i]), int(ent["count"][i]), int(ent["origin"][i])
            exits_until(t)
            res = word & 0x7FFFFFFF
            x = tuple(int(v) for v in ext[i])
            rejected = any(res == r and origin in ids for r, _, ids in AUTH)
            kind = None
            if INBOUND[res] and not rejected:
                kind = self.node.check(self.conf, t, count, self.load, self.cpu)
            e = (t, 0, word, count, abi.LOCAL_ENTRY, origin)
            if rejected or kind is not None:
                st, wait = self._oracle((t, 0, res, count, abi.LOCAL_ENTRY, RESERVED if kind is not None else origin),
                                        (x[0], x[1], x[2], 1), args, values)
                # the guard: the equivalence holds only while the count-0 rule is what rejected the entry
                assert (st, wait) == (FLOW, 0), "the oracle did not answer {BLOCK_FLOW, 0} at a rewritten entry"
                st, wait = (SYS, kind) if kind is not None else (abi.LOCAL_BLOCK_AUTHORITY, 0)
                if kind is not None:
                    self.kinds[kind] += 1
            else:
                st, wait = self._oracle(e, x, args, values)
            if INBOUND[res]:
                if st == abi.LOCAL_PASS:
                    self.node.on_pass(t, count)
                elif st == abi.LOCAL_PASS_WAIT:
                    self.node.on_pass_wait()
                else:
                    self.node.on_block(t, count)
            if st in (abi.LOCAL_PASS, abi.LOCAL_PASS_WAIT):
                self.seq += 1
                te = t + wait + int(rt[i])
                heapq.heappush(self.pending, (te, self.seq, (te, t, res, count, abi.LOCAL_EXIT_ERROR if er[i] else
                                                             abi.LOCAL_EXIT, origin), x))
            ev.append(e)
            xo.append(x)
            want.append((st, wait))
        exits_until(t_end)
        return (np.array(ev, abi.LOCAL_EVENT_DTYPE), np.array(xo, abi.SLOT_EXT_DTYPE), np.array(want, abi.LOCAL_RES_DTYPE))


@functools.lru_cache(maxsize=None)
def chain_case():
    """The reference of the whole-chain trace (computed once, shared by the flag variants, never modified)."""
    from tests.test_slot_chain_gpu import Pool
    base, frules, params = _rules()
    chk = SysChecker(base, frules, params)
    rng = np.random.default_rng(20261020)
    pool = Pool()
    t = T0 + 137
    batches = []
    for b, (n, span) in enumerate(BATCHES):
        chk.conf = SystemConf(SYS_RULES[b])
        ent = np.zeros(n, abi.LOCAL_EVENT_DTYPE)
        ent["ts_ms"] = t + np.sort(rng.integers(0, span, n))
        res = rng.integers(0, N_RES, n).astype(np.uint32)
        ent["count"] = np.where(rng.random(n) < 0.1, rng.integers(2, 4, n), 1)
        ent["origin"] = np.where(res < 7, 0, rng.integers(0, N_ORIGINS + 1, n))  # inbound entries: origin 0
        ent["resource"] = res | np.where(rng.random(n) < 0.05, np.uint32(abi.KEY_PRIO), np.uint32(0))
        ext = pool.draw(rng, n)
        ext["context"] = rng.integers(0, N_CTX, n)
        args, values = pool.arrays()
        rt = rng.integers(0, 41, n).astype(np.int32)
        er = rng.random(n) < 0.05
        ev, xo, want = chk.batch(ent, ext, rt, er, t + span, args, values)
        for a in (ev, xo, want, args, values):
            a.setflags(write=False)
        batches.append((ev, xo, args, values, want, chk.node.w.dump(), chk.node.threads))
        t += span
    # MetricTimerListener.run once, here: it moves the oracle's minute windows and lastFetchTime, and the reference is
    # shared, so the device fetches its rows at the same time before the states are compared
    rows = chk.ora.metrics(t + 2000)
    rows.setflags(write=False)
    return base, frules, params, chk, batches, pool, (t + 2000, rows)


def test_chain_trace_meets_its_conditions():
    base, frules, params, chk, batches, pool, t_end = chain_case()
    assert chk.kept == len(frules)
    ev = np.concatenate([b[0] for b in batches])
    st = np.concatenate([b[4]["status"] for b in batches])
    entries = ev["kind"] == abi.LOCAL_ENTRY
    assert (np.isin(st[entries], (abi.LOCAL_PASS, abi.LOCAL_PASS_WAIT))).mean() >= 0.30
    assert chk.kinds.sum() >= 50 and (chk.kinds[:3] >= 5).all(), chk.kinds
    assert not (batches[0][4]["status"] == SYS).any() and (batches[1][4]["status"] == SYS).any()
    assert {abi.LOCAL_PASS, FLOW, abi.LOCAL_BLOCK_DEGRADE, abi.LOCAL_BLOCK_PARAM, abi.LOCAL_BLOCK_AUTHORITY, SYS,
            abi.LOCAL_PASS_WAIT} <= set(st.tolist())
    blocked = st == SYS
    assert ((ev["resource"][blocked] & np.uint32(abi.KEY_PRIO)) != 0).any()       # a prioritized system block
    assert (ev["resource"][blocked] & np.uint32(0x7FFFFFFF) == 4).any()           # ... one on the param-rule resource
    assert (ev["resource"][blocked] & np.uint32(0x7FFFFFFF) == 3).any()           # ... and one on the RELATE member


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, abi.FLAG_SERIAL_ONLY, abi.FLAG_WAVE_ONLY])
def test_whole_chain_against_the_oracle(flags):
    from sentinel_amd.cluster import ENTRY_NODE_RESOURCE
    from sentinel_amd.engine import FlowEngine
    from tests.test_slot_chain_gpu import _compare
    base, frules, params, chk, batches, pool, t_end = chain_case()
    eng = FlowEngine(device=0, max_batch=1 << 16, flags=flags)
    eng.local_load_rules(base, 2, 1000, 500)
    assert eng.local_load_flow_rules(frules, N_ORIGINS, N_CTX) == chk.kept
    eng.pslot_load_rules(params, n_resources=N_RES)
    assert eng.local_load_authority_rules(*to_abi(AUTH), N_ORIGINS) == len(AUTH)
    eng.local_set_entry_types(INBOUND)
    for b, (ev, xo, args, values, want, entry_sec, entry_thr) in enumerate(batches):
        rows = np.zeros(len(SYS_RULES[b]), abi.SYSTEM_RULE_DTYPE)
        for i, r in enumerate(SYS_RULES[b]):
            rows[i] = r
        assert eng.local_load_system_rules(rows) == 1
        got = eng.slot_decide_host(ev, xo, args, values)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            i = bad[0]
            raise AssertionError(f"batch {b}: {len(bad)} results differ; first at {i}: ev={ev[i]} ext={xo[i]} "
                                 f"expected={want[i]} gpu={got[i]}")
        sec, thr = eng.local_entry_node()
        assert np.array_equal(sec, entry_sec) and thr == entry_thr, f"ENTRY_NODE after batch {b}:\n{sec}\nvs\n{entry_sec}"
        assert eng.local_system_last_path() == (2 if (want["status"] == SYS).any() else 1), b
    now, m_o = t_end
    m_g = eng.local_metrics(now)
    e_o, e_g = m_o[m_o["resource"] == ENTRY_NODE_RESOURCE], m_g[m_g["resource"] == ENTRY_NODE_RESOURCE]
    assert len(e_o) > 0 and np.array_equal(e_o, e_g), "ENTRY_NODE metric rows"
    assert np.array_equal(m_o, m_g), "metric rows"
    _compare(eng, chk.ora, chk.ps, frules[:0], params, N_RES, N_ORIGINS, N_CTX, pool)
    for i in range(len(frules)):  # the oracle's controllers follow the rules the checker added
        w = chk.ora.controller(i + chk.n_added)
        if w is not None:
            assert np.array_equal(w, eng.local_controller(i)), f"controller of rule {i}"
