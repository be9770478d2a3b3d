"""LogSlot's rollup on the device (sg_local_block_log_enable / sg_local_block_log) against the model of
tests/blocklog_ref.py: device rows equal model rows exactly — every field, order included. The statuses the rows are
built from are the oracle's (or, for AuthoritySlot and SystemSlot, which the oracle lacks, tests/test_authority_kat.py's
predicate and tests/system_ref.py's chain), and the device's results are compared with them first; the failing flow
rule of the mixed-limitApp resources comes from blocklog_ref.MixedFlow, which tests/test_blocklog_kat.py pins to the
oracle on these same traces."""
import numpy as np
import pytest

from oracle.binding import LocalChain, ParamFlowSlot, degrade_rule, local_flow_rule, local_rule
from sentinel_amd import abi
from tests import blocklog_ref as ref
from tests.blocklog_ref import DEFAULT, FLOW, T0, Args, BlockLog, entries, log_batch
from tests.test_authority_kat import BLACK, to_abi
from tests.test_oracle_pslot_kat import rule as prule

pytestmark = pytest.mark.gpu
BLOCK0 = local_rule(0.0, abi.FLOW_GRADE_QPS)   # the lane walkers' one rule, count 0: every entry is a FlowException


def _engine(base, frules=None, n_origins=0, log2=10, max_batch=1 << 13, flags=0, kept=None):
    from sentinel_amd.engine import FlowEngine
    eng = FlowEngine(device=0, max_batch=max_batch, flags=flags)
    eng.local_load_rules(np.array(base), 2, 1000, 500)
    if frules is not None:
        assert eng.local_load_flow_rules(frules, n_origins) == (len(frules) if kept is None else kept)
    if log2 is not None:
        eng.block_log_enable(log2)
    return eng


def _oracle(base, frules=None, n_origins=0, kept=None):
    ora = LocalChain(2, 1000, 500)
    ora.load_rules(np.array(base))
    if frules is not None:
        assert ora.load_flow_rules(frules, n_origins) == (len(frules) if kept is None else kept)
    return ora


def _same(got, want, what="rows"):
    assert got.dtype == want.dtype and len(got) == len(want) and np.array_equal(got, want), \
        f"{what}: device\n{got}\nmodel\n{want}"


def _fetch(eng, now, want, lost=(0, 0)):
    rows, le, lc = eng.block_log(now)
    _same(rows, want)
    assert (le, lc) == lost, f"lost {(le, lc)}, expected {lost}"


# ---------------------------------------------------------------- sizes, seconds, counts

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2049, 8193])   # a wave's span + 1, a block's four spans + 1
def test_one_key_wave_combine_tail_and_cross_wave_add(n):
    eng, ora = _engine([BLOCK0], max_batch=1 << 14), _oracle([BLOCK0])
    ev = entries(T0 + np.arange(n) * 999 // n, 0)
    want = ora.decide(ev)
    assert (want["status"] == FLOW).all()
    _same(eng.local_decide_host(ev), want, "results")
    log = BlockLog()
    log_batch(log, ev, want)
    rows = log.roll(T0 + 1000)
    assert len(rows) == 1 and rows[0]["count"] == n
    _fetch(eng, T0 + 1000, rows)


def test_alternating_keys_and_a_second_boundary_inside_a_wave():
    fr = np.array([local_flow_rule(0, 0.0)], abi.LOCAL_FLOW_RULE_DTYPE)
    eng, ora = _engine([local_rule()], fr, 1), _oracle([local_rule()], fr, 1)
    n = 128
    ts = np.where(np.arange(n) < 40, T0 + 900 + np.arange(n), T0 + 1000 + np.arange(n))
    ev = entries(ts, 0, 1, np.arange(n) % 2)          # origins 0, 1 lane by lane; the second turns at lane 40
    want = ora.decide(ev)
    _same(eng.local_decide_host(ev), want, "results")
    log = BlockLog()
    log_batch(log, ev, want)
    rows = log.roll(T0 + 2000)
    assert [int(c) for c in rows["count"]] == [20, 20, 44, 44]
    _fetch(eng, T0 + 2000, rows)


def test_counts_above_one_and_a_sum_past_2_to_31():
    eng, ora = _engine([BLOCK0, BLOCK0]), _oracle([BLOCK0, BLOCK0])
    big = np.iinfo(np.int32).max
    ev = entries(T0 + np.arange(7), [0, 0, 0, 1, 1, 1, 1], [big, big - 1, big, 2, 3, 1, 5])
    want = ora.decide(ev)
    assert (want["status"] == FLOW).all()
    _same(eng.local_decide_host(ev), want, "results")
    log = BlockLog()
    log_batch(log, ev, want)
    rows = log.roll(T0 + 1000)
    assert [int(c) for c in rows["count"]] == [3 * big - 1, 11] and 3 * big - 1 > 1 << 32
    _fetch(eng, T0 + 1000, rows)


# ---------------------------------------------------------------- FlowException: which rule failed

@pytest.mark.parametrize("reload", [False, True])
def test_mixed_limit_apps_a_second_over_two_batches_and_a_fetch_between(reload):
    """{origin 1, other, default} on resource 0, each failing first for some entry of one saturated second; the second
    spans the two batches (one row per key comes out); a fetch between them takes nothing; with `reload` the flow
    rules are loaded again between the batches and the pending rows stay."""
    batches, decided, _ = ref.mixed_case()
    fr = ref.mixed_flow_rules()
    base = [local_rule()] * ref.MIXED_N_RES
    eng = _engine(base, fr, ref.MIXED_N_ORIGINS)
    for b, (ev, (st, app)) in enumerate(zip(batches, decided)):
        got = eng.local_decide_host(ev)
        assert np.array_equal(got["status"], st) and not got["wait_ms"].any(), f"results of batch {b}"
        if b == 0:
            _fetch(eng, T0 + 999, np.zeros(0, abi.BLOCK_ROW_DTYPE))      # the open second stays
            if reload:
                assert eng.local_load_flow_rules(fr, ref.MIXED_N_ORIGINS) == len(fr)
    rows, log = ref.mixed_rows(T0 + 1000)
    _fetch(eng, T0 + 1000, rows)
    _fetch(eng, T0 + 1000, rows[:0])                                     # a second fetch returns nothing
    _fetch(eng, T0 + 2000, log.roll(T0 + 2000))                          # the survivors were put back whole
    assert log.pending() == 0
    _fetch(eng, T0 + 9000, rows[:0])


def _hot_case(rules, dropped=()):
    """dropped: rules the load drops (an invalid ClusterFlowConfig), with limitApps of their own."""
    fr = np.array([local_flow_rule(0, c, limit_app=a) for c, a in rules] +
                  [local_flow_rule(0, c, limit_app=a, cluster_mode=abi.CLUSTER_MODE_INVALID) for c, a in dropped],
                  abi.LOCAL_FLOW_RULE_DTYPE)
    ev = entries(T0 + np.sort(np.arange(1500) * 997 % 1000), 0, 1, 0)   # one saturated second, long enough for a wave
    model = ref.MixedFlow([(0, c, a) for c, a in rules])
    out = [model.entry(int(e["ts_ms"]), 0, 0, 1) for e in ev]
    st = np.array([s for s, _ in out], np.int32)
    app = [DEFAULT if a is None else a for _, a in out]
    want = np.zeros(len(ev), abi.LOCAL_RES_DTYPE)
    want["status"] = st
    _same(_oracle([local_rule()], fr, 1, kept=len(rules)).decide(ev), want, "model against the oracle")
    log = BlockLog()
    log_batch(log, ev, want, flow_app=lambda i: app[i])
    return fr, ev, want, log.roll(T0 + 1000)


def test_dead_periods_stay_for_a_uniform_resource_and_stop_for_a_mixed_one(monkeypatch):
    """The wave walker's counters (SG_DEBUG bit 64): a cx resource whose rules share one limitApp still starts dead
    periods with the log on — also when a rule with another limitApp was dropped at load, so the table is computed
    over the rules the library keeps —; a mixed-limitApp resource walks entry by entry (no dead chunk). All give the
    oracle's results and the model's rows."""
    monkeypatch.setenv("SG_DEBUG", "64")
    for rules, dropped, dead in (([(5.0, DEFAULT), (9.0, DEFAULT)], (), True),
                                 ([(5.0, DEFAULT), (9.0, DEFAULT)], [(1.0, 1)], True),
                                 ([(5.0, DEFAULT), (9.0, 1)], (), False)):
        fr, ev, want, rows = _hot_case(rules, dropped)
        eng = _engine([local_rule()], fr, 1, kept=len(rules))
        _same(eng.local_decide_host(ev), want, "results")
        d = eng.debug_copy(5, np.uint64, 32)
        assert d[20] > 0, "the wave walker took no segment"
        assert (d[23] > 0) == dead, f"dead chunks {d[23]} with rules {rules}"
        assert len(rows) == 1 and rows[0]["count"] == 1495
        _fetch(eng, T0 + 1000, rows)


# ---------------------------------------------------------------- the other exception classes

def test_embedded_server_blocked_logs_the_cluster_rules_limit_app():
    """FLOW on an embedded token server's BLOCKED: a mixed-limitApp resource whose cluster-mode rule ("default") the
    server refuses, beside an origin rule that fails first for its origin."""
    from sentinel_amd.engine import FlowEngine
    fr, ev, st, app = ref.embedded_case()
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"] = 1
    c3 = np.zeros(1, abi.RULE_DTYPE)
    c3["flow_id"], c3["count"], c3["threshold_type"] = 77, float(ref.EMB_SERVER_COUNT), abi.THRESHOLD_GLOBAL
    c3["sample_count"], c3["window_interval_ms"], c3["namespace_id"] = 2, 1000, 0
    eng = FlowEngine(device=0, max_batch=1 << 10)
    eng.set_namespaces(ns)
    eng.load_rules(c3)
    eng.local_load_rules(np.array([local_rule()]), 2, 1000, 500)
    assert eng.local_load_flow_rules(fr, 2) == 2
    eng.local_set_cluster_state(abi.CLUSTER_SERVER)
    eng.block_log_enable(6)
    got = eng.local_decide_host(ev)
    assert np.array_equal(got["status"], st) and not got["wait_ms"].any(), got
    want = np.zeros(len(ev), abi.LOCAL_RES_DTYPE)
    want["status"] = st
    log = BlockLog()
    log_batch(log, ev, want, flow_app=lambda i: app[i])
    rows = log.roll(T0 + 1000)
    assert [(int(r["app"]), int(r["origin"]), int(r["count"])) for r in rows] == [(0, 0, 2), (0, 2, 1), (1, 1, 3)]
    _fetch(eng, T0 + 1000, rows)


def test_priority_wait_passes_and_logs_nothing():
    base, ev = ref.wait_case()
    eng, ora = _engine(base), _oracle(base)
    want = ora.decide(ev)
    assert (want["status"] == abi.LOCAL_PASS_WAIT).any()
    _same(eng.local_decide_host(ev), want, "results")
    log = BlockLog()
    log_batch(log, ev, want)
    rows = log.roll(T0 + 1000)
    assert len(rows) == 1 and rows[0]["count"] == int((want["status"] == FLOW).sum())
    _fetch(eng, T0 + 1000, rows)


def test_degrade_exception_and_exits_log_nothing():
    brk = [degrade_rule(abi.DEGRADE_EXCEPTION_COUNT, 1.0, 10, 1, 1000)]
    base = [local_rule(0.0, abi.FLOW_GRADE_NONE, brk)]
    ev = np.zeros(10, abi.LOCAL_EVENT_DTYPE)
    for i in range(2):                                   # two entries that fail: the breaker opens
        ev[2 * i] = (T0 + 10 * i, 0, 0, 1, abi.LOCAL_ENTRY, 0)
        ev[2 * i + 1] = (T0 + 10 * i + 5, T0 + 10 * i, 0, 1, abi.LOCAL_EXIT_ERROR, 0)
    for i in range(6):
        ev[4 + i] = (T0 + 100 + i, 0, 0, 2, abi.LOCAL_ENTRY, 0)
    eng, ora = _engine(base), _oracle(base)
    want = ora.decide(ev)
    assert (want["status"][4:] == abi.LOCAL_BLOCK_DEGRADE).all()
    _same(eng.local_decide_host(ev), want, "results")
    log = BlockLog()
    log_batch(log, ev, want)
    rows = log.roll(T0 + 1000)
    assert len(rows) == 1 and rows[0]["count"] == 12 and rows[0]["app"] == 0
    _fetch(eng, T0 + 1000, rows)


def test_param_flow_exception_arguments():
    """A scalar, a labelled and an unlabelled collection, a negative paramIdx; a null argument, an index beyond the
    arguments, args_null and passes log nothing."""
    params = np.array([prule(res=0, idx=0, count=1.0), prule(res=1, idx=-1, count=1.0)], abi.PSLOT_RULE_DTYPE)
    base = [local_rule()] * 2
    calls, res = Args(), []
    for r, a in ((0, (5,)), (0, (5,)), (0, (5,)), (0, (None,)), (0, (None,)), (0, ()), (0, ()),
                 (0, (("coll", 9, [11, 12]),)), (0, (("coll", 9, [11, 12]),)),
                 (0, (("coll", 0, [13]),)), (0, (("coll", 0, [13]),)), (0, (("coll", 0, [14]),)), (0, (("coll", 0, [14]),)),
                 (1, (7, 8)), (1, (7, 8)), (1, (6, 8))):
        calls.call(*a)
        res.append(r)
    calls.call(args_null=True)
    res.append(0)
    ext, args, values = calls.arrays()
    ev = entries(T0 + np.arange(len(res)), res, 1)
    ora = _oracle(base)
    ps = ParamFlowSlot(params, n_resources=2)
    ora.attach_params(ps)
    want = ora.decide_ext(ev, ext, args, values)
    eng = _engine(base)
    eng.pslot_load_rules(params, n_resources=2)
    _same(eng.slot_decide_host(ev, ext, args, values), want, "results")
    idx = [ps.param_idx(0), ps.param_idx(1)]
    assert idx == [0, 1]
    log = BlockLog()
    log_batch(log, ev, want, ext=ext, args=args, values=values, param_idx=idx)
    rows = log.roll(T0 + 1000)
    got = [(int(r["resource"]), int(r["app_kind"]), int(r["app"]), int(r["count"])) for r in rows]
    # one token a second per value: 5 blocks twice, [11, 12] once (at 11), [13] and [14] once each — unlabelled
    # collections share a row —, and the rule with paramIdx -1 reads the second of two arguments: 8 blocks twice
    assert got == [(0, abi.BLOCK_APP_VALUE, 5, 2), (0, abi.BLOCK_APP_LABEL, 0, 2), (0, abi.BLOCK_APP_LABEL, 9, 1),
                   (1, abi.BLOCK_APP_VALUE, 8, 2)], got
    _fetch(eng, T0 + 1000, rows)


def test_authority_exception_with_origin():
    base = [local_rule()] * 2
    fr = np.zeros(0, abi.LOCAL_FLOW_RULE_DTYPE)
    eng = _engine(base, fr, 3)
    assert eng.local_load_authority_rules(*to_abi([(1, BLACK, [1, 3])]), 3) == 1
    n = 90
    ev = entries(T0 + np.arange(n) * 20, np.arange(n) % 2, 1, np.arange(n) % 4)
    rejected = (ev["resource"] == 1) & np.isin(ev["origin"], (1, 3))
    want = np.zeros(n, abi.LOCAL_RES_DTYPE)
    want["status"] = np.where(rejected, abi.LOCAL_BLOCK_AUTHORITY, abi.LOCAL_PASS)
    _same(eng.local_decide_host(ev), want, "results")
    log = BlockLog()
    log_batch(log, ev, want)
    rows = log.roll(T0 + 2000)
    assert len(rows) == 4 and set(rows["app"].tolist()) == {1, 3} and (rows["app"] == rows["origin"]).all()
    _fetch(eng, T0 + 2000, rows)


def test_system_block_exception_limit_types():
    eng = _engine([local_rule()] * 2)
    eng.local_set_entry_types(ref.SYS_INBOUND)
    log, kinds = BlockLog(), set()
    for rules, (load, cpu), ev, want in ref.system_case():
        rows = np.zeros(len(rules), abi.SYSTEM_RULE_DTYPE)
        for i, r in enumerate(rules):
            rows[i] = r
        eng.local_load_system_rules(rows)
        eng.local_set_system_status(load, cpu)
        _same(eng.local_decide_host(ev), want, "results")
        log_batch(log, ev, want)
        kinds |= set(want["wait_ms"][want["status"] == abi.LOCAL_BLOCK_SYSTEM].tolist())
    assert kinds == {abi.SYSTEM_QPS, abi.SYSTEM_THREAD, abi.SYSTEM_RT, abi.SYSTEM_LOAD}
    _fetch(eng, T0 + 4000, log.roll(T0 + 4000))


# ---------------------------------------------------------------- the table

def _keys_batch(t, n_keys, first=0):
    """n_keys resources blocked in one second, key k with k % 3 + 1 entries of count k + 1."""
    res = np.concatenate([np.full(k % 3 + 1, first + k) for k in range(n_keys)])
    cnt = np.concatenate([np.full(k % 3 + 1, k + 1) for k in range(n_keys)])
    order = np.argsort((np.arange(len(res)) * 7) % len(res), kind="stable")
    return entries(t + np.arange(len(res)), res[order], cnt[order])


def test_small_table_probing_loss_and_removal():
    K = 64
    eng = _engine([BLOCK0] * K, log2=4)
    ev = _keys_batch(T0, 12)
    want = np.zeros(len(ev), abi.LOCAL_RES_DTYPE)
    want["status"] = FLOW
    _same(eng.local_decide_host(ev), want, "results")
    log = BlockLog()
    log_batch(log, ev, want)
    _fetch(eng, T0 + 1000, log.roll(T0 + 1000))            # 12 keys in 16 slots: probing, wrap-around, none lost
    ev = _keys_batch(T0 + 1000, 20)
    want = np.zeros(len(ev), abi.LOCAL_RES_DTYPE)
    want["status"] = FLOW
    _same(eng.local_decide_host(ev), want, "results")      # a full table never changes a decision
    rows, le, lc = eng.block_log(T0 + 2000)
    assert len(rows) == 16 and len(set(rows["resource"].tolist())) == 16
    for r in rows:                                         # every row that made it is exact
        k = int(r["resource"])
        assert int(r["count"]) == (k % 3 + 1) * (k + 1) and r["timestamp"] == T0 + 1000
    lost = sorted(set(range(20)) - set(rows["resource"].tolist()))
    assert le == sum(k % 3 + 1 for k in lost) and lc == sum((k % 3 + 1) * (k + 1) for k in lost)
    assert len(ev) == le + sum(k % 3 + 1 for k in rows["resource"].tolist())
    assert int(ev["count"].sum()) == lc + int(rows["count"].sum())
    ev = _keys_batch(T0 + 2000, 16, first=30)              # the fetch removed the rows: sixteen new keys fit again
    want = np.zeros(len(ev), abi.LOCAL_RES_DTYPE)
    want["status"] = FLOW
    _same(eng.local_decide_host(ev), want, "results")
    log = BlockLog()
    log_batch(log, ev, want)
    _fetch(eng, T0 + 3000, log.roll(T0 + 3000))


def test_a_loss_is_reported_by_a_fetch_that_returns_no_row():
    """Twenty keys into sixteen slots, then the timer fires while the second is still open: no row leaves, and the
    totals of what did not fit are reported by that very call — once."""
    eng = _engine([BLOCK0] * 32, log2=4)
    ev = _keys_batch(T0, 20)
    eng.local_decide_host(ev)
    rows, le, lc = eng.block_log(T0 + 999)
    assert len(rows) == 0 and le > 0 and lc > 0
    rows2, le2, lc2 = eng.block_log(T0 + 1000)
    assert (le2, lc2) == (0, 0) and len(rows2) == 16
    assert len(ev) == le + sum(k % 3 + 1 for k in rows2["resource"].tolist())
    assert int(ev["count"].sum()) == lc + int(rows2["count"].sum())


def test_contracts():
    from sentinel_amd.engine import EngineError
    import ctypes as C
    eng = _engine([BLOCK0] * 3, log2=None)
    with pytest.raises(EngineError) as e:
        eng.block_log(T0)
    assert e.value.code == abi.SG_E_INVAL                  # fetch without enable
    eng.block_log_enable(6)
    eng.block_log_enable(6)                                # the same capacity again: nothing
    with pytest.raises(EngineError) as e:
        eng.block_log_enable(7)
    assert e.value.code == abi.SG_E_INVAL
    ev = entries(T0 + np.arange(9), np.arange(9) % 3)
    eng.local_decide_host(ev)
    out = np.zeros(2, abi.BLOCK_ROW_DTYPE)
    n, le, lc = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = eng._L.sg_local_block_log(eng.h, T0 + 1000, abi.ptr(out), 2, C.byref(n), C.byref(le), C.byref(lc))
    assert rc == abi.SG_E_CAPACITY and n.value == 3 and not out.view(np.uint8).any()
    rows, le, lc = eng.block_log(T0 + 1000)                # ... and nothing changed
    assert [(int(r["resource"]), int(r["count"])) for r in rows] == [(0, 3), (1, 3), (2, 3)] and (le, lc) == (0, 0)
    rows, le, lc = eng.block_log(T0 + 1000)
    assert len(rows) == 0


def test_enable_before_the_rules_and_after_batches():
    from sentinel_amd.engine import FlowEngine
    eng = FlowEngine(device=0, max_batch=1 << 10)
    eng.block_log_enable(5)                                # before any rule: the table belongs to the handle
    eng.local_load_rules(np.array([BLOCK0]), 2, 1000, 500)
    eng.local_decide_host(entries(T0 + np.arange(5), 0))
    rows, le, lc = eng.block_log(T0 + 1000)
    assert [(int(r["resource"]), int(r["count"])) for r in rows] == [(0, 5)] and (le, lc) == (0, 0)
    late = _engine([BLOCK0], log2=None)
    late.local_decide_host(entries(T0 + np.arange(5), 0))  # decided before the log: not recorded
    late.block_log_enable(5)
    late.local_decide_host(entries(T0 + 10 + np.arange(3), 0))
    rows, le, lc = late.block_log(T0 + 1000)
    assert [(int(r["resource"]), int(r["count"])) for r in rows] == [(0, 3)] and (le, lc) == (0, 0)


# ---------------------------------------------------------------- every batch entry point

PATH_BASE = [local_rule(2.0, abi.FLOW_GRADE_QPS), local_rule(), local_rule(50.0, abi.FLOW_GRADE_QPS)]


def _path_case():
    fr = np.array([local_flow_rule(0, 2.0), local_flow_rule(1, 3.0), local_flow_rule(1, 7.0),
                   local_flow_rule(2, 50.0)], abi.LOCAL_FLOW_RULE_DTYPE)
    rng = np.random.default_rng(5)
    ora = _oracle(PATH_BASE, fr, 0)
    log, batches, t = BlockLog(), [], T0 + 400
    for n in (400, 300, 500):
        ev = entries(t + np.sort(rng.integers(0, 900, n)), rng.integers(0, 3, n), rng.integers(1, 3, n))
        want = ora.decide(ev)
        log_batch(log, ev, want)
        batches.append((ev, want))
        t += 900
    rows = log.roll(t + 2000)
    assert len(rows) >= 6
    return fr, batches, rows, t + 2000


@pytest.mark.parametrize("path", ["local_device", "slot_device", "slot_device_ext", "local_host", "slot_host",
                                  "enqueue"])
def test_same_rows_through_every_entry_point(path):
    import torch
    fr, batches, rows, now = _path_case()
    eng = _engine(PATH_BASE, fr, 0)
    dev = torch.device("cuda:0")
    keep, tickets = [], []
    for ev, want in batches:
        n = len(ev)
        if path in ("local_host", "slot_host"):
            ext = np.zeros(n, abi.SLOT_EXT_DTYPE)
            ext["args_null"] = 1
            got = eng.local_decide_host(ev) if path == "local_host" else eng.slot_decide_host(ev, ext, None, None)
            _same(got, want, "results")
            continue
        ev_t = torch.from_numpy(ev.view(np.uint8).copy()).to(dev)
        out_t = torch.zeros(n * abi.LOCAL_RES_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        keep.append((ev_t, out_t, want))
        torch.cuda.synchronize()
        if path == "local_device":
            eng.local_decide_device(ev_t.data_ptr(), n, out_t.data_ptr())
        elif path == "slot_device":
            eng.slot_decide_device(ev_t.data_ptr(), 0, n, 0, 0, 0, 0, out_t.data_ptr())
        elif path == "slot_device_ext":
            ext = np.zeros(n, abi.SLOT_EXT_DTYPE)
            ext["args_null"] = 1
            ext_t = torch.from_numpy(ext.view(np.uint8).copy()).to(dev)
            torch.cuda.synchronize()
            eng.slot_decide_device(ev_t.data_ptr(), ext_t.data_ptr(), n, 0, 0, 0, 0, out_t.data_ptr())
        else:
            tickets.append(eng.local_enqueue(ev_t.data_ptr(), n, out_t.data_ptr()))   # three batches on the pipeline
    for t in tickets:
        eng.local_wait(t)
    torch.cuda.synchronize()
    for ev_t, out_t, want in keep:
        _same(out_t.cpu().numpy().view(abi.LOCAL_RES_DTYPE), want, "results")
    _fetch(eng, now, rows)


# ---------------------------------------------------------------- the log changes nothing else

def test_log_on_and_off_decide_and_count_alike():
    batches, decided, _ = ref.mixed_case()
    fr = ref.mixed_flow_rules()
    base = [local_rule()] * ref.MIXED_N_RES
    on, off = _engine(base, fr, ref.MIXED_N_ORIGINS), _engine(base, fr, ref.MIXED_N_ORIGINS, log2=None)
    for ev in batches:
        assert on.local_decide_host(ev).tobytes() == off.local_decide_host(ev).tobytes()
    for r in range(ref.MIXED_N_RES):
        for a, b in zip(on.local_state(r), off.local_state(r)):
            assert a.tobytes() == b.tobytes(), f"ClusterNode of resource {r}"
        for o in range(1, ref.MIXED_N_ORIGINS + 1):
            for a, b in zip(on.local_origin_state(r, o), off.local_origin_state(r, o)):
                assert a.tobytes() == b.tobytes(), f"origin node ({r}, {o})"
    for i in range(len(fr)):
        assert on.local_controller(i).tobytes() == off.local_controller(i).tobytes()
    m_on, m_off = on.local_metrics(T0 + 5000), off.local_metrics(T0 + 5000)
    assert len(m_on) > 0 and m_on.tobytes() == m_off.tobytes()


# ---------------------------------------------------------------- one randomized trace

def test_random_trace():
    K, rules, batches, decided = ref.random_case()
    fr = np.array([local_flow_rule(r, c, limit_app=a) for r, c, a in rules], abi.LOCAL_FLOW_RULE_DTYPE)
    eng = _engine([local_rule()] * K, fr, 4, log2=12)
    log = BlockLog()
    for b, (ev, (st, app)) in enumerate(zip(batches, decided)):
        got = eng.local_decide_host(ev)
        assert np.array_equal(got["status"], st), f"results of batch {b}"
        want = np.zeros(len(ev), abi.LOCAL_RES_DTYPE)
        want["status"] = st
        log_batch(log, ev, want, flow_app=lambda i: int(app[i]))
    rows = log.roll(T0 + 10_000)
    assert len(rows) > 200
    _fetch(eng, T0 + 10_000, rows)
