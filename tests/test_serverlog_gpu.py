"""The token server's stat log on the device (sg_server_log_enable / sg_server_log) against the model of
tests/serverlog_ref.py: device rows equal model rows exactly — every field, order included. The model is fed with the
oracle's results (ClusterTokenService: ClusterFlowChecker / SimpleClusterFlowChecker / ClusterParamFlowChecker,
ConcurrentTokenService), and the device's results are compared with them first, so a row can only differ through the
log itself; param|block's value comes from serverlog_ref.ParamChecker, which asserts its verdicts against the oracle."""
import ctypes as C

import numpy as np
import pytest

from sentinel_amd import abi
from tests.serverlog_ref import T0, ServerLog
from tests.test_flow_gpu import _ns, _pair, _rules, _trace

pytestmark = pytest.mark.gpu

B, BR, OB = abi.SLOG_FLOW_BLOCK, abi.SLOG_FLOW_BLOCK_REQUEST, abi.SLOG_FLOW_OCCUPIED_BLOCK
NO_ROWS = np.zeros(0, abi.SERVER_ROW_DTYPE)


def _logged_pair(rules, log2=12, **kw):
    eng, ora = _pair(rules, **kw)
    eng.server_log_enable(log2)
    return eng, ora


def _same(got, want, what="rows"):
    assert got.dtype == want.dtype and len(got) == len(want) and np.array_equal(got, want), \
        f"{what}: device\n{got}\nmodel\n{want}"


def _fetch(eng, now, want, lost=(0, 0)):
    rows, le, lc = eng.server_log(now)
    _same(rows, want)
    assert (le, lc) == lost, f"lost {(le, lc)}, expected {lost}"


def _step(eng, ora, log, rules, req):
    """One batch through the oracle, the device (sg_flow_decide_batch_host) and the model."""
    want = ora.decide(req)
    _same(eng.decide_host(req), want, "results")
    log.flow_batch(rules, req, want)
    return want


def _blocked_rules(n=1):
    r = _rules(n, np.random.default_rng(0), counts=np.zeros(n))  # threshold 0: every request is BLOCKED
    r["flow_id"] = np.arange(n) * 1000 + 123
    return r


def _requests(ts, key=0, acquire=1, prio=False):
    req = np.zeros(len(ts), abi.REQ_DTYPE)
    req["ts_ms"], req["acquire"] = ts, acquire
    req["key"] = np.asarray(key, np.uint32) | np.where(prio, np.uint32(abi.KEY_PRIO), np.uint32(0))
    return req


def _later(req):
    """A fetch time at which every second of the batch is complete."""
    return int(req["ts_ms"][-1]) + 2000


# ---------------------------------------------------------------- the flow add kernel: sizes, seconds, counts

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2049, 8193])   # a wave, a wave + 1, a span + 1, a block's four spans + 1
def test_one_flow_id_wave_combine_tail_and_cross_wave_add(n):
    rules = _blocked_rules()
    eng, ora = _logged_pair(rules, max_batch=1 << 14)
    i = np.arange(n)
    req = _requests(T0 + i * 999 // n, 0, 1 + 2 * (i % 5 == 0), i % 7 == 3)
    log = ServerLog()
    want = _step(eng, ora, log, rules, req)
    assert (want["status"] == abi.BLOCKED).all()
    rows = log.take(T0 + 1000)
    by_event = {int(r["event"]): int(r["count"]) for r in rows}
    assert by_event[B] == int(req["acquire"].sum()) and by_event[BR] == n
    assert by_event.get(OB, 0) == int((i % 7 == 3).sum()) and (rows["flow_id"] == 123).all()
    _fetch(eng, T0 + 1000, rows)


def test_a_sum_past_2_to_31():
    rules = _blocked_rules(2)
    eng, ora = _logged_pair(rules)
    big = np.iinfo(np.int32).max
    req = _requests(T0 + np.arange(7), [0, 0, 0, 1, 1, 1, 1], [big, big - 1, big, 2, 3, 1, 5])
    log = ServerLog()
    _step(eng, ora, log, rules, req)
    rows = log.take(T0 + 1000)
    assert [int(c) for c in rows["count"]] == [3 * big - 1, 11, 3, 4] and 3 * big - 1 > 1 << 32
    _fetch(eng, T0 + 1000, rows)


def test_two_flow_ids_alternating_and_a_second_boundary_inside_a_wave():
    rules = _blocked_rules(2)
    eng, ora = _logged_pair(rules)
    n = 128
    ts = np.where(np.arange(n) < 40, T0 + 900 + np.arange(n), T0 + 1000 + np.arange(n))
    req = _requests(ts, np.arange(n) % 2)      # sorted by flowId each has 64 records: the second turns at record 20
    log = ServerLog()
    _step(eng, ora, log, rules, req)
    rows = log.take(T0 + 2000)
    assert [(int(r["timestamp"] - T0), int(r["event"]), int(r["flow_id"]), int(r["count"])) for r in rows] == [
        (0, B, 123, 20), (0, B, 1123, 20), (0, BR, 123, 20), (0, BR, 1123, 20),
        (1000, B, 123, 44), (1000, B, 1123, 44), (1000, BR, 123, 44), (1000, BR, 1123, 44)]
    _fetch(eng, T0 + 2000, rows)


def test_every_status_with_priorities_and_a_namespace_limiter():
    """OK, BLOCKED, SHOULD_WAIT and TOO_MANY_REQUEST in one trace (plus rejected requests): passes and limited requests
    log nothing, a wait one row, a block two or three."""
    rng = np.random.default_rng(11)
    rules = _rules(50, rng)
    ns = _ns()
    ns["limiter_enabled"], ns["max_allowed_qps"] = 1, 2500
    eng, ora = _logged_pair(rules, ns=ns, max_batch=1 << 13)
    log = ServerLog()
    seen = set()
    t = T0 + 300
    for _ in range(2):
        req = _trace(rng, 6000, 50, t, 2200, zipf=1.1, prio=0.2)
        req["key"][::97] = abi.KEY_NO_RULE
        req["acquire"][5::101] = 0
        t = int(req["ts_ms"][-1]) + 3
        seen |= set(int(s) for s in _step(eng, ora, log, rules, req)["status"])
    assert {abi.OK, abi.BLOCKED, abi.SHOULD_WAIT, abi.TOO_MANY_REQUEST, abi.NO_RULE_EXISTS, abi.BAD_REQUEST} <= seen
    rows = log.take(t + 2000)
    assert {int(e) for e in rows["event"]} == {abi.SLOG_FLOW_WAITING, B, BR, OB}
    _fetch(eng, t + 2000, rows)


def test_skipped_ranges_are_logged():
    """A saturated long segment whose tail the wave walker skips: k_skip_apply writes those results, and the add runs
    behind it."""
    rng = np.random.default_rng(77)
    rules = _rules(3, rng, counts=np.array([10.0, 2.0, 7.5]), S=10, interval=1000)
    eng, ora = _logged_pair(rules, flags=abi.FLAG_WAVE_ONLY, max_batch=1 << 18)
    eng.enable_stats(True)
    log = ServerLog()
    t, skipped = T0 + 10, 0
    for n in (200_000, 100_000):
        req = _trace(rng, n, 3, t, 2300, zipf=1.5, prio=0.01, multi=0.2)
        t = int(req["ts_ms"][-1]) + 1
        _step(eng, ora, log, rules, req)
        skipped += eng.stats()["skipped_ranges"]
    assert skipped > 0
    _fetch(eng, t + 2000, log.take(t + 2000))


# ---------------------------------------------------------------- the three record layouts, the walkers

def _layout_trace(rng, n, n_keys, t):
    req = _trace(rng, n, n_keys, t, int(rng.integers(200, 2500)), zipf=1.2, prio=0.05)
    req["key"][rng.random(n) < 0.03] = abi.KEY_NO_RULE       # rejected requests: no sorted copy in the compact layout,
    req["key"][rng.random(n) < 0.03] = abi.KEY_BAD           # the sentinel key in the 8-byte ones
    req["acquire"][rng.random(n) < 0.03] = 0
    req["key"][n // 2], req["key"][n // 3], req["acquire"][n // 5] = abi.KEY_NO_RULE, abi.KEY_BAD, 0   # at any n
    return req


@pytest.mark.parametrize("n_keys,n", [(7, 63), (300, 4097), (5000, 60_000)])
def test_same_rows_on_the_radix_path_and_both_binned_layouts(monkeypatch, n_keys, n):
    """SG_BIN=0 (two-pass radix sort), SG_BIN=2 (binned, 4-byte sorted records) and SG_BIN=2 SG_REC4=0 (binned, 8-byte
    records), at the rule and batch sizes tests/test_rec4_gpu.py uses to reach the compact records."""
    rng = np.random.default_rng(n_keys * 11 + n)
    rules = _rules(n_keys, rng, counts=rng.integers(0, 6, n_keys))
    engines = []
    for env in ({"SG_BIN": "0", "SG_REC4": "1"}, {"SG_BIN": "2", "SG_REC4": "1"}, {"SG_BIN": "2", "SG_REC4": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)      # read when an engine is created
        engines.append(_logged_pair(rules, log2=17, max_batch=1 << 16)[0])
    _, ora = _pair(rules, max_batch=1 << 16)
    log = ServerLog()
    t = T0 + 11
    for _ in range(4):                    # the hot set of batch i is batch i - 1's longest segments
        req = _layout_trace(rng, n, n_keys, t)
        t = int(req["ts_ms"][-1]) + int(rng.integers(0, 300))
        want = ora.decide(req)
        log.flow_batch(rules, req, want)
        for e in engines:
            _same(e.decide_host(req), want, "results")
        # the layout each engine really took: the compact engine's front records are 4-byte words at the request's
        # own index with the acquire code in the low byte (k_prep<true>), the other two's are 8-byte records
        from tests.test_rec4_gpu import _front_codes
        ok = ((req["key"] & abi.KEY_INDEX) < n_keys) & (req["acquire"] > 0)
        assert ok.sum() > n // 2 and (~ok).any()          # accepted requests, and rejected ones for the stale tail
        codes = _front_codes(req)[ok]
        c4 = [e.debug_copy(0, np.uint32, n)[ok] & np.uint32(0xFF) for e in engines]
        assert np.array_equal(c4[1], codes), "SG_BIN=2 SG_REC4=1 did not take the compact layout"
        c8 = engines[2].debug_copy(0, np.uint64, n)[ok]
        assert np.array_equal(c8 & np.uint64(0xFF), codes.astype(np.uint64)), "SG_REC4=0: 8-byte front records expected"
        assert not np.array_equal(c4[0], codes) and not np.array_equal(c4[2], codes)
    rows = log.take(t + 2000)
    assert len(rows) > 3
    for e in engines:
        _fetch(e, t + 2000, rows)


@pytest.mark.parametrize("flags", [abi.FLAG_SERIAL_ONLY, abi.FLAG_WAVE_ONLY])
def test_same_rows_from_the_serial_and_the_wave_walker(flags):
    rng = np.random.default_rng(31)
    rules = _rules(40, rng, counts=rng.integers(0, 10, 40))
    eng, ora = _logged_pair(rules, flags=flags, max_batch=1 << 15)
    log = ServerLog()
    t = T0 + 5
    for _ in range(2):
        req = _trace(rng, 20_000, 40, t, 1800, zipf=1.3, prio=0.1)
        t = int(req["ts_ms"][-1]) + 2
        _step(eng, ora, log, rules, req)
    _fetch(eng, t + 2000, log.take(t + 2000))


# ---------------------------------------------------------------- entry points

@pytest.mark.parametrize("entry", ["device", "host", "submit", "enqueue"])
def test_same_rows_through_every_entry_point(entry):
    """sg_flow_decide_batch, _host, sg_flow_submit and sg_flow_enqueue with 4 batches in flight."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(41)
    n_keys, n, n_batches = 300, 20_000, 6
    rules = _rules(n_keys, rng, counts=rng.integers(0, 12, n_keys))
    eng, ora = _logged_pair(rules, log2=14, max_batch=n)
    log = ServerLog()
    t, reqs = T0 + 7, []
    for _ in range(n_batches):
        reqs.append(_trace(rng, n, n_keys, t, 900, zipf=1.2, prio=0.05))
        t = int(reqs[-1]["ts_ms"][-1]) + 7
    want = [ora.decide(r) for r in reqs]
    for r, w in zip(reqs, want):
        log.flow_batch(rules, r, w)
    if entry == "host":
        got = [eng.decide_host(r) for r in reqs]
    elif entry == "submit":
        ins = [eng.host_array(n, abi.REQ_DTYPE) for _ in reqs]
        got = [eng.host_array(n, abi.RES_DTYPE) for _ in reqs]
        tickets = []
        for b in range(n_batches):
            ins[b][:] = reqs[b]
            if b >= 2:
                eng.wait(tickets[b - 2])
            tickets.append(eng.submit(ins[b], got[b]))
        for tk in tickets[-2:]:
            eng.wait(tk)
    else:
        ins = [torch.from_numpy(r.view(np.uint8).copy()).to(dev) for r in reqs]
        outs = [torch.empty(n * abi.RES_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in reqs]
        torch.cuda.synchronize()
        if entry == "device":
            for b in range(n_batches):
                eng.decide_device(ins[b].data_ptr(), n, outs[b].data_ptr(), torch.cuda.current_stream().cuda_stream)
        else:
            tickets = []
            for b in range(n_batches):
                if b >= 4:
                    eng.wait(tickets[b - 4])
                tickets.append(eng.enqueue_device(ins[b].data_ptr(), n, outs[b].data_ptr()))
            # no wait for the last four: the fetch drains the pipeline itself
    rows = log.take(t + 2000)
    assert len(rows) > 100
    _fetch(eng, t + 2000, rows)
    if entry in ("device", "enqueue"):
        torch.cuda.synchronize()
        got = [o.cpu().numpy().view(abi.RES_DTYPE) for o in outs]
    for b in range(n_batches):
        _same(np.asarray(got[b]), want[b], f"results of batch {b}")


def test_a_second_over_two_batches_with_a_fetch_between_and_a_refused_batch():
    from sentinel_amd.engine import EngineError
    rules = _blocked_rules(3)
    eng, ora = _logged_pair(rules)
    log = ServerLog()
    a = _requests(T0 + 200 + np.arange(300), np.arange(300) % 3, 2)             # T0+200 .. T0+499
    b = _requests(T0 + 800 + np.arange(400), np.arange(400) % 3, 1, True)       # T0+800 .. T0+1199: the second turns
    _step(eng, ora, log, rules, a)
    _fetch(eng, T0 + 999, NO_ROWS)                                              # the open second stays
    _step(eng, ora, log, rules, b)
    bad = _requests(T0 + 1300 - np.arange(50), 0)                               # time-reversed: SG_E_TIME
    with pytest.raises(EngineError) as ei:
        eng.decide_host(bad)
    assert ei.value.code == abi.SG_E_TIME                                       # it decided nothing and logs nothing
    rows = log.take(T0 + 1000)
    assert [int(c) for c in rows["count"]] == [200 + 67, 200 + 67, 200 + 66, 100 + 67, 100 + 67, 100 + 66, 67, 67, 66]
    _fetch(eng, T0 + 1000, rows)                                                # whole: both batches' shares
    _fetch(eng, T0 + 1000, NO_ROWS)                                             # a second fetch returns nothing
    rows = log.take(T0 + 2000)
    assert len(rows) == 9 and int(rows["count"].sum()) == 3 * 200
    _fetch(eng, T0 + 2000, rows)                                                # the survivors were put back whole
    assert not log.counts
    _fetch(eng, T0 + 9000, NO_ROWS)


# ---------------------------------------------------------------- RLS

def test_rls_logs_passes_and_the_mode_does_not_stick():
    """sg_rls_should_rate_limit: pass, pass_request, block and block_request rows (SimpleClusterFlowChecker); a
    descriptor without a rule and a request with hits_addend < 0 log nothing; a plain flow batch afterwards logs no
    passes again."""
    from sentinel_amd.rls import rls_rules
    rng = np.random.default_rng(3)
    K = 30
    rules = _rules(K, rng, counts=rng.integers(0, 15, K))
    rules = rls_rules(rules)
    eng, ora = _logged_pair(rules, max_batch=1 << 13)
    rows_in, t = [], T0 + 100
    for _ in range(2500):
        t += int(rng.integers(0, 2))
        d = [int(x) if rng.random() < 0.9 else -1 for x in rng.integers(0, K, int(rng.integers(1, 4)))]
        rows_in.append((t, int(rng.choice([0, 1, 2, 5, -1], p=[0.1, 0.6, 0.15, 0.1, 0.05])), d))
    req = np.zeros(len(rows_in), abi.RLS_REQ_DTYPE)
    desc, b = [], 0
    for j, (ts, hits, d) in enumerate(rows_in):
        req[j] = (ts, hits, b, len(d), 0)
        desc += d
        b += len(d)
    desc = np.array(desc, np.int32)
    g_all, g_st = eng.rls_should_rate_limit(req, desc)
    w_all, w_st = ora.should_rate_limit(req, desc)
    assert np.array_equal(g_all, w_all) and np.array_equal(g_st, w_st)
    log = ServerLog()
    n_pass = n_block = 0
    for j, (ts, hits, d) in enumerate(rows_in):
        for x, r in enumerate(d):
            st = w_st[int(req["desc_begin"][j]) + x]
            if hits < 0 or r < 0:
                assert st["has_rule"] == 0    # never requested: nothing to log
                continue
            ok = st["code"] == abi.RLS_OK
            log.flow(ts, int(rules["flow_id"][r]), hits or 1, False, abi.OK if ok else abi.BLOCKED, rls=True)
            n_pass, n_block = n_pass + ok, n_block + (not ok)
    assert n_pass > 100 and n_block > 100 and (req["hits_addend"] < 0).any() and (desc < 0).any()
    # the same handle as a plain token server afterwards: OK logs nothing
    plain = _trace(rng, 4000, K, t + 1, 2500, prio=0.0)
    want = ora.decide(plain)
    _same(eng.decide_host(plain), want, "results")
    assert (want["status"] == abi.OK).any() and (want["status"] == abi.BLOCKED).any()
    log.flow_batch(rules, plain, want)
    end = _later(plain)
    rows = log.take(end)
    tail = rows[rows["timestamp"] > t + 1000]
    assert len(tail) and not np.isin(tail["event"], (abi.SLOG_FLOW_PASS, abi.SLOG_FLOW_PASS_REQUEST)).any()
    assert {int(e) for e in rows["event"]} == {abi.SLOG_FLOW_PASS, abi.SLOG_FLOW_PASS_REQUEST, B, BR}
    _fetch(eng, end, rows)


# ---------------------------------------------------------------- the table and the contract of the calls

def _raw_fetch(eng, now, cap):
    out = np.zeros(max(1, cap), abi.SERVER_ROW_DTYPE)
    n, le, lc = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = eng._L.sg_server_log(eng.h, now, abi.ptr(out), cap, C.byref(n), C.byref(le), C.byref(lc))
    return rc, out, n.value, le.value, lc.value


def test_a_full_table_loses_whole_keys_counts_them_and_changes_no_decision():
    """capacity_log2 = 4 and 40 flowIds blocked in one second: 16 keys get a slot (a key is either wholly in or wholly
    lost: the table only fills), their rows equal the model's, the lost totals are the rest."""
    rules = _blocked_rules(40)
    eng, ora = _logged_pair(rules, log2=4)
    n = 4000
    i = np.arange(n)
    req = _requests(T0 + i * 999 // n, i % 40, 1 + i % 3)
    log = ServerLog()
    _step(eng, ora, log, rules, req)            # decisions untouched: equal to the oracle's
    model = log.take(T0 + 1000)
    rows, le, lc = eng.server_log(T0 + 1000)
    got_ids = sorted(set(int(f) for f in rows["flow_id"]))
    assert len(got_ids) == 16 and len(rows) == 32
    _same(rows, model[np.isin(model["flow_id"], got_ids)])
    rest = model[~np.isin(model["flow_id"], got_ids)]
    assert le == int(rest["count"][rest["event"] == BR].sum()) and lc == int(rest["count"][rest["event"] == B].sum())
    assert le == n - 16 * 100
    _fetch(eng, T0 + 1000, NO_ROWS)             # the lost totals were reported once and cleared


def test_cap_too_small_enable_twice_before_enable_and_a_reload_that_renumbers_the_rules():
    from sentinel_amd.engine import EngineError
    rules = _blocked_rules(5)
    eng, ora = _pair(rules)
    with pytest.raises(EngineError) as ei:
        eng.server_log(T0)                      # before the enable
    assert ei.value.code == abi.SG_E_INVAL
    for bad in (3, 25):
        with pytest.raises(EngineError) as ei:
            eng.server_log_enable(bad)
        assert ei.value.code == abi.SG_E_INVAL
    eng.server_log_enable(4)
    eng.server_log_enable(4)                    # the same capacity again: nothing happens
    with pytest.raises(EngineError) as ei:
        eng.server_log_enable(5)
    assert ei.value.code == abi.SG_E_INVAL
    log = ServerLog()
    req = _requests(T0 + np.arange(50), np.arange(50) % 5, 3, np.arange(50) % 2 == 0)
    _step(eng, ora, log, rules, req)
    # the rules reversed: index k is another flowId now; pending rows keep the flowId they were decided under
    new = rules[::-1].copy()
    eng.load_rules(new)
    ora.load_rules(new)
    req2 = _requests(T0 + 100 + np.arange(50), np.arange(50) % 5, 1)
    _step(eng, ora, log, new, req2)
    rows = log.take(T0 + 1000)
    assert len(rows) == 15 and [int(c) for c in rows["count"][:5]] == [40] * 5
    rc, _, n, le, lc = _raw_fetch(eng, T0 + 1000, 14)
    assert (rc, n, le, lc) == (abi.SG_E_CAPACITY, 15, 0, 0)   # the rows needed; nothing changed
    rc, out, n, le, lc = _raw_fetch(eng, T0 + 1000, 15)
    assert (rc, n, le, lc) == (0, 15, 0, 0)
    _same(out[:15], rows)
    _fetch(eng, T0 + 5000, NO_ROWS)


# ---------------------------------------------------------------- concurrent tokens

def test_concurrent_tokens_pass_block_and_release_rows():
    """Acquire pass and block, releases of tokens of the same and of an earlier batch, double releases, unknown ids,
    expired tokens (RegularExpireStrategy logs nothing) and NO_RULE_EXISTS after a reload that drops and renumbers
    rules: rows equal the model's, and nowCalls / live tokens still equal the oracle's with the log on."""
    from tests.test_conc_gpu import Trace, _check_state
    from tests.test_conc_gpu import _pair as conc_pair
    from tests.test_conc_gpu import _rules as conc_rules
    rng = np.random.default_rng(9)
    k = 60
    rules = conc_rules(rng, k)
    eng, ora = conc_pair(rules, (rng.integers(200, 3000, k), rng.integers(100, 1500, k)))
    eng.server_log_enable(14)
    tr, log = Trace(9, k), ServerLog()
    seen = set()

    def step(rules, n, span):
        q = tr.batch(n, span)
        base = tr.seq
        want = ora.decide(q)
        _same(eng.conc_decide_host(q), want, "results")
        log.conc_batch(rules, q, want)
        rel = q["kind"] == abi.CONC_RELEASE
        own = rel & (q["token_id"] > base) & (q["token_id"] <= base + len(q))
        for name, m in (("pass", ~rel & (want["status"] == abi.OK)), ("block", ~rel & (want["status"] == abi.BLOCKED)),
                        ("release own", own & (want["status"] == abi.RELEASE_OK)),
                        ("release older", rel & ~own & (want["status"] == abi.RELEASE_OK)),
                        ("already", rel & (want["status"] == abi.ALREADY_RELEASE)),
                        ("no rule release", rel & (want["status"] == abi.NO_RULE_EXISTS))):
            if m.any():
                seen.add(name)
        tr.absorb(q, want)
        return q, want

    step(rules, 8000, 700)
    live_before = set(tr.live)
    online = (rng.random(22) < 0.5).astype(np.uint8)
    removed = ora.expire(tr.t + 4000, online)
    assert eng.conc_expire(tr.t + 4000, online) == removed and removed > 0
    tr.t += 4000
    q, want = step(rules, 8000, 700)
    expired = np.isin(q["token_id"], list(live_before)) & (want["status"] == abi.ALREADY_RELEASE)
    assert expired.any()                                      # a release of an expired token: nothing logged
    _check_state(eng, ora, k)
    new = np.concatenate([rules[10:40][::-1], conc_rules(rng, 20, fid0=5000)])   # 30 survive renumbered, 20 new
    eng.load_rules(new)
    ora.load_rules(new)
    tr.k = len(new)
    step(new, 8000, 700)
    _check_state(eng, ora, len(new))
    assert seen == {"pass", "block", "release own", "release older", "already", "no rule release"}
    rows = log.take(tr.t + 2000)
    assert {int(e) for e in rows["event"]} == {abi.SLOG_CONC_PASS, abi.SLOG_CONC_BLOCK, abi.SLOG_CONC_RELEASE}
    _fetch(eng, tr.t + 2000, rows)


# ---------------------------------------------------------------- cluster param tokens

def _param_pair(rules, ns=None, hot=None, flags=0, log2=14):
    from oracle.binding import ClusterTokenService
    from sentinel_amd.engine import FlowEngine
    from tests.serverlog_ref import ParamChecker
    if ns is None:
        ns = np.zeros(1, abi.NS_DTYPE)
        ns["connected_count"] = 1
    eng = FlowEngine(device=0, max_batch=1 << 16, flags=flags)
    eng.set_namespaces(ns)
    eng.cparam_load_rules(rules, hot, 12)
    eng.server_log_enable(log2)
    ora = ClusterTokenService()
    ora.set_namespaces(ns)
    ora.load_param_rules(rules, hot)
    return eng, ParamChecker(ora, rules, ns, hot)


def _param_step(eng, chk, log, req, values):
    """One batch through the restated checker over the oracle (verdicts asserted inside), the device and the model."""
    want, blocks = chk.decide(req, values)
    _same(eng.cparam_decide_host(req, values), want, "results")
    log.param_batch(chk.rules, req, want, blocks)
    return want, blocks


def test_param_single_value_and_the_blocking_value_first_middle_last_and_repeated():
    from tests.test_serverlog_kat import blocking_value_case
    rules, ns, req, values, status, block = blocking_value_case()
    eng, chk = _param_pair(rules, ns)
    log = ServerLog()
    want, blocks = _param_step(eng, chk, log, req, values)
    assert [int(s) for s in want["status"]] == status and blocks == block
    rows = log.take(T0 + 1000)
    assert [(int(r["event"]), int(r["value"]), int(r["count"])) for r in rows] == [
        (abi.SLOG_PARAM_PASS, 0, 3), (abi.SLOG_PARAM_BLOCK, 1 << 50, 6)]
    _fetch(eng, T0 + 1000, rows)


def _param_noise(rng, n, n_rules, t, span, multi, bad=0.01):
    from tests.test_cparam_gpu import _trace as ptrace
    return ptrace(rng, n, n_rules, 30, t, span, multi=multi, zipf=1.2, bad=bad)


@pytest.mark.parametrize("L,rounds", [(8, None), (100, 65)])
def test_param_fixed_point_rounds_and_the_group_fallback(L, rounds):
    """A chain of L two-value requests under a threshold of one (each outcome depends on the previous one, one link
    settles per round) among ordinary traffic: L = 8 converges in several rounds (the checks in chk[] name the blocking
    values), L = 100 outlasts the 64-round budget and the linked group is replayed (k_cpfb_replay names them)."""
    from tests.test_cparam_gpu import _chain, _merge
    from tests.test_cparam_gpu import _rules as prules
    rng = np.random.default_rng(70 + L)
    rules = prules(5, rng)
    rules["count"][0] = 1
    eng, chk = _param_pair(rules)
    log = ServerLog()
    t = T0 + 200
    for b in range(2):
        noise = _param_noise(rng, 3000, 4, t, 900, 0.3, bad=0.0)
        noise[0]["key"] += 1                         # rules 1..4; rule 0 (threshold 1) carries the chain alone
        req, vals = _merge([noise, _chain(L, 0, t + 50, 1, v0=(1 << 40) + 10_000 * b)])
        want, blocks = _param_step(eng, chk, log, req, vals)
        r = eng.cparam_last_rounds()
        assert r > 1 and (rounds is None and r <= 64 or r == rounds), r
        chain = np.nonzero(req["key"] == 0)[0]
        assert (want["status"][chain[0::2]] == abi.OK).all() and (want["status"][chain[1::2]] == abi.BLOCKED).all()
        # a blocked link fails at its first value: the previous link passed and added it
        assert all(blocks[i] == int(vals[req["value_begin"][i]]) for i in chain[1::2])
        multi_blocked = (req["value_count"] > 1) & (want["status"] == abi.BLOCKED) & (req["key"] != 0)
        assert multi_blocked.any()
        t = int(req["ts_ms"][-1]) + 1
    _fetch(eng, t + 2000, log.take(t + 2000))


def test_param_every_group_replayed_without_rounds(monkeypatch):
    monkeypatch.setenv("SG_CP_MAX_ROUNDS", "0")
    from tests.test_cparam_gpu import _rules as prules
    rng = np.random.default_rng(13)
    rules = prules(4, rng)
    eng, chk = _param_pair(rules)
    log = ServerLog()
    req, vals = _param_noise(rng, 4000, 4, T0, 1500, 0.4)
    want, _ = _param_step(eng, chk, log, req, vals)
    assert eng.cparam_last_rounds() == 1             # max_rounds (0) + 1: the group replay
    assert ((req["value_count"] > 1) & (want["status"] == abi.BLOCKED)).any()
    _fetch(eng, T0 + 4000, log.take(T0 + 4000))


def test_param_limited_requests_log_nothing():
    """A namespace limiter in front of the param checker: TOO_MANY_REQUEST results return before any log call."""
    from tests.test_cparam_gpu import _rules as prules
    rng = np.random.default_rng(14)
    ns = np.zeros(2, abi.NS_DTYPE)
    ns["connected_count"] = [2, 1]
    ns["limiter_enabled"], ns["max_allowed_qps"] = [1, 0], [1500, 0]
    rules = prules(8, rng)
    rules["namespace_id"] = np.arange(8) % 2
    eng, chk = _param_pair(rules, ns)
    log = ServerLog()
    t, seen = T0 + 40, set()
    for _ in range(2):
        req, vals = _param_noise(rng, 5000, 8, t, int(rng.integers(300, 1500)), 0.2)
        want, _ = _param_step(eng, chk, log, req, vals)
        seen |= set(int(s) for s in want["status"])
        t = int(req["ts_ms"][-1])
    assert {abi.TOO_MANY_REQUEST, abi.OK, abi.BLOCKED} <= seen
    _fetch(eng, t + 2000, log.take(t + 2000))


def test_param_a_saturated_hot_slot_with_skipped_ranges():
    """One hot value far above its threshold on the wave walker: the saturated tails of its periods are handed to
    k_cp_skipfill (single-value requests BLOCKED, multi-value checks 0, repeated values 1); multi-value requests that
    carry the hot value second or twice still name it."""
    from tests.test_cparam_gpu import _merge
    from tests.test_cparam_gpu import _rules as prules
    rng = np.random.default_rng(21)
    rules = prules(2, rng)
    rules["count"] = [5, 1000]
    eng, chk = _param_pair(rules, flags=abi.FLAG_WAVE_ONLY)
    log = ServerLog()
    # first the hot value alone: a batch of single-value requests walks once, so the skip pass's range count is still
    # there afterwards (a batch with multi-value requests clears it between its rounds) and pins that a slot saturated
    # like this one reaches k_cp_skipfill
    solo = np.zeros(6000, abi.CPARAM_REQ_DTYPE)
    solo["ts_ms"] = T0 - 3000 + np.sort(rng.integers(0, 900, len(solo)))
    solo["acquire"], solo["value_count"], solo["value_begin"] = 1, 1, np.arange(len(solo))
    want, _ = _param_step(eng, chk, log, solo, np.full(len(solo), 77, np.uint64))
    assert (want["status"] == abi.BLOCKED).sum() > 5000
    assert int(eng.debug_copy(6, np.uint32, 1)[0]) > 0, "no saturated range reached k_cp_skipfill"
    hot, n = np.uint64(77), 12_000
    req = np.zeros(n, abi.CPARAM_REQ_DTYPE)
    req["ts_ms"] = T0 + np.sort(rng.integers(0, 1800, n))
    req["acquire"] = 1
    shape = rng.random(n)
    lists = [[hot] if s < 0.9 else [np.uint64(1000 + i), hot] if s < 0.95 else [np.uint64(1000 + i), hot, hot]
             for i, s in enumerate(shape)]
    req["value_count"] = [len(x) for x in lists]
    req["value_begin"] = np.concatenate([[0], np.cumsum(req["value_count"])[:-1]])
    vals = np.array([v for x in lists for v in x], np.uint64)
    want, blocks = _param_step(eng, chk, log, req, vals)
    blocked = want["status"] == abi.BLOCKED
    assert blocked.sum() > 10_000 and all(blocks[i] == 77 for i in np.nonzero(blocked)[0])
    rows = log.take(T0 + 4000)
    assert set(int(v) for v in rows["value"][rows["event"] == abi.SLOG_PARAM_BLOCK]) == {77}
    _fetch(eng, T0 + 4000, rows)
