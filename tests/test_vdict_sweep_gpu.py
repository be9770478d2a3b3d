"""sg_vdict_sweep on the device against tests/vdict_ref.py, the Python model of the dictionary: which ids stay live
(one id per kind of source, each named by that source alone), what the freed ids answer, which ids later values take
through sg_vdict_intern, sg_codec_decode_param and sg_gateway_parse_batch, and that no decision changes — a gateway
trace and a param-flow trace decided on a swept engine, on a never-swept engine and by the oracles.

Sizes: the dictionary of the exact-live-set case has capacity 2^12 and about 2,100 values, so its per-id passes cross a
256-lane block and the 2,048-element scan tile; everything else is smaller. Every reference is computed once."""
import ctypes as C
import struct

import numpy as np
import pytest

from gateway_ref import Item, Parser, Rule, pack_requests, rules_to_abi
from oracle.binding import ClusterTokenService, ParamFlowSlot, local_rule
from param_frames import RefDecoder, param_frame
from sentinel_amd import abi
from vdict_ref import VDictModel, key_of

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
I, L, B, DBL, F, S, Z, STR = range(8)
ROUTE = abi.GW_RESOURCE_MODE_ROUTE_ID
FIELDS = ("live", "removed", "free_ids", "high", "arena_before", "arena_after")


def _engine(cap_log2, arena, max_values=1 << 12, max_batch=1 << 12):
    from sentinel_amd.engine import FlowEngine
    eng = FlowEngine(device=0, max_batch=max_batch)
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"], ns["max_allowed_qps"] = 1, 1e9
    eng.set_namespaces(ns)
    eng.ns = ns
    if cap_log2:
        eng.vdict_init(cap_log2, arena, max_values)
    return eng


def _code(call, *args):
    from sentinel_amd.engine import EngineError
    with pytest.raises(EngineError) as e:
        call(*args)
    return e.value.code


def _intern(eng, model, keys):
    """One batch through the device and the model: the ids must agree."""
    want = model.intern_keys(keys)
    got = eng.vdict_intern(keys)
    assert [int(x) for x in got] == want
    return want


def _assert_same(eng, model):
    """Size, a lookup of every id in [1, high + 1], against the model."""
    assert eng.vdict_size() == (model.size(), model.arena())
    live = model.live_ids()
    if live:
        assert eng.vdict_lookup(np.array(live, np.uint64)) == [model.key[i] for i in live]
    for i in model.dead_ids() + [0, model.high + 1]:
        assert _code(eng.vdict_lookup, [i]) == abi.SG_E_INVAL, i


def _sweep(eng, model, keep, live):
    """The device sweep with keep list `keep`; `live` = every id the test expects to stay (keep included)."""
    want = model.sweep(live)
    got = eng.vdict_sweep(keep)
    assert got == want, (got, want)
    return got


# ------------------------------------------------------------------------------------ 1, 2: the exact live set

def _values():
    """About 2,100 distinct values of all eight types, with the NaN spellings and BOOLEAN spellings that collapse,
    and strings of length 0, 8, 9, 40 and 300 (two of each but the empty one)."""
    keys = [(I, struct.pack(">i", 10**6)), (STR, b""), (STR, b"a" * 8), (STR, b"b" * 8), (STR, b"a" * 9), (STR, b"b" * 9),
            (STR, b"a" * 40), (STR, b"b" * 40), (STR, b"a" * 300), (STR, b"b" * 300),
            (Z, b"\x00"), (Z, b"\x01"), (Z, b"\x02"), (Z, b"\xFF")]   # ids 1 .. 12: under the alternating run
    keys += [(I, struct.pack(">i", k - 150)) for k in range(300)]
    keys += [(L, struct.pack(">q", (k - 150) * 2**33)) for k in range(300)]
    keys += [(B, struct.pack(">b", k - 128)) for k in range(256)]
    keys += [(DBL, struct.pack(">d", k / 8)) for k in range(200)]
    keys += [(DBL, struct.pack(">Q", x)) for x in (0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000000)]
    keys += [(F, struct.pack(">f", k / 8)) for k in range(200)]
    keys += [(F, struct.pack(">I", x)) for x in (0x7FC00000, 0x7F800001, 0xFFC00000)]
    keys += [(S, struct.pack(">h", k * 100 - 15000)) for k in range(300)]
    keys += [(STR, b"10.%d.%d.%d" % (k >> 8, k & 255, k % 7)) for k in range(540)]   # 8 to 13 bytes
    return keys


def _pattern(i):
    """The keep list's live / dead pattern over ids: alternating and solid runs around the bitmap's word edges
    (31, 32, 33, 63, 64, 65), across the 256-lane block and the 2,048-element scan tile."""
    if i <= 30:
        return i % 2 == 0
    if i <= 33:
        return i != 32            # 31 live, 32 dead, 33 live
    if i <= 62:
        return False              # a solid dead run up to the word's last bit
    if i <= 65:
        return i != 64            # 63 live, 64 dead, 65 live
    if i <= 130:
        return True               # solid live across 95 / 96 and 127 / 128
    if i <= 300:
        return False              # solid dead across 255 / 256 / 257
    if i <= 2030:
        return i % 3 == 0
    if i <= 2070:
        return True               # solid live across 2047 / 2048 / 2049
    return i <= 2100 and i % 2 == 1


SRC = {"param": 140, "thread": 150, "chain": 160, "keys": 170, "hot": 180, "cphot": 190, "blog": 200, "slog": 210}


def _chain_events(rows):
    """rows: [(ts, create_ts, resource, kind, value id)] → (ev, ext, args, values) of the slot chain."""
    n = len(rows)
    ev = np.zeros(n, abi.LOCAL_EVENT_DTYPE)
    ext = np.zeros(n, abi.SLOT_EXT_DTYPE)
    args = np.zeros(n, abi.PSLOT_ARG_DTYPE)
    for k, (ts, create, res, kind, _) in enumerate(rows):
        ev[k] = (ts, create, res, 1, kind, 0)
        ext[k] = (0, k, 1, 0)
        args[k] = (k, 1, abi.ARG_VALUE, 0)
    return ev, ext, args, np.array([r[4] for r in rows], np.uint64)


def _cp_req(rows):
    """rows: [(ts, value id)] → single-value requests of cluster param rule 0."""
    req = np.zeros(len(rows), abi.CPARAM_REQ_DTYPE)
    req["ts_ms"], req["acquire"], req["value_count"] = [r[0] for r in rows], 1, 1
    req["value_begin"] = np.arange(len(rows))
    return req, np.array([r[1] for r in rows], np.uint64)


@pytest.fixture(scope="module")
def zoo():
    """One engine with every kind of source, swept once. Returns what the tests assert on."""
    from types import SimpleNamespace
    eng, model = _engine(12, 1 << 16), VDictModel()
    keys = _values()
    ids = _intern(eng, model, keys)
    assert 2090 <= model.high <= 2200 and len(set(ids)) == model.high < len(keys)   # the spellings collapsed
    nan_d, nan_f = ids[keys.index((DBL, struct.pack(">Q", 0x7FF8000000000000)))], ids[keys.index((F, struct.pack(">I", 0x7FC00000)))]
    assert ids[keys.index((DBL, struct.pack(">Q", 0xFFF8000000000000)))] == nan_d
    assert ids[keys.index((F, struct.pack(">I", 0x7F800001)))] == nan_f
    key_before = dict(model.key)
    # gateway: a client-IP rule and an item-less rule on resource 2 ("$NM", "$D" take the next two ids); behind
    # them a QPS rule with a hot item on resource 0 and a THREAD rule of one thread on resource 1
    grules = [Rule(2, count=1000, item=Item(abi.GW_PARSE_CLIENT_IP), capacity_log2=6), Rule(2, count=1000, capacity_log2=4)]
    ref = Parser(grules, dictionary=model)
    extra = np.zeros(2, abi.PSLOT_RULE_DTYPE)
    extra["resource"], extra["grade"] = [0, 1], [abi.FLOW_GRADE_QPS, abi.FLOW_GRADE_THREAD]
    extra["rule"]["count"], extra["rule"]["duration_sec"], extra["rule"]["capacity_log2"] = [5.0, 1.0], 1, 4
    extra["rule"]["hot_count"][0] = 1
    hot = np.zeros(1, abi.PARAM_HOT_DTYPE)
    hot["value"], hot["threshold"] = SRC["hot"], 7
    rules_abi, blob = rules_to_abi(grules)
    loaded, _, _ = eng.gateway_load_rules(rules_abi, blob, 3, extra, hot)
    assert (ref.nm_id, ref.d_id) == (model.high - 1, model.high) and eng.vdict_size()[0] == model.size()
    q_rule = int(np.nonzero(loaded["resource"] == 0)[0][0])
    t_rule = int(np.nonzero(loaded["resource"] == 1)[0][0])
    eng.local_load_rules(np.array([local_rule() for _ in range(3)], abi.LOCAL_RULE_DTYPE), 2, 1000, 500)
    eng.block_log_enable(8)
    cp = np.zeros(1, abi.CPARAM_RULE_DTYPE)
    cp["flow_id"], cp["count"], cp["threshold_type"], cp["sample_count"], cp["window_interval_ms"] = 77, 1, abi.THRESHOLD_GLOBAL, 10, 1000
    cp["hot_count"] = 1
    cphot = np.zeros(1, abi.PARAM_HOT_DTYPE)
    cphot["value"], cphot["threshold"] = SRC["cphot"], 9
    eng.cparam_load_rules(cp, cphot, 4)
    eng.server_log_enable(8)
    # the chain: the blocked value enters, is blocked (logged) and leaves; another value enters and stays; a third
    # passes the QPS rule and leaves
    E, X = abi.LOCAL_ENTRY, abi.LOCAL_EXIT
    t = T0 + 5000
    out = eng.slot_decide_host(*_chain_events([
        (t, 0, 1, E, SRC["blog"]), (t + 1, 0, 1, E, SRC["blog"]), (t + 2, t, 1, X, SRC["blog"]),
        (t + 3, 0, 1, E, SRC["thread"]), (t + 4, 0, 0, E, SRC["chain"]), (t + 5, t + 4, 0, X, SRC["chain"])]))
    assert [int(s) for s in out["status"][[0, 1, 3, 4]]] == [abi.LOCAL_PASS, abi.LOCAL_BLOCK_PARAM, abi.LOCAL_PASS, abi.LOCAL_PASS]
    # the cluster param rule of 1 per second: the second request of a value is blocked (logged); a sweep 100 s later
    # drops its ring, then another value arrives
    res = eng.cparam_decide_host(*_cp_req([(t, SRC["slog"]), (t + 1, SRC["slog"])]))
    assert [int(s) for s in res["status"]] == [abi.OK, abi.BLOCKED]
    assert eng.cparam_sweep(t + 100_000)["values_removed"] == 1
    res = eng.cparam_decide_host(*_cp_req([(t + 100_000, SRC["keys"])]))
    assert int(res["status"][0]) == abi.OK
    # sg_param_decide_batch on the QPS rule's table, then the table sweep at that time: thread counts at 0 go
    req = np.zeros(1, abi.PARAM_REQ_DTYPE)
    req[0] = (t + 10, SRC["param"], q_rule, 1)
    assert int(eng.param_decide_host(req)[0]) == 1
    assert eng.param_sweep(t + 10)["threads_removed"] == 2
    # the premise: each of these ids is named by its one source
    assert eng.pslot_thread_count(1, 0, SRC["thread"]) == 1 and eng.pslot_thread_count(1, 0, SRC["blog"]) == 0
    assert eng.param_state(q_rule, SRC["chain"])[0] and eng.param_state(q_rule, SRC["param"])[0]
    assert not eng.param_state(t_rule, SRC["blog"])[0] and not eng.param_state(t_rule, SRC["thread"])[0]
    assert eng.cparam_sum(0, SRC["keys"], t + 100_000) == 1 and eng.cparam_sum(0, SRC["slog"], t + 100_000) == 0
    keep = [i for i in range(1, model.high + 1) if _pattern(i)]
    assert not any(_pattern(i) for i in SRC.values()) and not _pattern(ref.nm_id) and not _pattern(ref.d_id)
    live = set(keep) | set(SRC.values()) | {ref.nm_id, ref.d_id}
    size_before = eng.vdict_size()
    want = model.sweep(live)
    got = eng.vdict_sweep(keep)
    return SimpleNamespace(eng=eng, model=model, ref=ref, got=got, want=want, key_before=key_before, live=live,
                           size_before=size_before, t=t)


def test_exact_live_set(zoo):
    eng, model = zoo.eng, zoo.model
    assert zoo.got == zoo.want, (zoo.got, zoo.want)
    assert zoo.want["removed"] > 900 and zoo.want["live"] > 600 and zoo.want["arena_after"] < zoo.want["arena_before"]
    assert zoo.size_before == (zoo.want["high"], zoo.want["arena_before"])
    assert eng.vdict_size() == (zoo.want["live"], zoo.want["arena_after"])
    live = sorted(zoo.live)
    looked = eng.vdict_lookup(np.array(live, np.uint64))
    assert looked == [model.key[i] for i in live]                     # the same type and bytes as before
    assert all(looked[k] == zoo.key_before[i] for k, i in enumerate(live) if i in zoo.key_before)
    assert zoo.want["arena_after"] == sum(len(p) for _, p in looked if len(p) > 8)
    lens = {len(p) for t, p in looked if t == STR}
    assert {0, 8, 9, 40, 300} <= lens                                # both sides of the inline / arena boundary live ...
    assert {8, 9, 40, 300} <= {len(zoo.key_before[i][1]) for i in model.dead_ids() if zoo.key_before[i][0] == STR}
    assert {t for t, _ in looked} == set(range(8))
    for i in model.dead_ids():
        assert _code(eng.vdict_lookup, [i]) == abi.SG_E_INVAL, i
    # the log rows fetched after the sweep resolve to the values that were blocked
    rows, _, _ = eng.block_log(zoo.t + 200_000)
    hit = rows[(rows["app_kind"] == abi.BLOCK_APP_VALUE) & (rows["status"] == abi.LOCAL_BLOCK_PARAM)]
    assert [int(x) for x in hit["app"]] == [SRC["blog"]]
    assert eng.vdict_lookup(hit["app"]) == [zoo.key_before[SRC["blog"]]]
    rows, _, _ = eng.server_log(zoo.t + 200_000)
    hit = rows[rows["event"] == abi.SLOG_PARAM_BLOCK]
    assert [int(x) for x in hit["value"]] == [SRC["slog"]]
    assert eng.vdict_lookup(hit["value"]) == [zoo.key_before[SRC["slog"]]]


def _decode(eng, frames, ts):
    from tests.test_param_codec_gpu import _decode_gpu
    return _decode_gpu(eng, frames, ts)


def test_id_reuse(zoo):
    """After the sweep above: kept, freed and never-seen values with duplicates, through the codec, the gateway parser
    and one sg_vdict_intern batch that uses the free list up and goes on at high + 1."""
    eng, model, ref = zoo.eng, zoo.model, zoo.ref
    kept = [model.key[i] for i in model.live_ids()[:40]]
    freed = [zoo.key_before[i] for i in model.dead_ids()]
    assert len(freed) > 900 and model.free[0] == 1
    # the codec: one small batch (a frame's parameters in order; the decoder's reference numbers them the same way)
    params = [kept[0], freed[0], (STR, b"never-seen-1"), freed[0], freed[1], kept[1], (I, struct.pack(">i", 10**9)), (STR, b"never-seen-1")]
    frames = [param_frame(k, 77, 1, params[2 * k: 2 * k + 2]) for k in range(4)]
    d = _decode(eng, frames, T0 + 300_000 + np.arange(4))
    assert [int(x) for x in d.values] == model.intern_keys(params)
    assert sorted(set(int(x) for x in d.values) - {model.ids[key_of(*kept[0])], model.ids[key_of(*kept[1])]}) == [1, 3, 5, 7]
    # the gateway parser: client IPs of resource 2, "$D" behind each
    ips = [freed[-1][1] if freed[-1][0] == STR else b"10.0.0.1", b"203.0.113.77", b"10.0.0.1", b"203.0.113.77", b"b" * 300]
    requests = [(2, ROUTE, [(ip, False)]) for ip in ips]
    want_args, want_values, _ = ref.parse(requests)
    args, values, _, _ = eng.gateway_parse_host(*pack_requests(requests))
    assert np.array_equal(values, want_values) and np.array_equal(args, want_args)
    # one intern batch: more fresh values than free ids
    new = [(STR, b"fresh-%d" % k) for k in range(300)] + [(L, struct.pack(">q", 7 * 2**50 + k)) for k in range(100)]
    batch = kept + freed[2:] + new + freed[2:50] + kept[:10] + new[:10]
    n_free, high = len(model.free), model.high
    fresh, _ = model.fresh(batch)
    assert fresh > n_free > 800
    ids = _intern(eng, model, batch)
    assert max(ids) == high + fresh - n_free and not model.free and model.high == max(ids)
    _assert_same(eng, model)
    size = eng.vdict_size()
    assert [int(x) for x in eng.vdict_intern(batch)] == ids and eng.vdict_size() == size   # the second time: no change
    _assert_same(eng, model)


# ------------------------------------------------------------------------------------ 3: no decision changes

GW_RES = 4


def _gw_trace_rules():
    rules = []
    for r in range(GW_RES):
        rules.append(Rule(r, count=2, interval_sec=1, item=Item(abi.GW_PARSE_CLIENT_IP), capacity_log2=11))
        rules.append(Rule(r, count=150 + 10 * r, capacity_log2=4))
    return rules


def _gw_engine(rules):
    eng = _engine(13, 1 << 18, 1 << 13, 1 << 13)
    rules_abi, blob = rules_to_abi(rules)
    eng.gateway_load_rules(rules_abi, blob, GW_RES)
    return eng


def _gw_decide(eng, events):
    """Parse on the device into the event records, decide from the parser's device buffers → (results, values)."""
    import torch
    n = len(events)
    requests = [e[2] for e in events]
    pev = np.zeros(n, abi.PSLOT_EVENT_DTYPE)
    pev["ts_ms"], pev["kind"], pev["count"] = [e[0] for e in events], [e[1] for e in events], 1
    pev["resource"] = [r[0] for r in requests]
    args, values, _, _, dev = eng.gateway_parse_host(*pack_requests(requests), pev=pev, with_device=True)
    out_t = torch.zeros(n * abi.PSLOT_RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    eng.pslot_decide_device(dev["pev"].data_ptr(), n, dev["args"].data_ptr(), len(args), dev["values"].data_ptr(),
                            len(values), out_t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out_t.cpu().numpy().view(abi.PSLOT_RES_DTYPE), values


def test_gateway_decisions_do_not_change():
    """Four waves of 500 clients on four routes; a wave's entries leave in the next batch and the wave returns four
    batches (12 s) later. Engine A sweeps tables and dictionary after every batch, engine B never; the oracle keeps
    every value under its first id."""
    rng = np.random.default_rng(2901)
    rules = _gw_trace_rules()
    ref = Parser(rules)                                   # never swept: the oracle's numbering
    conv, hot, _ = ref.pslot_rules()
    ora = ParamFlowSlot(conv, hot, n_resources=GW_RES)
    A, B = _gw_engine(rules), _gw_engine(rules)
    waves = [[b"172.%d.%d.%d" % (16 + w, k >> 8, k & 255) for k in range(500)] for w in range(4)]
    open_entries, t = [], T0 + 1000
    a_live, a_before, b_size, blocked_by = [], [], [], set()
    for b in range(8):
        ent = []
        for c, ip in enumerate(waves[b % 4]):                 # a client stays on its route
            for _ in range(int(rng.integers(2, 5))):
                ent.append((abi.LOCAL_ENTRY, (c % GW_RES, ROUTE, [(ip, False)])))
        rows = ent + [(abi.LOCAL_EXIT, req) for req in open_entries]
        order = rng.permutation(len(rows))
        ts = t + np.sort(rng.integers(0, 600, len(rows)))
        events = [(int(ts[k]), rows[j][0], rows[j][1]) for k, j in enumerate(order)]
        n = len(events)
        want_args, want_values, spans = ref.parse([e[2] for e in events])
        full = np.zeros(n, abi.PSLOT_EVENT_DTYPE)
        full["ts_ms"], full["kind"], full["count"] = [e[0] for e in events], [e[1] for e in events], 1
        full["resource"] = [e[2][0] for e in events]
        full["arg_begin"], full["arg_count"] = [s[0] for s in spans], [s[1] for s in spans]
        want = ora.decide(full, want_args, want_values)
        content = [k for k in ref.dict.keys()]
        for name, eng in (("A", A), ("B", B)):
            got, values = _gw_decide(eng, events)
            if not np.array_equal(got, want):
                i = np.nonzero(got != want)[0][0]
                raise AssertionError(f"batch {b}, engine {name}, event {i}: {events[i]} oracle={want[i]} gpu={got[i]}")
            assert eng.vdict_lookup(values) == [content[int(v) - 1] for v in want_values], (b, name)   # by content
        entry = full["kind"] == abi.LOCAL_ENTRY
        assert (want["pass"][entry] == 1).any() and (want["pass"][entry] == 0).any()
        blocked_by |= {int(conv["param_idx"][r]) for r in want["rule"][entry & (want["pass"] == 0)]}
        open_entries = [e[2] for e, w in zip(events, want) if e[1] == abi.LOCAL_ENTRY and w["pass"] == 1]
        now = int(ts[-1])
        a_before.append(A.vdict_size()[0])
        A.param_sweep(now)
        st = A.vdict_sweep()
        assert st["live"] == A.vdict_size()[0]
        a_live.append(st["live"])
        b_size.append(B.vdict_size()[0])
        t += 3000
    assert blocked_by == {0, 1}                                       # the client-IP rule and the item-less rule
    assert b_size == sorted(b_size) and b_size[3] == b_size[-1] == 2002
    assert all(x < y for x, y in zip(a_live[1:], a_before[1:]))       # every sweep after the first gives ids back
    assert max(a_live[1:]) < 600 and max(a_before) < 1100             # one wave and "$NM", "$D", never the population


def test_param_codec_decisions_do_not_change():
    """The same shape through the param-flow codec and sg_cparam_decide_batch, with sg_cparam_sweep."""
    import torch
    rng = np.random.default_rng(2902)
    cp = np.zeros(3, abi.CPARAM_RULE_DTYPE)
    cp["flow_id"], cp["count"], cp["threshold_type"] = [11, 22, 33], [2, 3, 5], abi.THRESHOLD_GLOBAL
    cp["sample_count"], cp["window_interval_ms"] = [10, 4, 1], 1000
    ora = ClusterTokenService()
    engs = {}
    for name in "AB":
        eng = _engine(12, 1 << 17, 1 << 13, 1 << 13)
        eng.cparam_load_rules(cp, None, 11)
        engs[name] = eng
    ora.set_namespaces(engs["A"].ns)
    ora.load_param_rules(cp, None)
    ref = RefDecoder(cp["flow_id"])
    waves = [[(STR, b"user-%d-%d-of-a-long-name" % (w, k)) if k % 2 else (L, struct.pack(">q", w * 10**6 + k))
              for k in range(400)] for w in range(4)]
    a_live, a_before, b_size, t = [], [], [], T0 + 1000
    for b in range(8):
        frames = []
        for v in waves[b % 4]:
            for _ in range(int(rng.integers(1, 6))):
                frames.append(param_frame(len(frames), int(cp["flow_id"][rng.integers(0, 3)]), 1, [v]))
        frames = [frames[j] for j in rng.permutation(len(frames))]
        n = len(frames)
        ts = t + np.sort(rng.integers(0, 700, n)).astype(np.int64)
        want_req, want_values, _, want_kind = ref.decode(frames, ts)
        want = ora.decide_param(want_req, want_values)
        assert (want["status"] == abi.OK).any() and (want["status"] == abi.BLOCKED).any()
        content = list(ref.ids)
        for name, eng in engs.items():
            d = _decode(eng, frames, ts)
            res_t = torch.empty(n * abi.RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            eng.cparam_decide_device(d.req_t.data_ptr(), n, d.val_t.data_ptr(), d.n_values, res_t.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = res_t.cpu().numpy().view(abi.RES_DTYPE)
            assert np.array_equal(d.kind, want_kind)
            if not np.array_equal(got, want):
                i = np.nonzero(got != want)[0][0]
                raise AssertionError(f"batch {b}, engine {name}, frame {i}: oracle={want[i]} gpu={got[i]}")
            assert eng.vdict_lookup(d.values) == [content[int(v) - 1] for v in want_values], (b, name)
        now = int(ts[-1])
        A = engs["A"]
        a_before.append(A.vdict_size()[0])
        A.cparam_sweep(now)
        a_live.append(A.vdict_sweep()["live"])
        b_size.append(engs["B"].vdict_size()[0])
        t += 3000
    assert b_size == sorted(b_size) and b_size[3] == b_size[-1] == 1600
    assert all(x < y for x, y in zip(a_live[1:], a_before[1:]))
    assert max(a_live[1:]) <= 400 and max(a_before) <= 800


# ------------------------------------------------------------------------------------ 4: capacity comes back

def test_capacity_comes_back():
    eng, model = _engine(4, 1 << 10, 64), VDictModel()
    _intern(eng, model, [(I, struct.pack(">i", k)) for k in range(16)])            # exactly full
    more = [(I, struct.pack(">i", 100)), (I, struct.pack(">i", 3))]
    assert _code(eng.vdict_intern, more) == abi.SG_E_CAPACITY
    _assert_same(eng, model)
    _sweep(eng, model, [2, 9], [2, 9])
    assert _intern(eng, model, more) == [1, 3]                                     # the value 3 was freed: fresh again
    _assert_same(eng, model)


def test_arena_comes_back():
    eng, model = _engine(4, 100, 64), VDictModel()
    _intern(eng, model, [(STR, bytes([65 + k]) * 25) for k in range(4)])           # exactly full
    more = [(STR, b"nine-byte")]
    assert _code(eng.vdict_intern, more) == abi.SG_E_CAPACITY
    _assert_same(eng, model)
    st = _sweep(eng, model, [3], [3])
    assert (st["arena_before"], st["arena_after"]) == (100, 25)
    assert _intern(eng, model, more + [(STR, b"Q" * 66)]) == [1, 2]                # 25 + 9 + 66: exactly full again
    assert _code(eng.vdict_intern, [(STR, b"123456789")]) == abi.SG_E_CAPACITY
    _assert_same(eng, model)


# ------------------------------------------------------------------------------------ 5: edges

def _mixed(lo, hi):
    """Values of three kinds; every third one lives in the arena, every 29th past the cooperative-copy threshold."""
    out = []
    for k in range(lo, hi):
        out.append((STR, (b"long-value-%d-" % k) * (40 if k % 29 == 0 else 1)) if k % 3 == 0 else
                   (STR, b"s%d" % k) if k % 3 == 1 else (L, struct.pack(">q", k)))
    return out


def test_empty_dictionary():
    eng, model = _engine(4, 1 << 10, 16), VDictModel()
    assert _sweep(eng, model, [], []) == dict.fromkeys(FIELDS, 0)
    assert _code(eng.vdict_sweep, [1]) == abi.SG_E_INVAL
    assert _intern(eng, model, _mixed(0, 3)) == [1, 2, 3]


def test_twice_everything_dead_nothing_dead():
    eng, model = _engine(10, 1 << 16, 1 << 10), VDictModel()
    _intern(eng, model, _mixed(0, 600))
    keep = [i for i in range(1, 601) if i % 5 < 2]
    first = _sweep(eng, model, keep, keep)
    assert first["removed"] == 360
    second = _sweep(eng, model, keep, keep)                                        # twice in a row
    assert second == dict(first, removed=0, arena_before=first["arena_after"])
    _assert_same(eng, model)
    ids = _intern(eng, model, _mixed(600, 650))
    assert ids[:3] == [2, 3, 4]
    everything = model.live_ids()
    assert _sweep(eng, model, everything, everything)["removed"] == 0              # nothing dead
    _assert_same(eng, model)
    st = _sweep(eng, model, [], [])                                                # everything dead
    assert (st["live"], st["free_ids"], st["arena_after"]) == (0, model.high, 0)
    assert _intern(eng, model, _mixed(700, 705)) == [1, 2, 3, 4, 5]
    _assert_same(eng, model)


def test_grow_after_a_sweep_and_a_sweep_after_a_grow():
    eng, model = _engine(9, 1 << 15, 1 << 10), VDictModel()
    _intern(eng, model, _mixed(0, 500))
    keep = [i for i in range(1, 501) if i % 7 in (0, 1, 5)]
    _sweep(eng, model, keep, keep)
    _intern(eng, model, _mixed(1000, 1020))                                        # part of the free list is used
    assert model.free
    eng.vdict_grow(11, 1 << 16)                                                    # holes and a non-empty free list
    _assert_same(eng, model)
    nxt = model.free[:3]
    assert _intern(eng, model, _mixed(2000, 2003)) == nxt
    _intern(eng, model, _mixed(3000, 3900))                                        # past the old capacity
    assert model.high > 512 and not model.free
    _assert_same(eng, model)
    keep = [i for i in model.live_ids() if i % 2]
    _sweep(eng, model, keep, keep)                                                 # a sweep after the grow
    _assert_same(eng, model)
    assert _intern(eng, model, _mixed(5000, 5003)) == [2, 4, 6]


# ------------------------------------------------------------------------------------ 6: refusals

def test_refusals_change_nothing():
    from sentinel_amd.engine import load_library
    bare = _engine(0, 0)
    assert _code(bare.vdict_sweep) == abi.SG_E_INVAL                               # before sg_vdict_init
    eng, model = _engine(8, 1 << 12, 256), VDictModel()
    _intern(eng, model, _mixed(0, 100))
    keep = list(range(1, 101, 2))
    _sweep(eng, model, keep, keep)
    _intern(eng, model, _mixed(200, 210))
    free = model.free[0]
    L = load_library()
    st = abi.sg_vdict_sweep_stats()
    calls = [lambda: L.sg_vdict_sweep(eng.h, None, 3, C.byref(st)),                # a list promised and not given
             lambda: _code(eng.vdict_sweep, [1, 0]),                               # 0
             lambda: _code(eng.vdict_sweep, [1, model.high + 1]),                  # above high
             lambda: _code(eng.vdict_sweep, [1, free])]                            # already free
    for call in calls:
        assert call() == abi.SG_E_INVAL
        _assert_same(eng, model)
    assert [getattr(st, f) for f in FIELDS] == [0] * 6
    nxt = model.free[:2]
    assert _intern(eng, model, _mixed(300, 302)) == nxt
    _sweep(eng, model, [1], [1])                                                   # and the handle still sweeps


# ------------------------------------------------------------------------------------ 7: in flight

def test_sweep_with_local_tickets_outstanding():
    """sg_vdict_sweep drains the pipeline first: tickets issued before it complete with their own answers, and the
    batch enqueued after it decides on."""
    from tests.test_local_pipeline_gpu import _check, _compare, _enqueue_all, _results, _rules, _trace
    rng = np.random.default_rng(2907)
    lrules = _rules(12, rng, lo=3, hi=30)
    trace, ora = _trace(lrules, [(9_000, 600), (9_000, 600), (9_000, 600)], 2, 1000, 500, seed=2907)
    eng, model = _engine(8, 1 << 12, 256, 1 << 14), VDictModel()
    eng.local_load_rules(lrules, 2, 1000, 500)
    _intern(eng, model, _mixed(0, 120))
    bufs = _enqueue_all(eng, [trace[0][0], trace[1][0]])
    keep = list(range(1, 121, 3))
    _sweep(eng, model, keep, keep)
    bufs += _enqueue_all(eng, [trace[2][0]])
    for k, (_, d_out, ticket) in enumerate(bufs):
        eng.local_wait(ticket)
        _check(_results(d_out), trace[k][1], k)
    _compare(eng, ora, len(lrules), 2)
    _assert_same(eng, model)
    assert _intern(eng, model, _mixed(500, 502)) == [2, 3]
