"""GatewayFlowSlot on the device (sg_gateway_*, gateway.hip) against the pure-Python restatement of the adapter
(tests/gateway_ref.py) and, for the decisions, the oracle's ParamFlowSlot / LocalChain fed the reference's converted
rules and args. Everything is compared for equality: arg spans, arg kinds, value ids, counts, the dictionary's
contents, every decision with the rule that threw, thread counts and token states."""
import numpy as np
import pytest

from gateway_ref import D, NM, Item, Parser, Rule, pack_requests, random_rules, rules_to_abi
from oracle.binding import LocalChain, ParamFlowSlot, degrade_rule, local_flow_rule, local_rule
from sentinel_amd import abi

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
ROUTE, API = abi.GW_RESOURCE_MODE_ROUTE_ID, abi.GW_RESOURCE_MODE_CUSTOM_API_NAME
STAGE = 16384   # gateway.hip kGwStage: LDS bytes staged per 256-item step


@pytest.fixture(autouse=True, scope="module")
def _torch_first():
    """These tests hand torch device buffers to the library: torch's HIP runtime has to initialise before the
    library's (the order smoke() uses); initialised second it finds no device."""
    import torch
    torch.cuda.init()
    yield


def _engine(cap_log2=14, arena=1 << 20, max_values=1 << 15, max_batch=1 << 15, vdict=True):
    from sentinel_amd.engine import FlowEngine
    eng = FlowEngine(device=0, max_batch=max_batch)
    if vdict:
        eng.vdict_init(cap_log2, arena, max_values)
    return eng


def _load(eng, rules, n_resources, extra=None, extra_hot=None):
    rules_abi, blob = rules_to_abi(rules)
    return eng.gateway_load_rules(rules_abi, blob, n_resources, extra, extra_hot)


def _assert_dictionary(eng, ref):
    size, arena = eng.vdict_size()
    assert size == len(ref.dict.ids) and arena == ref.dict.arena()
    assert eng.vdict_lookup(np.arange(1, size + 1, dtype=np.uint64)) == ref.dict.keys()


def _assert_parsed(eng, ref, requests, **pack):
    """Device parse of `requests` against the reference: args, values, counts and both span outputs."""
    req, items, data = pack_requests(requests, **pack)
    n = len(req)
    ext = np.zeros(n, abi.SLOT_EXT_DTYPE)
    ext["context"], ext["arg_begin"], ext["arg_count"], ext["args_null"] = np.arange(n) % 7, 99, 98, 1
    pev = np.zeros(n, abi.PSLOT_EVENT_DTYPE)
    pev["ts_ms"], pev["resource"], pev["count"], pev["kind"] = T0 + np.arange(n), req["resource"], 3, np.arange(n) % 2
    pev["arg_begin"], pev["arg_count"], pev["args_null"] = 77, 76, 1
    args, values, ext_out, pev_out = eng.gateway_parse_host(req, items, data, ext=ext, pev=pev)
    want_args, want_values, spans = ref.parse(requests)
    assert (len(args), len(values)) == (len(want_args), len(want_values))   # n_args / n_values
    if not np.array_equal(args, want_args):
        i = np.nonzero(args != want_args)[0][0]
        raise AssertionError(f"arg {i}: {args[i]} vs {want_args[i]}")
    if not np.array_equal(values, want_values):
        i = np.nonzero(values != want_values)[0][0]
        raise AssertionError(f"value {i}: {values[i]} vs {want_values[i]}")
    if n:
        begin, count = np.array([s[0] for s in spans]), np.array([s[1] for s in spans])
        for out, src in ((ext_out, ext), (pev_out, pev)):
            assert np.array_equal(out["arg_begin"], begin) and np.array_equal(out["arg_count"], count)
            assert not out["args_null"].any()
        assert np.array_equal(ext_out["context"], ext["context"])                       # the other fields are left
        for f in ("ts_ms", "resource", "count", "kind"):
            assert np.array_equal(pev_out[f], pev[f])
    _assert_dictionary(eng, ref)
    return want_args, want_values


POOL = [None, b"", b"a", b"12345678", b"123456789", b"x" * 300, NM, b"Wow", b"warn", b"ab", b"abc", b"zzabczz",
        b"10.0.0.7", b"id=5", b"\xc3\xa9t\xc3\xa9", b"l" * 297 + b"abc", b"x" * 9, D]


def _random_requests(rng, ref, n, n_resources, extra_strings=()):
    pool = POOL + list(extra_strings)
    out = []
    for _ in range(n):
        res = int(rng.integers(0, n_resources + 1))   # n_resources itself: a resource the tables do not have
        k = ref.mgr.n_item_rules(res)
        raw = [(pool[int(rng.integers(len(pool)))], bool(rng.random() < 0.5)) for _ in range(k)]
        out.append((res, int(rng.integers(0, 2)), raw))
    return out


def test_parser_parity():
    rng = np.random.default_rng(11)
    n_res = 40
    rules = random_rules(rng, n_res)
    eng, ref = _engine(), Parser(rules)
    loaded, hot, source = _load(eng, rules, n_res)
    want, want_hot, want_source = ref.pslot_rules()
    assert np.array_equal(loaded, want) and np.array_equal(hot, want_hot) and np.array_equal(source, want_source)
    for r in range(n_res + 1):
        assert eng.gateway_param_rule_count(r) == (ref.mgr.n_item_rules(r), ref.mgr.has_item_less(r))
    _assert_dictionary(eng, ref)                      # "$NM" = 1, "$D" = 2
    requests = _random_requests(rng, ref, 3000, n_res)
    args, values = _assert_parsed(eng, ref, requests)
    # the trace holds what it is meant to hold
    assert any(res == n_res for res, _, _ in requests)
    assert (args["kind"] == abi.ARG_NULL).sum() > 100 and (values == ref.nm_id).sum() > 100
    assert (values == ref.d_id).sum() > 100 and len(ref.dict.ids) > 15
    assert sum(1 for a in ref.parse(requests)[2] if a[1] == 0) > 100    # emptied arrays and unknown resources
    # a second batch reuses the ids and adds new strings behind them
    before = len(ref.dict.ids)
    more = [b"new-%d" % i for i in range(40)] + [b"n%d" % i for i in range(40)]
    _assert_parsed(eng, ref, _random_requests(rng, ref, 2000, n_res, more), gap=b"#")
    assert len(ref.dict.ids) > before + 40
    # a reload keeps "$NM" and "$D" where they are
    _load(eng, rules, n_res)
    _assert_dictionary(eng, ref)


def _one_rule_parser(pattern=b"ab", match=abi.GW_MATCH_CONTAINS):
    rules = [Rule(0, count=5, item=Item(abi.GW_PARSE_HEADER, "h", pattern, match))]
    eng, ref = _engine(), Parser(rules)
    _load(eng, rules, 1)
    return eng, ref


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_item_counts_at_the_grid_edges(n):
    eng, ref = _one_rule_parser()
    rng = np.random.default_rng(n)
    strings = [b"v%d" % (i % 97) if rng.random() < 0.5 else b"ab-%d" % i for i in range(n)]
    _assert_parsed(eng, ref, [(0, ROUTE, [(s, False)]) for s in strings])


@pytest.mark.parametrize("last", [63, 64, 65])
def test_step_bytes_around_the_stage(last):
    """A 256-item step of 16383 / 16384 / 16385 bytes (one below the stage, exactly it, one above: read in place), then a
    second step that starts at an unaligned offset."""
    eng, ref = _one_rule_parser()
    first = [(b"%04d" % i) + (b"ab" if i % 3 else b"zz") * 30 for i in range(255)] + [(b"%04d" % 255) + b"a" * (last - 4)]
    assert sum(len(s) for s in first) == STAGE - 64 + last
    second = [b"tail-%d-ab" % i if i % 2 else b"tail-%d" % i for i in range(100)]
    _assert_parsed(eng, ref, [(0, ROUTE, [(s, False)]) for s in first + second])
    assert len(ref.dict.ids) == 2 + 170 + 50         # the strings without "ab" are "$NM"


def test_strings_larger_than_the_stage_unaligned_offsets_and_empty_strings_at_step_boundaries():
    eng, ref = _one_rule_parser()
    rng = np.random.default_rng(5)
    strings = [b"s%d" % i + (b"ab" if i % 2 else b"") for i in range(600)]
    strings[100] = b"q" * 20_000 + b"ab"             # larger than the stage, inside a step
    strings[300] = b"q" * 20_000 + b"ab"             # ... and again: one id
    strings[301] = b"q" * 20_001 + b"b"
    for i in (0, 255, 256, 257, 511, 512, 599):      # zero-length strings where the steps begin and end
        strings[i] = b""
    requests = [(0, ROUTE, [(s if rng.random() > 0.03 else None, False)]) for s in strings]
    _assert_parsed(eng, ref, requests, gap=b"\x01")  # every string starts one byte off the previous one's end
    _assert_parsed(eng, ref, requests, align=4)
    assert len(ref.dict.ids) < 2 + 600


def test_refusals_change_nothing():
    from sentinel_amd.engine import EngineError
    rules = [Rule(0, count=5, item=Item(abi.GW_PARSE_CLIENT_IP)), Rule(0, count=9)]

    def refused(eng, code, requests=None, packed=None, **kw):
        size = eng.vdict_size()
        req, items, data = packed if packed is not None else pack_requests(requests)
        with pytest.raises(EngineError) as e:
            eng.gateway_parse_host(req, items, data, **kw)
        assert e.value.code == code and eng.vdict_size() == size
        return e.value

    def ips(lo, hi, width=4):
        return [(0, ROUTE, [(b"%0*d" % (width, i), False)]) for i in range(lo, hi)]

    # a dictionary of 2^4 values: "$NM", "$D" and 14 more
    eng, ref = _engine(cap_log2=4, arena=1 << 10, max_values=64), Parser(rules)
    _load(eng, rules, 1)
    refused(eng, abi.SG_E_CAPACITY, ips(0, 15))
    _assert_parsed(eng, ref, ips(20, 30) + ips(20, 24))       # the ids a fresh handle gives: the refusal left no trace
    refused(eng, abi.SG_E_CAPACITY, ips(28, 35))              # 2 known + 5 new > the 4 free
    _assert_parsed(eng, ref, ips(26, 34))
    assert eng.vdict_size() == (16, 0)
    _assert_parsed(eng, ref, ips(20, 34))                     # full, and every known string still resolves
    # an arena of 30 bytes: strings of 11 bytes
    eng, ref = _engine(cap_log2=8, arena=30, max_values=64), Parser(rules)
    _load(eng, rules, 1)
    refused(eng, abi.SG_E_CAPACITY, ips(0, 3, width=11))
    _assert_parsed(eng, ref, ips(1, 3, width=11) + ips(0, 5))
    assert eng.vdict_size() == (9, 22)
    refused(eng, abi.SG_E_CAPACITY, ips(7, 8, width=11))
    # caps one short: the counts come back, nothing is interned
    e = refused(eng, abi.SG_E_CAPACITY, ips(100, 110), args_cap=19)
    assert (e.n_args, e.n_values) == (20, 20)
    e = refused(eng, abi.SG_E_CAPACITY, ips(100, 110), values_cap=19)
    assert (e.n_args, e.n_values) == (20, 20)
    refused(eng, abi.SG_E_CAPACITY, ips(100, 165))            # more requests than max_batch_values
    refused(eng, abi.SG_E_CAPACITY, ips(100, 140))            # 80 values: more than max_batch_values
    # a wrong item_count, also for a request the predicate empties; ranges out of bounds; an item of two requests
    for mode in (ROUTE, API):
        refused(eng, abi.SG_E_INVAL, [(0, mode, [])])
        refused(eng, abi.SG_E_INVAL, [(0, mode, [(b"a", False), (b"b", False)])])
    refused(eng, abi.SG_E_INVAL, [(1, ROUTE, [(b"a", False)])])   # a resource without rules has no item rule
    req, items, data = pack_requests(ips(200, 203))
    bad = req.copy()
    bad["item_begin"][2] = 3
    refused(eng, abi.SG_E_INVAL, packed=(bad, items, data))
    bad = req.copy()
    bad["item_begin"][2] = 1
    refused(eng, abi.SG_E_INVAL, packed=(bad, items, data))
    bad = items.copy()
    bad["len"][1] = len(data)
    refused(eng, abi.SG_E_INVAL, packed=(req, bad, data))
    bad = items.copy()
    bad["off"][0], bad["len"][0] = 0xFFFFFFF0, 0x20
    refused(eng, abi.SG_E_INVAL, packed=(req, bad, data))
    bad = items.copy()
    bad["len"][0] = 1 << 24
    refused(eng, abi.SG_E_INVAL, packed=(req, bad, data))
    _assert_parsed(eng, ref, ips(200, 203))                   # and the handle still parses
    # parse before load, load before sg_vdict_init
    eng = _engine()
    refused(eng, abi.SG_E_INVAL, ips(0, 1))
    eng = _engine(vdict=False)
    with pytest.raises(EngineError) as e:
        _load(eng, rules, 1)
    assert e.value.code == abi.SG_E_INVAL
    eng = _engine()
    for bad_rule, blob, n_res in ((Rule(1, count=1), b"", 1), (Rule(0, count=1, item=Item(0, None, b"abc")), b"ab", 1)):
        with pytest.raises(EngineError) as e:
            eng.gateway_load_rules(rules_to_abi([bad_rule])[0], blob, n_res)
        assert e.value.code == abi.SG_E_INVAL


# ---- GatewayFlowSlot end to end

N_RES = 8
IP_IDX, TIER_IDX, URL_IDX, SID_IDX, DEFAULT_IDX = range(5)


def _gateway_rules():
    """Per route: a client-IP QPS rule with burst over 2 s, an EXACT-pattern rule whose non-matching traffic passes
    whatever its count (0: every "vip" is blocked), a throttle rule, a THREAD rule and an item-less rule; behind them,
    on the even routes, an ordinary ParamFlowRule on the client IP. The caller's order interleaves the routes and,
    on the odd ones, names the item-less rule first: it still takes the last index."""
    per_route, extra = [], []
    for r in range(N_RES):
        mine = [Rule(r, count=3, interval_sec=2, burst=2, item=Item(abi.GW_PARSE_CLIENT_IP), capacity_log2=10),
                Rule(r, count=0, item=Item(abi.GW_PARSE_HEADER, "X-Tier", b"vip", abi.GW_MATCH_EXACT), capacity_log2=10),
                Rule(r, count=25, control_behavior=2, max_queueing_timeout_ms=60,
                     item=Item(abi.GW_PARSE_URL_PARAM, "u", b"id=", abi.GW_MATCH_CONTAINS), capacity_log2=10),
                Rule(r, grade=0, count=6, item=Item(abi.GW_PARSE_COOKIE, "sid"), capacity_log2=10)]
        default = Rule(r, count=30 + r, capacity_log2=10)
        per_route.append([default] + mine if r % 2 else mine + [default])
        if r % 2 == 0:
            p = np.zeros((), abi.PSLOT_RULE_DTYPE)
            p["resource"], p["param_idx"], p["grade"] = r, IP_IDX, 1
            p["rule"]["count"], p["rule"]["duration_sec"], p["rule"]["capacity_log2"] = 2.0, 1, 10
            extra.append(p)
    routes = np.random.default_rng(3).permutation(N_RES)
    return [per_route[r][k] for k in range(5) for r in routes], np.array(extra, abi.PSLOT_RULE_DTYPE)


class Trace:
    """Entries with gateway requests, and the exits of entries that passed in an earlier batch (same request)."""

    def __init__(self, seed):
        self.rng, self.open, self.t = np.random.default_rng(seed), [], T0 + 250
        self.ip_p = 1.0 / np.arange(1, 41) ** 1.1
        self.ip_p /= self.ip_p.sum()

    def _request(self):
        rng = self.rng
        res = int(min(rng.zipf(1.4), N_RES + 1)) - 1           # N_RES: a route without rules
        if res >= N_RES:
            return res, ROUTE, []
        raw = [None] * 4                                       # by item index: the item rules' order per route
        raw[IP_IDX] = (b"10.1.0.%d" % rng.choice(40, p=self.ip_p), False)
        u = rng.random()
        raw[TIER_IDX] = ((b"vip" if u < 0.15 else None if u < 0.25 else b"tier-%d" % rng.integers(0, 5)), False)
        u = rng.random()
        raw[URL_IDX] = ((b"x&id=%d" % rng.integers(0, 3) if u < 0.6 else b"other" if u < 0.9 else None), False)
        raw[SID_IDX] = ((b"session-%d" % rng.integers(0, 12) if rng.random() < 0.9 else None), False)
        return res, (API if rng.random() < 0.03 else ROUTE), raw

    def batch(self, n, span):
        rng = self.rng
        ts = self.t + np.sort(rng.integers(0, span, n))
        out = []
        for i in range(n):
            if self.open and rng.random() < 0.4:
                request, create = self.open.pop(int(rng.integers(len(self.open))))
                out.append((int(ts[i]), abi.LOCAL_EXIT, request, create))
            else:
                out.append((int(ts[i]), abi.LOCAL_ENTRY, self._request(), 0))
        self.t += span
        return out

    def absorb(self, events, passed):
        for (ts, kind, request, _), ok in zip(events, passed):
            if kind == abi.LOCAL_ENTRY and ok:
                self.open.append((request, ts))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _e2e_setup():
    rules, extra = _gateway_rules()
    ref = Parser(rules)
    for r in rules:
        if r.item is not None:   # the indices Trace lays its items out by
            assert r.item.index == {0: IP_IDX, 2: TIER_IDX, 3: URL_IDX, 4: SID_IDX}[r.item.parse_strategy]
    conv, hot, source = ref.pslot_rules()
    shifted = extra.copy()
    shifted["rule"]["hot_begin"] += len(hot)
    all_rules = np.concatenate([conv, shifted])
    ora = ParamFlowSlot(all_rules, hot, n_resources=N_RES)
    eng = _engine(max_batch=1 << 15)
    loaded, loaded_hot, loaded_source = _load(eng, rules, N_RES, extra)
    assert np.array_equal(loaded, all_rules) and np.array_equal(loaded_hot, hot)
    assert np.array_equal(loaded_source, np.concatenate([source, np.full(len(extra), -1)]))
    kind_of = []       # what a loaded rule is: "item", "default", "thread" or "ordinary"
    for k in range(len(all_rules)):
        if k >= len(conv):
            kind_of.append("ordinary")
        else:
            g = rules[int(source[k])]
            kind_of.append("default" if g.item is None else "thread" if g.grade == 0 else "item")
    return rules, ref, all_rules, ora, eng, kind_of


def _not_vacuous(all_rules, kind_of, entries):
    """Conditions on the oracle's answers that keep the end-to-end test from passing vacuously. entries: (request,
    pass, rule) of all entries on routes with rules."""
    n = len(entries)
    blocked = [rule for _, ok, rule in entries if not ok]
    assert 0.1 * n <= len(blocked) <= 0.9 * n, (len(blocked), n)
    kinds = {kind_of[rule] for rule in blocked}
    assert kinds == {"item", "default", "thread", "ordinary"}, kinds
    nm = 0
    for (res, mode, raw), ok, rule in entries:
        tier = raw[TIER_IDX][0]
        if mode == ROUTE and tier is not None and tier != b"vip":   # "$NM" at the pattern rule
            nm += 1
            assert ok or int(all_rules[rule]["param_idx"]) != TIER_IDX, (res, raw, rule)
    assert nm > 0.3 * n


def _requests_of(events):
    return [request for _, _, request, _ in events]


def test_gateway_flow_slot_end_to_end():
    import torch
    rules, ref, all_rules, ora, eng, kind_of = _e2e_setup()
    tr = Trace(7)
    seen, stream = [], torch.cuda.current_stream().cuda_stream
    for n, span in ((1300, 1500), (1400, 1700), (1300, 900)):
        events = tr.batch(n, span)
        requests = _requests_of(events)
        want_args, want_values, spans = ref.parse(requests)
        pev = np.zeros(n, abi.PSLOT_EVENT_DTYPE)
        pev["ts_ms"], pev["kind"], pev["count"] = [e[0] for e in events], [e[1] for e in events], 1
        pev["resource"] = [r[0] for r in requests]
        full = pev.copy()
        full["arg_begin"], full["arg_count"] = [s[0] for s in spans], [s[1] for s in spans]
        want = ora.decide(full, want_args, want_values)
        # device: parse into the event records, decide from the parser's device buffers
        req, items, data = pack_requests(requests)
        args, values, _, pev_out, dev = eng.gateway_parse_host(req, items, data, pev=pev, with_device=True)
        assert np.array_equal(args, want_args) and np.array_equal(values, want_values) and np.array_equal(pev_out, full)
        out_t = torch.zeros(n * abi.PSLOT_RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        eng.pslot_decide_device(dev["pev"].data_ptr(), n, dev["args"].data_ptr(), len(args), dev["values"].data_ptr(),
                                len(values), out_t.data_ptr(), stream)
        torch.cuda.synchronize()
        got = out_t.cpu().numpy().view(abi.PSLOT_RES_DTYPE)
        if not np.array_equal(got, want):
            i = np.nonzero(got != want)[0][0]
            raise AssertionError(f"event {i}: {events[i]} oracle={want[i]} gpu={got[i]}")
        tr.absorb(events, want["pass"] == 1)
        seen += [(e[2], bool(w["pass"]), int(w["rule"])) for e, w in zip(events, want)
                 if e[1] == abi.LOCAL_ENTRY and e[2][0] < N_RES]
    _not_vacuous(all_rules, kind_of, seen)
    ids = range(1, len(ref.dict.ids) + 1)
    for res in range(N_RES):
        for v in ids:
            for idx in (SID_IDX, IP_IDX):
                assert eng.pslot_thread_count(res, idx, v) == ora.thread_count(res, idx, v), (res, idx, v)
    touched = 0
    for ri in range(len(all_rules)):
        for v in ids:
            f, lt, tk = ora.token_state(ri, v)
            if f:
                touched += 1
                gf, glt, gtk = eng.param_state(ri, v)
                assert (gf, glt if f & 1 else 0, gtk if f & 2 else 0) == (f, lt if f & 1 else 0, tk if f & 2 else 0)
    assert touched > 100


def test_whole_chain_with_gateway_args():
    import torch
    rules, ref, all_rules, ps, eng, kind_of = _e2e_setup()
    base = np.array([local_rule(0.0, abi.FLOW_GRADE_NONE, [degrade_rule(abi.DEGRADE_EXCEPTION_RATIO, 0.4, 1, 5, 1000)])
                     for _ in range(N_RES)], abi.LOCAL_RULE_DTYPE)
    frules = np.array([local_flow_rule(r, 14.0 + r) for r in range(N_RES)], abi.LOCAL_FLOW_RULE_DTYPE)
    ora = LocalChain(2, 1000, 500)
    ora.load_rules(base)
    kept = ora.load_flow_rules(frules)
    ora.attach_params(ps)
    eng.local_load_rules(base, 2, 1000, 500)
    assert eng.local_load_flow_rules(frules) == kept
    eng.block_log_enable(12)
    tr = Trace(9)
    stream = torch.cuda.current_stream().cuda_stream
    gateway_block, statuses = None, set()
    for n, span in ((1000, 1400), (1000, 1200)):
        events = [e for e in tr.batch(n, span) if e[2][0] < N_RES]      # the chain knows N_RES resources
        n = len(events)
        requests = _requests_of(events)
        want_args, want_values, spans = ref.parse(requests)
        ev = np.zeros(n, abi.LOCAL_EVENT_DTYPE)
        ev["ts_ms"], ev["create_ts"], ev["count"] = [e[0] for e in events], [e[3] for e in events], 1
        ev["resource"] = [r[0] for r in requests]
        err = tr.rng.random(n) < 0.3
        ev["kind"] = [abi.LOCAL_ENTRY if e[1] == abi.LOCAL_ENTRY else abi.LOCAL_EXIT_ERROR if x else abi.LOCAL_EXIT
                      for e, x in zip(events, err)]
        ext = np.zeros(n, abi.SLOT_EXT_DTYPE)
        full = ext.copy()
        full["arg_begin"], full["arg_count"] = [s[0] for s in spans], [s[1] for s in spans]
        want = ora.decide_ext(ev, full, want_args, want_values)
        req, items, data = pack_requests(requests)
        args, values, ext_out, _, dev = eng.gateway_parse_host(req, items, data, ext=ext, with_device=True)
        assert np.array_equal(ext_out, full) and np.array_equal(values, want_values)
        ev_t = _dev(ev)
        out_t = torch.zeros(n * abi.LOCAL_RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        eng.slot_decide_device(ev_t.data_ptr(), dev["ext"].data_ptr(), n, dev["args"].data_ptr(), len(args),
                               dev["values"].data_ptr(), len(values), out_t.data_ptr(), stream)
        torch.cuda.synchronize()
        got = out_t.cpu().numpy().view(abi.LOCAL_RES_DTYPE)
        if not np.array_equal(got, want):
            i = np.nonzero(got != want)[0][0]
            raise AssertionError(f"event {i}: {events[i]} oracle={want[i]} gpu={got[i]}")
        entry = ev["kind"] == abi.LOCAL_ENTRY
        tr.absorb(events, entry & ((want["status"] == abi.LOCAL_PASS) | (want["status"] == abi.LOCAL_PASS_WAIT)))
        statuses |= set(int(s) for s in want["status"][entry])
        for i in np.nonzero(entry & (want["status"] == abi.LOCAL_BLOCK_PARAM))[0]:
            rule = int(want["wait_ms"][i])
            if gateway_block is None and kind_of[rule] == "item":
                a = want_args[spans[i][0] + int(all_rules[rule]["param_idx"])]
                gateway_block = (int(ev["ts_ms"][i]) // 1000 * 1000, int(ev["resource"][i]),
                                 int(want_values[a["value_begin"]]))
    assert {abi.LOCAL_PASS, abi.LOCAL_BLOCK_PARAM, abi.LOCAL_BLOCK_FLOW, abi.LOCAL_BLOCK_DEGRADE} <= statuses
    # LogSlot: the row of a gateway block names the matched value by its dictionary id
    rows, _, _ = eng.block_log(tr.t + 2000)
    second, res, value = gateway_block
    hit = rows[(rows["timestamp"] == second) & (rows["resource"] == res) & (rows["status"] == abi.LOCAL_BLOCK_PARAM) &
               (rows["app_kind"] == abi.BLOCK_APP_VALUE) & (rows["app"] == value)]
    assert len(hit) == 1 and hit[0]["count"] >= 1
    assert eng.vdict_lookup([value])[0] in ref.dict.keys()
