"""Gateway API definitions and request expansion on the device (sg_gateway_load_apis, sg_gateway_verdict_ids,
sg_gateway_set_item_fields, sg_gateway_expand_batch; gateway_api.hip) against the pure-Python restatement
(tests/gateway_api_ref.py) and, end to end, the existing gateway reference and the oracle's slot chain fed the entries
the Python reference expands. Everything is compared for equality: entries, their order, source indices, events,
contexts, every item's bytes and flags, counts, and every decision."""
import re

import numpy as np
import pytest

from gateway_api_ref import (HOST, Api, Gateway, HttpReq, Pred, apis_to_abi, entries_to_abi, pack_http, random_apis,
                             random_path)
from gateway_ref import Item, Parser, Rule, random_rules, rules_to_abi
from oracle.binding import LocalChain, ParamFlowSlot, local_flow_rule, local_rule
from sentinel_amd import abi
from test_gateway_api_kat import ANT_KAT

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
PREFIX, REGEX = abi.GW_URL_MATCH_PREFIX, abi.GW_URL_MATCH_REGEX
IP, HOSTK, HEADER, URL, COOKIE = range(5)
STAGE = 16384   # gateway_api.hip kGwxStage: LDS bytes staged per 256-request step
FILL = 0xAB     # what the output buffers hold before a call


@pytest.fixture(autouse=True, scope="module")
def _torch_first():
    """These tests hand torch device buffers to the library: torch's HIP runtime has to initialise before the
    library's (the order smoke() uses); initialised second it finds no device."""
    import torch
    torch.cuda.init()
    yield


def _engine(max_batch=1 << 15):
    from sentinel_amd.engine import FlowEngine
    eng = FlowEngine(device=0, max_batch=max_batch)
    eng.vdict_init(14, 1 << 20, 1 << 15)
    return eng


def _load(eng, apis, rules, n_resources, field_ids=None, default_context=0, extra=None):
    a, preds, blob = apis_to_abi(apis)
    eng.gateway_load_apis(a, preds, blob, n_resources, default_context)
    rules_abi, rblob = rules_to_abi(rules)
    eng.gateway_load_rules(rules_abi, rblob, n_resources, extra)
    if field_ids is not None:
        eng.gateway_set_item_fields(field_ids)
    return Gateway(apis, rules, field_ids, default_context)


def _expected_items(entries):
    return [it for e in entries for it in e[6]]


def _assert_outputs(out, entries, data):
    req, src, ev, ctx = entries_to_abi(entries)
    n = len(entries)
    assert len(out["req"]) == n, (len(out["req"]), n)
    for name, got, want in (("req", out["req"], req), ("src", out["src"], src), ("ev", out["ev"], ev),
                            ("context", out["ext"]["context"], ctx)):
        if not np.array_equal(got, want):
            i = np.nonzero(got != want)[0][0]
            raise AssertionError(f"{name} of entry {i}: {got[i]} vs {want[i]} ({entries[i]})")
    # the arg fields are the parser's: left as they were
    for f in ("arg_begin", "arg_count", "args_null"):
        assert (out["ext"][f].view(np.uint32) == FILL * 0x01010101).all()
    items = _expected_items(entries)
    assert len(out["items"]) == len(items)
    for i, (got, (raw, verdict)) in enumerate(zip(out["items"], items)):
        flags = abi.GW_ITEM_REGEX_MATCH if verdict else 0
        if raw is None:
            assert (int(got["off"]), int(got["len"]), int(got["flags"])) == (0, 0, flags | abi.GW_ITEM_NULL), (i, got)
        else:
            assert int(got["flags"]) == flags and data[int(got["off"]):int(got["off"]) + int(got["len"])] == raw, (i, got)
    # nothing is written behind the counts
    for name, size, count in (("req", 16, n), ("src", 4, n), ("ev", 32, n), ("ext", 16, n), ("items", 16, len(items))):
        assert set(out["raw"][name][size * count:]) <= {FILL}, name


def _assert_expanded(eng, gw, requests, slack=3, order=None, **pack):
    """Device expansion of `requests` against the reference. order: the request records are handed over in this
    order, their bytes staying where the original order laid them."""
    req, fields, verdicts, data = pack_http(requests, **pack)
    if order is not None:
        req, requests = req[order], [requests[i] for i in order]
    entries = gw.expand(requests)
    out = eng.gateway_expand_host(req, fields, verdicts, data, len(entries) + slack,
                                  len(_expected_items(entries)) + slack, fill=FILL)
    _assert_outputs(out, entries, data)
    return entries


# ---- known answers

def test_known_answers_on_the_device():
    patterns = sorted({p for p, _, _ in ANT_KAT})
    apis = [Api(k, [Pred(p.encode(), PREFIX)]) for k, p in enumerate(patterns)]
    trap = len(apis)
    apis += [Api(trap, [Pred(b"/abc", PREFIX)]), Api(trap + 1, [Pred(b"/abc")])]       # PREFIX without a wildcard
    # SentinelGatewayFilterTest.testPickMatchingApiDefinitions
    apis += [Api(trap + 2, [Pred(b"/product/**", PREFIX)]),
             Api(trap + 3, [Pred(b"/something"), Pred(b"/other/**", PREFIX)])]
    eng = _engine()
    gw = _load(eng, apis, [], trap + 4)
    paths = sorted({s.encode() for _, s, _ in ANT_KAT}) + [b"/abc", b"/product/123", b"/products", b"/something",
                                                            b"/other/foo/3"]
    requests = [HttpReq(T0 + k, None, path=s) for k, s in enumerate(paths)]
    entries = _assert_expanded(eng, gw, requests)
    matched = {(paths[e[0]], e[1]) for e in entries}
    for pattern, path, want in ANT_KAT:
        assert ((path.encode(), patterns.index(pattern)) in matched) is want, (pattern, path)
    assert (b"/abc", trap) not in matched and (b"/abc", trap + 1) in matched
    picks = {s: sorted(r for p, r in matched if p == s and r >= trap + 2) for s in paths[-4:]}
    assert picks == {b"/product/123": [trap + 2], b"/products": [], b"/something": [trap + 3],
                     b"/other/foo/3": [trap + 3]}


# ---- random parity

def _random_requests(rng, gw, n, n_resources, vids):
    names = [0, 1, 2, 3]
    out = []
    for k in range(n):
        fields = []
        for _ in range(int(rng.integers(0, 6))):
            kind = int(rng.integers(0, 6))      # 5: a kind no rule reads
            fields.append((kind, names[int(rng.integers(4))] if kind >= HEADER else 0, b"v%d" % rng.integers(0, 50)))
        verdicts = tuple(v for v in range(vids) if rng.random() < 0.04)
        route = None if rng.random() < 0.2 else int(rng.integers(0, n_resources + 1))   # n_resources: no rules
        path = random_path(rng) if rng.random() < 0.93 else b"a/" + random_path(rng)[1:]
        out.append(HttpReq(T0 + k, route, int(rng.integers(0, 4)), int(rng.integers(0, 9)), path, fields, verdicts))
    return out


def test_expansion_parity():
    rng = np.random.default_rng(23)
    n_res = 40
    apis = random_apis(rng, 60, n_res)
    apis = [Api(0, [Pred(b"/a")], name_blank=True), Api(1, None), Api(2, [])] + apis    # whatever the draw held
    rules = random_rules(rng, n_res)
    field_ids = rng.integers(0, 4, len(rules)).astype(np.uint32)
    eng = _engine()
    gw = _load(eng, apis, rules, n_res, field_ids, default_context=7)
    d = gw.defs
    assert eng.gateway_verdict_ids() == gw.verdict_ids()
    n_api_vids, n_vids = len(d.vid_pred), len(gw.verdict_ids())
    assert n_vids > n_api_vids > 0
    # at most a tenth of the predicates is the caller's: the rest is decided on the device
    assert 0 < d.cls.count(HOST) <= 0.1 * len(d.cls)
    requests = _random_requests(rng, gw, 3000, n_res, n_vids)
    entries = _assert_expanded(eng, gw, requests)
    # the run holds what it is meant to hold
    how = [d.explain(q.path, q.verdicts) for q in requests]
    for kind in ("exact", "bucket", "wild", "host"):
        assert sum(1 for h in how if any(kind in w for _, w in h)) > 30, kind
    assert sum(1 for h in how if len(h) > 1) > 100 and sum(1 for h in how if not h) > 100
    assert sum(1 for q, h in zip(requests, how) if q.route is None and not h) > 20      # no entry at all
    names = [a.resource for a in apis if a.preds is not None and not a.name_blank]
    assert len(names) > len(set(names))                                                 # duplicate names
    assert any(a.name_blank for a in apis) and any(a.preds is None for a in apis) and any(a.preds == [] for a in apis)
    items = _expected_items(entries)
    assert sum(1 for raw, _ in items if raw is not None) > 200 and sum(1 for raw, _ in items if raw is None) > 200
    assert sum(1 for _, v in items if v) > 10
    # before sg_gateway_set_item_fields every item is null; the verdict bits stay
    eng2 = _engine()
    gw2 = _load(eng2, apis, rules, n_res, None, default_context=7)
    assert all(raw is None for raw, _ in _expected_items(_assert_expanded(eng2, gw2, requests[:600])))


# ---- edge shapes

def _simple(default_context=0):
    """Route 0 with a client-IP rule and a header rule; API 1 = /p/** or exactly /e; API 2 = /?/x."""
    apis = [Api(1, [Pred(b"/p/**", PREFIX), Pred(b"/e")]), Api(2, [Pred(b"/?/x", PREFIX)])]
    rules = [Rule(0, 0, count=5, item=Item(IP)), Rule(1, 1, count=5, item=Item(HEADER, "h")), Rule(2, 1, count=4)]
    eng = _engine()
    return eng, _load(eng, apis, rules, 3, [0, 9, 0], default_context)


@pytest.mark.parametrize("n", [0, 1, 256, 257, 513])
def test_request_counts_at_the_grid_edges(n):
    eng, gw = _simple()
    paths = [b"/p/%d" % k if k % 3 == 0 else b"/e" if k % 3 == 1 else b"/none" for k in range(n)]
    requests = [HttpReq(T0 + k, 0 if k % 2 else None, 1, 2, s, [(IP, 0, b"10.0.0.%d" % (k % 200)), (HEADER, 9, b"h%d" % k)])
                for k, s in enumerate(paths)]
    entries = _assert_expanded(eng, gw, requests)
    assert len(entries) == sum(1 for k in range(n) if k % 2) + sum(1 for k in range(n) if k % 3 != 2)


def test_no_route_and_no_match_throughout():
    eng, gw = _simple()
    assert _assert_expanded(eng, gw, [HttpReq(T0, None, path=b"/none")]) == []
    assert _assert_expanded(eng, gw, [HttpReq(T0 + k, None, path=b"/none/%d" % k) for k in range(300)]) == []
    entries = _assert_expanded(eng, gw, [HttpReq(T0 + k, None, path=b"/p/%d" % k) for k in range(300)])
    assert len(entries) == 300 and all(e[2] == 1 for e in entries)


@pytest.mark.parametrize("last", [63, 64, 65])
@pytest.mark.parametrize("lead", [b"", b"#", b"###"])
def test_step_bytes_around_the_stage(last, lead):
    """A 256-request step whose paths take 16383 / 16384 / 16385 bytes from the aligned start (one below the stage,
    exactly it, one above: read in place), starting 0, 1 and 3 bytes off a 4-byte boundary, then a second step."""
    eng, gw = _simple()
    first = [(b"/p/%03d/" % k) + (b"ab" if k % 3 else b"zz") * 28 + b"c" for k in range(255)]
    assert all(len(s) == 64 for s in first)
    first.append(b"/p/" + b"a" * (last - 3 - len(lead)))
    assert len(lead) + sum(len(s) for s in first) == STAGE - 64 + last
    second = [b"/e" if k % 2 else b"/x/e" for k in range(100)]
    entries = _assert_expanded(eng, gw, [HttpReq(T0 + k, None, path=s) for k, s in enumerate(first + second)], lead=lead)
    assert len(entries) == 256 + 50


def test_long_paths_odd_layouts_and_small_paths():
    eng, gw = _simple()
    long_hit, long_miss = b"/p/" + b"q" * 20_000, b"/q/" + b"q" * 20_000     # longer than the stage: read in place
    paths = [b"/p/%d" % k for k in range(600)]
    paths[100], paths[300], paths[301] = long_hit, long_miss, long_hit + b"/x"
    small = [b"/", b"", b"//", b"///p//a//", b"//e", b"/e", b"/e/", b"/\xc3\xa9/x", b"/ab/x", b"/\xe2\x82\xac/x", b"p/a",
             b"/p", b"/p/", b"/a/x/"]
    for k, s in zip((0, 255, 256, 257, 511, 512, 599, 7, 8, 9, 10, 11, 12, 13), small):
        paths[k] = s
    requests = [HttpReq(T0 + k, None, path=s) for k, s in enumerate(paths)]
    got = {paths[e[0]]: e[1] for e in _assert_expanded(eng, gw, requests, gap=b"\x01")}     # every path one byte off
    _assert_expanded(eng, gw, requests, align=4)
    _assert_expanded(eng, gw, requests, order=np.arange(len(requests))[::-1])               # offsets descending
    _assert_expanded(eng, gw, requests, order=np.random.default_rng(1).permutation(len(requests)))
    want = {b"///p//a//": 1, b"/e": 1, b"/\xc3\xa9/x": 2, b"/\xe2\x82\xac/x": 2, b"/p": 1, b"/p/": 1, long_hit: 1,
            long_hit + b"/x": 1}
    assert {s: r for s, r in got.items() if not s.startswith(b"/p/") or s in want} == want


# ---- refusals

def test_refusals_change_nothing():
    from sentinel_amd.engine import EngineError, FlowEngine
    eng, gw = _simple()
    ids = eng.gateway_verdict_ids()
    good = [HttpReq(T0 + k, 0, 1, 2, b"/p/%d" % k, [(IP, 0, b"10.0.0.1"), (HEADER, 9, b"x")]) for k in range(5)]
    packed = pack_http(good)

    def refused(code, packed, req_cap=64, items_cap=64, engine=None, **kw):
        with pytest.raises(EngineError) as e:
            (engine or eng).gateway_expand_host(*packed, req_cap, items_cap, fill=FILL, **kw)
        assert e.value.code == code, e.value
        for name, raw in e.value.raw.items():
            assert set(raw) <= {FILL}, name                  # outputs as they were
        return e.value

    def edited(which, field, index, value):
        arrays = [a.copy() if isinstance(a, np.ndarray) else a for a in packed]
        arrays[which][field][index] = value
        return tuple(arrays)

    req, fields, verdicts, data = packed
    refused(abi.SG_E_INVAL, edited(0, "path_len", 4, len(data)))                 # a path past the blob
    refused(abi.SG_E_INVAL, edited(0, "path_off", 2, 0xFFFFFFF0))
    refused(abi.SG_E_INVAL, edited(0, "field_count", 4, 3))                      # a field range past fields[]
    refused(abi.SG_E_INVAL, edited(0, "field_begin", 0, 0xFFFFFFFF))
    refused(abi.SG_E_INVAL, edited(1, "len", 3, len(data)))                      # a field's bytes past the blob
    refused(abi.SG_E_INVAL, edited(0, "verdict_count", 1, 1))                    # a verdict range past verdicts[]
    refused(abi.SG_E_INVAL, packed, byte_shift=1)                                # misaligned bytes
    refused(abi.SG_E_INVAL, packed, byte_shift=2)
    # verdict slices: this handle has no verdict id at all, one with two ids below
    with_v = [HttpReq(T0, 0, 1, 2, b"/p/1", [], (0,))]
    refused(abi.SG_E_INVAL, pack_http(with_v))
    # caps one short: the counts come back
    e = refused(abi.SG_E_CAPACITY, packed, req_cap=9)
    assert (e.n_req, e.n_items) == (10, 10)
    e = refused(abi.SG_E_CAPACITY, packed, items_cap=9)
    assert (e.n_req, e.n_items) == (10, 10)
    # the handle is as it was
    assert eng.gateway_verdict_ids() == ids
    _assert_expanded(eng, gw, good)
    # n above max_batch
    small = FlowEngine(device=0, max_batch=4)
    small.vdict_init(10, 1 << 12, 64)
    gws = _load(small, gw.defs.apis, gw.mgr.rules, 3, [0, 9, 0])
    refused(abi.SG_E_CAPACITY, packed, engine=small)
    _assert_expanded(small, gws, good[:4])
    # failed loads leave the old definitions and fields in force
    for apis, n_res in (([Api(3, [Pred(b"/p/**", PREFIX)])], 3),):
        with pytest.raises(EngineError) as e:
            eng.gateway_load_apis(*apis_to_abi(apis), n_res)
        assert e.value.code == abi.SG_E_INVAL
    a, preds, blob = apis_to_abi([Api(1, [Pred(b"/zz/**", PREFIX)])])
    bad = a.copy()
    bad["pred_count"] = 2
    for args in ((bad, preds, blob, 3), (a, preds, blob[:-1], 3)):
        with pytest.raises(EngineError) as e:
            eng.gateway_load_apis(*args)
        assert e.value.code == abi.SG_E_INVAL
    with pytest.raises(EngineError) as e:
        eng.gateway_set_item_fields([1, 2])                                      # not the rule count
    assert e.value.code == abi.SG_E_INVAL
    _assert_expanded(eng, gw, good)


def test_verdict_slices_and_calls_before_the_loads():
    from sentinel_amd.engine import EngineError
    apis = [Api(1, [Pred(b"/r1.*", REGEX)]), Api(2, [Pred(b"/r2.*", REGEX), Pred(b"/e")])]
    rules = [Rule(0, 0, count=5, item=Item(HEADER, "h", b"x+", abi.GW_MATCH_REGEX))]
    a, preds, blob = apis_to_abi(apis)
    rules_abi, rblob = rules_to_abi(rules)
    eng = _engine()

    def refused(requests):
        with pytest.raises(EngineError) as e:
            eng.gateway_expand_host(*pack_http(requests), 16, 16, fill=FILL)
        assert e.value.code == abi.SG_E_INVAL
        assert all(set(raw) <= {FILL} for raw in e.value.raw.values())

    one = [HttpReq(T0, 0, path=b"/e")]
    refused(one)                                             # before both loads
    eng.gateway_load_apis(a, preds, blob, 3)
    refused(one)                                             # before sg_gateway_load_rules
    eng.gateway_load_rules(rules_abi, rblob, 3)
    gw = Gateway(apis, rules, None)
    _assert_expanded(eng, gw, one)                           # fields never set: null items, and no refusal
    eng.gateway_set_item_fields([4])
    gw = Gateway(apis, rules, [4])
    assert eng.gateway_verdict_ids() == [(0, 0), (0, 1), (1, 0)]
    ok = [HttpReq(T0 + k, 0, path=b"/q", fields=[(HEADER, 4, b"xx")], verdicts=v)
          for k, v in enumerate([(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)])]
    entries = _assert_expanded(eng, gw, ok)
    assert [len([e for e in entries if e[0] == k]) for k in range(8)] == [1, 2, 2, 1, 3, 2, 2, 3]
    for v in ((1, 0), (0, 0), (3,), (0, 1, 2, 2), (2, 1), (0xFFFFFFFF,)):
        refused(ok[:3] + [HttpReq(T0, 0, path=b"/q", verdicts=v)] + ok[3:])
    _assert_expanded(eng, gw, ok)


def test_reloads_renumber_the_verdict_ids():
    eng = _engine()
    apis = [Api(1, [Pred(b"/r.*", REGEX), Pred(b"/a/{x}", PREFIX)])]
    rules = [Rule(0, 0, count=5, item=Item(IP, None, b"1.*", abi.GW_MATCH_REGEX)), Rule(0, 0, count=5, item=Item(HOSTK)),
             Rule(2, 0, count=5, item=Item(IP, None, b"2.*", abi.GW_MATCH_REGEX))]
    gw = _load(eng, apis, rules, 3, [0, 0, 0])
    assert eng.gateway_verdict_ids() == gw.verdict_ids() == [(0, 0), (0, 1), (1, 0), (1, 2)]
    q = [HttpReq(T0, 0, path=b"/z", fields=[(IP, 0, b"1.1.1.1"), (HOSTK, 0, b"h")], verdicts=(2,)),
         HttpReq(T0, 2, path=b"/z", fields=[(IP, 0, b"2.2.2.2")], verdicts=(1, 3))]
    _assert_expanded(eng, gw, q)
    # fewer API predicates: the rules' ids move down
    apis2 = [Api(1, [Pred(b"/a/**", PREFIX), Pred(b"/a/{x}", PREFIX)])]
    a, preds, blob = apis_to_abi(apis2)
    eng.gateway_load_apis(a, preds, blob, 3)
    gw = Gateway(apis2, rules, [0, 0, 0])
    assert eng.gateway_verdict_ids() == gw.verdict_ids() == [(0, 1), (1, 0), (1, 2)]
    q2 = [HttpReq(T0, 0, path=b"/z", fields=[(IP, 0, b"1.1.1.1")], verdicts=(1,)),
          HttpReq(T0, 2, path=b"/a/y", fields=[(IP, 0, b"2.2.2.2")], verdicts=(0, 2))]
    _assert_expanded(eng, gw, q2)                            # the fields survive a reload of the definitions
    # other rules: new ids, and the fields are dropped
    rules2 = [rules[1], rules[2], rules[0]]
    rules_abi, rblob = rules_to_abi(rules2)
    eng.gateway_load_rules(rules_abi, rblob, 3)
    gw = Gateway(apis2, rules2, None)
    assert eng.gateway_verdict_ids() == gw.verdict_ids() == [(0, 1), (1, 1), (1, 2)]
    entries = _assert_expanded(eng, gw, q2)
    assert all(raw is None for raw, _ in _expected_items(entries))
    eng.gateway_set_item_fields([0, 0, 0])
    _assert_expanded(eng, Gateway(apis2, rules2, [0, 0, 0]), q2)


# ---- end to end: expand → parse → slot chain

N_ROUTES, N_RES = 4, 7      # routes 0 .. 3, custom APIs 4 .. 6
TIER, UID, SID = 1, 2, 3    # the caller's field name ids
TIER_RE, SID_RE, PATH_RE = rb"v\d+", rb"s-[0-4]", rb"/r/\d+"


def _e2e_rules():
    rules, field_ids = [], []
    for r in range(N_ROUTES):
        rules += [Rule(r, 0, count=3, interval_sec=2, burst=1, item=Item(IP), capacity_log2=10),
                  Rule(r, 0, count=1, item=Item(HEADER, "X-Tier", TIER_RE, abi.GW_MATCH_REGEX), capacity_log2=10),
                  Rule(r, 0, count=40 + r, capacity_log2=10)]
        field_ids += [0, TIER, 0]
    for r in range(N_ROUTES, N_RES):
        rules += [Rule(r, 1, count=2, item=Item(URL, "uid"), capacity_log2=10),
                  Rule(r, 1, count=1, item=Item(COOKIE, "sid", SID_RE, abi.GW_MATCH_REGEX), capacity_log2=10)]
        field_ids += [UID, SID]
    order = np.random.default_rng(4).permutation(len(rules))
    return [rules[i] for i in order], [field_ids[i] for i in order]


E2E_APIS = [Api(4, [Pred(b"/product/**", PREFIX)]), Api(5, [Pred(b"/something"), Pred(b"/other/**", PREFIX)]),
            Api(6, [Pred(PATH_RE, REGEX), Pred(b"/*/special", PREFIX)]), Api(5, None)]
E2E_PATHS = [b"/product/1", b"/product/special", b"/something", b"/other/x", b"/r/17", b"/r/special", b"/none", b"/"]


def _e2e_requests(rng, gw, n, t):
    """Requests in time order with the verdicts a host computes: java.util.regex's part, here Python's re."""
    ts = t + np.sort(rng.integers(0, 1500, n))
    out = []
    for k in range(n):
        fields = [(IP, 0, b"10.1.0.%d" % min(rng.zipf(1.5), 20))]
        if rng.random() < 0.8:
            fields.append((HEADER, TIER, b"v%d" % rng.integers(0, 3) if rng.random() < 0.5 else b"basic"))
        fields.append((HEADER, 77, b"unread"))
        if rng.random() < 0.7:
            fields += [(URL, UID, b"u%d" % rng.integers(0, 6)), (URL, UID, b"second-is-ignored")]     # a duplicate field
        if rng.random() < 0.7:
            fields.append((COOKIE, SID, b"s-%d" % rng.integers(0, 9)))
        route = None if rng.random() < 0.15 else int(rng.integers(0, N_ROUTES))
        q = HttpReq(int(ts[k]), route, int(rng.integers(0, 3)), 0 if route is None else 1 + route % 2,
                    E2E_PATHS[int(rng.integers(len(E2E_PATHS)))], fields)
        verdicts = [v for v, pi in enumerate(gw.defs.vid_pred) if re.fullmatch(gw.defs.flat[pi][1].pattern, q.path)]
        for i, vid in gw.rule_vid.items():
            item = gw.mgr.rules[i].item
            value = next((val for kind, name, val in fields if kind == item.parse_strategy and
                          (kind < HEADER or name == gw.field_ids[i])), None)
            if value is not None and re.fullmatch(item.pattern, value):
                verdicts.append(vid)
        q.verdicts = tuple(sorted(verdicts))
        out.append(q)
    return out


def test_expand_parse_and_slot_chain_end_to_end():
    import torch
    rules, field_ids = _e2e_rules()
    ref = Parser(rules)
    conv, hot, _ = ref.pslot_rules()
    ps = ParamFlowSlot(conv, hot, n_resources=N_RES)
    base = np.array([local_rule() for _ in range(N_RES)], abi.LOCAL_RULE_DTYPE)
    frules = np.array([local_flow_rule(r, 12.0 + r) for r in range(N_RES)] +
                      [local_flow_rule(0, 3.0, limit_app=1),                                   # origin 1 on route 0
                       local_flow_rule(4, 4.0, strategy=abi.STRATEGY_CHAIN, ref=0)],            # API 4 from context 0
                      abi.LOCAL_FLOW_RULE_DTYPE)
    ora = LocalChain(2, 1000, 500)
    ora.load_rules(base)
    kept = ora.load_flow_rules(frules, 2, 3)
    ora.attach_params(ps)
    eng = _engine()
    gw = _load(eng, E2E_APIS, rules, N_RES, field_ids, default_context=0)
    assert gw.verdict_ids() == eng.gateway_verdict_ids() and len(gw.verdict_ids()) == 1 + N_RES
    eng.local_load_rules(base, 2, 1000, 500)
    assert eng.local_load_flow_rules(frules, 2, 3) == kept
    rng = np.random.default_rng(31)
    stream = torch.cuda.current_stream().cuda_stream
    statuses, t, per_request, nm, regex_kept = set(), T0 + 250, [], 0, 0
    for n in (900, 1000):
        requests = _e2e_requests(rng, gw, n, t)
        t += 1500
        entries = gw.expand(requests)
        want_args, want_values, spans = ref.parse([(e[1], e[2], e[6]) for e in entries])
        _, _, ev, ctx = entries_to_abi(entries)
        ext = np.zeros(len(entries), abi.SLOT_EXT_DTYPE)
        ext["context"] = ctx
        ext["arg_begin"], ext["arg_count"] = [s[0] for s in spans], [s[1] for s in spans]
        want = ora.decide_ext(ev, ext, want_args, want_values)
        # device: expand, parse the expansion's buffers where they lie, decide
        req, fields, verdicts, data = pack_http(requests)
        n_items = len(_expected_items(entries))
        out = eng.gateway_expand_host(req, fields, verdicts, data, len(entries), n_items, with_device=True)
        _assert_outputs_e2e(out, entries, ev, ctx)
        dev = out["dev"]
        cap = n_items + len(entries)
        a_t = torch.zeros(max(cap, 1) * 16, dtype=torch.uint8, device="cuda")
        v_t = torch.zeros(max(cap, 1) * 8, dtype=torch.uint8, device="cuda")
        na, nv = eng.gateway_parse_device(dev["req"].data_ptr(), len(entries), dev["items"].data_ptr(), n_items,
                                          dev["data"].data_ptr(), len(data), a_t.data_ptr(), cap, v_t.data_ptr(), cap,
                                          dev["ext"].data_ptr(), 0, stream)
        assert (na, nv) == (len(want_args), len(want_values))
        torch.cuda.synchronize()
        assert np.array_equal(a_t.cpu().numpy().view(abi.PSLOT_ARG_DTYPE)[:na], want_args)
        assert np.array_equal(v_t.cpu().numpy().view(np.uint64)[:nv], want_values)
        assert np.array_equal(dev["ext"].cpu().numpy().view(abi.SLOT_EXT_DTYPE)[:len(entries)], ext)
        out_t = torch.zeros(len(entries) * abi.LOCAL_RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        eng.slot_decide_device(dev["ev"].data_ptr(), dev["ext"].data_ptr(), len(entries), a_t.data_ptr(), na,
                               v_t.data_ptr(), nv, out_t.data_ptr(), stream)
        torch.cuda.synchronize()
        got = out_t.cpu().numpy().view(abi.LOCAL_RES_DTYPE)
        if not np.array_equal(got, want):
            i = np.nonzero(got != want)[0][0]
            raise AssertionError(f"entry {i}: {entries[i]} oracle={want[i]} gpu={got[i]}")
        statuses |= set(int(s) for s in want["status"])
        per_request += [len([e for e in entries if e[0] == k]) for k in range(n)]
        nm += int((want_values == ref.nm_id).sum())
        regex_kept += sum(1 for e in entries for raw, v in e[6] if v)
    assert {abi.LOCAL_PASS, abi.LOCAL_BLOCK_PARAM, abi.LOCAL_BLOCK_FLOW} <= statuses
    assert {0, 1, 2, 3} <= set(per_request)                  # no entry, route only, route + API, route + two APIs
    assert nm > 100 and regex_kept > 100                     # REGEX item rules both ways, through the verdict ids


def _assert_outputs_e2e(out, entries, ev, ctx):
    req, src, _, _ = entries_to_abi(entries)
    assert np.array_equal(out["req"], req) and np.array_equal(out["src"], src) and np.array_equal(out["ev"], ev)
    assert np.array_equal(out["ext"]["context"], ctx)
