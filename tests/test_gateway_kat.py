"""The gateway adapter's JUnit expectations over the pure-Python restatement (tests/gateway_ref.py):
GatewayParamParserTest, GatewayRuleManagerTest and GatewayRuleConverterTest of sentinel-api-gateway-adapter-common.
Routes and API names are resource indices, strings are bytes, and a `\\d+` verdict is computed here with Python's re
(the caller's side of the REGEX contract). The Java tests read indices through getIndex(), so caller-order indices
satisfy them."""
import re

from gateway_ref import (D, NM, Item, Manager, Rule, apply_to_param_rule, is_valid_rule, parse_parameter_for)
from sentinel_amd import abi

ROUTE, API = abi.GW_RESOURCE_MODE_ROUTE_ID, abi.GW_RESOURCE_MODE_CUSTOM_API_NAME
ROUTE_A, ROUTE_B = 0, 1


def _raw(mgr, resource, by_rule):
    """The RequestItemParser mock: {rule → returned string}, laid out by the rules' indices."""
    n = mgr.n_item_rules(resource)
    raw = [(None, False)] * n
    for rule, value in by_rule:
        verdict = False
        if rule.item.pattern and rule.item.match_strategy == abi.GW_MATCH_REGEX and value is not None:
            verdict = re.fullmatch(rule.item.pattern.decode(), value.decode()) is not None   # Matcher.matches()
        raw[rule.item.index] = (value, verdict)
    return raw


def test_parse_parameters_no_param_item():
    rules = [Rule(ROUTE_A, count=5, interval_sec=1),
             Rule(ROUTE_A, count=10, control_behavior=2, max_queueing_timeout_ms=1000)]
    mgr = Manager(rules)
    assert len(parse_parameter_for(mgr, ROUTE_A, ROUTE, [])) == 1


def test_parse_parameters_with_items():
    no_param = Rule(ROUTE_A, count=10, interval_sec=10)
    r1 = Rule(ROUTE_A, count=2, interval_sec=2, burst=2, item=Item(abi.GW_PARSE_CLIENT_IP))
    r2 = Rule(ROUTE_A, count=10, interval_sec=1, control_behavior=2, max_queueing_timeout_ms=600,
              item=Item(abi.GW_PARSE_HEADER, "X-Sentinel-Flag"))
    r3 = Rule(ROUTE_A, count=20, interval_sec=1, burst=5, item=Item(abi.GW_PARSE_URL_PARAM, "p"))
    r4 = Rule(ROUTE_A, count=120, interval_sec=10, burst=30, item=Item(abi.GW_PARSE_HOST))
    r5 = Rule(ROUTE_A, count=50, interval_sec=30, item=Item(abi.GW_PARSE_COOKIE, "myCookie"))
    api1 = Rule(ROUTE_B, resource_mode=API, count=5, interval_sec=1, item=Item(abi.GW_PARSE_URL_PARAM, "p"))
    mgr = Manager([r1, r2, r3, r4, r5, no_param, api1])
    raw = _raw(mgr, ROUTE_A, [(r1, b"66.77.88.99"), (r2, b"Sentinel"), (r3, b"17"), (r4, b"hello.test.sentinel"),
                              (r5, b"Sentinel-Foo")])
    params = parse_parameter_for(mgr, ROUTE_A, ROUTE, raw)
    assert len(params) == 6   # 5 with parameters, 1 normal flow with the generated constant
    assert params[r1.item.index] == b"66.77.88.99"
    assert params[r2.item.index] == b"Sentinel"
    assert params[r3.item.index] == b"17"
    assert params[r4.item.index] == b"hello.test.sentinel"
    assert params[r5.item.index] == b"Sentinel-Foo"
    assert params[-1] == D
    assert len(parse_parameter_for(mgr, ROUTE_B, ROUTE, _raw(mgr, ROUTE_B, [(api1, b"17")]))) == 0
    params = parse_parameter_for(mgr, ROUTE_B, API, _raw(mgr, ROUTE_B, [(api1, b"fs")]))
    assert len(params) == 1 and params[api1.item.index] == b"fs"


def test_parse_parameters_with_empty_item_pattern():
    r1 = Rule(ROUTE_A, count=10, interval_sec=2,
              item=Item(abi.GW_PARSE_HEADER, "X-Sentinel-Flag", b"", abi.GW_MATCH_EXACT))
    mgr = Manager([r1])
    params = parse_parameter_for(mgr, ROUTE_A, ROUTE, _raw(mgr, ROUTE_A, [(r1, b"Sent1nel")]))
    assert len(params) == 1
    assert params[r1.item.index] == b"Sent1nel"   # an empty pattern does not take effect


def test_parse_parameters_with_item_pattern_matching():
    r1 = Rule(ROUTE_A, count=10, interval_sec=1, control_behavior=2, max_queueing_timeout_ms=600,
              item=Item(abi.GW_PARSE_HEADER, "X-Sentinel-Flag", b"Wow", abi.GW_MATCH_EXACT))
    r2 = Rule(ROUTE_A, count=20, interval_sec=1, burst=5,
              item=Item(abi.GW_PARSE_URL_PARAM, "p", b"warn", abi.GW_MATCH_CONTAINS))
    api1 = Rule(ROUTE_B, resource_mode=API, count=5, interval_sec=1,
                item=Item(abi.GW_PARSE_URL_PARAM, "p", rb"\d+", abi.GW_MATCH_REGEX))
    mgr = Manager([r1, r2, api1])

    def route(header, param):
        return parse_parameter_for(mgr, ROUTE_A, ROUTE, _raw(mgr, ROUTE_A, [(r1, header), (r2, param)]))

    params = route(b"Wow", b"warn")
    assert len(params) == 2 and params[r1.item.index] == b"Wow" and params[r2.item.index] == b"warn"
    params = route(b"Wow_foo", b"warn_foo")
    assert len(params) == 2 and params[r1.item.index] == NM and params[r2.item.index] == b"warn_foo"
    params = route(b"foo", b"foo")
    assert len(params) == 2 and params[r1.item.index] == NM and params[r2.item.index] == NM
    params = parse_parameter_for(mgr, ROUTE_B, API, _raw(mgr, ROUTE_B, [(api1, b"23")]))
    assert len(params) == 1 and params[api1.item.index] == b"23"
    params = parse_parameter_for(mgr, ROUTE_B, API, _raw(mgr, ROUTE_B, [(api1, b"some233")]))
    assert len(params) == 1 and params[api1.item.index] == NM


def test_load_and_get_gateway_rules():
    rule1 = Rule(0, count=500, interval_sec=1)
    rule2 = Rule(0, count=20, interval_sec=2, burst=5, item=Item(abi.GW_PARSE_CLIENT_IP))
    rule3 = Rule(1, count=10, interval_sec=1, control_behavior=2, max_queueing_timeout_ms=600,
                 item=Item(abi.GW_PARSE_HEADER, "X-Sentinel-Flag"))
    mgr = Manager([rule1, rule2, rule3])
    assert [p for p in mgr.converted if p.resource == 0]
    assert rule2.item.index == 0 and rule3.item.index == 0
    kept = [r for _, r in mgr.by_resource[0]]
    assert rule1 in kept and rule2 in kept
    # the item-less rule sits on the last index, behind the one item rule
    assert [(p.param_idx, p.source) for p in mgr.converted if p.resource == 0] == [(0, 1), (1, 0)]


def test_is_valid_rule():
    bad1 = Rule(resource=None)                       # new GatewayFlowRule(): no resource
    bad2 = Rule(0, interval_sec=0)
    bad3 = Rule(0, item=Item(abi.GW_PARSE_URL_PARAM))
    bad4 = Rule(0, item=Item(abi.GW_PARSE_URL_PARAM, "p", b"def", -1))
    good1 = Rule(0)
    good2 = Rule(0, item=Item(0))
    good3 = Rule(0, item=Item(field_name="Origin", pattern=b"def", match_strategy=abi.GW_PARSE_HEADER))
    for r in (bad1, bad2, bad3, bad4):
        assert not is_valid_rule(r)
    for r in (good1, good2, good3):
        assert is_valid_rule(r)


def test_convert_and_apply_to_param_rule():
    r1 = Rule(0, count=2, interval_sec=2, burst=2, item=Item(abi.GW_PARSE_CLIENT_IP))
    p = apply_to_param_rule(r1, 1)
    assert (p.resource, p.count, p.behavior, p.duration_sec, p.burst, p.param_idx) == (0, 2.0, 0, 2, 2, 1)
    assert r1.item.index == 1 and p.hot == ()
    r2 = Rule(0, count=2, item=Item(abi.GW_PARSE_CLIENT_IP, pattern=b""))
    assert apply_to_param_rule(r2, 0).hot == ((NM, 10_000_000),)   # a non-null pattern, even an empty one


def test_equal_item_less_rules_collapse():
    rules = [Rule(3, count=5), Rule(3, count=5), Rule(3, count=6), Rule(3, count=5, item=Item(0)),
             Rule(3, count=5, capacity_log2=9)]
    mgr = Manager(rules)
    assert [(p.param_idx, p.source) for p in mgr.converted] == [(0, 3), (1, 0), (1, 2)]
    assert mgr.has_item_less(3) and mgr.n_item_rules(3) == 1
