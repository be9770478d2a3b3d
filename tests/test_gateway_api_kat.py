"""Known answers of the gateway's API matching through the Python restatement (tests/gateway_api_ref.py): the Ant
matcher's contract (include/sentinel_gpu.h), predicate classification, and the reference's JUnit expectations
(GatewayApiDefinitionManagerTest.testIsValidApi, SentinelGatewayFilterTest.testPickMatchingApiDefinitions). The device
and the sanitizer-built host program answer the same tables (tests/test_gateway_api_gpu.py,
tests/cpp/test_gateway_api_host.cpp)."""
import pytest

from gateway_api_ref import (ANT, EXACT, HOST, NEVER, SKIP, Api, Definitions, Gateway, HttpReq, Pred, ant_match, classify,
                             is_valid_api, seg_match)
from gateway_ref import Item, Rule
from sentinel_amd import abi

PREFIX, REGEX = abi.GW_URL_MATCH_PREFIX, abi.GW_URL_MATCH_REGEX

ANT_KAT = [
    ("/product/**", "/product", True), ("/product/**", "/product/", True), ("/product/**", "/product/a/b", True),
    ("/product/**", "/products", False), ("/a/*", "/a/b", True), ("/a/*", "/a/", True), ("/a/*", "/a", False),
    ("/a/*", "/a/b/c", False), ("/a/?", "/a/b", True), ("/a/?", "/a/é", True), ("/a/?", "/a/bc", False),
    ("/a/*.html", "/a/x.html", True), ("/a/*.html", "/a/b/x.html", False), ("/**/x.jsp", "/x.jsp", True),
    ("/**/x.jsp", "/a/b/x.jsp", True), ("/a/**/b", "/a/b", True), ("/a/**/b", "/a/x/y/b", True),
    ("/a/**/b", "/a/b/c", False), ("/a/b", "/a/b/", False), ("/a/b/", "/a/b", False), ("a/*", "/a/b", False),
    ("/a/b*", "/a//bc", True), ("/A/*", "/a/b", False),
]


@pytest.mark.parametrize("pattern,path,want", ANT_KAT)
def test_ant_known_answers(pattern, path, want):
    assert ant_match(pattern.encode(), path.encode()) is want


def test_ant_edges():
    for pattern, path, want in [("/**", "/", True), ("/**", "", False), ("**", "", True), ("/*", "/", True),
                                ("/a/**/", "/a/b", True), ("/a/**/b/", "/a/b", False), ("/a/**/b/", "/a/x/b/", True),
                                ("/a**b", "/axyb", True), ("/a**b", "/ab", True), ("/a**b", "/a/b", False),
                                ("/??", "/€", False), ("/?", "/€", True), ("/*??", "/€", False), ("/*?", "/😀", True),
                                ("/a/**/b/c", "/a/c", False), ("/a/**/b/c", "/a/b/b/c", True),
                                ("/*a*b", "/xaxbxab", True), ("/*a*b", "/xaxbxa", False), ("/a/*", "/a//", True)]:
        assert ant_match(pattern.encode(), path.encode()) is want, (pattern, path)
    assert seg_match(b"*", b"") and not seg_match(b"?", b"") and seg_match(b"a?c", "aéc".encode())


def test_prefix_without_a_wildcard_never_matches_its_own_text():
    assert classify(Pred(b"/abc", PREFIX)) == NEVER
    d = Definitions([Api(0, [Pred(b"/abc", PREFIX)])])
    assert d.match(b"/abc") == []
    assert Definitions([Api(0, [Pred(b"/abc")])]).match(b"/abc") == [0]


def test_classification():
    assert [classify(Pred(b"/abc", s)) for s in (0, 7, -1)] == [EXACT] * 3          # the switch's default branch
    assert classify(Pred(b"/a/**", PREFIX)) == ANT and classify(Pred(b"/a?", PREFIX)) == ANT
    assert classify(Pred(b"/a/.*", REGEX)) == HOST
    assert classify(Pred(b"/a/(", REGEX, regex_invalid=True)) == NEVER
    assert classify(Pred(b"/a/{id}", PREFIX)) == HOST and classify(Pred(b"/a}", PREFIX)) == HOST
    assert classify(Pred(b"/**/a/**", PREFIX)) == HOST and classify(Pred(b"/**/a**", PREFIX)) == ANT
    assert [classify(p) for p in (Pred(None), Pred(b""), Pred(b" \t\x1f", PREFIX), Pred(b"/a", is_path=False))] == [SKIP] * 4


def test_is_valid_api():
    """GatewayApiDefinitionManagerTest.testIsValidApi."""
    assert not is_valid_api(Api(0, None, name_blank=True))      # new ApiDefinition()
    assert not is_valid_api(Api(0, None))                       # new ApiDefinition("foo")
    assert is_valid_api(Api(0, [Pred(b"/abc")]))


def test_pick_matching_api_definitions():
    """SentinelGatewayFilterTest.testPickMatchingApiDefinitions: some_customized_api = 0, another_customized_api = 1."""
    d = Definitions([Api(0, [Pred(b"/product/**", PREFIX)]),
                     Api(1, [Pred(b"/something"), Pred(b"/other/**", PREFIX)])])
    assert d.match(b"/product/123") == [0]
    assert d.match(b"/products") == []
    assert d.match(b"/something") == [1]
    assert d.match(b"/other/foo/3") == [1]


def test_winner_order_verdicts_and_dropped_definitions():
    apis = [Api(2, [Pred(b"/old")]), Api(5, [Pred(b"/x")], name_blank=True),
            Api(7, [Pred(b"/*/b", PREFIX), Pred(b"/a/{id}", PREFIX)]),
            Api(2, [Pred(b"/a/b"), Pred(b"/a/b"), Pred(b"/a/.*", REGEX)]), Api(9, []),
            Api(4, [Pred(b"/a/b"), Pred(b"/abc", PREFIX), Pred(b"a/**", PREFIX), Pred(b"/(", REGEX, regex_invalid=True)])]
    d = Definitions(apis)
    assert d.winners == [2, 3, 4, 5] and d.vid_pred == [3, 6]
    assert d.match(b"/old") == [] and d.match(b"/x") == []
    assert d.match(b"/a/b") == [7, 2, 4]                        # entry order: the definitions' caller order
    assert d.match(b"/q", (0,)) == [7] and d.match(b"/q", (1,)) == [2] and d.match(b"/q", (0, 1)) == [7, 2]
    assert d.match(b"a/z") == [4] and d.match(b"/a/z") == [] and d.match(b"/abc") == []


def test_expansion_order_fields_and_verdict_ids():
    H, U, C_ = abi.GW_PARSE_HEADER, abi.GW_PARSE_URL_PARAM, abi.GW_PARSE_COOKIE
    rules = [Rule(1, 1, count=5, item=Item(H, "X-A", b"^v", abi.GW_MATCH_REGEX)),
             Rule(0, 0, count=5, item=Item(abi.GW_PARSE_CLIENT_IP)),
             Rule(1, 1, count=5, item=Item(U, "u")), Rule(1, 1, count=-1, item=Item(C_, "c", b"x", abi.GW_MATCH_REGEX)),
             Rule(0, 0, count=5, item=Item(9, "z", b"p", abi.GW_MATCH_REGEX)), Rule(0, 0, count=3)]
    apis = [Api(1, [Pred(b"/a/**", PREFIX), Pred(b"/r.*", REGEX)])]
    gw = Gateway(apis, rules, field_ids=[10, 0, 11, 12, 13, 0], default_context=6)
    assert gw.verdict_ids() == [(0, 1), (1, 0), (1, 4)]         # the dropped rule 3 has no id
    q = HttpReq(1000, 0, origin=3, context=2, path=b"/a/x", verdicts=(1,),
                fields=[(H, 11, b"no"), (U, 11, b"first"), (H, 10, b"v1"), (U, 11, b"second"), (0, 0, b"10.0.0.1")])
    assert gw.expand([q]) == [(0, 0, 0, 3, 2, 1000, [(b"10.0.0.1", False), (None, False)]),
                              (0, 1, 1, 0, 6, 1000, [(b"v1", True), (b"first", False)])]
    q2 = HttpReq(1001, None, path=b"/rx", verdicts=(0, 2))
    assert gw.expand([q2]) == [(0, 1, 1, 0, 6, 1001, [(None, False), (None, False)])]
    assert gw.expand([HttpReq(5, None, path=b"/zzz")]) == []
    never_set = Gateway(apis, rules)                            # no sg_gateway_set_item_fields: every item is null
    assert never_set.expand([q])[0][6] == [(None, False), (None, False)]
