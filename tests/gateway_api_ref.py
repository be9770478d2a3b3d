"""Pure-Python restatement of the gateway's API definitions and of the entries the gateway filter makes of a request
(sentinel-api-gateway-adapter-common api/GatewayApiDefinitionManager.java isValidApi :148-151; sentinel-spring-cloud
-gateway-adapter api/GatewayApiMatcherManager.java, api/matcher/WebExchangeApiMatcher.java :42-69,
route/AntRoutePathMatcher.java :36-50, SentinelGatewayFilter.java filter :72-100), over the inputs the C ABI takes:
API names and routes are resource indices, patterns and paths are bytes, predicates the device does not decide take the
caller's verdict ids. The Ant matcher follows the contract in include/sentinel_gpu.h (Spring 5.3.18
AntPathMatcher.doMatch, patterns with at most one `**` segment), on token lists and with a table-filling glob.

Written from the Java and the contract, not from the HIP: the device tests compare against this file.
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from gateway_ref import Manager
from sentinel_amd import abi

SKIP, EXACT, ANT, NEVER, HOST = range(5)
WHITESPACE = set(range(9, 14)) | set(range(28, 33))     # Character.isWhitespace over ASCII


@dataclass
class Pred:             # ApiPathPredicateItem (defaults as in the Java class), or another ApiPredicateItem
    pattern: Optional[bytes] = None
    strategy: int = abi.GW_URL_MATCH_EXACT
    is_path: bool = True
    regex_invalid: bool = False     # Pattern.compile throws


@dataclass
class Api:              # ApiDefinition; the name is the caller's resource index
    resource: int = 0
    preds: Optional[list] = None    # None: getPredicateItems() == null
    name_blank: bool = False


@dataclass
class HttpReq:
    ts_ms: int = 0
    route: Optional[int] = None     # None: no GATEWAY_ROUTE_ATTR
    origin: int = 0
    context: int = 0
    path: bytes = b"/"
    fields: list = field(default_factory=list)      # [(kind, name_id, bytes)] in the request's order
    verdicts: tuple = ()                            # the verdict ids that are true, ascending


def is_valid_api(api):
    return api is not None and not api.name_blank and api.preds is not None


def is_blank(pattern):
    return pattern is None or all(c in WHITESPACE for c in pattern)


def tokens(s):
    return [t for t in s.split(b"/") if t]


def classify(pred):
    if not pred.is_path or is_blank(pred.pattern):
        return SKIP
    if pred.strategy == abi.GW_URL_MATCH_REGEX:
        return NEVER if pred.regex_invalid else HOST
    if pred.strategy != abi.GW_URL_MATCH_PREFIX:
        return EXACT
    p = pred.pattern
    if b"{" in p or b"}" in p:
        return HOST
    if b"*" not in p and b"?" not in p:
        return NEVER
    return HOST if tokens(p).count(b"**") >= 2 else ANT


def units(seg):
    """A segment as code points: the sequence length from the lead byte, cut at the end; any other byte is one."""
    out, i = [], 0
    while i < len(seg):
        c = seg[i]
        n = 1 if c < 0x80 else 2 if c >> 5 == 6 else 3 if c >> 4 == 14 else 4 if c >> 3 == 30 else 1
        out.append(seg[i:i + n])
        i += n
    return out


def seg_match(pat, seg):
    """Whole-segment glob: `?` one code point, `*` any run, everything else literal bytes."""
    if b"*" not in pat and b"?" not in pat:
        return pat == seg
    # literal runs of the pattern are compared as bytes against runs of whole code points
    s = units(seg)
    pieces, lit = [], b""
    for c in pat:
        if c in b"*?":
            if lit:
                pieces.append(lit)
                lit = b""
            pieces.append(bytes([c]))
        else:
            lit += bytes([c])
    if lit:
        pieces.append(lit)
    reach = {0}                         # positions in s reachable after the pieces so far
    for piece in pieces:
        nxt = set()
        if piece == b"*":
            lo = min(reach) if reach else None
            nxt = set(range(lo, len(s) + 1)) if lo is not None else set()
        elif piece == b"?":
            nxt = {i + 1 for i in reach if i < len(s)}
        else:
            for i in reach:
                j, got = i, b""
                while j < len(s) and len(got) < len(piece):
                    got += s[j]
                    j += 1
                if got == piece:
                    nxt.add(j)
        reach = nxt
        if not reach:
            return False
    return len(s) in reach


def ant_match(pattern, path):
    """Points 1-5 of the contract, for a pattern with at most one `**` segment."""
    assert tokens(pattern).count(b"**") <= 1
    if pattern.startswith(b"/") != path.startswith(b"/"):
        return False
    pt, st = tokens(pattern), tokens(path)
    p_slash, s_slash = pattern.endswith(b"/"), path.endswith(b"/")
    head = pt.index(b"**") if b"**" in pt else len(pt)
    k = 0
    while k < head and k < len(st):
        if not seg_match(pt[k], st[k]):
            return False
        k += 1
    if k == len(st):                                    # the path is exhausted
        if k == len(pt):
            return p_slash == s_slash
        rest = pt[k:]
        return (rest == [b"*"] and s_slash) or all(t == b"**" for t in rest)
    if k == len(pt):                                    # the pattern is exhausted first
        return False
    tail, open_path = pt[head + 1:], st[k:]             # pt[k] is the `**`
    for j in range(1, len(tail) + 1):
        if j > len(open_path):
            return False                                # the path ran out: more than `**` is left
        if not seg_match(tail[-j], open_path[-j]):
            return False
        if j == 1 and p_slash != s_slash:
            return False
    return True


class Definitions:
    """GatewayApiDefinitionManager + GatewayApiMatcherManager after loadApiDefinitions(apis). The predicates are
    numbered as apis_to_abi flattens them: definition by definition in caller order."""

    def __init__(self, apis):
        self.apis = list(apis)
        self.flat = []                  # [(definition index, Pred)] = the ABI's preds[]
        self.pred_begin = []
        for i, api in enumerate(self.apis):
            self.pred_begin.append(len(self.flat))
            self.flat += [(i, p) for p in (api.preds or [])]
        self.cls = [classify(p) for _, p in self.flat]
        self.vid_pred = [k for k, c in enumerate(self.cls) if c == HOST]    # verdict id → predicate index
        self.vid_of = {k: v for v, k in enumerate(self.vid_pred)}
        last = {}
        for i, api in enumerate(self.apis):
            if is_valid_api(api):
                last[api.resource] = i  # the last in caller order is the definition
        self.winners = sorted(last.values())
        self._memo = {}                 # explain's answers: paths repeat

    def explain(self, path, verdicts=()):
        """[(definition index, the classes of its predicates that matched)] ascending, matching definitions only."""
        key = (path, tuple(v for v in verdicts if v < len(self.vid_pred)))
        if key not in self._memo:
            self._memo[key] = self._explain(path, key[1])
        return self._memo[key]

    def _explain(self, path, verdicts):
        out = []
        for i in self.winners:
            how = set()
            for k, pred in enumerate(self.apis[i].preds):
                pi = self.pred_begin[i] + k
                c = self.cls[pi]
                if c == EXACT and pred.pattern == path:
                    how.add("exact")
                elif c == ANT and ant_match(pred.pattern, path):
                    first = tokens(pred.pattern)[0]
                    how.add("wild" if b"*" in first or b"?" in first else "bucket")
                elif c == HOST and self.vid_of[pi] in verdicts:
                    how.add("host")
            if how:
                out.append((i, how))
        return out

    def match(self, path, verdicts=()):
        """pickMatchingApiDefinitions: the matching API resources, by ascending caller index of the definition."""
        return [self.apis[i].resource for i, _ in self.explain(path, verdicts)]


class Gateway:
    """Both loads and sg_gateway_set_item_fields: what sg_gateway_verdict_ids and sg_gateway_expand_batch answer."""

    def __init__(self, apis, rules, field_ids=None, default_context=0):
        self.defs, self.mgr = Definitions(apis), Manager(rules)
        self.field_ids, self.default_context = field_ids, default_context
        self.items = {}                 # resource → [(caller rule index, Item)] by item index
        regex = []
        for res, lst in self.mgr.by_resource.items():
            mine = sorted(((r.item.index, i, r.item) for i, r in lst if r.item is not None), key=lambda t: t[0])
            assert [m[0] for m in mine] == list(range(len(mine)))
            self.items[res] = [(i, item) for _, i, item in mine]
            regex += [i for i, item in self.items[res] if item.match_strategy == abi.GW_MATCH_REGEX]
        n_api = len(self.defs.vid_pred)
        self.rule_vid = {i: n_api + k for k, i in enumerate(sorted(regex))}

    def verdict_ids(self):
        return [(0, k) for k in self.defs.vid_pred] + [(1, i) for i in sorted(self.rule_vid)]

    def _items(self, resource, q):
        out = []
        for i, item in self.items.get(resource, []):
            raw = None
            if self.field_ids is not None and 0 <= item.parse_strategy <= abi.GW_PARSE_COOKIE:
                for kind, name_id, value in q.fields:
                    if kind == item.parse_strategy and (kind < abi.GW_PARSE_HEADER or name_id == self.field_ids[i]):
                        raw = value
                        break
            out.append((raw, self.rule_vid.get(i) in q.verdicts if i in self.rule_vid else False))
        return out

    def expand(self, requests):
        """[(source request, resource, resource mode, origin, context, ts_ms, [(bytes or None, verdict)])]: the route
        entry first, then the matching APIs."""
        out = []
        for k, q in enumerate(requests):
            if q.route is not None:
                out.append((k, q.route, 0, q.origin, q.context, q.ts_ms, self._items(q.route, q)))
            for res in self.defs.match(q.path, q.verdicts):
                out.append((k, res, 1, 0, self.default_context, q.ts_ms, self._items(res, q)))
        return out


# ---- the ABI's arrays

def apis_to_abi(apis):
    """[Api] → (abi.GATEWAY_API_DTYPE, abi.GATEWAY_API_PRED_DTYPE, the pattern blob); predicates flattened in order."""
    a = np.zeros(len(apis), abi.GATEWAY_API_DTYPE)
    preds, blob = [], bytearray()
    for k, api in enumerate(apis):
        flags = (abi.GW_API_NAME_BLANK if api.name_blank else 0) | (abi.GW_API_PREDS_NULL if api.preds is None else 0)
        a[k] = (api.resource, len(preds), len(api.preds or []), flags)
        for p in api.preds or []:
            flags = ((abi.GW_PRED_PATTERN_NULL if p.pattern is None else 0) | (0 if p.is_path else abi.GW_PRED_NOT_PATH)
                     | (abi.GW_PRED_REGEX_INVALID if p.regex_invalid else 0))
            preds.append((p.strategy, flags, len(blob), len(p.pattern or b"")))
            blob += p.pattern or b""
    preds = np.array(preds, abi.GATEWAY_API_PRED_DTYPE) if preds else np.zeros(0, abi.GATEWAY_API_PRED_DTYPE)
    return a, preds, bytes(blob)


def pack_http(requests, gap=b"", align=1, lead=b""):
    """[HttpReq] → (abi.GATEWAY_HTTP_REQ_DTYPE, abi.GATEWAY_FIELD_DTYPE, u32 verdicts, bytes): `lead`, then the paths
    back to back in request order (each start rounded up to `align`, `gap` in front of every path), then the fields'
    bytes."""
    req = np.zeros(len(requests), abi.GATEWAY_HTTP_REQ_DTYPE)
    data, fields, verdicts = bytearray(lead), [], []
    for k, q in enumerate(requests):
        data += gap
        while len(data) % align:
            data += b"\xEE"
        r = req[k]
        r["ts_ms"], r["route"] = q.ts_ms, abi.GW_NO_ROUTE if q.route is None else q.route
        r["origin"], r["context"], r["path_off"], r["path_len"] = q.origin, q.context, len(data), len(q.path)
        data += q.path
    for k, q in enumerate(requests):
        r = req[k]
        r["field_begin"], r["field_count"] = len(fields), len(q.fields)
        for kind, name_id, value in q.fields:
            fields.append((kind, name_id, len(data), len(value)))
            data += value
        r["verdict_begin"], r["verdict_count"] = len(verdicts), len(q.verdicts)
        verdicts += list(q.verdicts)
    fields = np.array(fields, abi.GATEWAY_FIELD_DTYPE) if fields else np.zeros(0, abi.GATEWAY_FIELD_DTYPE)
    return req, fields, np.array(verdicts, np.uint32), bytes(data)


def entries_to_abi(entries):
    """Expected (req, src, ev, ext context) arrays of Gateway.expand's entries."""
    n = len(entries)
    req, src = np.zeros(n, abi.GATEWAY_REQ_DTYPE), np.zeros(n, np.uint32)
    ev, ctx = np.zeros(n, abi.LOCAL_EVENT_DTYPE), np.zeros(n, np.uint32)
    at = 0
    for k, (s, res, mode, origin, context, ts, items) in enumerate(entries):
        req[k] = (res, mode, at, len(items))
        at += len(items)
        src[k], ctx[k] = s, context
        ev[k]["ts_ms"], ev[k]["resource"], ev[k]["count"] = ts, res, 1
        ev[k]["kind"], ev[k]["origin"] = abi.LOCAL_ENTRY, origin
    return req, src, ev, ctx


# ---- generators

SEGMENTS = [b"a", b"b", b"c", b"api", b"v1", b"x.html", b"\xc3\xa9"]


def random_path(rng, max_depth=4):
    depth = int(rng.integers(0, max_depth + 1))
    path = b"/" + b"/".join(SEGMENTS[int(rng.integers(len(SEGMENTS)))] for _ in range(depth))
    if depth and rng.random() < 0.15:
        path += b"/"
    if depth and rng.random() < 0.05:
        path = path.replace(b"/", b"//", 1)
    return path


def pick(rng, options):
    return options[int(rng.integers(len(options)))]


def random_pred(rng):
    """Mostly exact paths and Ant patterns the device decides; a few of every other class. Host-verdict predicates stay
    well under a tenth (0.04 by construction)."""
    seg = lambda: SEGMENTS[int(rng.integers(len(SEGMENTS)))]
    u = rng.random()
    if u < 0.30:
        return Pred(random_path(rng), int(rng.choice([0, 0, 0, 5, -1])))
    if u < 0.60:
        return Pred(b"/" + seg() + pick(rng, [b"/**", b"/*", b"/**/" + seg(), b"/*/" + seg(), b"/" + seg() + b"/**"]),
                    abi.GW_URL_MATCH_PREFIX)
    if u < 0.72:
        return Pred(pick(rng, [b"/*/" + seg(), b"/**/" + seg(), b"/?", b"/a*/**", b"/*", b"/**/*.html", b"*"]),
                    abi.GW_URL_MATCH_PREFIX)
    if u < 0.76:
        return pick(rng, [Pred(b"/a/.*", abi.GW_URL_MATCH_REGEX), Pred(b"/" + seg() + b"/{id}", abi.GW_URL_MATCH_PREFIX),
                           Pred(b"/**/" + seg() + b"/**", abi.GW_URL_MATCH_PREFIX)])
    if u < 0.89:
        return pick(rng, [Pred(random_path(rng), abi.GW_URL_MATCH_PREFIX),          # no wildcard: never
                           Pred(b"/a/(", abi.GW_URL_MATCH_REGEX, regex_invalid=True)])
    return pick(rng, [Pred(None), Pred(b""), Pred(b" \t"), Pred(b"/a", is_path=False),
                       Pred(None, abi.GW_URL_MATCH_PREFIX)])


def random_apis(rng, n_apis, n_resources):
    apis = []
    for _ in range(n_apis):
        u = rng.random()
        res = int(rng.integers(n_resources))
        if u < 0.05:
            apis.append(Api(res, [random_pred(rng)], name_blank=True))
        elif u < 0.10:
            apis.append(Api(res, None))
        elif u < 0.17:
            apis.append(Api(res, []))
        else:
            apis.append(Api(res, [random_pred(rng) for _ in range(int(rng.integers(1, 5)))]))
    return apis
