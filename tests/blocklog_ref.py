"""A small Python model of LogSlot and its StatLogger for the tests, written from the Java sources:

  LogSlot.entry                     core/slots/logger/LogSlot.java:35-47 — every BlockException of the slots behind it:
                                    statLogger.stat(resource, e.getClass().getSimpleName(), e.getRuleLimitApp(),
                                    context.getOrigin()).count(count)
  EagleEyeLogUtil / StatLogger      one COUNT_SUM entry per (time slot, key); time slot = t - t % 1000
  ruleLimitApp by exception class   FlowRuleChecker.java:53, DegradeSlot.java:55, AuthoritySlot.java:64,
                                    SystemRuleManager.java:307-330 (SystemBlockException(resource, limitType) passes
                                    limitType on as BlockException.ruleLimitApp), ParamFlowSlot.java:81-91
  FlowRuleChecker.checkFlow         for QPS DefaultController DIRECT rules with limitApp default / other / an origin
                                    (selectNodeByRequesterAndStrategy :115-145, FlowRuleManager.isOtherOrigin,
                                    DefaultController.canPass :49-76), over ClusterNode and origin-node second windows

The oracle reports pass / block but not which flow rule failed: MixedFlow restates checkFlow and adds that output; every
test that uses it first asserts that its statuses equal the oracle's on every event.
"""
import functools

import numpy as np

from sentinel_amd import abi
from tests.system_ref import PASS, Leap

T0 = 1_700_000_000_000  # a whole second
FLOW, DEGRADE, PARAM, AUTHORITY, SYSTEM = (abi.LOCAL_BLOCK_FLOW, abi.LOCAL_BLOCK_DEGRADE, abi.LOCAL_BLOCK_PARAM,
                                           abi.LOCAL_BLOCK_AUTHORITY, abi.LOCAL_BLOCK_SYSTEM)
BLOCKS = (FLOW, DEGRADE, PARAM, AUTHORITY, SYSTEM)
DEFAULT, OTHER = abi.LIMIT_APP_DEFAULT, abi.LIMIT_APP_OTHER


def u64_app(limit_app):
    """sg_block_row.app of an int32 limit_app (the low word)."""
    return limit_app & 0xFFFFFFFF


# ---------------------------------------------------------------- ruleLimitApp

def rule_limit_app(status, wait_ms=0, origin=0, flow_app=DEFAULT, param_idx=None, args=None):
    """(app_kind, app) of the BlockException of an entry. flow_app: limitApp of the FlowRule that failed; param_idx:
    the ParamFlowRule's index after applyRealParamIdx; args: the call's arguments as None (a null argument), an int
    (a scalar's value id) or ("coll", label id)."""
    if status == FLOW:
        return abi.BLOCK_APP_LIMIT_APP, u64_app(flow_app)
    if status == DEGRADE:
        return abi.BLOCK_APP_LIMIT_APP, u64_app(DEFAULT)  # sg_degrade_rule has no limitApp: AbstractRule's default
    if status == AUTHORITY:
        return abi.BLOCK_APP_ORIGIN, origin
    if status == SYSTEM:
        return abi.BLOCK_APP_SYSTEM, wait_ms  # super(limitType): BlockException(String ruleLimitApp)
    assert status == PARAM
    if args is None or param_idx is None or param_idx < 0 or len(args) <= param_idx:
        return abi.BLOCK_APP_NO_ARG, 0        # triggeredParam stays ""
    a = args[param_idx]
    if a is None:
        return abi.BLOCK_APP_NULL_ARG, 0      # String.valueOf((Object) null)
    if isinstance(a, tuple):
        return abi.BLOCK_APP_LABEL, a[1]
    return abi.BLOCK_APP_VALUE, a


# ---------------------------------------------------------------- StatLogger

class BlockLog:
    """StatLogger "sentinel-block-log": StatRollingData per time slot, COUNT_SUM per key."""

    def __init__(self):
        self.slots = {}

    def stat(self, t, res, status, kind, app, origin, count):
        slot = self.slots.setdefault(t - t % 1000, {})
        key = (res, status, kind, app, origin)
        slot[key] = slot.get(key, 0) + count

    def roll(self, now):
        """The rolling task at `now`: the complete seconds' entries as sg_block_row, in the device's row order."""
        limit = now - now % 1000
        out = []
        for ts in sorted(self.slots):
            if ts + 1000 <= limit:
                for (res, status, kind, app, origin), c in sorted(self.slots.pop(ts).items()):
                    out.append((ts, c, app, res, origin, status, kind))
        return np.array(out, abi.BLOCK_ROW_DTYPE)

    def pending(self):
        return sum(len(s) for s in self.slots.values())


def decode_args(x, args, values):
    """One event's arguments (sg_slot_ext + sg_pslot_arg + values) in rule_limit_app's form, None for Object[] null."""
    if x is None or x["args_null"]:
        return None
    out = []
    for a in args[int(x["arg_begin"]): int(x["arg_begin"]) + int(x["arg_count"])]:
        if a["kind"] == abi.ARG_NULL:
            out.append(None)
        elif a["kind"] == abi.ARG_VALUE:
            out.append(int(values[int(a["value_begin"])]))
        else:
            out.append(("coll", int(a["reserved"])))
    return out


def log_batch(log, ev, res, flow_app=None, ext=None, args=None, values=None, param_idx=None):
    """LogSlot over a decided batch: ev / res the events and their results; flow_app(i) the failing flow rule's
    limitApp of FLOW-blocked event i; param_idx[rule] each param rule's index after applyRealParamIdx."""
    for i in range(len(ev)):
        st = int(res["status"][i])
        if ev["kind"][i] != abi.LOCAL_ENTRY or st not in BLOCKS:
            continue
        wait = int(res["wait_ms"][i])
        origin = int(ev["origin"][i])
        kind, app = rule_limit_app(st, wait, origin, flow_app(i) if st == FLOW and flow_app else DEFAULT,
                                   param_idx[wait] if st == PARAM else None,
                                   decode_args(ext[i] if ext is not None else None, args, values) if st == PARAM else None)
        log.stat(int(ev["ts_ms"][i]), int(ev["resource"][i]) & 0x7FFFFFFF, st, kind, app, origin, int(ev["count"][i]))


# ---------------------------------------------------------------- FlowRuleChecker.checkFlow, with the failing rule

class MixedFlow:
    """checkFlow for QPS / DefaultController / DIRECT rules (no cluster mode, no prioritized entries, no exits), rules
    as (resource, count, limit_app) in load order. entry() → (status, limitApp of the failing rule or None)."""

    def __init__(self, rules, sample_count=2, interval_ms=1000):
        self.S, self.interval = sample_count, interval_ms
        self.rules = {}
        for res, count, app in rules:
            self.rules.setdefault(res, []).append((count, app))
        for v in self.rules.values():  # FlowRuleComparator: stable, limitApp "default" last
            v.sort(key=lambda r: r[1] == DEFAULT)
        self.nodes = {}

    def node(self, res, origin=None):
        if (res, origin) not in self.nodes:
            self.nodes[(res, origin)] = Leap(self.S, self.interval)
        return self.nodes[(res, origin)]

    def uniform(self, res):
        apps = {a for _, a in self.rules.get(res, [])}
        return apps.pop() if len(apps) == 1 else (DEFAULT if not apps else None)

    def entry(self, t, res, origin, count):
        cluster = self.node(res)                                   # ClusterBuilderSlot
        onode = self.node(res, origin) if origin > 0 else None     # getOrCreateOriginNode for a non-empty origin
        named = {a for _, a in self.rules.get(res, [])}
        failed = None
        for limit, app in self.rules.get(res, []):
            if app == origin and origin > 0:
                sel = onode
            elif app == DEFAULT:
                sel = cluster
            elif app == OTHER and origin > 0 and origin not in named:  # isOtherOrigin
                sel = onode
            else:
                continue
            cur = int(sel.total(t, PASS) / (self.interval / 1000.0))   # (int) node.passQps()
            if cur + count > limit:
                failed = app
                break
        for n in (cluster, onode):
            if n is not None:
                n.c[n.current(t)][1 if failed is not None else PASS] += count
        return (FLOW if failed is not None else abi.LOCAL_PASS), failed


# ---------------------------------------------------------------- event builders

def entries(ts, res, count=1, origin=0):
    ts = np.asarray(ts, np.int64)
    ev = np.zeros(len(ts), abi.LOCAL_EVENT_DTYPE)
    ev["ts_ms"], ev["resource"], ev["count"], ev["origin"] = ts, res, count, origin
    ev["kind"] = abi.LOCAL_ENTRY
    return ev


class Args:
    """The ext / args / values arrays of a sequence of calls; an argument is None, an int or ("coll", label, [ids])."""

    def __init__(self):
        self.ext, self.args, self.values = [], [], []

    def call(self, *arguments, args_null=False, context=0):
        self.ext.append((context, len(self.args), 0 if args_null else len(arguments), 1 if args_null else 0))
        if args_null:
            return self
        for a in arguments:
            if a is None:
                self.args.append((0, 0, abi.ARG_NULL, 0))
            elif isinstance(a, tuple):
                self.args.append((len(self.values), len(a[2]), abi.ARG_COLLECTION, a[1]))
                self.values += list(a[2])
            else:
                self.args.append((len(self.values), 1, abi.ARG_VALUE, 0))
                self.values.append(a)
        return self

    def arrays(self):
        return (np.array(self.ext, abi.SLOT_EXT_DTYPE), np.array(self.args or [(0, 0, 0, 0)], abi.PSLOT_ARG_DTYPE),
                np.array(self.values or [0], np.uint64))


# ---------------------------------------------------------------- the traces the CPU and GPU tests share

MIXED_RULES = [(0, 8.0, DEFAULT), (0, 2.0, OTHER), (0, 3.0, 1),      # resource 0: origin 1, other, default
               (1, 4.0, DEFAULT), (1, 9.0, DEFAULT),                 # resource 1: two "default" rules — uniform, cx
               (2, 1.0, OTHER), (2, 5.0, DEFAULT)]                   # resource 2: other + default, no origin rule
MIXED_N_RES, MIXED_N_ORIGINS = 4, 3


def mixed_flow_rules():
    from oracle.binding import local_flow_rule
    return np.array([local_flow_rule(r, c, limit_app=a) for r, c, a in MIXED_RULES], abi.LOCAL_FLOW_RULE_DTYPE)


@functools.lru_cache(maxsize=None)
def mixed_case():
    """One saturated second on a resource whose rules {origin 1, other, default} each fail first for some entry, a
    uniform cx resource beside it, and a second batch that ends the second and starts the next. → (batches, model
    statuses + failing limitApps per batch)."""
    rng = np.random.default_rng(7)
    batches = []
    t = T0
    for n, span in ((300, 700), (300, 700)):
        ts = t + np.sort(rng.integers(0, span, n))
        ev = entries(ts, rng.integers(0, 3, n), np.where(rng.random(n) < 0.2, 2, 1), rng.integers(0, 4, n))
        ev.setflags(write=False)
        batches.append(ev)
        t += span
    model = MixedFlow(MIXED_RULES)
    decided = []
    for ev in batches:
        st, app = [], []
        for e in ev:
            s, a = model.entry(int(e["ts_ms"]), int(e["resource"]), int(e["origin"]), int(e["count"]))
            st.append(s)
            app.append(DEFAULT if a is None else a)
        decided.append((np.array(st, np.int32), np.array(app, np.int64)))
    return batches, decided, model


def mixed_rows(now):
    batches, decided, _ = mixed_case()
    log = BlockLog()
    for ev, (st, app) in zip(batches, decided):
        res = np.zeros(len(ev), abi.LOCAL_RES_DTYPE)
        res["status"] = st
        log_batch(log, ev, res, flow_app=lambda i: int(app[i]))
    return log.roll(now), log


@functools.lru_cache(maxsize=None)
def random_case():
    """A few thousand entries, 64 resources with Zipf weights, 4 origins, rule sets inside MixedFlow's scope (every
    third resource mixed), three seconds in two batches."""
    rng = np.random.default_rng(20261020)
    K = 64
    rules = []
    for r in range(K):
        if r % 3 == 0:
            rules += [(r, float(rng.integers(2, 9)), DEFAULT), (r, float(rng.integers(1, 4)), int(rng.integers(1, 5))),
                      (r, float(rng.integers(1, 3)), OTHER)]
        elif r % 3 == 1:
            rules += [(r, float(rng.integers(1, 6)), DEFAULT)]
        else:
            rules += [(r, float(rng.integers(1, 4)), OTHER)]
    w = 1.0 / np.arange(1, K + 1)
    w /= w.sum()
    batches, t = [], T0 + 250
    for n, span in ((2500, 1500), (2500, 1500)):
        ts = t + np.sort(rng.integers(0, span, n))
        ev = entries(ts, rng.choice(K, n, p=w), np.where(rng.random(n) < 0.1, 3, 1), rng.integers(0, 5, n))
        ev.setflags(write=False)
        batches.append(ev)
        t += span
    model = MixedFlow(rules)
    decided = []
    for ev in batches:
        st, app = [], []
        for e in ev:
            s, a = model.entry(int(e["ts_ms"]), int(e["resource"]), int(e["origin"]), int(e["count"]))
            st.append(s)
            app.append(DEFAULT if a is None else a)
        decided.append((np.array(st, np.int32), np.array(app, np.int64)))
    return K, rules, batches, decided


SYS_INBOUND = [1, 0]
# (system rules as tests/system_ref.py SystemConf takes them, (load, cpu) status, entries [(dt, res)], exits after)
SYS_STEPS = [([(-1.0, -1.0, 3.0, -1, -1)], (-1.0, -1.0), [(i * 10, i % 2) for i in range(12)], False),   # qps 3
             ([(-1.0, -1.0, -1.0, -1, 1)], (-1.0, -1.0), [(i * 10, 0) for i in range(4)], True),         # maxThread 1
             ([(-1.0, -1.0, -1.0, 5, -1)], (-1.0, -1.0), [(i * 10, i % 2) for i in range(6)], False),     # avgRt 5
             ([(1.0, -1.0, -1.0, -1, -1)], (2.0, -1.0), [(i * 10, 0) for i in range(20)], False)]         # load 1 < 2


@functools.lru_cache(maxsize=None)
def system_case():
    """SystemSlot blocks of every limit type the device decides from ENTRY_NODE: one batch per rule set (a second
    each; the batch with exits returns every thread 40 ms after its entry) → [(rules, status, events, results)]."""
    from tests.system_ref import PlainChain, SystemConf
    chain = PlainChain(2, SYS_INBOUND)
    out, t, open_ = [], T0, []
    for rules, (load, cpu), ents, exits in SYS_STEPS:
        chain.conf, chain.load, chain.cpu = SystemConf(rules), load, cpu
        ev, res = [], []
        for dt, r in ents:
            st, wait = chain.entry_event(t + dt, r, 1, 0)
            ev.append((t + dt, 0, r, 1, abi.LOCAL_ENTRY, 0))
            res.append((st, wait))
            if st == abi.LOCAL_PASS:
                open_.append((t + dt, r))
        if exits:
            te = t + 500
            for create, r in open_:
                chain.exit_event(te, create, r, 1, 0, False)
                ev.append((te, create, r, 1, abi.LOCAL_EXIT, 0))
                res.append((0, 0))
            open_ = []
        e, w = np.array(ev, abi.LOCAL_EVENT_DTYPE), np.array(res, abi.LOCAL_RES_DTYPE)
        e.setflags(write=False)
        out.append((rules, (load, cpu), e, w))
        t += 1000
    return out


def wait_case():
    """A saturated second on a lane-walker resource (QPS 2) with prioritized entries among the late ones: the first of
    them occupies the next bucket (PriorityWaitException: passes after its wait, never reaches LogSlot), the plain
    ones are FlowExceptions. → (base rules, events)."""
    from oracle.binding import local_rule
    ev = entries(T0 + np.array([100, 110, 600, 610, 620, 630, 640, 650]), 0, 1)   # two passes, then the next bucket
    ev["resource"][[3, 5]] |= np.uint32(abi.KEY_PRIO)
    return [local_rule(2.0, abi.FLOW_GRADE_QPS)], ev


EMB_SERVER_COUNT, EMB_ORIGIN_COUNT = 3, 2


def embedded_case():
    """An embedded token server: resource 0 with a local rule for origin 1 (count 2) and a cluster-mode rule, limitApp
    "default", whose flowId the server limits to 3 a second — mixed limitApps, and FlowRuleComparator puts the cluster
    rule last. Everything inside one window bucket, so the model is plain counting: an origin-1 entry fails its own
    rule once two of them passed (no token is asked for), any other entry asks the server and is BLOCKED once three
    tokens are out. → (flow rules, events, model statuses, failing limitApps)."""
    from oracle.binding import local_flow_rule
    fr = np.array([local_flow_rule(0, 100.0, cluster_mode=abi.CLUSTER_MODE_FALLBACK, cluster_config=1, cluster_key=0),
                   local_flow_rule(0, float(EMB_ORIGIN_COUNT), limit_app=1)], abi.LOCAL_FLOW_RULE_DTYPE)
    origins = [1, 1, 1, 0, 0, 1, 0, 2, 1]
    ev = entries(T0 + 100 + np.arange(len(origins)) * 7, 0, 1, origins)
    tokens = o1 = 0
    st, app = [], []
    for o in origins:
        if o == 1 and o1 + 1 > EMB_ORIGIN_COUNT:
            st.append(FLOW)
            app.append(1)
        elif tokens + 1 > EMB_SERVER_COUNT:
            st.append(FLOW)
            app.append(DEFAULT)
        else:
            st.append(abi.LOCAL_PASS)
            app.append(DEFAULT)
            tokens += 1
            o1 += o == 1
    return fr, ev, np.array(st, np.int32), app
