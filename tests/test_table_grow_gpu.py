"""The exact value tables and the value dictionary grown in place (sg_param_resize, sg_cparam_resize, sg_vdict_grow,
their node forms and the *_table_used counts).

The oracles (ParamFlowChecker, ParamFlowSlot, ClusterTokenService, LocalChain) have no capacity: each replays the
accepted history and never sees a refused batch. A grown handle must decide every later batch, and answer every state
read, exactly as the oracle and as a handle that was large from the start. Sub-tables hold 2 to 64 slots and a batch at
most 20,000 requests; the value sets come from tests/value_tables.py (probe chains homed at the last slot under the
old mask and under the new one). Every reference is computed once per case, shared by the walker variants, and never
modified. The batch builders are those of tests/test_value_tables_gpu.py, the suite this one continues."""
import functools
import struct

import numpy as np
import pytest

from oracle.binding import ClusterTokenService, ParamFlowChecker, ParamFlowSlot, local_flow_rule, local_rule
from sentinel_amd import abi
from tests import test_value_tables_gpu as vt
from tests.value_tables import MARKER, home, homed_values, random_values

pytestmark = pytest.mark.gpu

WALKERS = vt.WALKERS
T0 = vt.T0
N = vt.N


def _used(eng, n_rules, cparam=False):
    return [(eng.cparam_table_used(r) if cparam else eng.param_table_used(r)) for r in range(n_rules)]


# ------------------------------------------------------------------------------------------------ sg_param_resize

P_LG = vt.P_LG  # (1, 4, 2): token bucket, token bucket with burst, throttle


@functools.lru_cache(maxsize=None)
def _param_refused_grown_case():
    """Rules of 2, 16 and 4 slots filled exactly over two batches (more than one duration each); then for every rule
    in turn a batch with one value too many, which the oracle accepts."""
    rng = np.random.default_rng(1101)
    rules = vt._param_rules()
    sets = [vt._value_set(rng, vt.P_KIND[r], P_LG[r], 1 << P_LG[r]) for r in range(3)]
    pairs = [(r, v) for r in range(3) for v in sets[r] + [MARKER]]
    half = [(r, v) for r in range(3) for v in sets[r][:max(1, len(sets[r]) // 2)] + [MARKER]]
    ora = ParamFlowChecker()
    ora.load_rules(rules)
    steps, t = [], T0 + 11
    steps.append(vt._param_step(ora, rng, half, half, t, 2300))
    t = int(steps[-1][0]["ts_ms"][-1]) + 400
    steps.append(vt._param_step(ora, rng, pairs, pairs, t, 2700))
    over = []
    for r in range(3):
        extra = vt._value_set(rng, vt.P_KIND[r], P_LG[r], 1, [v for rr, v in pairs if rr == r])[0]
        pairs = pairs + [(r, extra)]
        t = int((over[-1] if over else steps[-1])[0]["ts_ms"][-1]) + int(rng.integers(0, 700))
        over.append(vt._param_step(ora, rng, pairs, pairs, t, 1800))
    return rules, steps, over


@pytest.mark.parametrize("flags", WALKERS)
def test_param_refused_grown_accepted(flags):
    """Case 1: a full rule refuses one value too many (SG_E_CAPACITY, nothing changed); after sg_param_resize of that
    rule by one bit the same batch is accepted and equals the oracle, with every known pair's state. Without the
    feature the second send is refused again."""
    rules, steps, over = _param_refused_grown_case()
    eng = vt._engine(flags)
    eng.param_load_rules(rules)
    for b, step in enumerate(steps):
        vt._param_check(eng, step, f"batch {b}")
    assert [u[0] for u in _used(eng, 3)] == [1 << lg for lg in P_LG]
    lg = list(P_LG)
    for r, step in enumerate(over):
        before = _used(eng, 3)
        assert vt._code(eng.param_decide_host, step[0]) == abi.SG_E_CAPACITY, f"one more value for rule {r}"
        assert _used(eng, 3) == before
        grow = [0, 0, 0]
        grow[r] = lg[r] = lg[r] + 1
        eng.param_resize(grow)
        assert [u[2] for u in _used(eng, 3)] == [1 << x for x in lg]
        vt._param_check(eng, step, f"the batch rule {r} refused, after its growth")
    assert [u[:2] for u in _used(eng, 3)] == [((1 << P_LG[r]) + 1,) * 2 for r in range(3)]


@functools.lru_cache(maxsize=None)
def _param_two_masks_case():
    """Every rule: values all homed at the last slot of its old mask, the value 0 and the marker; after one bit of
    growth, new values all homed at the last slot of the new mask, up to exactly full again."""
    rng = np.random.default_rng(1102)
    rules = vt._param_rules()
    old, new = [], []
    for r in range(3):
        m0, m1 = (1 << P_LG[r]) - 1, (2 << P_LG[r]) - 1
        o = homed_values(rng, m0, m0, m0, (0,)) + [0]
        assert all(home(v, m0) == m0 for v in o[:-1]) and len(o) == m0 + 1
        n = homed_values(rng, m0 + 1, m1, m1, o)
        assert all(home(v, m1) == m1 for v in n)
        old.append(o)
        new.append(n)
    p_old = [(r, v) for r in range(3) for v in old[r] + [MARKER]]
    p_all = p_old + [(r, v) for r in range(3) for v in new[r]]
    ora = ParamFlowChecker()
    ora.load_rules(rules)
    a = vt._param_step(ora, rng, p_old, p_old, T0 + 21, 2400)
    b = vt._param_step(ora, rng, p_all, p_all, int(a[0]["ts_ms"][-1]) + 1, 2600)
    c = vt._param_step(ora, rng, p_all, p_all, int(b[0]["ts_ms"][-1]) + 900, 1500)
    return rules, a, b, c


@pytest.mark.parametrize("flags", WALKERS)
def test_param_chains_under_both_masks(flags):
    """Case 2: probe chains that wrap under the old mask are re-inserted under the new one, and chains that wrap
    under the new mask grow beside them; the used counts are what was inserted."""
    rules, a, b, c = _param_two_masks_case()
    eng = vt._engine(flags)
    eng.param_load_rules(rules)
    vt._param_check(eng, a, "before the growth")
    assert _used(eng, 3) == [(1 << lg, 1 << lg, 1 << lg) for lg in P_LG]
    eng.param_resize([lg + 1 for lg in P_LG])
    assert _used(eng, 3) == [(1 << lg, 1 << lg, 2 << lg) for lg in P_LG]
    vt._param_states(eng, a[2], "after the growth")
    vt._param_check(eng, b, "the batch that fills the grown tables")
    assert _used(eng, 3) == [(2 << lg, 2 << lg, 2 << lg) for lg in P_LG]
    vt._param_check(eng, c, "last batch")


# The twin trace: four rules, five batches. `grow` lists the resize calls before each batch (a call of zeros compacts).
TW_START = (1, 4, 2, 1)
TW_FINAL = (4, 6, 5, 1)
TW_GROW = [
    [[2, 0, 0, 0]],                     # before any batch
    [[3, 5, 0, 0]],                     # mid-duration, several rules at once with zeros mixed in
    [[0, 0, 3, 0], [4, 0, 4, 0]],       # twice in a row
    [[0, 6, 5, 0]],
    [[0, 0, 0, 0]],                     # no size changes
]
TW_VALUES = [(4, 16, 4, 2), (8, 32, 4, 2), (16, 32, 16, 2), (16, 64, 32, 2), (16, 64, 32, 2)]  # known after each batch


def _twin_rules(lg):
    r = np.zeros(4, abi.PARAM_RULE_DTYPE)
    r["count"] = [40, 25, 60, 30]
    r["duration_sec"] = [1, 1, 1, 2]
    r["burst"] = [0, 4, 0, 1]
    r["behavior"] = [abi.BEHAVIOR_DEFAULT, abi.BEHAVIOR_DEFAULT, abi.BEHAVIOR_RATE_LIMITER, abi.BEHAVIOR_DEFAULT]
    r["max_queueing_ms"] = [0, 0, 40, 0]
    r["capacity_log2"] = lg
    return r


def _twin_step(ora, rng, pairs, t, span):
    req = vt._param_batch(rng, pairs, N, t, span)
    want = ora.decide(req)
    assert set(want.tolist()) == {0, 1}
    states = {p: ora.state(*p) for p in pairs}
    vt._frozen(req, want)
    return req, want, states


@functools.lru_cache(maxsize=None)
def _twin_case():
    rng = np.random.default_rng(1103)
    ora = ParamFlowChecker()
    ora.load_rules(_twin_rules(TW_FINAL))
    sets = [[], [], [], []]
    steps, t = [], T0 + 31
    for b, counts in enumerate(TW_VALUES):
        for r in range(4):
            sets[r] += random_values(rng, counts[r] - len(sets[r]), sets[r] + [0])
        pairs = [(r, v) for r in range(4) for v in sets[r] + [MARKER]]
        steps.append(_twin_step(ora, rng, pairs, t, (2500, 900, 1400, 2100, 700)[b]))
        t = int(steps[-1][0]["ts_ms"][-1]) + (0, 1, 300, 0, 0)[b]  # batches 1 and 4 start inside batch 0's / 3's second
    return steps


def _twin_engines(flags):
    small, large = vt._engine(flags), vt._engine(flags)
    small.param_load_rules(_twin_rules(TW_START))
    large.param_load_rules(_twin_rules(TW_FINAL))
    return small, large


def _twin_batch(small, large, step, what):
    req, want, states = step
    got_s, got_l = small.param_decide_host(req), large.param_decide_host(req)
    vt._same(got_s, got_l, f"{what}: grown against large from the start")
    vt._same(got_s, want, what)
    for (r, v), st in states.items():
        s, l = small.param_state(r, v), large.param_state(r, v)
        assert s == l, f"{what}: state of rule {r} value {v:#x}: grown {s}, large from the start {l}"
    vt._param_states(small, states, what)


@pytest.mark.parametrize("flags", WALKERS)
def test_param_growth_is_invisible(flags):
    """Cases 3 and 4: one engine starts small and grows along the trace, its twin is large from the start: the same
    outputs, the same state of every (rule, value), both the oracle's. After every resize used == live."""
    steps = _twin_case()
    small, large = _twin_engines(flags)
    for b, step in enumerate(steps):
        for grow in TW_GROW[b]:
            small.param_resize(grow)
            assert all(u == l for u, l, _ in _used(small, 4)), f"before batch {b}: {_used(small, 4)}"
        _twin_batch(small, large, step, f"batch {b}")
    assert [c for _, _, c in _used(small, 4)] == [1 << lg for lg in TW_FINAL]
    assert _used(small, 4) == _used(large, 4)


def test_param_resize_refusals_change_nothing():
    """Case 9: every refusal returns its code with the tables as they were: the twin comparison goes on."""
    steps = _twin_case()
    fresh = vt._engine()
    assert vt._code(fresh.param_resize, [2]) == abi.SG_E_INVAL                  # before a load
    assert vt._code(fresh.param_resize, []) == abi.SG_E_INVAL
    small, large = _twin_engines(0)
    for grow in TW_GROW[0]:
        small.param_resize(grow)
    _twin_batch(small, large, steps[0], "batch 0")
    before = _used(small, 4)
    refusals = [
        ([1, 0, 0, 0], abi.SG_E_INVAL),          # a shrink (rule 0 holds 4 slots)
        ([0, 3, 0, 0], abi.SG_E_INVAL),          # a shrink among kept sizes
        ([31, 0, 0, 0], abi.SG_E_INVAL),         # out of range
        ([0, 0, -1, 0], abi.SG_E_INVAL),
        ([3, 5, 0], abi.SG_E_INVAL),             # a wrong n
        ([3, 5, 0, 0, 0], abi.SG_E_INVAL),
        ([30, 30, 30, 30], abi.SG_E_UNSUPPORTED),  # 2^32 slots or more
        ([31, 30, 30, 30], abi.SG_E_INVAL),      # the arguments are judged before the total
    ]
    for grow, code in refusals:
        assert vt._code(small.param_resize, grow) == code, grow
        assert _used(small, 4) == before, grow
    for b in range(1, len(steps)):
        for grow in TW_GROW[b]:
            small.param_resize(grow)
        _twin_batch(small, large, steps[b], f"batch {b}")
    # a total whose records would overflow for the handle's max_batch: 25 index bits + 8 + 32 slot bits
    wide = vt._engine(0, max_batch=(1 << 24) + 2)
    wide.param_load_rules(_twin_rules(TW_FINAL))
    req, want, states = steps[0]
    vt._same(wide.param_decide_host(req), want, "batch 0 on the wide handle")
    before = _used(wide, 4)
    assert vt._code(wide.param_resize, [30, 30, 30, 0]) == abi.SG_E_UNSUPPORTED
    assert _used(wide, 4) == before
    vt._param_states(wide, states, "after the refusal")
    vt._same(wide.param_decide_host(steps[1][0]), steps[1][1], "batch 1 on the wide handle")


# ------------------------------------------------------------------------------------------------ sg_cparam_resize

CP_S = (10, 4, 1)   # stride 10: rules 1 and 2 use fewer buckets than a slot carries
CP_LG = 2


def _cp_grow_rules(counts, flow_id0=7):
    r = vt._cp_rules(counts, flow_id0=flow_id0)
    r["sample_count"] = CP_S
    r["namespace_id"] = [0, 0, 1]   # rule 2's namespace has a limiter
    return r


def _cp_ns():
    ns = np.zeros(2, abi.NS_DTYPE)
    ns["connected_count"] = 1
    ns["limiter_enabled"][1], ns["max_allowed_qps"][1] = 1, 2500.0
    return ns


@functools.lru_cache(maxsize=None)
def _cp_grow_case():
    rng = np.random.default_rng(1201)
    rules = _cp_grow_rules(rng.integers(20, 200, 3))
    first = vt._cp_sets(rng, CP_LG)                                            # 4 values and the marker: exactly full
    more = vt._cp_sets(rng, CP_LG, 1 << CP_LG, first, marker=False)            # 4 more: full again at 8 slots
    both = [a + b for a, b in zip(first, more)]
    known = [(r, v) for r in range(3) for v in first[r]]
    bknown = [(r, v) for r in range(3) for v in both[r]]
    need = (abi.OK, abi.BLOCKED, abi.TOO_MANY_REQUEST)
    ora = ClusterTokenService()
    ora.set_namespaces(_cp_ns())
    ora.load_param_rules(rules)
    a = vt._cp_step(ora, rng, first, known, T0 + 41, 1700, 0.5, rules, need)
    # window sums at later times from a second oracle that sees batch a only: reading a sum at a time moves the
    # reference's windows there (currentWindow), so the oracle that goes on to batch b is read at its own time only
    later = ClusterTokenService()
    later.set_namespaces(_cp_ns())
    later.load_param_rules(rules)
    assert np.array_equal(later.decide_param(a[0], a[1]), a[2])
    sums_at = {dt: {p: later.param_sum(p[0], p[1], a[3] + dt) for p in known} for dt in (0, 250, 400, 500, 600, 999, 1500)}
    assert len({tuple(s.values()) for s in sums_at.values()}) >= 2  # buckets leave the window between the reads
    # mid-window: the next batch starts in the window period batch a ended in
    b = vt._cp_step(ora, rng, both, bknown, a[3], 1900, 0.5, rules, need)
    # the reload: rule 0 survives as rule 2, rule 2 as rule 0 (each keeps its window shape), rule 1's flowId is new
    new = np.concatenate([rules[2:3], _cp_grow_rules(rng.integers(20, 200, 3), flow_id0=2000)[1:2], rules[0:1]])
    new["namespace_id"] = [1, 0, 0]
    ora.load_param_rules(new)
    nsets = [both[2], both[1], both[0]]
    nknown = [(r, v) for r in range(3) for v in nsets[r]]
    now = b[3] + 1
    kept = {(nr, v): ora.param_sum(nr, v, now) for nr, r in ((0, 2), (2, 0)) for v in both[r]}
    assert sum(s > 0 for s in kept.values()) > 8
    c = vt._cp_step(ora, rng, nsets, nknown, now, 2200, 0.5, new, need)
    return rules, new, a, sums_at, b, now, kept, c


@pytest.mark.parametrize("flags", WALKERS)
def test_cparam_grown_mid_window_then_reloaded(flags):
    """Case 5: rules of 10, 4 and 1 buckets in slots of 10, multi-value requests (the fixed point runs more than one
    round) and a namespace limiter on one rule. Exactly full; one value too many is refused; grown mid-window the
    decisions, the window sums at several times and the top values equal the oracle's. A reload naming the old
    capacity is SG_E_UNSUPPORTED as before; one naming the new capacity keeps the surviving flowIds' state."""
    rules, new, a, sums_at, b, now, kept, c = _cp_grow_case()
    eng = vt._engine(flags)
    eng.set_namespaces(_cp_ns())
    eng.cparam_load_rules(rules, None, CP_LG)
    vt._cp_check(eng, a, "first batch", CP_LG)
    rounds = eng.cparam_last_rounds()
    assert _used(eng, 3, True) == [(4, 4, 4)] * 3
    assert vt._code(eng.cparam_decide_host, b[0], b[1]) == abi.SG_E_CAPACITY
    vt._cp_sums(eng, a, "after the refusal", CP_LG)
    assert _used(eng, 3, True) == [(4, 4, 4)] * 3
    eng.cparam_resize(CP_LG + 1)
    assert _used(eng, 3, True) == [(4, 4, 8)] * 3
    for dt, sums in sums_at.items():
        for (r, v), s in sums.items():
            assert eng.cparam_sum(r, v, a[3] + dt) == s, f"window sum of rule {r} value {v:#x} at +{dt} ms"
    vt._cp_sums(eng, a, "after the growth", CP_LG + 1)
    vt._cp_check(eng, b, "the refused batch, after the growth", CP_LG + 1)
    assert max(rounds, eng.cparam_last_rounds()) > 1
    assert _used(eng, 3, True) == [(8, 8, 8)] * 3
    assert vt._code(eng.cparam_load_rules, new, None, CP_LG) == abi.SG_E_UNSUPPORTED
    vt._cp_sums(eng, b, "after the refused reload", CP_LG + 1)
    eng.cparam_load_rules(new, None, CP_LG + 1)
    for (r, v), s in kept.items():
        assert eng.cparam_sum(r, v, now) == s, f"survivor's window sum of rule {r} value {v:#x}"
    vt._cp_check(eng, c, "after the reload", CP_LG + 1)


def test_cparam_resize_compacts_and_refuses():
    """Cases 4 and 9 for the cluster tables. k_cp_prep2 claims a slot for every value before the namespace limiter
    runs: a value whose every request the limiter turns away in an accepted batch holds a slot and no bucket —
    used > live. A same-size resize returns the slot, and the next new value is accepted where the same history
    without the compaction is refused. Refusals change nothing."""
    rng = np.random.default_rng(1202)
    lg, ns = 2, vt._ns(2000.0)
    rules = vt._cp_rules([30.0, 50.0, 40.0])
    sets = vt._cp_sets(rng, lg, (1 << lg) - 1)                   # 3 values and the marker: one slot free
    dead = random_values(rng, 1, sets[0])[0]
    late = random_values(rng, 1, sets[0] + [dead])[0]

    def oracle():
        o = ClusterTokenService()
        o.set_namespaces(ns)
        o.load_param_rules(rules)
        return o

    fresh = vt._engine()
    fresh.set_namespaces(ns)
    assert vt._code(fresh.cparam_resize, 4) == abi.SG_E_INVAL   # before a load
    req, vals = vt._cp_batch(rng, sets, 6000, T0 + 51, 1500, 0.0)
    # the limiter's verdicts do not depend on the values: requests it turns away get the dead value
    turned = oracle().decide_param(req, vals)["status"] == abi.TOO_MANY_REQUEST
    at = np.nonzero((req["key"] == 0) & turned)[0][:20]
    assert len(at) == 20
    vals[req["value_begin"][at]] = dead
    ora = oracle()
    want = ora.decide_param(req, vals)
    assert (want["status"][at] == abi.TOO_MANY_REQUEST).all() and {abi.OK, abi.BLOCKED} <= set(want["status"].tolist())
    first = [(4, 3, 4), (3, 3, 4), (3, 3, 4)]                    # rule 0: three live values and the dead claim
    eng, ctl = vt._engine(), vt._engine()                        # ctl: the same history without the compaction
    for e in (eng, ctl):
        e.set_namespaces(ns)
        e.cparam_load_rules(rules, None, lg)
        vt._same(e.cparam_decide_host(req, vals), want, "the batch with the value the limiter turns away")
        assert _used(e, 3, True) == first
    grown = [sets[0] + [late], sets[1], sets[2]]
    req2, vals2 = vt._cp_batch(rng, grown, 6000, int(req["ts_ms"][-1]) + 1, 1500, 0.3)
    want2 = ora.decide_param(req2, vals2)
    assert vt._code(ctl.cparam_decide_host, req2, vals2) == abi.SG_E_CAPACITY   # the dead claim holds the last slot
    for arg in (lg - 1, 29, 0, -3):                              # a shrink, sizes out of range
        assert vt._code(eng.cparam_resize, arg) == abi.SG_E_INVAL, arg
        assert _used(eng, 3, True) == first
    eng.cparam_resize(lg)                                        # the same size: a compaction
    assert _used(eng, 3, True) == [(3, 3, 4)] * 3
    vt._same(eng.cparam_decide_host(req2, vals2), want2, "the refused batch, after the compaction")
    assert [u[0] for u in _used(eng, 3, True)] == [4, 3, 3]
    now = int(req2["ts_ms"][-1])
    for r in range(3):
        for v in grown[r] + [dead]:
            assert eng.cparam_sum(r, v, now) == ora.param_sum(r, v, now)


# ------------------------------------------------------------------------------------------------ the slot chain

@functools.lru_cache(maxsize=None)
def _chain_grow_case():
    """tests/test_value_tables_gpu.py's chain (six resources with one QPS param rule of 4 slots each, two authority
    rules): filled exactly, then a batch in which every resource meets one more value."""
    from types import SimpleNamespace
    from tests.test_authority_kat import AuthChecker
    from tests.test_oracle_pslot_kat import rule as prule
    from tests.test_slot_chain_gpu import _entries
    rng = np.random.default_rng(1301)
    n_res, n_origins, n = len(vt.SC_KIND), 2, 7000
    base = np.array([local_rule() for _ in range(n_res)], abi.LOCAL_RULE_DTYPE)
    frules = np.array([local_flow_rule(r, c) for r, c in enumerate([15.0, 6.0, 50.0, 10.0, 25.0, 8.0])],
                      abi.LOCAL_FLOW_RULE_DTYPE)
    params = np.array([prule(res=0, idx=0, count=8.0), prule(res=1, idx=0, count=5.0, dur=2),
                       prule(res=2, idx=0, count=20.0, behavior=abi.BEHAVIOR_RATE_LIMITER, max_q=50),
                       prule(res=3, idx=0, count=6.0), prule(res=4, idx=0, count=12.0), prule(res=5, idx=0, count=4.0)],
                      abi.PSLOT_RULE_DTYPE)
    params["rule"]["capacity_log2"] = vt.SC_LG
    params["rule"]["burst"][3] = 3
    chk = AuthChecker(base, frules, params, vt.SC_AUTH, n_res, n_origins, 0)
    taken = [[] for _ in range(n_res)]

    def fresh(k):
        out = []
        for r in range(n_res):
            out.append(vt._value_set(rng, vt.SC_KIND[r], vt.SC_LG, k, taken[r]))
            taken[r] += out[-1]
        return out

    full = [s + [MARKER] for s in fresh(1 << vt.SC_LG)]
    extra, junk = fresh(1), fresh(6)
    over = [a + b for a, b in zip(full, extra)]
    pool = vt._ArgPool()
    t = T0 + 90_000 + int(rng.integers(0, 1000))
    batches = []

    def step(sets, span):
        nonlocal t
        ent = _entries(rng, n, n_res, t, span, n_origins, zipf=0.4, prio=0.0)
        rej = chk.rejected(ent)
        ext = pool.ext(rng, ent, sets, rej, junk)
        args, values = pool.arrays()
        ev, xo, want, k = chk.batch(ent, ext, rng.integers(0, 41, n).astype(np.int32),
                                    (rng.random(n) < 0.05).astype(np.uint8), t + span, args, values)
        used = {(int(r), int(values[args["value_begin"][x["arg_begin"]]])) for r, x in
                zip(ent["resource"][~rej] & np.uint32(0x7FFFFFFF), ext[~rej]) if not x["args_null"]}
        assert used == {(r, v) for r in range(n_res) for v in sets[r]}  # every value of every rule
        assert abi.LOCAL_BLOCK_PARAM in want["status"] and abi.LOCAL_PASS in want["status"]
        vt._frozen(ev, xo, args, values, want)
        batches.append((ev, xo, args, values, want))
        t += span

    step(full, 2500)
    step(over, 2000)
    step(over, 2800)
    probe = SimpleNamespace(values=sorted({v for r in range(n_res) for v in over[r] + junk[r][:2]}))
    return base, frules, params, chk, batches, probe, full


@pytest.mark.parametrize("flags", WALKERS)
def test_slot_chain_refused_grown_accepted(flags):
    """Case 6: the chain's lookup finds a rule's table full while the batch is still being validated:
    SG_E_CAPACITY, the thread counts as they were. After sg_param_resize the same batch equals
    LocalChain.decide_ext, and so do the later one and the whole state."""
    from tests.test_authority_gpu import _check_batches, _check_state
    from tests.test_authority_kat import to_abi
    base, frules, params, chk, batches, probe, full = _chain_grow_case()
    eng = vt._engine(flags)
    eng.local_load_rules(base, 2, 1000, 500)
    assert eng.local_load_flow_rules(frules, 2, 0) == chk.kept
    eng.pslot_load_rules(params, n_resources=len(base))
    rules, ids = to_abi(vt.SC_AUTH)
    assert eng.local_load_authority_rules(rules, ids, 2) == len(vt.SC_AUTH)
    _check_batches(eng, batches[:1])
    n_res = len(base)
    assert [u[0] for u in _used(eng, n_res)] == [1 << vt.SC_LG] * n_res
    threads = [eng.pslot_thread_count(r, 0, v) for r in range(n_res) for v in full[r]]
    states = [eng.param_state(r, v) for r in range(n_res) for v in full[r]]
    assert vt._code(eng.slot_decide_host, *batches[1][:4]) == abi.SG_E_CAPACITY
    assert [eng.pslot_thread_count(r, 0, v) for r in range(n_res) for v in full[r]] == threads
    assert [eng.param_state(r, v) for r in range(n_res) for v in full[r]] == states
    eng.param_resize([vt.SC_LG + 1] * n_res)
    assert [eng.pslot_thread_count(r, 0, v) for r in range(n_res) for v in full[r]] == threads
    assert _used(eng, n_res) == [(1 << vt.SC_LG, 1 << vt.SC_LG, 2 << vt.SC_LG)] * n_res
    _check_batches(eng, batches[1:])
    _check_state(eng, chk, n_res, 2, 0, probe)


def test_embedded_token_server_grows_ahead():
    """Case 6, SERVER: a cluster-mode param rule's tokens come from this handle's cluster param tables, which the
    walker fills as it adds. Grown by sg_cparam_resize before the third value arrives, the chain goes on equal to the
    oracles, window sums included."""
    rng = np.random.default_rng(1302)
    rules = vt._ps_rules(2, 4)
    rules["cluster_mode"], rules["cluster_key"] = abi.CLUSTER_MODE_FALLBACK, [0, 1]
    two = [random_values(rng, 2) for _ in range(2)]
    three = [s + random_values(rng, 1, s) for s in two]
    cp = vt._cp_rules([40.0, 25.0])
    cts = ClusterTokenService()
    cts.set_namespaces(vt._ns())
    cts.load_param_rules(cp)
    ora = ParamFlowSlot(rules, n_resources=2)
    ora.attach_cluster(cts, abi.CLUSTER_SERVER)
    eng = vt._engine()
    eng.set_namespaces(vt._ns())
    eng.cparam_load_rules(cp, None, 1)
    eng.local_set_cluster_state(abi.CLUSTER_SERVER)
    eng.pslot_load_rules(rules, n_resources=2)
    a = vt._ps_step(ora, vt._ps_batch(rng, two, 3000, T0, 1500))
    vt._ps_check(eng, a, "two values per rule")
    assert _used(eng, 2, True) == [(2, 2, 2)] * 2   # the shim watches this and grows ahead of the refusal
    eng.cparam_resize(3)
    t = int(a[0]["ts_ms"][-1])
    for b in range(2):
        step = vt._ps_step(ora, vt._ps_batch(rng, three, 5000, t, 1200))
        vt._ps_check(eng, step, f"batch {b} after the growth")
        t = int(step[0]["ts_ms"][-1])
    assert _used(eng, 2, True) == [(3, 3, 8)] * 2
    for k in range(2):
        for v in three[k]:
            assert eng.cparam_sum(k, v, t) == cts.param_sum(k, v, t)


def test_resize_with_local_tickets_outstanding():
    """Case 6, ordering: sg_param_resize drains the pipeline before it reads the tables. Tickets issued before it
    complete with their own answers, and the batch enqueued after it decides on."""
    from tests.test_local_pipeline_gpu import _check, _compare, _enqueue_all, _results, _rules, _trace
    rng = np.random.default_rng(1303)
    rules = _rules(12, rng, lo=3, hi=30)
    trace, ora = _trace(rules, [(9_000, 600), (9_000, 600), (9_000, 600)], 2, 1000, 500, seed=1303)
    eng = vt._engine()
    eng.local_load_rules(rules, 2, 1000, 500)
    eng.param_load_rules(_twin_rules((2, 2, 2, 2)))
    bufs = _enqueue_all(eng, [trace[0][0], trace[1][0]])
    eng.param_resize([3, 0, 4, 0])
    assert [u[2] for u in _used(eng, 4)] == [8, 4, 16, 4]
    bufs += _enqueue_all(eng, [trace[2][0]])
    for b, (_, d_out, ticket) in enumerate(bufs):
        eng.local_wait(ticket)
        _check(_results(d_out), trace[b][1], b)
    _compare(eng, ora, len(rules), 2)


# ------------------------------------------------------------------------------------------------ the node handle

@functools.lru_cache(maxsize=None)
def _node_cp_case():
    rng = np.random.default_rng(1401)
    lg, R = 2, 6
    rules = vt._cp_rules(rng.integers(20, 200, R))
    first = [vt._value_set(rng, vt.CP_KIND[r % 3], lg, 1 << lg) + [MARKER] for r in range(R)]
    more = [vt._value_set(rng, vt.CP_KIND[r % 3], lg, 1 << lg, first[r]) for r in range(R)]
    both = [a + b for a, b in zip(first, more)]
    ora = ClusterTokenService()
    ora.set_namespaces(vt._ns())
    ora.load_param_rules(rules)
    a = vt._cp_step(ora, rng, first, [(r, v) for r in range(R) for v in first[r]], T0 + 61, 2000, 0.3, rules)
    b = vt._cp_step(ora, rng, both, [(r, v) for r in range(R) for v in both[r]], a[3], 1700, 0.3, rules)
    return lg, rules, a, b


@pytest.mark.parametrize("shards", [2, 3])
def test_node_cparam_resize(shards):
    """Case 7: same-device shards, every owner's tables exactly full, grown through the node, full again at twice the
    size: equal to the oracle's replay, the counts answered by each rule's owner."""
    from sentinel_amd.engine import NodeEngine
    lg, rules, a, b = _node_cp_case()
    R = len(rules)
    node = NodeEngine([0] * shards, max_batch=vt.MAX_BATCH)
    node.set_namespaces(vt._ns())
    node.cparam_load_rules(rules, None, lg)
    vt._cp_check(node, a, "first batch")
    assert [node.cparam_table_used(r) for r in range(R)] == [(4, 4, 4)] * R
    assert vt._code(node.cparam_resize, lg - 1) == abi.SG_E_INVAL
    node.cparam_resize(lg + 1)
    assert [node.cparam_table_used(r) for r in range(R)] == [(4, 4, 8)] * R
    vt._cp_sums(node, a, "after the growth")
    vt._cp_check(node, b, "the batch that fills the grown tables")
    assert [node.cparam_table_used(r) for r in range(R)] == [(8, 8, 8)] * R


@pytest.mark.parametrize("shards", [2, 3])
def test_node_param_resize(shards):
    """Case 7: the chain of test_slot_chain_refused_grown_accepted over the node: the front and every shard grow, the
    refused batch is then the oracle's, and a rule's counts come from the owner of its resource."""
    from sentinel_amd.engine import NodeEngine
    from tests.test_authority_gpu import _check_batches
    from tests.test_authority_kat import to_abi
    base, frules, params, chk, batches, probe, full = _chain_grow_case()
    n_res = len(base)
    node = NodeEngine([0] * shards, max_batch=vt.MAX_BATCH)
    node.local_load_rules(base, 2, 1000, 500)
    assert node.local_load_flow_rules(frules, 2, 0) == chk.kept
    node.pslot_load_rules(params, n_resources=n_res)
    rules, ids = to_abi(vt.SC_AUTH)
    assert node.local_load_authority_rules(rules, ids, 2) == len(vt.SC_AUTH)
    _check_batches(node, batches[:1])
    assert [node.param_table_used(r) for r in range(n_res)] == [(1 << vt.SC_LG, 1 << vt.SC_LG, 1 << vt.SC_LG)] * n_res
    assert vt._code(node.param_resize, [vt.SC_LG + 1] * (n_res - 1)) == abi.SG_E_INVAL
    assert vt._code(node.param_resize, [1] * n_res) == abi.SG_E_INVAL
    node.param_resize([vt.SC_LG + 1] * n_res)
    assert [node.param_table_used(r) for r in range(n_res)] == [(1 << vt.SC_LG, 1 << vt.SC_LG, 2 << vt.SC_LG)] * n_res
    _check_batches(node, batches[1:])
    for r in range(n_res):
        for v in probe.values:
            f, lt, tk = chk.ps.token_state(r, v)
            gf, glt, gtk = node.param_state(r, v)
            assert (gf, glt if f & 1 else 0, gtk if f & 2 else 0) == (f, lt if f & 1 else 0, tk if f & 2 else 0), \
                f"token state of rule {r} value {v:#x}"


# ------------------------------------------------------------------------------------------------ sg_vdict_grow

I, L, STR = abi.PARAM_TYPE_INTEGER, abi.PARAM_TYPE_LONG, abi.PARAM_TYPE_STRING


def _vd_engine(cap_log2, arena):
    from tests.test_param_codec_gpu import _engine
    return _engine([11, 12], cap_log2=cap_log2, arena=arena, max_values=4096, max_batch=4096)


def _vd_keys(lo, hi):
    """Short values and strings longer than 8 bytes, alternating (12 arena bytes per string)."""
    return [(STR, b"value-%06d" % i) if i % 2 else (I, struct.pack(">i", i)) for i in range(lo, hi)]


def test_vdict_grow_keeps_every_id():
    """Case 8: filled to capacity, one more value is SG_E_CAPACITY; after sg_vdict_grow every old value has its old
    id and its bytes, new values continue the numbering, and a decoded stream equals the same stream over a dictionary
    that was large from the start, and RefDecoder. Refusals and growing the arena alone."""
    from param_frames import RefDecoder, param_frame
    from tests.test_param_codec_gpu import _assert_decoded, _assert_dictionary, _decode_gpu
    fresh = vt._engine()
    assert vt._code(fresh.vdict_grow, 8, 1 << 12) == abi.SG_E_INVAL      # before sg_vdict_init
    old = _vd_keys(0, 64)
    arena = 12 * 32
    eng, twin, ref = _vd_engine(6, arena), _vd_engine(8, 4096), RefDecoder([11, 12])
    for e in (eng, twin):
        assert list(e.vdict_intern(old)) == list(range(1, 65))
    ref.intern(old)
    assert eng.vdict_size() == (64, arena)
    assert vt._code(eng.vdict_intern, [(I, struct.pack(">i", 1000))]) == abi.SG_E_CAPACITY
    for lg, ab in ((5, arena), (29, arena), (0, arena), (6, arena - 1), (8, 0)):   # shrinks and sizes out of range
        assert vt._code(eng.vdict_grow, lg, ab) == abi.SG_E_INVAL, (lg, ab)
        assert eng.vdict_size() == (64, arena)
    assert list(eng.vdict_intern(old[::-1])) == list(range(64, 0, -1))
    eng.vdict_grow(8, 4096)
    assert eng.vdict_size() == (64, arena)
    assert list(eng.vdict_intern(old)) == list(range(1, 65))
    assert eng.vdict_lookup(np.arange(1, 65, dtype=np.uint64)) == old
    new = _vd_keys(64, 200)
    for e in (eng, twin):
        assert list(e.vdict_intern(new[:10] + old[:3])) == list(range(65, 75)) + [1, 2, 3]
    ref.intern(new[:10])
    rng = np.random.default_rng(1501)
    keys = old + new
    frames = [param_frame(i, 11 + i % 2, 1, [keys[int(j)] for j in rng.integers(0, len(keys), 1 + i % 3)])
              for i in range(900)]
    ts = np.full(len(frames), T0, np.int64)
    d, dt = _decode_gpu(eng, frames, ts), _decode_gpu(twin, frames, ts)
    assert np.array_equal(d.values, dt.values) and np.array_equal(d.req, dt.req)
    _assert_decoded(d, ref.decode(frames, ts))
    _assert_dictionary(eng, ref)
    _assert_dictionary(twin, ref)
    # the arena alone: 4 strings fit, the fifth does not until the arena grows
    small = _vd_engine(6, 48)
    strs = [(STR, b"string-%05d" % i) for i in range(6)]
    assert list(small.vdict_intern(strs[:4])) == [1, 2, 3, 4]
    assert vt._code(small.vdict_intern, strs[4:5]) == abi.SG_E_CAPACITY
    small.vdict_grow(6, 96)
    assert list(small.vdict_intern(strs[4:] + strs[:2])) == [5, 6, 1, 2]
    assert small.vdict_lookup([1, 4, 5, 6]) == [strs[0], strs[3], strs[4], strs[5]]
    assert small.vdict_size() == (6, 72)
