"""The exact open-addressing value tables at capacity (param_slot, cp_slot / cp_find and their callers): parity with
the oracles when every sub-table is exactly full, probe chains that wrap past a sub-table's end, unequal sub-table
sizes in one load, the marker value 0xFFFF…FFFF (the tables' empty word, kept in each rule's side slot) and the value
0, SG_E_CAPACITY for one value too many, and refused batches, which change no state: not a counter, not a window sum,
and not the tables' free slots.

The oracles have no capacity limit, so each case has a reference for as long as the device accepts the batch. The
value sets come from tests/value_tables.py: one rule's values all start their probe at the last slot of its sub-table.
Every reference is computed once (per case, shared by the walker variants) and never modified."""
import functools

import numpy as np
import pytest

from oracle.binding import ClusterTokenService, ParamFlowChecker, ParamFlowSlot, local_flow_rule, local_rule
from sentinel_amd import abi
from tests.value_tables import MARKER, home, homed_values, random_values

pytestmark = pytest.mark.gpu

WALKERS = [0, abi.FLAG_SERIAL_ONLY, abi.FLAG_WAVE_ONLY]
T0 = 1_700_000_000_000
N = 20_000            # requests per batch
MAX_BATCH = 1 << 15


def _engine(flags=0, max_batch=MAX_BATCH):
    from sentinel_amd.engine import FlowEngine
    return FlowEngine(device=0, max_batch=max_batch, flags=flags)


def _code(call, *args):
    from sentinel_amd.engine import EngineError
    with pytest.raises(EngineError) as e:
        call(*args)
    return e.value.code


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {len(bad)} differ; first at {bad[0]}: oracle={want[bad[0]]} gpu={got[bad[0]]}")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _value_set(rng, kind, lg, k, exclude=()):
    """k values for a sub-table of 2^lg slots: 'last' — all homed at its last slot (every probe chain wraps to slot
    0); 'zero' — random ones, the value 0 among them; 'random'."""
    mask = (1 << lg) - 1
    if kind == "last":
        out = homed_values(rng, k, mask, mask, exclude)
        assert all(home(v, mask) == mask for v in out)
        return out
    if kind == "zero" and 0 not in exclude:
        return [0] + random_values(rng, k - 1, tuple(exclude) + (0,))
    return random_values(rng, k, exclude)


# ------------------------------------------------------------------------------------------------ sg_param_*

P_LG = (1, 4, 2)                    # unequal sub-tables in one load: rule_of_slot's binary search over table_base
P_KIND = ("last", "zero", "last")


def _param_rules():
    r = np.zeros(3, abi.PARAM_RULE_DTYPE)
    r["count"] = [40, 25, 60]
    r["duration_sec"] = 1
    r["burst"] = [0, 4, 0]
    r["behavior"] = [abi.BEHAVIOR_DEFAULT, abi.BEHAVIOR_DEFAULT, abi.BEHAVIOR_RATE_LIMITER]
    r["max_queueing_ms"] = [0, 0, 40]
    r["capacity_log2"] = P_LG
    return r


def _param_batch(rng, pairs, n, t, span):
    """n requests over the (rule, value) pairs, every pair at least once."""
    pick = np.concatenate([np.arange(len(pairs)), rng.integers(0, len(pairs), n - len(pairs))])
    rng.shuffle(pick)
    q = np.zeros(n, abi.PARAM_REQ_DTYPE)
    q["ts_ms"] = t + np.sort(rng.integers(0, span, n))
    q["rule"] = np.array([pairs[i][0] for i in pick], np.uint32)
    q["value"] = np.array([pairs[i][1] for i in pick], np.uint64)
    q["acquire"] = rng.integers(1, 3, n)
    return q


def _param_step(ora, rng, pairs, known, t, span):
    """One accepted batch through the oracle: (requests, pass bits, the state of every known pair afterwards)."""
    req = _param_batch(rng, pairs, N, t, span)
    want = ora.decide(req)
    for r in range(3):  # the premise: every rule both passes and blocks
        assert set(want[req["rule"] == r].tolist()) == {0, 1}, f"rule {r}"
    states = {p: ora.state(*p) for p in known}
    _frozen(req, want)
    return req, want, states


def _param_check(eng, step, what):
    req, want, states = step
    _same(eng.param_decide_host(req), want, what)
    _param_states(eng, states, what)


def _param_states(eng, states, what):
    for (r, v), st in states.items():
        got = eng.param_state(r, v)
        assert got == st if st[0] else got[0] == 0, f"{what}: state of rule {r} value {v:#x}: oracle {st} gpu {got}"


@functools.lru_cache(maxsize=None)
def _param_full_case():
    """Every rule sees exactly 2^capacity_log2 ordinary values plus the marker, over three batches."""
    rng = np.random.default_rng(101)
    rules = _param_rules()
    sets = [_value_set(rng, P_KIND[r], P_LG[r], 1 << P_LG[r]) for r in range(3)]
    pairs = [(r, v) for r in range(3) for v in sets[r] + [MARKER]]
    assert (1, 0) in pairs
    ora = ParamFlowChecker()
    ora.load_rules(rules)
    steps, t = [], T0 + 7
    for span in (2600, 1000, 1900):
        steps.append(_param_step(ora, rng, pairs, pairs, t, span))
        t = int(steps[-1][0]["ts_ms"][-1]) + int(rng.integers(0, 1200))
    # one value too many for each rule in turn, among requests over the known pairs (never shown to the oracle)
    over = []
    for r in range(3):
        extra = _value_set(rng, P_KIND[r], P_LG[r], 1, sets[r])[0]
        over.append(_param_batch(rng, pairs + [(r, extra)], 4000, int(steps[0][0]["ts_ms"][-1]) + 1, 300))
    return rules, pairs, steps, over


@pytest.mark.parametrize("flags", WALKERS)
def test_param_tables_exactly_full(flags):
    """Case 1: three rules of 2, 16 and 4 slots (token bucket, token bucket with burst, throttle), each exactly full
    and with its side slot in use; two of them with every value homed at the last slot."""
    rules, pairs, steps, _ = _param_full_case()
    eng = _engine(flags)
    eng.param_load_rules(rules)
    for b, step in enumerate(steps):
        _param_check(eng, step, f"batch {b}")


@pytest.mark.parametrize("flags", WALKERS)
def test_param_one_value_too_many(flags):
    """Case 2: a full rule meets one more distinct value: SG_E_CAPACITY, nothing changes, the next batches go on."""
    rules, pairs, steps, over = _param_full_case()
    eng = _engine(flags)
    eng.param_load_rules(rules)
    _param_check(eng, steps[0], "first batch")
    for r, req in enumerate(over):
        assert _code(eng.param_decide_host, req) == abi.SG_E_CAPACITY, f"one more value for rule {r}"
        _param_states(eng, steps[0][2], f"after the refusal for rule {r}")
    _param_check(eng, steps[1], "batch after the refusals")
    _param_check(eng, steps[2], "last batch")


P_SPARE = (1, 5, 2)  # slots left free by the first batch


@functools.lru_cache(maxsize=None)
def _param_refusal_case():
    rng = np.random.default_rng(103)
    rules = _param_rules()
    taken = [[], [], []]

    def fresh(r, k):
        out = _value_set(rng, P_KIND[r], P_LG[r], k, taken[r])
        taken[r] += out
        return out

    first = [fresh(r, (1 << P_LG[r]) - P_SPARE[r]) for r in range(3)]
    flood = [fresh(r, 1 << P_LG[r]) for r in range(3)]          # 2^lg new values: more than the free slots
    few = [fresh(r, P_SPARE[r] + 1) for r in range(3)]          # one more than the free slots
    last = [fresh(r, P_SPARE[r]) for r in range(3)]             # exactly the free slots
    known = [(r, v) for r in range(3) for v in first[r] + [MARKER]]
    full = known + [(r, v) for r in range(3) for v in last[r]]
    ora = ParamFlowChecker()
    ora.load_rules(rules)
    a = _param_step(ora, rng, known, known, T0 + 50_000, 2200)
    t = int(a[0]["ts_ms"][-1]) + 3
    refused = {
        # older than the first batch
        "time": _param_batch(rng, known + [(r, v) for r in range(3) for v in flood[r]], 6000, T0, 1500),
        "capacity": _param_batch(rng, known + [(r, v) for r in range(3) for v in few[r]], 6000, t, 1500),
    }
    b = _param_step(ora, rng, full, full, t, 1700)
    c = _param_step(ora, rng, full, full, int(b[0]["ts_ms"][-1]), 2400)
    gone = [(r, v) for r in range(3) for v in flood[r] + few[r]]
    return rules, a, refused, b, c, gone


@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("why", ["time", "capacity"])
def test_param_refused_batch_uses_no_capacity(why, flags):
    """Case 3: k_pprep claims a slot for every new value before the batch's verdict is known. A batch refused for its
    timestamps or for a full table gives the slots back: the batch after it fills every rule to exactly full."""
    rules, a, refused, b, c, gone = _param_refusal_case()
    eng = _engine(flags)
    eng.param_load_rules(rules)
    _param_check(eng, a, "first batch")
    assert _code(eng.param_decide_host, refused[why]) == (abi.SG_E_TIME if why == "time" else abi.SG_E_CAPACITY)
    _param_states(eng, a[2], "after the refusal")
    for r, v in gone:
        assert eng.param_state(r, v)[0] == 0
    _param_check(eng, b, "the batch that fills the tables")
    _param_check(eng, c, "last batch")


# ------------------------------------------------------------------------------------------------ sg_cparam_*

CP_KIND = ("last", "zero", "random")


def _cp_rules(counts, S=10, interval=1000, flow_id0=7):
    r = np.zeros(len(counts), abi.CPARAM_RULE_DTYPE)
    r["flow_id"] = np.arange(len(counts)) * 3 + flow_id0
    r["count"] = counts
    r["threshold_type"] = abi.THRESHOLD_GLOBAL
    r["sample_count"] = S
    r["window_interval_ms"] = interval
    return r


def _ns(lim_qps=0.0):
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"] = 1
    if lim_qps:
        ns["limiter_enabled"], ns["max_allowed_qps"] = 1, lim_qps
    return ns


def _cp_batch(rng, sets, n, t, span, multi=0.3):
    """n requests over the rules' value sets (sets[r]: rule r's values), every (rule, value) at least once; `multi` of
    them with 2 to 3 values drawn with repetition."""
    pairs = [(r, v) for r, s in enumerate(sets) for v in s]
    keys = np.concatenate([[r for r, _ in pairs], rng.integers(0, len(sets), n - len(pairs))]).astype(np.uint32)
    lead = np.concatenate([np.array([v for _, v in pairs], np.uint64), np.zeros(n - len(pairs), np.uint64)])
    forced = np.arange(n) < len(pairs)
    order = rng.permutation(n)
    keys, lead, forced = keys[order], lead[order], forced[order]
    req = np.zeros(n, abi.CPARAM_REQ_DTYPE)
    req["ts_ms"] = t + np.sort(rng.integers(0, span, n))
    req["key"] = keys
    req["acquire"] = rng.integers(1, 3, n)
    counts = np.where(rng.random(n) < multi, rng.integers(2, 4, n), 1).astype(np.uint32)
    req["value_count"] = counts
    req["value_begin"] = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32)
    owner = np.repeat(np.arange(n), counts)
    values = np.zeros(len(owner), np.uint64)
    for r, s in enumerate(sets):
        at = np.nonzero(keys[owner] == r)[0]
        values[at] = np.array(s, np.uint64)[rng.integers(0, len(s), len(at))]
    values[req["value_begin"][forced]] = lead[forced]
    return req, values


def _cp_step(ora, rng, sets, known, t, span, multi=0.3, rules=None, need=(abi.OK, abi.BLOCKED)):
    """One accepted batch through the oracle: requests, values, results, and afterwards every known (rule, value)'s
    window sum and each rule's top values (the values with a positive sum, qps = sum / intervalSec)."""
    req, vals = _cp_batch(rng, sets, N, t, span, multi)
    want = ora.decide_param(req, vals)
    for s in need:  # the premise
        assert (want["status"] == s).any(), f"no status {s} in the oracle's answers"
    now = int(req["ts_ms"][-1])
    sums = {p: ora.param_sum(p[0], p[1], now) for p in known}
    top = [{v: sums[(r, v)] / (rules["window_interval_ms"][r] / 1000.0) for (rr, v) in known if rr == r and sums[(r, v)] > 0}
           for r in range(len(sets))]
    _frozen(req, vals, want)
    return req, vals, want, now, sums, top


def _cp_check(eng, step, what, lg=None):
    req, vals, want, now, sums, top = step
    _same(eng.cparam_decide_host(req, vals), want, what)
    _cp_sums(eng, step, what, lg)


def _cp_sums(eng, step, what, lg=None):
    _, _, _, now, sums, top = step
    for (r, v), s in sums.items():
        assert eng.cparam_sum(r, v, now) == s, f"{what}: window sum of rule {r} value {v:#x}"
    if lg is not None:
        got = eng.cparam_top_values(now, len(top), (1 << lg) + 1)
        assert [dict(g) for g in got] == top, f"{what}: top values"
        assert all(len(g) == len(t) for g, t in zip(got, top))


def _cp_sets(rng, lg, k=None, exclude=None, marker=True):
    k = (1 << lg) if k is None else k
    exclude = exclude or [()] * 3
    return [_value_set(rng, CP_KIND[r], lg, k, exclude[r]) + ([MARKER] if marker else []) for r in range(3)]


@functools.lru_cache(maxsize=None)
def _cp_full_case(lg, S):
    rng = np.random.default_rng(200 + 10 * lg + S)
    rules = _cp_rules(rng.integers(20, 200, 3), S=S, interval=1000 if 1000 % S == 0 else 100 * S)  # S = 16: 1600 ms
    sets = _cp_sets(rng, lg)
    assert 0 in sets[1] and all(MARKER in s for s in sets)
    known = [(r, v) for r in range(3) for v in sets[r]]
    ora = ClusterTokenService()
    ora.set_namespaces(_ns())
    ora.load_param_rules(rules)
    steps, t = [], T0 + 3
    for span, multi in ((2500, 0.3), (1500, 0.8), (2900, 0.3)):
        steps.append(_cp_step(ora, rng, sets, known, t, span, multi, rules))
        t = int(steps[-1][0]["ts_ms"][-1]) + int(rng.integers(0, 900))
    for req, vals, want, *_ in steps:  # the marker alone and inside multi-value requests, both charged
        lone = (req["value_count"] == 1) & (vals[req["value_begin"]] == np.uint64(MARKER))
        inside = (req["value_count"] > 1) & np.array([(vals[b:b + c] == np.uint64(MARKER)).any()
                                                      for b, c in zip(req["value_begin"], req["value_count"])])
        assert (want["status"][lone] == abi.OK).any() and (want["status"][inside] == abi.OK).any()
    return rules, steps


@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("S", [10, 1, 16])
@pytest.mark.parametrize("lg", [1, 2, 4])
def test_cparam_tables_exactly_full(lg, S, flags, monkeypatch):
    """Case 4: three rules whose sub-tables are exactly full (the side slots in use, one rule's values homed at the
    last slot), single- and multi-value requests; once with the fixed point's rounds and once with none allowed
    (SG_CP_MAX_ROUNDS=0: every batch through the group fallback)."""
    rules, steps = _cp_full_case(lg, S)
    eng = _engine(flags)
    monkeypatch.setenv("SG_CP_MAX_ROUNDS", "0")
    eng0 = _engine(flags)
    monkeypatch.delenv("SG_CP_MAX_ROUNDS")
    rounds = []
    for e in (eng, eng0):
        e.set_namespaces(_ns())
        e.cparam_load_rules(rules, None, lg)
    for b, step in enumerate(steps):
        _cp_check(eng, step, f"batch {b}", lg)
        rounds.append(eng.cparam_last_rounds())
        _cp_check(eng0, step, f"batch {b}, group fallback", lg)
        assert eng0.cparam_last_rounds() == 1  # max_rounds (0) + 1
    assert max(rounds) > 1, rounds


@functools.lru_cache(maxsize=None)
def _cp_reload_case():
    lg = 2
    rng = np.random.default_rng(300)
    rules = _cp_rules(rng.integers(20, 200, 3))
    sets = _cp_sets(rng, lg)
    known = [(r, v) for r in range(3) for v in sets[r]]
    ora = ClusterTokenService()
    ora.set_namespaces(_ns())
    ora.load_param_rules(rules)
    a = _cp_step(ora, rng, sets, known, T0 + 11, 1800, 0.3, rules)
    assert a[4][(0, MARKER)] > 0 and all(a[4][(0, v)] > 0 for v in sets[0])  # full and charged, the side slot too
    # rule 0 (the wrapped chains) survives as rule 2 of the new set; the others are new flowIds
    new = np.concatenate([_cp_rules(rng.integers(20, 200, 2), flow_id0=1000), rules[:1]])
    ora.load_param_rules(new)
    nsets = [sets[1], sets[2], sets[0]]
    nknown = [(r, v) for r in range(3) for v in nsets[r]]
    now = a[3] + 1
    kept = {(2, v): ora.param_sum(2, v, now) for v in sets[0]}
    assert kept[(2, MARKER)] > 0
    b = _cp_step(ora, rng, nsets, nknown, now, 2100, 0.3, new)
    return lg, rules, new, a, now, kept, b


@pytest.mark.parametrize("flags", WALKERS)
def test_cparam_reload_moves_a_full_sub_table(flags):
    """Case 5: a reload keeps a surviving flowId's metric: k_cp_copy moves its 2^lg slots and the side slot."""
    lg, rules, new, a, now, kept, b = _cp_reload_case()
    eng = _engine(flags)
    eng.set_namespaces(_ns())
    eng.cparam_load_rules(rules, None, lg)
    _cp_check(eng, a, "before the reload", lg)
    eng.cparam_load_rules(new, None, lg)
    for (r, v), s in kept.items():
        assert eng.cparam_sum(r, v, now) == s, f"survivor's window sum of value {v:#x}"
    for r in (0, 1):
        for v in b[4]:
            if v[0] == r:
                assert eng.cparam_sum(r, v[1], now) == 0
    _cp_check(eng, b, "after the reload", lg)


CP_REFUSALS = {"time": abi.SG_E_TIME, "inval": abi.SG_E_INVAL, "unsupported": abi.SG_E_UNSUPPORTED,
               "capacity": abi.SG_E_CAPACITY, "time_limiter": abi.SG_E_TIME}


@functools.lru_cache(maxsize=None)
def _cp_refusal_case(why):
    lg, spare = 4, 5
    rng = np.random.default_rng(400 + sorted(CP_REFUSALS).index(why))
    lim = why == "time_limiter"
    if why == "unsupported":   # 1 ms window periods: a 70 s batch spans more than 65,536 of them
        rules = _cp_rules([500.0, 300.0, 800.0], S=10, interval=10)
    else:
        rules = _cp_rules(rng.integers(20, 200, 3))
    first = _cp_sets(rng, lg, (1 << lg) - spare)
    flood = _cp_sets(rng, lg, 1 << lg, first, marker=False)
    few = _cp_sets(rng, lg, spare + 1, [a + b for a, b in zip(first, flood)], marker=False)
    last = _cp_sets(rng, lg, spare, [a + b + c for a, b, c in zip(first, flood, few)], marker=False)
    full = [a + b for a, b in zip(first, last)]
    known = [(r, v) for r in range(3) for v in first[r]]
    fknown = [(r, v) for r in range(3) for v in full[r]]
    ns = _ns(4000.0 if lim else 0.0)
    ora = ClusterTokenService()
    ora.set_namespaces(ns)
    ora.load_param_rules(rules)
    need = (abi.OK, abi.BLOCKED) + ((abi.TOO_MANY_REQUEST,) if lim else ())
    a = _cp_step(ora, rng, first, known, T0 + 100_000, 2000, 0.3, rules, need)
    t = a[3] + 1
    both = [x + y for x, y in zip(first, flood)]
    if why in ("time", "time_limiter"):
        bad = _cp_batch(rng, both, 8000, T0, 1500)
    elif why == "unsupported":
        bad = _cp_batch(rng, both, 8000, t, 70_000)
    elif why == "capacity":
        bad = _cp_batch(rng, [x + y for x, y in zip(first, few)], 8000, t, 1500)
    else:  # two valid requests' value ranges overlap
        req, vals = _cp_batch(rng, both, 8000, t, 1500)
        req["value_begin"][4001] = req["value_begin"][4000]
        bad = (req, vals)
    _frozen(*bad)
    gone = [(r, v) for r in range(3) for v in flood[r] + few[r]]
    b = _cp_step(ora, rng, full, fknown, t, 1600, 0.3, rules, need)
    c = _cp_step(ora, rng, full, fknown, b[3], 2300, 0.3, rules, need)
    return lg, rules, ns, a, bad, gone, b, c


@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("why", sorted(CP_REFUSALS))
def test_cparam_refused_batch_uses_no_capacity_and_changes_no_sum(why, flags):
    """Case 6: k_cp_prep2 claims a slot for every new value before the verdict (also for requests the namespace
    limiter turns away). After each kind of refusal the window sums are the oracle's, the refused values are absent,
    and the next batch fills every rule to exactly full."""
    lg, rules, ns, a, bad, gone, b, c = _cp_refusal_case(why)
    eng = _engine(flags)
    eng.set_namespaces(ns)
    eng.cparam_load_rules(rules, None, lg)
    _cp_check(eng, a, "first batch", lg)
    assert _code(eng.cparam_decide_host, *bad) == CP_REFUSALS[why]
    _cp_sums(eng, a, "after the refusal", lg)
    for r, v in gone:
        assert eng.cparam_sum(r, v, a[3]) == 0
    _cp_check(eng, b, "the batch that fills the tables", lg)
    _cp_check(eng, c, "last batch", lg)


# ------------------------------------------------------------------------------------------------ the slot chain

SC_KIND = ("last", "zero", "last", "random", "random", "last")
SC_LG = 2
SC_AUTH = [(0, 1, [1]), (3, 0, [2])]  # resource 0: black list {1}; resource 3: white list {2}


class _ArgPool:
    """The argument pool of the chain's ext records: one VALUE argument per entry; it only grows, so every batch's
    exits find their entries' records."""

    def __init__(self):
        self.args = [(0, 0, abi.ARG_NULL, 0)]
        self.values = [0]

    def ext(self, rng, ent, sets, rejected=None, junk=None):
        """ext records for the entries: argument 0 drawn from the entry's resource's set — from `junk` for the
        entries in `rejected` — and a few entries without arguments."""
        n = len(ent)
        ext = np.zeros(n, abi.SLOT_EXT_DTYPE)
        res = ent["resource"] & np.uint32(0x7FFFFFFF)
        for i in range(n):
            if rng.random() < 0.04:
                ext[i]["args_null"] = 1
                continue
            s = junk[res[i]] if rejected is not None and rejected[i] else sets[res[i]]
            ext[i]["arg_begin"], ext[i]["arg_count"] = len(self.args), 1
            self.args.append((len(self.values), 1, abi.ARG_VALUE, 0))
            self.values.append(s[int(rng.integers(0, len(s)))])
        return ext

    def arrays(self):
        return np.array(self.args, abi.PSLOT_ARG_DTYPE), np.array(self.values, np.uint64)


@functools.lru_cache(maxsize=None)
def _chain_case():
    from types import SimpleNamespace
    from tests.test_authority_kat import AuthChecker
    from tests.test_oracle_pslot_kat import rule as prule
    from tests.test_slot_chain_gpu import _entries
    rng = np.random.default_rng(500)
    n_res, n_origins, n = len(SC_KIND), 2, 7000
    base = np.array([local_rule() for _ in range(n_res)], abi.LOCAL_RULE_DTYPE)
    frules = np.array([local_flow_rule(r, c) for r, c in enumerate([15.0, 6.0, 50.0, 10.0, 25.0, 8.0])],
                      abi.LOCAL_FLOW_RULE_DTYPE)
    params = np.array([prule(res=0, idx=0, count=8.0), prule(res=1, idx=0, count=5.0, dur=2),
                       prule(res=2, idx=0, count=20.0, behavior=abi.BEHAVIOR_RATE_LIMITER, max_q=50),
                       prule(res=3, idx=0, count=6.0), prule(res=4, idx=0, count=12.0), prule(res=5, idx=0, count=4.0)],
                      abi.PSLOT_RULE_DTYPE)
    params["rule"]["capacity_log2"] = SC_LG
    params["rule"]["burst"][3] = 3
    chk = AuthChecker(base, frules, params, SC_AUTH, n_res, n_origins, 0)
    taken = [[] for _ in range(n_res)]

    def fresh(k):
        out = []
        for r in range(n_res):
            out.append(_value_set(rng, SC_KIND[r], SC_LG, k, taken[r]))
            taken[r] += out[-1]
        return out

    first = [s + [MARKER] for s in fresh((1 << SC_LG) - 1)]
    flood, last, junk = fresh(1 << SC_LG), fresh(1), fresh(6)
    full = [a + b for a, b in zip(first, last)]
    pool = _ArgPool()
    t = T0 + 60_000 + int(rng.integers(0, 1000))
    batches, seen = [], set()

    def step(sets, span):
        nonlocal t
        ent = _entries(rng, n, n_res, t, span, n_origins, zipf=0.4, prio=0.0)
        rej = chk.rejected(ent)
        ext = pool.ext(rng, ent, sets, rej, junk)
        args, values = pool.arrays()
        ev, xo, want, k = chk.batch(ent, ext, rng.integers(0, 41, n).astype(np.int32),
                                    (rng.random(n) < 0.05).astype(np.uint8), t + span, args, values)
        assert k > 100 and len(ev) <= N  # entries the authority rules reject, all carrying junk values
        used = {(int(r), int(values[args["value_begin"][x["arg_begin"]]])) for r, x in
                zip(ent["resource"][~rej] & np.uint32(0x7FFFFFFF), ext[~rej]) if not x["args_null"]}
        assert used == {(r, v) for r in range(n_res) for v in sets[r]}  # every value of every rule
        seen.update(want["status"].tolist())
        _frozen(ev, xo, args, values, want)
        batches.append((ev, xo, args, values, want))
        t += span

    step(first, 2500)
    # the refused batch: entries older than the first batch, every resource with 2^lg new values
    old = _entries(rng, 4000, n_res, T0, 1500, n_origins, zipf=0.4, prio=0.0)
    old_ext = pool.ext(rng, old, flood)
    refused = (old, old_ext) + pool.arrays()
    _frozen(*refused)
    step(full, 2000)
    step(full, 2800)
    assert {abi.LOCAL_PASS, abi.LOCAL_BLOCK_FLOW, abi.LOCAL_BLOCK_PARAM, abi.LOCAL_BLOCK_AUTHORITY} <= seen
    probe = SimpleNamespace(values=sorted({v for r in range(n_res) for v in full[r] + flood[r][:2] + junk[r][:2]}))
    return base, frules, params, chk, batches, refused, probe


@pytest.mark.parametrize("flags", WALKERS)
def test_slot_chain_param_tables_exactly_full(flags):
    """Case 7: resources with one QPS param rule of 4 slots. k_local_prep looks every entry's value up before the
    batch's verdict: a batch refused for its timestamps gives the claimed slots back, and the entries AuthoritySlot
    rejects (they carry values no other entry has) never claim one — the next batch fills every rule to exactly full,
    the marker value among the arguments."""
    from tests.test_authority_gpu import _check_batches, _check_state
    from tests.test_authority_kat import to_abi
    base, frules, params, chk, batches, refused, probe = _chain_case()
    eng = _engine(flags)
    eng.local_load_rules(base, 2, 1000, 500)
    assert eng.local_load_flow_rules(frules, 2, 0) == chk.kept
    eng.pslot_load_rules(params, n_resources=len(base))
    rules, ids = to_abi(SC_AUTH)
    assert eng.local_load_authority_rules(rules, ids, 2) == len(SC_AUTH)
    _check_batches(eng, batches[:1])
    assert _code(eng.slot_decide_host, *refused) == abi.SG_E_TIME
    _check_batches(eng, batches[1:])
    _check_state(eng, chk, len(base), 2, 0, probe)


# ------------------------------------------------------------------------------------------------ sg_pslot_*

def _ps_batch(rng, sets, n, t, span, n_args=1, coll=0.25):
    """n entries over the resources' value sets: every argument a value, a collection of 1 to 3 values (`coll` of
    them) or null."""
    ev = np.zeros(n, abi.PSLOT_EVENT_DTYPE)
    ev["ts_ms"] = t + np.sort(rng.integers(0, span, n))
    ev["resource"] = rng.integers(0, len(sets), n)
    ev["count"] = rng.integers(1, 3, n)
    ev["kind"] = abi.LOCAL_ENTRY
    args, vals = [], []
    for i in range(n):
        s = sets[ev["resource"][i]]
        ev[i]["arg_begin"], ev[i]["arg_count"] = len(args), n_args
        for _ in range(n_args):
            u = rng.random()
            m = int(rng.integers(1, 4)) if u < coll else 1
            if coll <= u < coll + 0.04:
                args.append((0, 0, abi.ARG_NULL, 0))
                continue
            args.append((len(vals), m, abi.ARG_COLLECTION if u < coll else abi.ARG_VALUE, 0))
            vals += [s[int(j)] for j in rng.integers(0, len(s), m)]
    args, vals = np.array(args, abi.PSLOT_ARG_DTYPE), np.array(vals, np.uint64)
    assert set(vals.tolist()) == {v for s in sets for v in s}
    _frozen(ev, args, vals)
    return ev, args, vals


def _ps_rules(n_res, lg, idxs=(0,)):
    out = []
    for res in range(n_res):
        for idx in idxs:
            r = np.zeros((), abi.PSLOT_RULE_DTYPE)
            r["resource"], r["grade"], r["param_idx"] = res, 1, idx
            r["rule"]["count"] = [20.0, 8.0, 30.0, 12.0][res % 4]
            r["rule"]["duration_sec"] = 1 + res % 2
            r["rule"]["burst"] = 2 * (res % 2)
            r["rule"]["behavior"] = abi.BEHAVIOR_RATE_LIMITER if res % 4 == 2 else abi.BEHAVIOR_DEFAULT
            r["rule"]["max_queueing_ms"] = 60
            r["rule"]["capacity_log2"] = lg
            out.append(r)
    return np.array(out, abi.PSLOT_RULE_DTYPE)


def _ps_step(ora, batch):
    want = ora.decide(*batch)
    assert set(want["pass"].tolist()) == {0, 1}  # the premise
    want.setflags(write=False)
    return batch + (want,)


def _ps_check(eng, step, what):
    ev, args, vals, want = step
    _same(eng.pslot_decide_host(ev, args, vals), want, what)


def _ps_states(eng, ora, n_rules, values):
    for ri in range(n_rules):
        for v in values:
            f, lt, tk = ora.token_state(ri, v)
            gf, glt, gtk = eng.param_state(ri, v)
            assert (gf, glt if f & 1 else 0, gtk if f & 2 else 0) == (f, lt if f & 1 else 0, tk if f & 2 else 0), \
                f"token state of rule {ri} value {v:#x}"


@functools.lru_cache(maxsize=None)
def _pslot_case():
    rng = np.random.default_rng(600)
    n_res, lg, n = 4, 2, 8000
    kinds = ("last", "zero", "random", "last")
    rules = _ps_rules(n_res, lg)
    taken = [[] for _ in range(n_res)]

    def fresh(k):
        out = []
        for r in range(n_res):
            out.append(_value_set(rng, kinds[r], lg, k, taken[r]))
            taken[r] += out[-1]
        return out

    first = [s + [MARKER] for s in fresh((1 << lg) - 1)]
    flood, last = fresh(1 << lg), fresh(1)
    full = [a + b for a, b in zip(first, last)]
    ora = ParamFlowSlot(rules, n_resources=n_res)
    a = _ps_step(ora, _ps_batch(rng, first, n, T0 + 70_000, 2400))
    refused = _ps_batch(rng, flood, 4000, T0, 1500)
    t = int(a[0]["ts_ms"][-1])
    b = _ps_step(ora, _ps_batch(rng, full, n, t, 1800))
    c = _ps_step(ora, _ps_batch(rng, full, n, int(b[0]["ts_ms"][-1]) + 5, 2700))
    assert (c[1]["kind"] == abi.ARG_COLLECTION).any()
    probe = sorted({v for r in range(n_res) for v in full[r] + flood[r]})
    return rules, ora, a, refused, b, c, probe


def test_pslot_tables_exactly_full():
    """Case 8: the ParamFlowSlot batch finds or inserts its values inside the walker (ps_single), so a batch refused
    in validation has claimed nothing; values, collections and the marker value at exactly full. One variant: this
    path has a single walker (k_pswalk, one lane per resource) and reads none of the walker flags."""
    rules, ora, a, refused, b, c, probe = _pslot_case()
    eng = _engine()
    eng.pslot_load_rules(rules, n_resources=4)
    _ps_check(eng, a, "first batch")
    assert _code(eng.pslot_decide_host, *refused) == abi.SG_E_TIME
    _ps_check(eng, b, "the batch that fills the tables")
    _ps_check(eng, c, "last batch")
    _ps_states(eng, ora, len(rules), probe)


# ------------------------------------------------------------------------------------------------ the node handle

@functools.lru_cache(maxsize=None)
def _node_case():
    rng = np.random.default_rng(700)
    lg, R = 2, 6
    rules = _cp_rules(rng.integers(20, 200, R))
    taken = [[] for _ in range(R)]

    def fresh(k):
        out = []
        for r in range(R):
            out.append(_value_set(rng, CP_KIND[r % 3], lg, k, taken[r]))
            taken[r] += out[-1]
        return out

    first = [s + [MARKER] for s in fresh((1 << lg) - 1)]
    flood, last = fresh(1 << lg), fresh(1)
    full = [a + b for a, b in zip(first, last)]
    known = [(r, v) for r in range(R) for v in first[r]]
    fknown = [(r, v) for r in range(R) for v in full[r]]
    ora = ClusterTokenService()
    ora.set_namespaces(_ns())
    ora.load_param_rules(rules)
    a = _cp_step(ora, rng, first, known, T0 + 80_000, 2000, 0.3, rules)
    bad = _cp_batch(rng, [x + y for x, y in zip(first, flood)], 8000, T0, 1500)
    _frozen(*bad)
    b = _cp_step(ora, rng, full, fknown, a[3] + 1, 1700, 0.3, rules)
    c = _cp_step(ora, rng, full, fknown, b[3], 2600, 0.3, rules)
    gone = [(r, v) for r in range(R) for v in flood[r]]
    return lg, rules, a, bad, gone, b, c


@pytest.mark.parametrize("flags", WALKERS)
def test_node_cparam_tables_exactly_full(flags):
    """Case 9: two shards on one device, every rule with at most 4 ordinary values and the marker; each shard's batch
    takes its walker from the node's flags. The node's front refuses a batch out of time order before any shard sees
    it, so no shard's table loses a slot."""
    from sentinel_amd.engine import NodeEngine
    lg, rules, a, bad, gone, b, c = _node_case()
    node = NodeEngine([0, 0], max_batch=MAX_BATCH, flags=flags)
    node.set_namespaces(_ns())
    node.cparam_load_rules(rules, None, lg)
    _cp_check(node, a, "first batch")
    assert _code(node.cparam_decide_host, *bad) == abi.SG_E_TIME
    _cp_sums(node, a, "after the refusal")
    for r, v in gone:
        assert node.cparam_sum(r, v, a[3]) == 0
    _cp_check(node, b, "the batch that fills the tables")
    _cp_check(node, c, "last batch")


# ------------------------------------------------------------------------------------------------ full inside a walker

def test_table_full_inside_the_pslot_walker():
    """Case 10, ps_single: a resource with two param rules, and one with a collection argument, meet more distinct
    values than a 2-slot table holds while the walker is already changing state. The batch may be partly applied;
    pinned are the return code, that the handle goes on deciding, and that rules reloaded with more room give a
    fresh trace the fresh oracle's answers."""
    rng = np.random.default_rng(800)
    small, roomy = _ps_rules(2, 1, idxs=(0, 1)), _ps_rules(2, 4, idxs=(0, 1))
    two = [random_values(rng, 2) for _ in range(2)]
    three = [s + random_values(rng, 1, s) for s in two]
    eng = _engine()
    eng.pslot_load_rules(small, n_resources=2)
    ora = ParamFlowSlot(small, n_resources=2)
    _ps_check(eng, _ps_step(ora, _ps_batch(rng, two, 3000, T0, 1500, n_args=2, coll=0.0)), "two values per rule")
    for coll in (0.0, 0.5):  # the third value as a plain argument of two rules, and inside collections
        over = _ps_batch(rng, three, 3000, T0 + 2000, 1500, n_args=2, coll=coll)
        assert _code(eng.pslot_decide_host, *over) == abi.SG_E_CAPACITY
    ev, args, vals = _ps_batch(rng, two, 3000, T0 + 4000, 1500, n_args=2, coll=0.3)
    assert len(eng.pslot_decide_host(ev, args, vals)) == len(ev)  # still deciding
    eng.pslot_load_rules(roomy, n_resources=2)
    ora = ParamFlowSlot(roomy, n_resources=2)
    t = T0 + 10_000
    for b in range(2):
        step = _ps_step(ora, _ps_batch(rng, three, 6000, t, 2000, n_args=2, coll=0.3))
        _ps_check(eng, step, f"fresh batch {b}")
        t = int(step[0]["ts_ms"][-1])
    _ps_states(eng, ora, len(roomy), sorted({v for s in three for v in s}))


def test_table_full_inside_the_embedded_token_server():
    """Case 10, the embedded token server: a cluster-mode param rule's tokens come from this handle's cluster param
    table, whose values are inserted as the walker adds to them. Return code, the handle stays usable, and a reload
    with more room gives a fresh trace the fresh oracles' answers and window sums."""
    rng = np.random.default_rng(810)
    rules = _ps_rules(2, 4)
    rules["cluster_mode"], rules["cluster_key"] = abi.CLUSTER_MODE_FALLBACK, [0, 1]
    two = [random_values(rng, 2) for _ in range(2)]
    three = [s + random_values(rng, 1, s) for s in two]

    def server(flow_id0):
        cp = _cp_rules([40.0, 25.0], flow_id0=flow_id0)
        cts = ClusterTokenService()
        cts.set_namespaces(_ns())
        cts.load_param_rules(cp)
        ora = ParamFlowSlot(rules, n_resources=2)
        ora.attach_cluster(cts, abi.CLUSTER_SERVER)
        return cp, cts, ora

    cp, cts, ora = server(7)
    eng = _engine()
    eng.set_namespaces(_ns())
    eng.cparam_load_rules(cp, None, 1)
    eng.local_set_cluster_state(abi.CLUSTER_SERVER)
    eng.pslot_load_rules(rules, n_resources=2)
    _ps_check(eng, _ps_step(ora, _ps_batch(rng, two, 3000, T0, 1500)), "two values per rule")
    assert _code(eng.pslot_decide_host, *_ps_batch(rng, three, 3000, T0 + 2000, 1500)) == abi.SG_E_CAPACITY
    ev, args, vals = _ps_batch(rng, two, 3000, T0 + 4000, 1500)
    assert len(eng.pslot_decide_host(ev, args, vals)) == len(ev)  # still deciding
    cp, cts, ora = server(1000)  # new flowIds: fresh metrics, in tables of 16 slots
    eng.cparam_load_rules(cp, None, 4)
    eng.pslot_load_rules(rules, n_resources=2)
    t = T0 + 10_000
    for b in range(2):
        step = _ps_step(ora, _ps_batch(rng, three, 6000, t, 2000))
        _ps_check(eng, step, f"fresh batch {b}")
        t = int(step[0]["ts_ms"][-1])
    for k in range(2):
        for v in three[k]:
            assert eng.cparam_sum(k, v, t) == cts.param_sum(k, v, t), f"cluster param sum of rule {k} value {v:#x}"
