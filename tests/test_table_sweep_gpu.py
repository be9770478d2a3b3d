"""Idle values swept out of the exact value tables (sg_param_sweep, sg_cparam_sweep and their node forms).

The oracles (ParamFlowChecker, ParamFlowSlot, ClusterTokenService, LocalChain) are never swept: each replays the whole
accepted history. A swept handle must decide every later batch exactly as they do. Which entries a sweep removes is
computed here from oracle state by a Python restatement of sentinel_amd/csrc/table_sweep.h (_token_idle, _ring_verdict);
every case first asserts on the CPU that its inputs give removable and kept values, so a sweep that removes nothing
cannot pass. Sub-tables hold 2 to 16 slots and a batch at most 20,000 requests; builders are those of
tests/test_value_tables_gpu.py. Every reference is computed once per case, shared by the walker variants, and never
modified.

The thread-count table has a fixed 2^20 slots: test_thread_count_table_full_then_swept fills it exactly, through
16,384 resources whose lanes insert in parallel."""
import functools

import numpy as np
import pytest

from oracle.binding import ClusterTokenService, ParamFlowChecker, ParamFlowSlot, local_flow_rule, local_rule
from sentinel_amd import abi
from tests import test_value_tables_gpu as vt
from tests.value_tables import MARKER, home, random_values

pytestmark = pytest.mark.gpu

WALKERS = vt.WALKERS
T0 = vt.T0
N = vt.N


# ------------------------------------------------------------------------------------------------ the restatement

def _token_idle(state, behavior, tc, burst, dur_ms, now):
    """table_sweep.h sweep_token_idle for a state (flags, time, tokens) of the oracle; throttle is never idle."""
    flags, time, tokens = state
    if behavior == abi.BEHAVIOR_RATE_LIMITER or flags != 3 or tc <= 0:
        return False
    pt = now - time
    if pt <= dur_ms or pt * tc >= 1 << 63:
        return False
    return pt * tc // dur_ms + tokens > tc + burst


def _rule_idle(rule, state, now):
    return _token_idle(state, int(rule["behavior"]), int(rule["count"]), int(rule["burst"]),
                       int(rule["duration_sec"]) * 1000, now)


def _stats(removed=0, claims=0, threads=0, kept=0):
    return {"values_removed": removed, "claims_dropped": claims, "threads_removed": threads, "values_kept": kept}


def _used(eng, n_rules, cparam=False):
    return [(eng.cparam_table_used(r) if cparam else eng.param_table_used(r)) for r in range(n_rules)]


# ------------------------------------------------------------------------------------------------ sg_param_sweep

S_LG = (3, 4, 3)   # token bucket, token bucket with burst, throttle: 8, 16 and 8 slots


def _sweep_rules():
    r = vt._param_rules()
    r["capacity_log2"] = S_LG
    return r


def _split(rules, ora, pairs, now):
    """The known pairs → (removed, kept) by the restatement over the oracle's state."""
    gone = [p for p in pairs if _rule_idle(rules[p[0]], ora.state(*p), now)]
    return gone, [p for p in pairs if p not in gone]


@functools.lru_cache(maxsize=None)
def _param_sweep_case(kind):
    """Per rule 3 cold and 3 hot values ('last': all homed at the sub-table's last slot, the cold ones inserted first,
    so the kept ones sit behind them in one wrapped chain). The marker is cold for rule 0 (an idle side slot) and hot
    for rules 1 and 2 (kept side slots). Batch 0 names the cold pairs, batch 1 the hot ones for more than two
    durations; the sweep comes at batch 1's last timestamp; batches 2 and 3 mix removed, kept and new values."""
    rng = np.random.default_rng(2101 + (kind == "last"))
    rules = _sweep_rules()
    sets = [vt._value_set(rng, kind, S_LG[r], 6) for r in range(3)]
    if kind == "last":
        assert all(home(v, (1 << S_LG[r]) - 1) == (1 << S_LG[r]) - 1 for r in range(3) for v in sets[r])
    cold = [(r, v) for r in range(3) for v in sets[r][:3]] + [(0, MARKER)]
    hot = [(r, v) for r in range(3) for v in sets[r][3:]] + [(1, MARKER), (2, MARKER)]
    known = cold + hot
    new = [(r, v) for r in range(3) for v in vt._value_set(rng, kind, S_LG[r], 2, sets[r])]
    ora = ParamFlowChecker()
    ora.load_rules(rules)
    a = vt._param_step(ora, rng, cold, cold, T0 + 13, 2300)
    b = vt._param_step(ora, rng, hot, known, int(a[0]["ts_ms"][-1]) + 1, 2600)
    now = int(b[0]["ts_ms"][-1])
    gone, kept = _split(rules, ora, known, now)
    for r in (0, 1):   # the premise: every token-bucket rule has something to remove and something to keep
        assert any(p[0] == r for p in gone) and any(p[0] == r for p in kept), f"rule {r}"
    assert all(p[0] != 2 for p in gone) and (0, MARKER) in gone and (1, MARKER) in kept
    if kind == "last":
        assert {p for p in cold if p[0] != 2} <= set(gone)   # the first-inserted half of each chain
    kept_states = {p: b[2][p] for p in kept}
    later = known + new
    c = vt._param_step(ora, rng, later, later, now, 1900)
    d = vt._param_step(ora, rng, later, later, int(c[0]["ts_ms"][-1]) + 700, 2200)
    return rules, a, b, now, gone, kept, kept_states, c, d


@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("kind", ["random", "last"])
def test_param_sweep_is_invisible(kind, flags):
    """Cases 1 and 3: token bucket, token bucket with burst and throttle; half the values idle at the sweep. The stats
    and the used counts are the restatement's, a removed value reads absent and a kept one as the oracle has it
    (tokens intact, also behind the removed head of a wrapped probe chain), the side slot once idle and once kept,
    every throttle value kept — and every decision of the two later batches is the oracle's, which was never swept."""
    rules, a, b, now, gone, kept, kept_states, c, d = _param_sweep_case(kind)
    eng = vt._engine(flags)
    eng.param_load_rules(rules)
    vt._param_check(eng, a, "batch 0")
    vt._param_check(eng, b, "batch 1")
    before = _used(eng, 3)
    assert [u[:2] for u in before] == [(6, 6)] * 3
    n_gone = [sum(1 for r, v in gone if r == k and v != MARKER) for k in range(3)]
    got = eng.param_sweep(now)
    assert got == _stats(removed=sum(n_gone), kept=18 - sum(n_gone)), got
    assert n_gone[2] == 0
    assert _used(eng, 3) == [(u - g, l - g, c) for (u, l, c), g in zip(before, n_gone)]
    for p in gone:
        assert eng.param_state(*p)[0] == 0, f"removed rule {p[0]} value {p[1]:#x}"
    vt._param_states(eng, kept_states, "after the sweep")
    assert eng.param_sweep(now) == _stats(kept=18 - sum(n_gone))   # nothing more to give back
    vt._param_check(eng, c, "batch 2")
    vt._param_check(eng, d, "batch 3")


@functools.lru_cache(maxsize=None)
def _param_capacity_case():
    """Rules of 2, 16 and 4 slots exactly full. `early`: one more value per token-bucket rule right after the filling
    batch, when nothing is idle. Then a batch over half the values for more than two durations, and `over`: that half
    and one more value per token-bucket rule at its end."""
    rng = np.random.default_rng(2103)
    rules = vt._param_rules()
    lg = vt.P_LG
    sets = [vt._value_set(rng, vt.P_KIND[r], lg[r], 1 << lg[r]) for r in range(3)]
    pairs = [(r, v) for r in range(3) for v in sets[r] + [MARKER]]
    hot = [(r, v) for r in range(3) for v in sets[r][(1 << lg[r]) // 2:] + [MARKER]]
    extra = [(r, vt._value_set(rng, vt.P_KIND[r], lg[r], 1, sets[r])[0]) for r in (0, 1)]
    ora = ParamFlowChecker()
    ora.load_rules(rules)
    a = vt._param_step(ora, rng, pairs, pairs, T0 + 17, 2400)
    t_a = int(a[0]["ts_ms"][-1])
    assert _split(rules, ora, pairs, t_a)[0] == []            # the premise of the early sweep: nothing is idle
    early = vt._param_batch(rng, pairs + extra, 4000, t_a, 300)
    vt._frozen(early)
    b = vt._param_step(ora, rng, hot, pairs, t_a + 1, 2600)
    now = int(b[0]["ts_ms"][-1])
    gone, kept = _split(rules, ora, pairs, now)
    for r in (0, 1):
        assert any(p[0] == r and p[1] != MARKER for p in gone) and any(p[0] == r and p[1] != MARKER for p in kept), f"rule {r}"
    assert set(gone).isdisjoint(hot)
    later = hot + extra   # the values the sweep keeps and one new value per token-bucket rule
    over = vt._param_step(ora, rng, later, later, now, 1800)
    return rules, a, t_a, early, b, now, gone, over


@pytest.mark.parametrize("flags", WALKERS)
def test_param_sweep_gives_capacity_back(flags):
    """Case 2: a full rule refuses one value too many; a sweep at a time when nothing is idle removes nothing and the
    batch is refused again; after time has passed the sweep gives slots back and the batch that was refused is
    accepted, equal to the oracle."""
    rules, a, t_a, early, b, now, gone, over = _param_capacity_case()
    eng = vt._engine(flags)
    eng.param_load_rules(rules)
    vt._param_check(eng, a, "the filling batch")
    full = _used(eng, 3)
    assert [u[0] for u in full] == [1 << lg for lg in vt.P_LG]
    assert vt._code(eng.param_decide_host, early) == abi.SG_E_CAPACITY
    vt._param_states(eng, a[2], "after the refusal")
    assert eng.param_sweep(t_a) == _stats(kept=sum(1 << lg for lg in vt.P_LG))
    assert _used(eng, 3) == full
    assert vt._code(eng.param_decide_host, early) == abi.SG_E_CAPACITY
    vt._param_check(eng, b, "the batch over half the values")
    assert vt._code(eng.param_decide_host, over[0]) == abi.SG_E_CAPACITY
    vt._param_states(eng, b[2], "after the second refusal")
    assert _used(eng, 3) == full
    n_gone = [sum(1 for r, v in gone if r == k and v != MARKER) for k in range(3)]
    got = eng.param_sweep(now)
    assert got == _stats(removed=sum(n_gone), kept=sum(u[0] for u in full) - sum(n_gone)), got
    assert [u[0] for u in _used(eng, 3)] == [u[0] - g for u, g in zip(full, n_gone)]
    vt._param_check(eng, over, "the refused batch, after the sweep")


@pytest.mark.parametrize("flags", WALKERS)
def test_sweep_time_order(flags):
    """Case 6: a sweep before the last batch's last timestamp is SG_E_TIME and sweeps nothing; after a sweep at now_ms
    a batch that starts at now_ms - 1 is SG_E_TIME and one at now_ms is accepted. Both kinds of table."""
    rules, a, b, now, gone, kept, kept_states, c, d = _param_sweep_case("random")
    fresh = vt._engine(flags)
    assert vt._code(fresh.param_sweep, now) == abi.SG_E_INVAL       # before a load
    assert vt._code(fresh.cparam_sweep, now) == abi.SG_E_INVAL
    eng = vt._engine(flags)
    eng.param_load_rules(rules)
    vt._param_check(eng, a, "batch 0")
    vt._param_check(eng, b, "batch 1")
    before = _used(eng, 3)
    assert vt._code(eng.param_sweep, now - 1) == abi.SG_E_TIME
    assert vt._code(eng.param_sweep, -1) == abi.SG_E_TIME
    assert _used(eng, 3) == before
    vt._param_states(eng, b[2], "after the refused sweeps")
    assert eng.param_sweep(now)["values_removed"] > 0
    early = c[0].copy()
    early["ts_ms"] -= 1                                              # starts at now - 1
    assert vt._code(eng.param_decide_host, early) == abi.SG_E_TIME
    vt._param_check(eng, c, "a batch that starts at now_ms")

    S = 10
    cr, ns, ca, cb, cnow, want, known_sums, top, cc, cd, new, kept_sums, ce = _cp_sweep_case(S)
    eng = vt._engine(flags)
    eng.set_namespaces(ns)
    eng.cparam_load_rules(cr, None, CP_LG)
    for step in (ca, cb):
        vt._same(eng.cparam_decide_host(step[0], step[1]), step[2], "a filling batch")
    before = _used(eng, 3, True)
    assert vt._code(eng.cparam_sweep, int(cb[0]["ts_ms"][-1]) - 1) == abi.SG_E_TIME
    assert _used(eng, 3, True) == before
    assert eng.cparam_sweep(cnow)["values_removed"] > 0
    early = cc[0].copy()
    early["ts_ms"] -= int(early["ts_ms"][0]) - cnow + 1              # starts at now - 1
    assert vt._code(eng.cparam_decide_host, early, cc[1]) == abi.SG_E_TIME
    vt._cp_check(eng, cc, "a batch that starts at or after now_ms", CP_LG)


def test_sweep_with_local_tickets_outstanding():
    """Case 7, ordering: sg_param_sweep drains the pipeline before it reads the tables. Tickets issued before it
    complete with their own answers, and the batch enqueued after it decides on."""
    from tests.test_local_pipeline_gpu import _check, _compare, _enqueue_all, _results, _rules, _trace
    rng = np.random.default_rng(2107)
    lrules = _rules(12, rng, lo=3, hi=30)
    trace, ora = _trace(lrules, [(9_000, 600), (9_000, 600), (9_000, 600)], 2, 1000, 500, seed=2107)
    rules, a, b, now, gone, kept, kept_states, c, d = _param_sweep_case("random")
    eng = vt._engine()
    eng.local_load_rules(lrules, 2, 1000, 500)
    eng.param_load_rules(rules)
    vt._param_check(eng, a, "batch 0")
    vt._param_check(eng, b, "batch 1")
    bufs = _enqueue_all(eng, [trace[0][0], trace[1][0]])
    assert eng.param_sweep(now)["values_removed"] == sum(1 for _, v in gone if v != MARKER)
    bufs += _enqueue_all(eng, [trace[2][0]])
    for k, (_, d_out, ticket) in enumerate(bufs):
        eng.local_wait(ticket)
        _check(_results(d_out), trace[k][1], k)
    _compare(eng, ora, len(lrules), 2)
    vt._param_check(eng, c, "the param batch after the sweep")


# ------------------------------------------------------------------------------------------------ sg_cparam_sweep

CP_LG = 4


def _cp_merge(req, vals, extra):
    """The batch with the crafted single-value requests `extra` [(ts, rule, value, acquire)] merged in by time."""
    rows = [(int(q["ts_ms"]), int(q["key"]), int(q["acquire"]), [int(x) for x in vals[q["value_begin"]:q["value_begin"] + q["value_count"]]])
            for q in req]
    rows += [(ts, r, acq, [v]) for ts, r, v, acq in extra]
    rows.sort(key=lambda x: x[0])
    out = np.zeros(len(rows), abi.CPARAM_REQ_DTYPE)
    out["ts_ms"] = [x[0] for x in rows]
    out["key"] = [x[1] for x in rows]
    out["acquire"] = [x[2] for x in rows]
    out["value_count"] = [len(x[3]) for x in rows]
    out["value_begin"] = np.concatenate([[0], np.cumsum(out["value_count"])[:-1]]).astype(np.uint32)
    return out, np.array([v for x in rows for v in x[3]], np.uint64)


def _ring_history(rules, hist, steps):
    """hist[(rule, value)] = the latest window start at which a request with the value reached the metric (None: asked,
    but only by requests the namespace limiter turned away, so the slot was claimed and no bucket written), over the
    steps' requests and the oracle's results. Like the reference's getAvg → currentWindow, the walker opens the window
    of every request it checks, passed or blocked; every other written bucket of the ring is older."""
    for req, vals, want in steps:
        for q, w in zip(req, want):
            r, wl = int(q["key"]), int(rules["window_interval_ms"][q["key"]]) // int(rules["sample_count"][q["key"]])
            for v in vals[q["value_begin"]:q["value_begin"] + q["value_count"]]:
                p = (r, int(v))
                hist.setdefault(p, None)
                if w["status"] in (abi.OK, abi.BLOCKED):
                    start = int(q["ts_ms"]) - int(q["ts_ms"]) % wl
                    hist[p] = start if hist[p] is None else max(hist[p], start)
    return hist


def _ring_verdict(rules, p, start, now):
    """table_sweep.h sweep_ring over the latest written bucket (every other written bucket is older)."""
    if start is None:
        return "claim"
    return "idle" if now - start > int(rules["window_interval_ms"][p[0]]) else "keep"


def _cp_want(rules, hist, now):
    v = {p: _ring_verdict(rules, p, s, now) for p, s in hist.items()}
    per_rule = [{k: sum(1 for p, x in v.items() if p[0] == r and p[1] != MARKER and x == k) for k in ("idle", "claim", "keep")}
                for r in range(len(rules))]
    return v, per_rule


@functools.lru_cache(maxsize=None)
def _cp_sweep_case(S, lim=True):
    """Rules 0 and 1: S buckets over 1000 ms; rule 2: S buckets over 1000 + S ms, so that one sweep time meets both
    boundaries: rule 0's value X was last added in the bucket that starts at now - 1000 (now - start == interval:
    kept), rule 2's value Y in the one that starts at now - (1000 + S) - 1 (interval + 1: removed). X2 / Y2 lie one
    bucket further out / in. DEAD is only ever asked for more than rule 0 allows: a ring whose one bucket counts 0, as
    removable as any. With `lim` the namespace has a QPS limiter and CLAIM is named only by requests it turns away: a
    claimed slot with no bucket. Cold values are named by batch 0 alone (every ring deprecated by now), hot ones up
    to the sweep (a live bucket)."""
    rng = np.random.default_rng(2200 + S)
    wl0, wl2 = 1000 // S, 1000 // S + 1
    rules = vt._cp_rules(rng.integers(40, 200, 3), S=S)
    rules["window_interval_ms"] = [1000, 1000, 1000 + S]
    ns = vt._ns(6000.0 if lim else 0.0)   # batch 0 arrives at 8000 requests a second
    now = (T0 + 30_000) // wl0 * wl0
    while (now - (1000 + S) - 1) % wl2:
        now += wl0
    sets = vt._cp_sets(rng, CP_LG, 6, marker=False)
    cold = [s[:3] for s in sets]
    hot = [s[3:] for s in sets]
    cold[0].append(MARKER)   # an idle side slot
    hot[1].append(MARKER)    # a kept one
    x, x2, dead, claim = random_values(rng, 4, sets[0])
    y, y2 = random_values(rng, 2, sets[2])
    s_y = now - (1000 + S) - 1
    extra = [(now - 3000, 0, dead, 1_000_000), (now - 1000 - wl0 + 3, 0, x2, 1), (now - 1000 + 3, 0, x, 1),
             (s_y + 2, 2, y, 1), (s_y + wl2 + 2, 2, y2, 1)]
    ora = ClusterTokenService()
    ora.set_namespaces(ns)
    ora.load_param_rules(rules)
    req, vals = vt._cp_batch(rng, cold, N, now - 7000, 2500, 0.3)
    if lim:   # the limiter's verdicts do not depend on the values: requests it turns away get the value CLAIM
        probe = ClusterTokenService()
        probe.set_namespaces(ns)
        probe.load_param_rules(rules)
        turned = probe.decide_param(req, vals)["status"] == abi.TOO_MANY_REQUEST
        at = np.nonzero((req["key"] == 0) & (req["value_count"] == 1) & turned)[0][:20]
        assert len(at) == 20
        vals[req["value_begin"][at]] = claim
    a = (req, vals, ora.decide_param(req, vals))
    assert not lim or (a[2]["status"][at] == abi.TOO_MANY_REQUEST).all()
    req, vals = vt._cp_batch(rng, hot, N - len(extra), now - 4400, 4400, 0.3)
    req, vals = _cp_merge(req, vals, extra)
    b = (req, vals, ora.decide_param(req, vals))
    vt._frozen(*a, *b)
    assert int(b[0]["ts_ms"][-1]) <= now
    for step in (a, b):
        assert {abi.OK, abi.BLOCKED} <= set(step[2]["status"].tolist())
    hist = _ring_history(rules, {}, [a, b])
    verdict, per_rule = _cp_want(rules, hist, now)
    # the premises: both boundaries, a claim, and per rule something removed and something kept
    assert hist[(0, x)] == now - 1000 and verdict[(0, x)] == "keep"
    assert hist[(2, y)] == now - (1000 + S) - 1 and verdict[(2, y)] == "idle"
    assert verdict[(0, x2)] == "idle" and verdict[(2, y2)] == "keep" and verdict[(0, dead)] == "idle"
    assert not lim or verdict[(0, claim)] == "claim"
    assert verdict[(0, MARKER)] == "idle" and verdict[(1, MARKER)] == "keep"
    assert all(c["idle"] and c["keep"] for c in per_rule), per_rule
    known = sorted(hist)
    known_sums = {p: ora.param_sum(p[0], p[1], now) for p in known}
    for p, vd in verdict.items():   # what the oracle's state says of the same entries
        assert vd == "keep" or known_sums[p] == 0, p
    assert any(vd == "keep" and known_sums[p] > 0 for p, vd in verdict.items())
    top = [{v: known_sums[(r, v)] / (rules["window_interval_ms"][r] / 1000.0) for (rr, v) in known
            if rr == r and known_sums[(r, v)] > 0} for r in range(3)]
    every = [cold[r] + hot[r] + vt._value_set(rng, vt.CP_KIND[r], CP_LG, 2, sets[r] + [x, x2, dead, claim, y, y2]) for r in range(3)]
    every[0] += [x, x2]
    every[2] += [y, y2]
    eknown = [(r, v) for r in range(3) for v in every[r]]
    c = vt._cp_step(ora, rng, every, eknown, now, 1800, 0.3, rules)
    d = vt._cp_step(ora, rng, every, eknown, c[3] + 300, 2100, 0.3, rules)
    # the reload: rule 0 survives as rule 2, rule 2 as rule 0, rule 1's flowId is new
    fresh = vt._cp_rules(rng.integers(40, 200, 1), S=S, flow_id0=3000)
    new = np.concatenate([rules[2:3], fresh, rules[0:1]])
    ora.load_param_rules(new)
    t = d[3] + 1
    kept_sums = {(nr, v): ora.param_sum(nr, v, t) for nr, r in ((0, 2), (2, 0)) for v in every[r]}
    assert sum(s > 0 for s in kept_sums.values()) > 6
    nsets = [every[2], every[1], every[0]]
    e = vt._cp_step(ora, rng, nsets, [(r, v) for r in range(3) for v in nsets[r]], t, 2000, 0.3, new)
    return rules, ns, a, b, now, (verdict, per_rule), known_sums, top, c, d, new, kept_sums, e


def _cp_after_sweep(eng, now, known_sums, top, lg=None):
    for (r, v), s in known_sums.items():
        assert eng.cparam_sum(r, v, now) == s, f"window sum of rule {r} value {v:#x} after the sweep"
    if lg is not None:
        got = eng.cparam_top_values(now, len(top), (1 << lg) + 1)
        assert [dict(g) for g in got] == top, "top values after the sweep"


@pytest.mark.parametrize("flags", WALKERS)
@pytest.mark.parametrize("S", [2, 10])
def test_cparam_sweep_mid_stream(S, flags):
    """Case 4: swept mid-stream with rings fully deprecated, rings with a live bucket, both boundary distances and a
    claimed slot without a bucket. The stats and used counts are the restatement's; window sums, top values and the
    decisions of two later batches are the oracle's; a reload at the same capacity keeps the surviving flowIds."""
    rules, ns, a, b, now, (verdict, per_rule), known_sums, top, c, d, new, kept_sums, e = _cp_sweep_case(S)
    eng = vt._engine(flags)
    eng.set_namespaces(ns)
    eng.cparam_load_rules(rules, None, CP_LG)
    for k, step in enumerate((a, b)):
        vt._same(eng.cparam_decide_host(step[0], step[1]), step[2], f"batch {k}")
    before = _used(eng, 3, True)
    assert [u[:2] for u in before] == [(sum(c.values()), c["idle"] + c["keep"]) for c in per_rule]
    got = eng.cparam_sweep(now)
    assert got == _stats(removed=sum(c["idle"] for c in per_rule), claims=sum(c["claim"] for c in per_rule),
                         kept=sum(c["keep"] for c in per_rule)), got
    assert [u[:2] for u in _used(eng, 3, True)] == [(c["keep"], c["keep"]) for c in per_rule]
    _cp_after_sweep(eng, now, known_sums, top, CP_LG)
    assert eng.cparam_sweep(now) == _stats(kept=sum(c["keep"] for c in per_rule))
    vt._cp_check(eng, c, "batch 2", CP_LG)
    vt._cp_check(eng, d, "batch 3", CP_LG)
    eng.cparam_load_rules(new, None, CP_LG)
    for (r, v), s in kept_sums.items():
        assert eng.cparam_sum(r, v, d[3] + 1) == s, f"survivor's window sum of rule {r} value {v:#x}"
    vt._cp_check(eng, e, "after the reload", CP_LG)


@pytest.mark.parametrize("shards", [2, 3])
def test_node_cparam_sweep(shards):
    """Case 8: the same trace over same-device shards: the stats summed over the owners are the restatement's, and the
    later node batches equal the oracle."""
    from sentinel_amd.engine import NodeEngine
    rules, ns, a, b, now, (verdict, per_rule), known_sums, top, c, d, new, kept_sums, e = _cp_sweep_case(10, False)
    node = NodeEngine([0] * shards, max_batch=vt.MAX_BATCH)
    assert vt._code(node.cparam_sweep, now) == abi.SG_E_INVAL       # before a load
    node.set_namespaces(ns)
    node.cparam_load_rules(rules, None, CP_LG)
    for k, step in enumerate((a, b)):
        vt._same(node.cparam_decide_host(step[0], step[1]), step[2], f"batch {k}")
    assert vt._code(node.cparam_sweep, int(b[0]["ts_ms"][-1]) - 1) == abi.SG_E_TIME
    assert [node.cparam_table_used(r)[:2] for r in range(3)] == [(sum(c.values()), c["idle"] + c["keep"]) for c in per_rule]
    got = node.cparam_sweep(now)
    assert got == _stats(removed=sum(c["idle"] for c in per_rule), claims=sum(c["claim"] for c in per_rule),
                         kept=sum(c["keep"] for c in per_rule)), got
    assert [node.cparam_table_used(r)[:2] for r in range(3)] == [(c["keep"], c["keep"]) for c in per_rule]
    _cp_after_sweep(node, now, known_sums, top)
    early = c[0].copy()
    early["ts_ms"] -= int(early["ts_ms"][0]) - now + 1
    assert vt._code(node.cparam_decide_host, early, c[1]) == abi.SG_E_TIME
    vt._cp_check(node, c, "batch 2")
    vt._cp_check(node, d, "batch 3")


# ------------------------------------------------------------------------------------------------ the slot chain

SC_LG = 3
SC_KIND = ("last", "zero", "last", "random", "random", "last")


@functools.lru_cache(maxsize=None)
def _chain_sweep_case():
    """Six resources with one param rule of 8 slots each — QPS token buckets, a throttle (resource 2) and a THREAD
    rule (resource 5) — and two authority rules. Batch 0 names every value, batch 1 the hot half for more than two
    durations; the sweep comes at batch 1's last event; batches 2 and 3 name every value and new ones. Entries stay
    open for up to 40 ms, so at the sweep some thread counts are back at 0 and some are not."""
    from types import SimpleNamespace
    from tests.test_authority_kat import AuthChecker
    from tests.test_oracle_pslot_kat import rule as prule
    from tests.test_slot_chain_gpu import _entries
    rng = np.random.default_rng(2301)
    n_res, n_origins, n = len(SC_KIND), 2, 7000
    base = np.array([local_rule() for _ in range(n_res)], abi.LOCAL_RULE_DTYPE)
    frules = np.array([local_flow_rule(r, c) for r, c in enumerate([15.0, 6.0, 50.0, 10.0, 25.0, 8.0])],
                      abi.LOCAL_FLOW_RULE_DTYPE)
    params = np.array([prule(res=0, idx=0, count=8.0), prule(res=1, idx=0, count=5.0, dur=2),
                       prule(res=2, idx=0, count=20.0, behavior=abi.BEHAVIOR_RATE_LIMITER, max_q=50),
                       prule(res=3, idx=0, count=6.0), prule(res=4, idx=0, count=12.0),
                       prule(res=5, idx=0, count=2.0, grade=abi.FLOW_GRADE_THREAD)], abi.PSLOT_RULE_DTYPE)
    params["rule"]["capacity_log2"] = SC_LG
    params["rule"]["burst"][3] = 3
    chk = AuthChecker(base, frules, params, vt.SC_AUTH, n_res, n_origins, 0)
    taken = [[] for _ in range(n_res)]

    def fresh(k):
        out = []
        for r in range(n_res):
            out.append(vt._value_set(rng, SC_KIND[r], SC_LG, k, taken[r]))
            taken[r] += out[-1]
        return out

    cold, hot, new, junk = fresh(2), fresh(2), fresh(2), fresh(6)
    hot = [s + [MARKER] for s in hot]
    both = [a + b for a, b in zip(cold, hot)]
    every = [a + b for a, b in zip(both, new)]
    pool = vt._ArgPool()
    t = T0 + 120_000 + int(rng.integers(0, 1000))
    batches, passed, named = [], set(), set()

    def step(sets, span):
        nonlocal t
        ent = _entries(rng, n, n_res, t, span, n_origins, zipf=0.4, prio=0.0)
        rej = chk.rejected(ent)
        ext = pool.ext(rng, ent, sets, rej, junk)
        args, values = pool.arrays()
        ev, xo, want, k = chk.batch(ent, ext, rng.integers(0, 41, n).astype(np.int32),
                                    (rng.random(n) < 0.05).astype(np.uint8), t + span, args, values)
        assert len(ev) <= N
        used = {(int(r), int(values[args["value_begin"][x["arg_begin"]]])) for r, x in
                zip(ent["resource"][~rej] & np.uint32(0x7FFFFFFF), ext[~rej]) if not x["args_null"]}
        assert used == {(r, v) for r in range(n_res) for v in sets[r]}  # every value of every rule
        named.update(used)   # k_local_prep claims a slot for each of them under a QPS rule, before the verdict
        assert abi.LOCAL_BLOCK_PARAM in want["status"] and abi.LOCAL_PASS in want["status"]
        # ParamFlowStatisticEntryCallback: a passed entry with arguments puts (resource, 0, value) in the thread map
        ok = (ev["kind"] == abi.LOCAL_ENTRY) & np.isin(want["status"], (abi.LOCAL_PASS, abi.LOCAL_PASS_WAIT)) & (xo["args_null"] == 0)
        passed.update((int(r) & 0x7FFFFFFF, int(values[args["value_begin"][b]])) for r, b in
                      zip(ev["resource"][ok], xo["arg_begin"][ok]))
        vt._frozen(ev, xo, args, values, want)
        batches.append((ev, xo, args, values, want))
        t += span

    step(both, 2500)
    step(hot, 4600)
    now = int(batches[-1][0]["ts_ms"][-1])
    known = [(r, v) for r in range(n_res) for v in both[r]]
    states = {p: chk.ps.token_state(*p) for p in known}
    gone = [p for p in known if _rule_idle(params["rule"][p[0]], states[p], now)]
    counted = [p for p in known if states[p][0]]
    for r in (0, 1, 3, 4):   # the premise: every token-bucket rule removes and keeps
        assert any(p[0] == r for p in gone) and any(p[0] == r and p not in gone for p in counted), f"rule {r}"
    assert all(p[0] not in (2, 5) for p in gone)
    threads = {p: chk.ps.thread_count(p[0], 0, p[1]) for p in sorted(passed)}
    assert sum(1 for c in threads.values() if c == 0) >= 6 and sum(1 for c in threads.values() if c > 0) >= 3
    # claimed and never counted: named by an entry that reached ParamFlowSlot under a QPS rule, absent from the
    # oracle's maps (an entry's count never exceeds a rule's maxCount here and no tokenCount is 0, so there is none)
    assert set(known) == named
    claims = [p for p in sorted(named) if params["grade"][p[0]] == 1 and not states[p][0]]
    assert claims == []
    want = _stats(removed=sum(1 for p in gone if p[1] != MARKER), claims=sum(1 for p in claims if p[1] != MARKER),
                  threads=sum(1 for c in threads.values() if c == 0),
                  kept=sum(1 for p in counted if p not in gone and p[1] != MARKER))
    plain = [p for p in counted if p[1] != MARKER]
    used = ([sum(1 for p in plain if p[0] == r) for r in range(n_res)],                      # before the sweep
            [sum(1 for p in plain if p[0] == r and p not in gone) for r in range(n_res)])    # after it
    assert used[0][5] == 0   # the THREAD rule keeps no token state
    kept_states = {p: states[p] for p in counted if p not in gone}
    step(every, 2000)
    step(every, 2800)
    probe = SimpleNamespace(values=sorted({v for r in range(n_res) for v in every[r] + junk[r][:2]}))
    return base, frules, params, chk, batches, now, gone, kept_states, threads, want, probe, used


def _chain_states(eng, gone, kept_states, threads):
    for p in gone:
        assert eng.param_state(*p)[0] == 0, f"removed rule {p[0]} value {p[1]:#x}"
    for p, (f, lt, tk) in kept_states.items():
        gf, glt, gtk = eng.param_state(*p)
        assert (gf, glt if f & 1 else 0, gtk if f & 2 else 0) == (f, lt if f & 1 else 0, tk if f & 2 else 0), \
            f"kept rule {p[0]} value {p[1]:#x}"
    for (r, v), c in threads.items():
        assert eng.pslot_thread_count(r, 0, v) == c, f"thread count of resource {r} value {v:#x}"


@pytest.mark.parametrize("flags", WALKERS)
def test_slot_chain_sweep(flags):
    """Case 5: sg_param_sweep between slot-chain batches: token buckets of the cold values and thread counts back at 0
    go, throttle values and open entries' counts stay; threads_removed is exact, and every later result, thread count
    and token state is the oracle's."""
    from tests.test_authority_gpu import _check_batches, _check_state
    from tests.test_authority_kat import to_abi
    base, frules, params, chk, batches, now, gone, kept_states, threads, want, probe, used = _chain_sweep_case()
    n_res = len(base)
    eng = vt._engine(flags)
    eng.local_load_rules(base, 2, 1000, 500)
    assert eng.local_load_flow_rules(frules, 2, 0) == chk.kept
    eng.pslot_load_rules(params, n_resources=n_res)
    rules, ids = to_abi(vt.SC_AUTH)
    assert eng.local_load_authority_rules(rules, ids, 2) == len(vt.SC_AUTH)
    _check_batches(eng, batches[:2])
    assert [u[:2] for u in _used(eng, n_res)] == [(k, k) for k in used[0]]
    assert vt._code(eng.param_sweep, now - 1) == abi.SG_E_TIME
    got = eng.param_sweep(now)
    assert got == want, (got, want)
    assert [u[:2] for u in _used(eng, n_res)] == [(k, k) for k in used[1]]
    _chain_states(eng, gone, kept_states, threads)
    early = batches[2][0].copy()
    early["ts_ms"] -= int(early["ts_ms"][0]) - now + 1
    early["create_ts"] = np.minimum(early["create_ts"], early["ts_ms"])
    assert vt._code(eng.slot_decide_host, early, *batches[2][1:4]) == abi.SG_E_TIME
    _check_batches(eng, batches[2:])
    _check_state(eng, chk, n_res, 2, 0, probe)


@pytest.mark.parametrize("shards", [2, 3])
def test_node_param_sweep(shards):
    """Case 8: the same chain over the node: the front and every shard are swept, the stats summed over the shards
    are the restatement's, and the later node batches, thread counts and token states equal the oracle."""
    from sentinel_amd.engine import NodeEngine
    from tests.test_authority_gpu import _check_batches
    from tests.test_authority_kat import to_abi
    base, frules, params, chk, batches, now, gone, kept_states, threads, want, probe, used = _chain_sweep_case()
    n_res = len(base)
    node = NodeEngine([0] * shards, max_batch=vt.MAX_BATCH)
    node.local_load_rules(base, 2, 1000, 500)
    assert node.local_load_flow_rules(frules, 2, 0) == chk.kept
    assert vt._code(node.param_sweep, now) == abi.SG_E_INVAL         # before the param rules
    node.pslot_load_rules(params, n_resources=n_res)
    rules, ids = to_abi(vt.SC_AUTH)
    assert node.local_load_authority_rules(rules, ids, 2) == len(vt.SC_AUTH)
    _check_batches(node, batches[:2])
    assert vt._code(node.param_sweep, now - 1) == abi.SG_E_TIME
    assert [node.param_table_used(r)[:2] for r in range(n_res)] == [(k, k) for k in used[0]]
    got = node.param_sweep(now)
    assert got == want, (got, want)
    assert [node.param_table_used(r)[:2] for r in range(n_res)] == [(k, k) for k in used[1]]
    _chain_states(node, gone, kept_states, threads)
    _check_batches(node, batches[2:])
    for r in range(n_res):
        for v in probe.values:
            f, lt, tk = chk.ps.token_state(r, v)
            gf, glt, gtk = node.param_state(r, v)
            assert (gf, glt if f & 1 else 0, gtk if f & 2 else 0) == (f, lt if f & 1 else 0, tk if f & 2 else 0), \
                f"token state of rule {r} value {v:#x}"
            assert node.pslot_thread_count(r, 0, v) == chk.ps.thread_count(r, 0, v)


def test_embedded_token_server_sweep():
    """Case 5, SERVER: a cluster-mode param rule's tokens come from this handle's cluster param tables.
    sg_cparam_sweep between batches, after every window has run out, gives every ring back; sg_param_sweep is told
    the same time. The chain goes on equal to the oracles, window sums included."""
    rng = np.random.default_rng(2302)
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
    eng.cparam_load_rules(cp, None, 2)
    eng.local_set_cluster_state(abi.CLUSTER_SERVER)
    eng.pslot_load_rules(rules, n_resources=2)
    a = vt._ps_step(ora, vt._ps_batch(rng, two, 3000, T0, 1500))
    vt._ps_check(eng, a, "two values per rule")
    assert _used(eng, 2, True) == [(2, 2, 4)] * 2
    t = int(a[0]["ts_ms"][-1])
    assert vt._code(eng.cparam_sweep, t - 1) == abi.SG_E_TIME       # the chain's batches stamp the server's time
    mid = t + 200                                                    # inside the window: every ring has a live bucket
    assert all(cts.param_sum(k, v, mid) > 0 for k in range(2) for v in two[k])
    assert eng.cparam_sweep(mid) == _stats(kept=4)
    now = t + 1001                                                   # every bucket started at or before t
    assert eng.cparam_sweep(now) == _stats(removed=4)
    assert _used(eng, 2, True) == [(0, 0, 4)] * 2
    assert eng.param_sweep(now)["threads_removed"] == 0              # entries only: every count is above 0
    early = vt._ps_batch(rng, two, 100, now - 1, 50)
    assert vt._code(eng.pslot_decide_host, *early) == abi.SG_E_TIME
    t = now
    for b in range(2):
        step = vt._ps_step(ora, vt._ps_batch(rng, three, 5000, t, 1200))
        vt._ps_check(eng, step, f"batch {b} after the sweep")
        t = int(step[0]["ts_ms"][-1])
    for k in range(2):
        for v in three[k]:
            assert eng.cparam_sum(k, v, t) == cts.param_sum(k, v, t)


def test_slot_chain_embedded_server_sweep():
    """Case 5, SERVER, through the slot chain: cluster-mode param rules inside sg_slot_decide_batch take their tokens
    from this handle's cluster param tables and stamp their time. sg_cparam_sweep before the chain's last event is
    SG_E_TIME; at it, every ring with a positive window sum is kept; a window later every ring goes; a chain batch
    that starts before the sweep is SG_E_TIME, and the batches from it on, the whole chain state and the window sums
    equal the oracles."""
    from oracle.binding import LocalTraceGen
    from tests.test_oracle_pslot_kat import rule as prule
    from tests.test_pslot_cluster_gpu import N_CP, _server
    from tests.test_slot_chain_gpu import Pool, _entries, _run as chain_run, _setup as chain_setup
    rng = np.random.default_rng(2303)
    n_res, n_origins, n_ctx = 12, 2, 2
    params = []
    for res in range(n_res):
        r = prule(res=res, idx=0, count=float(rng.integers(2, 8)))
        r["cluster_mode"] = abi.CLUSTER_MODE_FALLBACK if res % 3 else abi.CLUSTER_MODE_NO_FALLBACK
        r["cluster_key"] = res % N_CP
        params.append(r)
    params = np.array(params, abi.PSLOT_RULE_DTYPE)
    ora, ps, eng, fr, params = chain_setup(rng, n_res, n_origins, n_ctx, params=params)
    ns, cp, cp_hot = _server(rng, 0.0)
    cts = ClusterTokenService()
    cts.set_namespaces(ns)
    cts.load_param_rules(cp, cp_hot)
    ora.attach_cluster(cts, abi.CLUSTER_SERVER)
    eng.set_namespaces(ns)
    eng.cparam_load_rules(cp, cp_hot, 8)
    eng.local_set_cluster_state(abi.CLUSTER_SERVER)
    pool, gen, n, t, span = Pool(), LocalTraceGen(ora), 8000, T0 + 140_000, 2500
    ent = _entries(rng, n, n_res, t, span, n_origins, zipf=0.9, prio=0.0)
    ext = pool.draw(rng, n)
    ext["context"] = rng.integers(0, n_ctx, n)
    args, values = pool.arrays()
    ev, xo, want = gen.run_ext(ent, ext, rng.integers(0, 41, n).astype(np.int32), (rng.random(n) < 0.05).astype(np.uint8),
                               t + span + 1000, args, values)   # every exit (rt and queueing waits) inside the batch: none is left for later
    assert abi.LOCAL_BLOCK_PARAM in want["status"] and gen.pending() == 0
    vt._same(eng.slot_decide_host(ev, xo, args, values), want, "the chain batch before the sweep")
    last = int(ev["ts_ms"][-1])
    assert vt._code(eng.cparam_sweep, last - 1) == abi.SG_E_TIME        # the chain stamped the token server's time
    before = _used(eng, N_CP, True)
    live = sum(1 for k in range(N_CP) for v in range(1, 40) if cts.param_sum(k, v, last) > 0)
    assert live >= 5 and sum(u[0] for u in before) >= live
    got = eng.cparam_sweep(last)
    assert got["values_kept"] >= live and got["threads_removed"] == 0
    assert got["values_removed"] + got["claims_dropped"] + got["values_kept"] == sum(u[0] for u in before)
    kept = got["values_kept"]
    assert sum(u[0] for u in _used(eng, N_CP, True)) == kept
    for k in range(N_CP):
        for v in range(1, 40):
            assert eng.cparam_sum(k, v, last) == cts.param_sum(k, v, last), f"window sum of rule {k} value {v}"
    now = last + 1001                                                     # every bucket started at or before `last`
    assert eng.cparam_sweep(now) == _stats(removed=kept)
    assert sum(u[0] for u in _used(eng, N_CP, True)) == 0
    early = ev[:50].copy()
    early["ts_ms"] = now - 1
    early["create_ts"] = now - 1
    early["kind"] = abi.LOCAL_ENTRY
    assert vt._code(eng.slot_decide_host, early, xo[:50], args, values) == abi.SG_E_TIME
    t, pool, gen = chain_run(ora, ps, eng, fr, params, n_res, n_origins, n_ctx, [(8000, 2500), (8000, 2500)], 2303,
                             pool=pool, gen=gen, t=now, zipf=0.9)
    for k in range(N_CP):
        for v in range(1, 40):
            assert eng.cparam_sum(k, v, t) == cts.param_sum(k, v, t), f"cluster param sum of rule {k} value {v}"


TC_RES, TC_PER = 1 << 14, 64   # 16,384 resources x 64 values = the thread-count table's 2^20 slots


def _tc_events(kind, t, res, per=TC_PER):
    """One event per resource of `res` whose argument 0 is the collection of the resource's `per` values."""
    ev = np.zeros(len(res), abi.PSLOT_EVENT_DTYPE)
    ev["ts_ms"], ev["resource"], ev["count"], ev["kind"] = t, res, 1, kind
    ev["arg_begin"], ev["arg_count"] = np.arange(len(res)), 1
    args = np.zeros(len(res), abi.PSLOT_ARG_DTYPE)
    args["value_begin"], args["value_count"], args["kind"] = np.arange(len(res)) * per, per, abi.ARG_COLLECTION
    values = ((res.astype(np.uint64)[:, None] << np.uint64(24)) | np.arange(1, per + 1, dtype=np.uint64)[None, :]).reshape(-1)
    return ev, args, values


def test_thread_count_table_full_then_swept():
    """Case 5, the table that cannot grow: 16,384 resources (one lane each) enter with a collection of 64 values and
    the table holds exactly 2^20 entries; the even resources exit, so half the entries count 0. One more value is
    SG_E_CAPACITY, nothing changed. The sweep removes exactly the 2^19 entries at 0 and rehashes the 2^19 above it
    (a table at load 1 into one at load 1/2, every lane claiming by CAS); then the refused batch is accepted and
    every decision and thread count is the oracle's, also after the odd resources exit and a second sweep empties
    the table. Measured on one MI355X: the filling batch 1.47 s, the refused batch (two scans of the full table) 1.15 s,
    the sweep 0.7 ms, the whole case about 4 s; the test prints the three times."""
    import time
    rules = np.zeros(TC_RES, abi.PSLOT_RULE_DTYPE)
    rules["resource"], rules["grade"], rules["param_idx"] = np.arange(TC_RES), abi.FLOW_GRADE_THREAD, 0
    rules["rule"]["count"], rules["rule"]["duration_sec"], rules["rule"]["capacity_log2"] = 1000.0, 1, 1
    ora = ParamFlowSlot(rules, n_resources=TC_RES)
    eng = vt._engine()
    eng.pslot_load_rules(rules, n_resources=TC_RES)
    every, even, odd = np.arange(TC_RES, dtype=np.uint32), np.arange(0, TC_RES, 2, dtype=np.uint32), np.arange(1, TC_RES, 2, dtype=np.uint32)
    fill = _tc_events(abi.LOCAL_ENTRY, T0, every)
    t0 = time.perf_counter()
    vt._same(eng.pslot_decide_host(*fill), ora.decide(*fill), "the filling batch")
    t_fill = time.perf_counter() - t0
    leave = _tc_events(abi.LOCAL_EXIT, T0 + 10, even)
    vt._same(eng.pslot_decide_host(*leave), ora.decide(*leave), "the even resources exit")
    probe = [(int(r), int(v)) for r in (0, 1, 2, 4097, TC_RES - 2, TC_RES - 1) for v in ((r << 24) | 1, (r << 24) | TC_PER)]
    assert [ora.thread_count(r, 0, v) for r, v in probe] == [0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1]   # the premise

    def counts(what):
        for r, v in probe:
            assert eng.pslot_thread_count(r, 0, v) == ora.thread_count(r, 0, v), f"{what}: resource {r} value {v:#x}"

    counts("full")
    more = _tc_events(abi.LOCAL_ENTRY, T0 + 20, np.array([3, 8], np.uint32), per=2)
    more[2][:] = [7, 8, 9, 10]                                    # four values the table has never seen
    t0 = time.perf_counter()
    assert vt._code(eng.pslot_decide_host, *more) == abi.SG_E_CAPACITY
    t_refused = time.perf_counter() - t0
    counts("after the refusal")
    assert eng.pslot_thread_count(3, 0, 7) == 0
    t0 = time.perf_counter()
    assert eng.param_sweep(T0 + 20) == _stats(threads=TC_RES * TC_PER // 2)
    t_sweep = time.perf_counter() - t0
    counts("after the sweep")
    vt._same(eng.pslot_decide_host(*more), ora.decide(*more), "the refused batch, after the sweep")
    assert [eng.pslot_thread_count(r, 0, v) for r, v in ((3, 7), (3, 8), (8, 9), (8, 10))] == [1] * 4
    assert [ora.thread_count(r, 0, v) for r, v in ((3, 7), (3, 8), (8, 9), (8, 10))] == [1] * 4
    leave = _tc_events(abi.LOCAL_EXIT, T0 + 30, odd)
    vt._same(eng.pslot_decide_host(*leave), ora.decide(*leave), "the odd resources exit")
    counts("after every exit")
    assert eng.param_sweep(T0 + 40) == _stats(threads=TC_RES * TC_PER // 2)   # resources 3 and 8 keep two entries each
    counts("after the second sweep")
    assert [eng.pslot_thread_count(r, 0, v) for r, v in ((3, 7), (8, 10))] == [1, 1]
    print(f"thread-count table: fill {t_fill:.2f} s, refused batch {t_refused:.2f} s, sweep {t_sweep * 1e3:.1f} ms")
