"""The traces of tests/test_shaping_edges_gpu.py and their premises, from the oracle alone (no GPU): the WarmUp,
RateLimiter and WarmUpRateLimiter controllers of the local chain away from their comfortable path — cold factors other
than 3, fractional counts, counts below the cold factor, a NaN or sub-1 warning QPS, saturated and wrapped token
constants, second windows other than (2, 1000), traces that start before t = 1000 or pause for longer than the minute
ring, and acquire counts up to 2^30. Every builder is a plain function of its arguments (fixed seeds) whose arrays are
frozen, every reference a cached replay through oracle.binding.LocalChain / LocalTraceGen, every premise a function of
the oracle's answers. The tests here assert the premises; the GPU tests run the same references against the device."""
import collections
import functools

import numpy as np
import pytest

from oracle.binding import Controller, LocalChain, LocalTraceGen, local_flow_rule, local_rule
from sentinel_amd import abi

D, WU, RL, WRL = abi.CONTROL_DEFAULT, abi.CONTROL_WARM_UP, abi.CONTROL_RATE_LIMITER, abi.CONTROL_WARM_UP_RATE_LIMITER
T0 = 1_700_000_000_437
COLD_FACTORS = [2, 3, 5, 10]
SHAPES = [(1, 1000), (5, 500), (2, 2000), (10, 1000), (2, 3000)]  # (sampleCount, intervalInMs) of the second window
STARTS = [0, 999, 1000, T0]
GAPS = [0, 70_000, 30 * 3_600_000]

# One lone flow rule per resource (rule i on resource i): `batches` holds (entries, rt, err, t_end) for
# LocalTraceGen.run, `marks` whatever the premises need to know about the trace.
Case = collections.namedtuple("Case", "frules S interval cold batches marks")
# `ora` is the chain after the last batch (read, never advanced); outs: per batch (events, results, controllers [n, 3]).
Reference = collections.namedtuple("Reference", "ora outs")


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _rules(specs):
    """(behavior, count, warm_up_sec, max_queueing_ms) per resource."""
    fr = np.array([local_flow_rule(r, c, behavior=b, warm_up_sec=w, max_queueing_ms=q)
                   for r, (b, c, w, q) in enumerate(specs)], abi.LOCAL_FLOW_RULE_DTYPE)
    return _freeze(fr)[0]


def _batch(rng, per_res, t, span, t_end=None, big=0.0, multi=0.1, nonpos=0.0, rt_min=0):
    """per_res[r] entries of resource r at uniform times in [t, t + span), no origin, none prioritized; one in ten
    acquires 2..4; `big`: the share acquiring one of {1, 2, 7, 1000, 2^30}; `nonpos`: the share acquiring -1 or 0."""
    per_res = np.asarray(per_res, np.int64)
    n = int(per_res.sum())
    e = np.zeros(n, abi.LOCAL_EVENT_DTYPE)
    ts = t + rng.integers(0, max(span, 1), n)
    order = np.argsort(ts, kind="stable")
    e["ts_ms"] = ts[order]
    e["resource"] = rng.permutation(np.repeat(np.arange(len(per_res), dtype=np.uint32), per_res))[order]
    cnt = np.ones(n, np.int32)
    m = rng.random(n) < multi
    cnt[m] = rng.integers(2, 5, int(m.sum()))
    m = rng.random(n) < big
    cnt[m] = rng.choice(np.array([1, 2, 7, 1000, 1 << 30], np.int32), int(m.sum()))
    m = rng.random(n) < nonpos
    cnt[m] = rng.choice(np.array([-1, -1, 0], np.int32), int(m.sum()))
    e["count"] = cnt
    rt = rng.integers(rt_min, 41, n).astype(np.int32)
    err = (rng.random(n) < 0.05).astype(np.uint8)
    return _freeze(e, rt, err) + (int(t + span if t_end is None else t_end),)


def eff_cold(cold):
    """SentinelConfig.coldFactor() (SentinelConfig.java:224-239): <= 1 becomes the default."""
    return cold if cold > 1 else 3


def tokens(case):
    """(warningToken, maxToken) of every warm-up rule (None for the others), from the oracle's constructor."""
    out = []
    for r in case.frules:
        b = int(r["control_behavior"])
        c = Controller(float(r["count"]), int(r["warm_up_period_sec"]), eff_cold(case.cold), behavior=b) \
            if b in (WU, WRL) else None
        out.append((c.warning_token, c.max_token) if c else None)
    return out


def replay(case):
    n = len(case.frules)
    ora = LocalChain(case.S, case.interval, 500, cold_factor=case.cold)
    base = np.zeros(n, abi.LOCAL_RULE_DTYPE)
    base[:] = local_rule(0.0, abi.FLOW_GRADE_NONE)
    ora.load_rules(base)
    assert ora.load_flow_rules(case.frules) == n
    gen = LocalTraceGen(ora)
    outs = []
    for ent, rt, err, t_end in case.batches:
        ev, want = gen.run(ent, rt, err, t_end)
        ctl = np.array([ora.controller(i) for i in range(n)], np.int64)
        outs.append(_freeze(ev, want, ctl))
    return Reference(ora, tuple(outs))


def entry_mask(ev, res=None):
    m = ev["kind"] == abi.LOCAL_ENTRY
    return m if res is None else m & ((ev["resource"] & abi.KEY_INDEX) == res)


def passed(want):
    return (want["status"] == abi.LOCAL_PASS) | (want["status"] == abi.LOCAL_PASS_WAIT)


# ------------------------------------------------------------------- 1. cold factor x count x warm-up period

COLD_COUNTS = [0.5, 2.0, 7.5, 20.0, 100.0, 333.3]
COLD_WARM = [1, 3, 10]
BURST, IDLE, TRICKLE, STEADY = 4000, 25_000, 12_000, 12_000  # ms


@functools.lru_cache(maxsize=None)
def cold_case(cold):
    """36 lone rules {WarmUp, WarmUpRateLimiter} x count x warmUpPeriodSec; a burst at 3 x count for 4 s, 25 s idle, a
    trickle at count / (2 * coldFactor) for 12 s (under the `passQps < (int)count / coldFactor` refill line), then
    0.8 x count for 12 s. One batch per phase; the idle phase is a gap between batches."""
    specs = [(b, c, w, 300) for b in (WU, WRL) for c in COLD_COUNTS for w in COLD_WARM]
    counts = np.array([s[1] for s in specs])
    rng = np.random.default_rng(100 + cold)
    per = lambda rate, ms: np.maximum(1, np.rint(rate * ms / 1000)).astype(np.int64)  # noqa: E731
    t1 = T0 + BURST + IDLE
    batches = (_batch(rng, per(3 * counts, BURST), T0, BURST),
               _batch(rng, per(counts / (2 * eff_cold(cold)), TRICKLE), t1, TRICKLE),
               _batch(rng, per(0.8 * counts, STEADY), t1 + TRICKLE, STEADY))
    return Case(_rules(specs), 2, 1000, cold, batches, None)


@functools.lru_cache(maxsize=None)
def cold_reference(cold):
    return replay(cold_case(cold))


def premise_cold(case, ref):
    n = len(case.frules)
    tok = tokens(case)
    beh = case.frules["control_behavior"]
    (ev0, want0, ctl0), (_, _, ctl1), (_, _, ctl2) = ref.outs
    both = 0
    for r in range(n):
        m = entry_mask(ev0, r)
        both += int(passed(want0)[m].sum() >= 10 and (~passed(want0))[m].sum() >= 10)
    assert both >= 8, f"{both} rules with >= 10 passes and >= 10 blocks in the burst"
    n_ent = np.zeros(n, np.int64)
    n_pass = np.zeros(n, np.int64)
    for ev, want, _ in ref.outs:
        m = entry_mask(ev)
        n_ent += np.bincount(ev["resource"][m], minlength=n)
        n_pass += np.bincount(ev["resource"][m & passed(want)], minlength=n)
    assert (n_ent > 0).all()
    assert any(beh[r] == WU and n_pass[r] == 0 for r in range(n)), "no WarmUp rule that passes nothing"
    assert any(beh[r] == WRL and tok[r] == (0, 0) and n_pass[r] == n_ent[r] for r in range(n)), \
        "no WarmUpRateLimiter rule without tokens that passes everything"
    warning = np.array([t[0] for t in tok])
    above = int((ctl1[:, 0] > warning).sum())
    below = int(((ctl0[:, 0] < warning) | (ctl2[:, 0] < warning)).sum())
    assert above >= 10, f"{above} rules above the warning line after the trickle"
    assert below >= 10, f"{below} rules below the warning line after the burst or the steady phase"


@pytest.mark.parametrize("cold", COLD_FACTORS + [0, 1])
def test_cold_premises(cold):
    case = cold_case(cold)
    sizes = [len(b[0]) for b in case.batches]
    assert sum(sizes) <= 72_000 and sizes[0] >= 30_000
    # the 333.3-count resources' burst segments are long ones (the wave walker's); the others' stay short
    per = np.bincount(case.batches[0][0]["resource"], minlength=36)
    assert (per[case.frules["count"] == 333.3] >= 3900).all() and (per[case.frules["count"] < 333.3] <= 1300).all()
    premise_cold(case, cold_reference(cold))


def test_cold_0_and_1_are_3():
    """The traces differ (their seeds do), the constants do not: SentinelConfig's default."""
    assert tokens(cold_case(0)) == tokens(cold_case(1)) == tokens(cold_case(3))
    assert tokens(cold_case(3)) != tokens(cold_case(2))


# ------------------------------------------------------------------- 2. window shapes under warm-up

SHAPE_SPECS = [(WU, 100.0, 3, 500), (WU, 20.0, 2, 500), (WU, 33.3, 3, 500), (WRL, 33.3, 2, 300)]
SHAPE_SPAN = 3500


@functools.lru_cache(maxsize=None)
def shape_case(S, interval):
    """Three lone WarmUp resources and a WarmUpRateLimiter far over their counts for three batches of 3.5 s; resource
    0 takes 12k entries a batch (a long segment), the others 2k each."""
    rng = np.random.default_rng(200 + S * 7 + interval)
    batches = tuple(_batch(rng, [12_000, 2_000, 2_000, 2_000], T0 + i * SHAPE_SPAN, SHAPE_SPAN) for i in range(3))
    return Case(_rules(SHAPE_SPECS), S, interval, 3, batches, None)


@functools.lru_cache(maxsize=None)
def shape_reference(S, interval):
    return replay(shape_case(S, interval))


def sync_inside_period(ev, want, res, wl):
    """Window periods [p, p + wl) of `res` with a block before the one-second boundary inside them and a pass after
    it: syncToken raised the limit in mid-period."""
    m = entry_mask(ev, res)
    ts, ok = ev["ts_ms"][m], passed(want)[m]
    hits = 0
    for p in np.unique(ts // wl * wl):
        sb = (p // 1000 + 1) * 1000
        if sb < p + wl:
            hits += int((~ok[(ts >= p) & (ts < sb)]).any() and ok[(ts >= sb) & (ts < p + wl)].any())
    return hits


def premise_shape(case, ref):
    ev = np.concatenate([o[0] for o in ref.outs])
    want = np.concatenate([o[1] for o in ref.outs])
    for r in np.nonzero(case.frules["control_behavior"] == WU)[0]:
        m = entry_mask(ev, r)
        secs = np.unique(ev["ts_ms"][m & passed(want)] // 1000)
        assert len(secs) >= 3, f"resource {r} passes in {len(secs)} seconds"
        assert (m & ~passed(want)).sum() >= 100, f"resource {r} has too few blocks"
    if (case.S, case.interval) == (2, 3000):
        assert any(sync_inside_period(ev, want, r, 1500) > 0 for r in range(len(case.frules)))


@pytest.mark.parametrize("S,interval", SHAPES)
def test_shape_premises(S, interval):
    premise_shape(shape_case(S, interval), shape_reference(S, interval))


# ------------------------------------------------------------------- 3. time edges

EDGE_SPECS = [(WU, 20.0, 2, 500), (WU, 7.5, 3, 500), (WU, 33.3, 2, 500), (WU, 100.0, 5, 500),
              (WRL, 20.0, 2, 300), (WRL, 4.5, 3, 500), (WRL, 33.3, 3, 300),
              (RL, 10.0, 10, 200), (RL, 33.3, 10, 500), (RL, 0.7, 10, 2000)]
EDGE_LOAD = np.array([300, 100, 300, 600, 300, 100, 300, 100, 300, 50])  # entries per second


@functools.lru_cache(maxsize=None)
def edge_case(t0):
    """From t0: the events before t = 1000 as a batch of their own (t0 < 1000), 3 s of load, 2 s more at once (gap 0);
    then after 70 s and again after 30 h of silence: one entry of resource 0 as a batch, one entry of every other
    resource, and 2 s of load. Every batch before a gap runs until its last exit."""
    rng = np.random.default_rng(300 + t0 % 1000)
    n = len(EDGE_SPECS)
    load = lambda ms: np.maximum(1, EDGE_LOAD * ms // 1000)  # noqa: E731
    one = np.eye(n, dtype=np.int64)[0]
    batches, marks, t = [], {"first_second": None, "after_gap": []}, t0
    if t0 < 1000:
        marks["first_second"] = 0
        batches.append(_batch(rng, load(1000), t, 1000 - t))  # t0 = 999: a second's load within 1 ms
        t = 1000
    batches.append(_batch(rng, load(3000), t, 3000))
    batches.append(_batch(rng, load(2000), t + 3000, 2000, t_end=t + 5000 + 2500))
    t += 5000
    for gap in GAPS[1:]:
        t += gap
        batches.append(_batch(rng, one, t + 7, 1, multi=0.0, rt_min=5))  # its exit: the next batch
        batches.append(_batch(rng, 1 - one, t + 8, 1, t_end=t + 2600, multi=0.0))
        marks["after_gap"].append(len(batches) - 1)
        batches.append(_batch(rng, load(2000), t + 2600, 2000, t_end=t + 4600 + 2500))
        t += 4600
    return Case(_rules(EDGE_SPECS), 2, 1000, 3, tuple(batches), marks)


@functools.lru_cache(maxsize=None)
def edge_reference(t0):
    return replay(edge_case(t0))


def premise_edge(case, ref):
    warm = np.isin(case.frules["control_behavior"], (WU, WRL))
    tok = tokens(case)
    if case.marks["first_second"] is not None:
        ev, want, ctl = ref.outs[case.marks["first_second"]]
        assert len(ev) > 0 and ev["ts_ms"].max() < 1000
        wu = case.frules["control_behavior"] == WU
        assert (np.bincount(ev["resource"][entry_mask(ev)], minlength=len(wu))[wu] > 0).all()
        assert (ctl[wu, 1] == 0).all() and (ctl[wu, 0] == 0).all(), "a sync before t = 1000"
    for b in case.marks["after_gap"]:
        assert len(ref.outs[b - 1][0]) == 1, "the batch after the gap is not one event"
        ctl = ref.outs[b][2]
        t = int(ref.outs[b][0]["ts_ms"][0])
        for r in np.nonzero(warm)[0]:
            assert ctl[r, 1] == t // 1000 * 1000
            assert ctl[r, 0] == tok[r][1] > 0, f"rule {r} after the gap: storedTokens {ctl[r, 0]}, maxToken {tok[r][1]}"


@pytest.mark.parametrize("t0", STARTS)
def test_edge_premises(t0):
    case = edge_case(t0)
    gaps = [int(b[0]["ts_ms"][0]) - int(a[0]["ts_ms"][-1]) for a, b in zip(case.batches, case.batches[1:])]
    assert sum(g > 69_000 for g in gaps) == 2 and max(gaps) > 30 * 3_600_000 - 10_000
    premise_edge(case, edge_reference(t0))


# ------------------------------------------------------------------- 4. large acquires, extreme counts

BIG_SPECS = [(RL, 1e-7, 10, 500), (RL, 33.3, 10, 500), (WU, 0.0, 10, 500), (WRL, 0.0, 10, 500),
             (WU, 3e8, 10, 500), (WU, 1e9, 3, 500), (WU, 2.0 ** 31, 1, 500), (WRL, 100.0, 3, 500),
             (WU, 2.0 ** 31, 2, 500)]
BIG_T0 = 1_700_000_000_000


@functools.lru_cache(maxsize=None)
def big_case():
    """Three batches of 18k entries over 3 s each, one in twenty acquiring one of {1, 2, 7, 1000, 2^30}. At
    t = 1.7e12 the 1e-7 rule (a cost of 1e10 ms a token) passes its first entry and then only those whose cost
    saturates Math.round and wraps `costTime + latestPassedTime` negative."""
    rng = np.random.default_rng(400)
    batches = tuple(_batch(rng, [2_000] * len(BIG_SPECS), BIG_T0 + i * 3000, 3000, big=0.05) for i in range(3))
    return Case(_rules(BIG_SPECS), 2, 1000, 3, batches, None)


@functools.lru_cache(maxsize=None)
def big_reference():
    return replay(big_case())


def premise_big(case, ref):
    ev = np.concatenate([o[0] for o in ref.outs])
    want = np.concatenate([o[1] for o in ref.outs])
    ok = passed(want)
    m = entry_mask(ev, 0)
    assert (m & ok & (ev["count"] == 1 << 30)).any(), "the 1e-7 rule passes no 2^30 acquire"
    assert (m & ~ok & (ev["count"] == 1)).any(), "the 1e-7 rule blocks no single acquire"
    assert (m & ok).sum() < (m & (ev["count"] == 1 << 30)).sum() + 2
    tok = tokens(case)
    # count >= 3e8: (int)(warmUpPeriodInSec * count) saturates and maxToken wraps negative, so coolDownTokens returns
    # a negative number and syncToken clamps the bucket to 0 every second — but for 2^31 / warmUp 1, where
    # 1073741823 + (int)(2 * 2^31 / 4.0) is INT_MAX exactly: that bucket fills to INT_MAX and stays above the line
    wrapped = [r for r in np.nonzero(case.frules["count"] >= 3e8)[0] if tok[r][1] < 0]
    assert len(wrapped) == 3 and tok[6] == (1073741823, 2147483647)
    for _, _, ctl in ref.outs:
        for r in wrapped:
            assert ctl[r, 0] == 0, f"rule {r} (maxToken {tok[r][1]}): storedTokens {ctl[r, 0]}"
        assert tok[6][0] < ctl[6, 0] <= tok[6][1]
    assert not (entry_mask(ev, 2) & ok).any(), "the count 0 WarmUp rule passes"
    assert ok[entry_mask(ev, 3)].all(), "the count 0 WarmUpRateLimiter rule blocks"
    for r in range(len(case.frules)):
        assert (entry_mask(ev, r) & (ev["count"] == 1 << 30)).sum() >= 5


def test_big_premises():
    premise_big(big_case(), big_reference())


# ------------------------------------------------------------------- 4b. acquire counts <= 0

NONPOS_SPECS = [(WRL, 400.0, 1, 500), (WRL, 100.0, 3, 500), (RL, 33.3, 10, 500), (WU, 20.0, 2, 500), (WU, 0.0, 10, 500)]


@functools.lru_cache(maxsize=None)
def nonpos_case():
    """Three batches of 10k entries over 3 s each, one in twenty acquiring -1 or 0 (SphU.entry takes any int). Only
    RateLimiterController looks at the sign (:48-50); the WarmUpRateLimiter's cost is then negative, and at count 400
    below the warning line it is Math.round(-2.5) == -2 for -1: the one place where Math.round's ties toward
    +Infinity differ from rounding half away from zero. The rule is over its rate, so most entries queue
    (latestPassedTime += costTime) and the difference stays in its state."""
    rng = np.random.default_rng(450)
    batches = tuple(_batch(rng, [2_000] * len(NONPOS_SPECS), BIG_T0 + 211 + i * 3000, 3000, nonpos=0.05)
                    for i in range(3))
    return Case(_rules(NONPOS_SPECS), 2, 1000, 3, batches, None)


@functools.lru_cache(maxsize=None)
def nonpos_reference():
    return replay(nonpos_case())


def premise_nonpos(case, ref):
    tok = tokens(case)
    queued = 0
    for ev, want, ctl in ref.outs:
        assert ctl[0, 0] < tok[0][0], "the count 400 rule ends a batch at or above the warning line"
        queued += int((entry_mask(ev, 0) & (ev["count"] == -1) & passed(want) & (want["wait_ms"] > 0)).sum())
        for r in range(len(case.frules)):
            assert (entry_mask(ev, r) & (ev["count"] <= 0)).sum() >= 20
    assert queued >= 10, f"{queued} queued entries with acquireCount -1 on the count 400 rule"


def test_nonpos_premises():
    premise_nonpos(nonpos_case(), nonpos_reference())


# ------------------------------------------------------------------- the oracle binding

def test_indivisible_window_is_refused():
    """LeapArray's constructor asserts intervalInMs % sampleCount == 0 (LeapArray.java:61-72): no chain, no crash."""
    with pytest.raises(ValueError):
        LocalChain(3, 1000)
    with pytest.raises(ValueError):
        LocalChain(0, 1000)
